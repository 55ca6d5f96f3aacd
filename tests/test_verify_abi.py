"""CPU tests of the verify call's boundary (include/zra_hip.h: ZraHipVerifyArchive, ZraHipGetVerifyStats): declared and exported, the
Python binding exists, NULL arguments and bad modes are refused before anything touches a device, no CPU result without a GPU, the
verifier's kernels compiled without scratch, and the pure-Python structure model the GPU tests use as their yardstick
(tests/verify_model.py) flags exactly the frames a test damages."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import verify_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY_CALLS = ["ZraHipVerifyArchive", "ZraHipGetVerifyStats"]
VERIFY_KERNELS = ["zra_vfy_structure_kernel", "zra_vfy_jobs_kernel", "zra_vfy_collect_kernel"]
MAXU64 = (1 << 64) - 1


def test_verify_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in VERIFY_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_VERIFY_STRUCTURE\s+1u", txt) and re.search(r"#define\s+ZRA_HIP_VERIFY_CONTENT\s+2u", txt)
    assert (zra.VERIFY_STRUCTURE, zra.VERIFY_CONTENT) == (1, 2)
    assert ctypes.sizeof(zra.ZraHipFrameFault) == 16


def test_verify_binding_exists(zra):
    assert callable(zra.Engine.verify) and callable(zra.Engine.verify_stats)
    assert zra.VERIFY_STATS == ("frames", "checked", "structure_faults", "content_faults", "decoded", "content_bytes", "passes")


def test_verify_refuses_null_arguments_and_bad_modes(zra):
    """{ZStdError, 42}; *nFaults is zeroed and the fault array left alone. Without an engine every combination of the other arguments is
    refused alike (the remaining cases need an engine: tests/test_gpu_verify.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for mode in (0, 1, 2, 3, 4, 7, 0x80000001):
        for args in ((None, 0), (P(64), 100), (None, 100)):
            arr = (zra.ZraHipFrameFault * 2)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n = ctypes.c_size_t(0x1234)
            assert L.ZraHipVerifyArchive(None, *args, mode, 0, MAXU64, 0, arr, 2, ctypes.byref(n)).tup() == (1, 42), (mode, args)
            assert n.value == 0 and bytes(arr) == b"\xEE" * 32
            assert L.ZraHipVerifyArchive(None, *args, mode, 0, MAXU64, 0, None, 0, None).tup() == (1, 42), (mode, args)


def test_verify_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetVerifyStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetVerifyStats(None, None)                                         # no-op


def test_verify_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        pytest.skip("a GPU is present; covered by tests/test_gpu_verify.py")
    with pytest.raises(zra.ZraError):
        zra.Engine(0).verify(64, 100)                                          # no engine without a GPU: never a CPU result


def test_verify_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    for k in VERIFY_KERNELS:
        assert k in res, k
        assert res[k]["source"] == "zra_verify.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])


def _lz(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 24, size=n).astype(np.uint8)
    for _ in range(n // 4096 + 1):
        src, ln = int(rng.randint(0, max(1, n - 600))), int(rng.randint(16, 512))
        dst = int(rng.randint(0, max(1, n - ln)))
        a[dst:dst + ln] = a[src:src + ln]
    return a.tobytes()


@pytest.mark.parametrize("fs,nfr,ck", [(4096, 9, True), (65536, 4, False), (262144, 2, True)])
def test_structure_model_flags_exactly_the_damaged_frames(fs, nfr, ck):
    data = _lz(nfr * fs + fs // 3, fs + ck)
    st, arc = O.zra_compress(data, 3, fs, ck)
    assert st == (0, 0) and M.crc_ok(arc)
    hs, t, F, fs2, U = M.fields(arc)
    e = M.entries(arc)
    assert (F, fs2, U) == (nfr + 1, fs, len(data)) and e[-1] == len(arc) - hs
    assert M.structure_faults(arc) == {}
    if fs == 262144:
        assert len(M.block_headers(arc[hs + e[0]:hs + e[1]])) >= 2               # the walk takes more than one step

    def edit(at, fn):
        a = bytearray(arc)
        a[at] = fn(a[at])
        return bytes(a)

    # a wrong magic
    assert M.structure_faults(edit(hs + e[1], lambda b: b ^ 1)) == {1: 10}
    # a table entry moved by one: the frame in front of it runs one byte long, the frame behind it starts one byte late
    assert set(M.structure_faults(M.set_entry(arc, 2, e[2] + 1))) == {1, 2}
    # the last entry is not the body size / points beyond the body
    assert M.structure_faults(M.set_entry(arc, F, e[F] - 1)) == {F - 1: 72}
    assert M.structure_faults(M.set_entry(arc, F, e[F] + 1000)) == {F - 1: 72}
    assert M.structure_faults(arc[:-3]) == {F - 1: 72}
    # an inverted span
    assert M.structure_faults(M.set_entry(arc, 1, e[2] + 1))[1] == 72
    # a declared content size (the encoder writes none: one is put in), right and wrong in both directions
    assert M.header_layout(arc[hs + e[0]:hs + e[1]])[2] == 0
    assert M.structure_faults(M.with_fcs(arc, 0, fs)) == {}
    assert M.structure_faults(M.with_fcs(arc, 0, fs + 1)) == {0: 70}
    assert M.structure_faults(M.with_fcs(arc, 0, fs - 1)) == {0: 20}
    assert M.structure_faults(M.with_fcs(arc, F - 1, U - (F - 1) * fs + 1)) == {F - 1: 70}
    # the reserved bit, reserved block type, Last_Block cleared
    k = F - 2
    assert M.structure_faults(edit(hs + e[k] + 4, lambda b: b | 8)) == {k: 14}
    last = M.block_headers(arc[hs + e[k]:hs + e[k + 1]])[-1]
    assert M.structure_faults(edit(hs + e[k] + last, lambda b: b | 6)) == {k: 20}
    got = M.structure_faults(edit(hs + e[k] + last, lambda b: b & 0xFE))
    assert set(got) == {k} and (ck or got == {k: 72})
    # the model agrees with the decoder of the oracle on which frames are bad
    for a in (edit(hs + e[1], lambda b: b ^ 1), edit(hs + e[k] + last, lambda b: b & 0xFE), M.with_fcs(arc, 0, fs - 1)):
        for f, code in M.structure_faults(a).items():
            out, err = O.decompress(a[hs + e[f]:hs + e[f + 1]], fs)
            assert out is None or len(out) != min(fs, U - f * fs), (f, code)
