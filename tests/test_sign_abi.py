"""CPU tests of the signature calls' boundary (include/zra_hip.h: ZraHipSignArchive, ZraHipDiffSignature, their stats and bring-up
times): declared and exported, the Python binding exists, without an engine every call is refused before anything touches a device,
the zra_sig_ kernels compiled without scratch, and the model the GPU tests use as their yardstick (tests/sign_model.py): its XXH64
is the oracle's, and "dirty = the words differ" gives the diff model's patch."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import diff_model as DM
import sign_model as SM
from test_diff_abi import _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_CALLS = ["ZraHipSignArchive", "ZraHipGetSignStats", "ZraHipDebugSignMs", "ZraHipDiffSignature", "ZraHipGetDiffSignatureStats",
              "ZraHipDebugDiffSignatureMs"]


def test_sign_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in SIGN_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    for name, value in (("SIGN_MIN_GRAIN", 64), ("SIGN_MAX_GRAIN", 8192), ("SIGDIFF_DECODE_ALL", 1)):
        assert re.search(r"#define\s+ZRA_HIP_%s\s+%du" % (name, value), txt), name
        assert getattr(zra, name) == value
    assert ctypes.sizeof(zra.ZraHipSignature) == 40
    assert [f[0] for f in zra.ZraHipSignature._fields_] == ["contentSize", "frameSize", "grain", "seed", "frames", "words"]


def test_sign_binding_exists(zra):
    for name in ("sign", "sign_stats", "sign_ms", "diff_signature", "diff_signature_stats", "diff_signature_ms"):
        assert callable(getattr(zra.Engine, name)), name
    assert zra.Signature._fields == ("content_size", "frame_size", "grain", "seed", "frames", "words")
    assert len(zra.SIGN_STATS) == 6 and zra.SIGN_STATS[:2] == ("frames", "signed")
    assert zra.SIGDIFF_STATS == ("frames", "equal_compressed", "decoded", "tail_decoded", "writes", "dirty_bytes", "passes", "dirty_grains")
    assert zra.signature_words(0, 1000, 64) == 0 and zra.signature_words(20700, 1000, 64) == 21 * 17 == SM.words(20700, 1000, 64)
    assert zra.signature_words(1000, 4, 64) == 500 and zra.signature_words(65536, 65536, 8192) == 9


def test_calls_without_an_engine_are_refused(zra):
    """{ZStdError, 42} for every combination of the other arguments; the outputs are zeroed and the host arrays are left alone (the
    remaining refusals need an engine: tests/test_gpu_sign.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for arc in ((None, 0), (P(64), 100), (None, 100)):
        for grain in (0, 63, 64, 4096, 8192, 16384):
            for sig in ((None, 0), (P(4096), 8), (None, 8)):
                info = zra.ZraHipSignature(1, 2, 3, 4, 5, 6)
                st = L.ZraHipSignArchive(None, *arc, grain, 7, 0, 0xFFFFFFFFFFFFFFFF, 0, *sig, ctypes.byref(info))
                assert st.tup() == (1, 42) and bytes(info) == bytes(40), (arc, grain, sig)
                assert L.ZraHipSignArchive(None, *arc, grain, 7, 0, 1, 0, *sig, None).tup() == (1, 42)
    good = zra.ZraHipSignature(2000, 1000, 64, 0, 2, 34)
    for sig in (None, good, zra.ZraHipSignature(2000, 1000, 63, 0, 2, 34)):
        for words in ((None, 0), (P(4096), 34), (None, 34)):
            for b in ((None, 0), (P(64), 100), (None, 100)):
                for mode in (0, 1, 2):
                    for data in ((None, 0), (P(8192), 64), (None, 64)):
                        arrs = [(ctypes.c_uint64 * 4)() for _ in range(3)]
                        for x in arrs:
                            ctypes.memset(x, 0xEE, 32)
                        w = [ctypes.c_uint64(0x1234) for _ in range(4)]
                        st = L.ZraHipDiffSignature(None, ctypes.byref(sig) if sig is not None else None, *words, *b, mode, 0, *arrs, 4, ctypes.byref(w[0]),
                                                   *data, ctypes.byref(w[1]), ctypes.byref(w[2]), ctypes.byref(w[3]))
                        assert st.tup() == (1, 42)
                        assert [x.value for x in w] == [0] * 4 and all(bytes(x) == b"\xEE" * 32 for x in arrs)
                        assert L.ZraHipDiffSignature(None, ctypes.byref(sig) if sig is not None else None, *words, *b, mode, 1, None, None, None, 0, None,
                                                     *data, None, None, None).tup() == (1, 42)
    assert L.ZraHipDebugSignMs(None) == 0.0 and L.ZraHipDebugDiffSignatureMs(None) == 0.0


def test_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    for f in (L.ZraHipGetSignStats, L.ZraHipGetDiffSignatureStats):
        out = (ctypes.c_uint64 * 8)(*([7] * 8))
        f(None, out)
        assert list(out) == [0] * 8
        f(None, None)                                                          # no-op


def test_sign_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_sign.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).sign(64, 100, 4096, 8)                                   # no engine without a GPU: never a CPU result


def test_sig_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    kernels = [k for k in res if k.startswith("zra_sig_")]
    assert sorted(kernels) == ["zra_sig_count_kernel", "zra_sig_fill_kernel", "zra_sig_grains_kernel", "zra_sig_jobs_kernel", "zra_sig_spans_kernel"], kernels
    for k in kernels:
        assert res[k]["source"] == "zra_sign.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
    # the shared steps stay where they were
    assert res["zra_diff_scan_kernel"]["source"] == res["zra_diff_tail_kernel"]["source"] == "zra_compare.hip"


def test_model_xxh64_is_the_oracles(oracle):
    L = oracle.lib()
    rng = np.random.RandomState(64)
    data = rng.randint(0, 256, size=8300).astype(np.uint8).tobytes()
    for seed in (0, 1, (1 << 64) - 1):
        for n in list(range(101)) + [8191, 8192, 8193, 8224]:
            for off in (0, 3):
                piece = data[off:off + n]
                buf = ctypes.create_string_buffer(piece, max(n, 1))
                assert SM.xxh64(piece, seed) == L.zo_xxh64(buf, n, seed), (seed, n, off)
    assert SM.xxh64(b"", 0) == 0xEF46DB3751D8E999                              # the published value of the empty input


def test_model_signature_diff_is_the_diff_model():
    """The 300 cases of the diff's model test with every byte and the frame size repeated 16 times, so that grain 64 cuts the frames
    (16, 64, 112, 256, 320 and 1,600 bytes): "the words differ" marks the grains the byte compare marks."""
    k, some, short, several = 16, 0, 0, 0
    for a, b, fs in _cases():
        a, b, fs = bytes(np.repeat(np.frombuffer(a, dtype=np.uint8), k)), bytes(np.repeat(np.frombuffer(b, dtype=np.uint8), k)), fs * k
        for grain, seed in ((64, 0), (128, 0x9E3779B97F4A7C15)):
            ga = SM.grain_words(a, fs, grain, seed)
            assert all(len(x) == SM.gpf(fs, grain) for x in ga) and len(ga) == -(-len(a) // fs)
            want = DM.patch(a, b, fs, grain)
            assert SM.patch(ga, len(a), b, fs, grain, seed) == want, (len(a), len(b), fs, grain)
            some += bool(want[0])
            short += fs % grain != 0 and bool(want[0])
            several += fs > grain and bool(want[0])
    assert some > 200 and short > 50 and several > 50, (some, short, several)


def test_model_signature_layout():
    """Record f at word f * (1 + gpf); a zero word behind the last grain of a short last frame; the frame word is over the span."""
    fs, grain = 100, 64
    plain = bytes(range(250))
    # a hand-made archive: 38 fixed bytes, no meta, a table of 4 entries, spans of 5, 0 and 7 bytes
    body = b"AAAAA" + b"CCCCCCC"
    table = b"".join(int(x).to_bytes(5, "little") for x in (0, 5, 5, 12))
    arc = bytearray(38) + table + body
    arc[4:8] = (38 + len(table) - 8).to_bytes(4, "little")
    w = SM.signature(bytes(arc), plain, fs, grain, 5)
    assert len(w) == 3 * 3 == SM.words(250, fs, grain)
    assert [w[0], w[3], w[6]] == [SM.xxh64(b"AAAAA", 5), SM.xxh64(b"", 5), SM.xxh64(b"CCCCCCC", 5)]
    assert w[1:3] == [SM.xxh64(plain[0:64], 5), SM.xxh64(plain[64:100], 5)] and w[7:9] == [SM.xxh64(plain[200:250], 5), 0]
