"""CPU tests of the diff call's boundary (include/zra_hip.h: ZraHipDiffArchives, ZraHipGetDiffStats, ZraHipDebugDiffMs): declared and
exported, the Python binding exists, without an engine every call is refused before anything touches a device, no CPU result without a
GPU, the diff kernels compiled without scratch, and the model the GPU tests use as their yardstick (tests/diff_model.py) agrees with
the compare's model at grain 1 and turns A's plaintext into B's at every grain."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import compare_model as CM
import diff_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFF_CALLS = ["ZraHipDiffArchives", "ZraHipGetDiffStats", "ZraHipDebugDiffMs"]
GRAINS = (1, 2, 16, 64, 8192)


def test_diff_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in DIFF_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_DIFF_DECODE_ALL\s+1u", txt) and re.search(r"#define\s+ZRA_HIP_DIFF_MAX_GRAIN\s+8192u", txt)
    assert (zra.DIFF_DECODE_ALL, zra.DIFF_MAX_GRAIN) == (1, 8192)
    assert "a patch that ZraHipUpdateArchive could apply" not in " ".join(txt.split())   # the gap the compare named is closed
    assert "a patch that `ZraHipUpdateArchive` could apply" not in " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())


def test_diff_binding_exists(zra):
    for name in ("diff", "diff_stats", "diff_ms"):
        assert callable(getattr(zra.Engine, name)), name
    assert zra.DIFF_STATS == ("frames", "equal_compressed", "decoded", "tail_decoded", "writes", "dirty_bytes", "passes", "dirty_grains")


def test_diff_without_an_engine_is_refused(zra):
    """{ZStdError, 42} for every combination of the other arguments; the four output words are zeroed and the host arrays are left
    alone (the remaining refusals need an engine: tests/test_gpu_diff.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for a in ((None, 0), (P(64), 100), (None, 100)):
        for b in ((None, 0), (P(64), 100)):
            for mode in (0, 1, 2):
                for grain in (0, 1, 3, 64, 8192, 16384):
                    for data in ((None, 0), (P(4096), 64), (None, 64)):
                        arrs = [(ctypes.c_uint64 * 4)() for _ in range(3)]
                        for x in arrs:
                            ctypes.memset(x, 0xEE, 32)
                        w = [ctypes.c_uint64(0x1234) for _ in range(4)]
                        st = L.ZraHipDiffArchives(None, *a, *b, mode, grain, 0, *arrs, 4, ctypes.byref(w[0]), *data, ctypes.byref(w[1]),
                                                  ctypes.byref(w[2]), ctypes.byref(w[3]))
                        assert st.tup() == (1, 42)
                        assert [x.value for x in w] == [0] * 4 and all(bytes(x) == b"\xEE" * 32 for x in arrs)
                        assert L.ZraHipDiffArchives(None, *a, *b, mode, grain, 1, None, None, None, 0, None, *data, None, None, None).tup() == (1, 42)
    assert L.ZraHipDebugDiffMs(None) == 0.0


def test_diff_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetDiffStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetDiffStats(None, None)                                           # no-op


def test_diff_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_diff.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).diff(64, 100, 64, 100, 4096, 64)                         # no engine without a GPU: never a CPU result


def test_diff_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    kernels = [k for k in res if k.startswith("zra_diff_")]
    assert sorted(kernels) == ["zra_diff_count_kernel", "zra_diff_fill_kernel", "zra_diff_scan_kernel", "zra_diff_tail_kernel"], kernels
    for k in kernels:
        assert res[k]["source"] == "zra_compare.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])


def _cases():
    """Pairs of short plaintexts over a two-letter alphabet, b at least as long as a, with a frame size that is no multiple of the
    larger grains."""
    rng = np.random.RandomState(16)
    for case in range(300):
        n = int(rng.randint(0, 60))
        a = rng.randint(0, 2, size=n).astype(np.uint8)
        b = a.copy()
        for _ in range(int(rng.randint(0, 5)) if case % 5 else 0):
            if n:
                p = int(rng.randint(0, n)); b[p:p + int(rng.randint(1, 6))] ^= 1
        b = np.concatenate((b, rng.randint(0, 2, size=int(rng.randint(0, 30)) if case % 3 else 0).astype(np.uint8)))
        yield bytes(a), bytes(b), int(rng.choice((1, 4, 7, 16, 20, 100)))


def test_model_at_grain_1_is_the_compare_model():
    some = 0
    for a, b, fs in _cases():
        w, data, ao, asz = M.patch(a, b, fs, 1)
        assert w == CM.ranges(a, b), (a, b, fs)
        assert data[:ao] == b"".join(b[o:o + n] for o, n in w) and data[ao:] == b[len(a):] and asz == len(b) - len(a)
        some += bool(w)
    assert some > 100


def test_model_patch_turns_a_into_b_at_every_grain():
    merged = short = across = 0
    for a, b, fs in _cases():
        ref = CM.ranges(a, b)
        for grain in GRAINS:
            w, data, ao, asz = M.patch(a, b, fs, grain)
            assert M.apply(a, w, data, ao, asz) == b, (a, b, fs, grain)
            assert ao == sum(n for _, n in w) and len(data) == ao + asz
            assert all(o + n < o2 for (o, n), (o2, _) in zip(w, w[1:]))        # ascending, no two writes share or touch a byte
            for o, n in w:                                                     # whole clipped grains, each with a differing byte at its ends' grains
                assert (o % fs) % grain == 0 and ((o + n) % fs % grain == 0 or (o + n) % fs == 0 or o + n == len(a)), (o, n, fs, grain)
            assert all(any(o <= r < o + n for o, n in w) for r, _ in ref)
            s = M.stats(a, b, fs, grain)
            assert s["dirty_bytes"] == ao and s["writes"] == len(w) and s["dirty_grains"] >= len(w)
            merged += len(w) < len(ref)
            short += any((o + n) % fs % grain != 0 for o, n in w)
            across += any(o // fs != (o + n - 1) // fs for o, n in w)
    assert merged > 50 and short > 50 and across > 50, (merged, short, across)   # (what the cases cover)
    assert M.patch(b"abcdefgh", b"abXdefgYZZ", 4, 2) == ([(2, 2), (6, 2)], b"XdgYZZ", 4, 2)
    assert M.patch(b"abcdefgh", b"abcXYfgh", 4, 2) == ([(2, 4)], b"cXYf", 4, 0)      # the last grain of frame 0 and the first of frame 1 are neighbours
    assert M.patch(b"abcde", b"abcdX", 4, 4) == ([(4, 1)], b"X", 1, 0)               # a grain clipped to C
    assert M.stats(b"aXXb" * 2, b"aYYb" * 2 + b"tail!", 4, 2, decoded={1}) == dict(
        frames=2, equal_compressed=1, decoded=1, tail_decoded=2, writes=1, dirty_bytes=8, passes=2, dirty_grains=4)
