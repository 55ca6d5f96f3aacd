"""CPU tests of the compare call's boundary (include/zra_hip.h: ZraHipCompareArchives, ZraHipGetCompareStats, ZraHipGetCompareSizes,
ZraHipDebugCompareMs): declared and exported, the Python binding exists, without an engine every call is refused before anything
touches a device, no CPU result without a GPU, the compare kernels compiled without scratch, and the model the GPU tests use as their
yardstick (tests/compare_model.py) agrees with a naive loop."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import compare_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARE_CALLS = ["ZraHipCompareArchives", "ZraHipGetCompareStats", "ZraHipDebugCompareMs", "ZraHipGetCompareSizes"]
MAXU64 = (1 << 64) - 1


def test_compare_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in COMPARE_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_COMPARE_DECODE_ALL\s+1u", txt)
    assert re.search(r"typedef struct ZraHipContentRange \{ uint64_t offset; uint64_t size; \} ZraHipContentRange;", txt)
    assert zra.COMPARE_DECODE_ALL == 1


def test_compare_binding_exists(zra):
    for name in ("compare", "compare_stats", "compare_sizes", "compare_ms"):
        assert callable(getattr(zra.Engine, name)), name
    assert zra.COMPARE_STATS == ("frames", "equal_compressed", "decoded", "content_bytes", "ranges", "listed", "passes")


def test_compare_without_an_engine_is_refused(zra):
    """{ZStdError, 42} for every combination of the other arguments; *nRanges and *differingBytes are zeroed and the range array is
    left alone (the remaining refusals need an engine: tests/test_gpu_compare.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for a in ((None, 0), (P(64), 100), (None, 100)):
        for b in ((None, 0), (P(64), 100), (None, 100)):
            for mode in (0, 1, 2, 0xFFFFFFFF):
                for off, size in ((0, MAXU64), (5, 0), (MAXU64, MAXU64 - 1)):
                    arr = (ctypes.c_uint64 * 8)()
                    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                    n, nb = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
                    assert L.ZraHipCompareArchives(None, *a, *b, mode, off, size, 0, arr, 4, ctypes.byref(n), ctypes.byref(nb)).tup() == (1, 42)
                    assert (n.value, nb.value) == (0, 0) and bytes(arr) == b"\xEE" * 64
                    assert L.ZraHipCompareArchives(None, *a, *b, mode, off, size, 0, None, 0, None, None).tup() == (1, 42)
                    assert L.ZraHipCompareArchives(None, *a, *b, mode, off, size, 1, None, 4, ctypes.byref(n), None).tup() == (1, 42)
    assert L.ZraHipDebugCompareMs(None) == 0.0


def test_compare_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetCompareStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetCompareStats(None, None)                                        # no-op
    two = (ctypes.c_uint64 * 2)(7, 7)
    L.ZraHipGetCompareSizes(None, two)
    assert list(two) == [0, 0]
    L.ZraHipGetCompareSizes(None, None)


def test_compare_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_compare.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).compare(64, 100, 64, 100)                                # no engine without a GPU: never a CPU result


def test_compare_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    kernels = [k for k in res if k.startswith("zra_cmp_")]
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_compare.hip")).read()
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_cmp_\w+)\s*\(", src))) and len(kernels) >= 4, kernels
    assert "zra_cmp_spans_kernel" in kernels
    for k in kernels:
        assert res[k]["source"] == "zra_compare.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])


def test_model_agrees_with_a_naive_loop():
    rng = np.random.RandomState(14)
    some = at_lo = at_hi = adjacent = ranged = 0
    for case in range(400):
        n = int(rng.randint(0, 40))
        a = rng.randint(0, 2, size=n).astype(np.uint8)
        b = a.copy() if case % 5 == 0 else rng.randint(0, 2, size=n + int(rng.randint(0, 3))).astype(np.uint8)
        if case % 2:
            a = np.concatenate((a, a[:3]))                                     # either side may be the longer one
        a, b = bytes(a), bytes(b)
        c = min(len(a), len(b))
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, c + 1)); hi = int(rng.randint(lo, c + 1))
        end = c if hi is None else hi
        want, s = [], None
        for p in range(lo, end):
            if a[p] != b[p] and s is None:
                s = p
            if a[p] == b[p] and s is not None:
                want.append((s, p - s)); s = None
        if s is not None:
            want.append((s, end - s))
        got = M.ranges(a, b, lo, hi)
        assert got == want, (a, b, lo, hi)
        some += bool(want); ranged += bool(want) and hi is not None
        at_lo += bool(want) and want[0][0] == lo
        at_hi += bool(want) and sum(want[-1]) == end
        adjacent += any(y[0] - sum(x) == 1 for x, y in zip(want, want[1:]))
    assert some > 100 and at_lo > 30 and at_hi > 30 and adjacent > 50 and ranged > 40, (some, at_lo, at_hi, adjacent, ranged)   # (what the cases cover)
    assert M.ranges(b"abcdef", b"abXdeY") == [(2, 1), (5, 1)] and M.ranges(b"abc", b"abcd") == [] and M.ranges(b"", b"") == []
    assert M.ranges(b"aXXb", b"aYYb", 2) == [(2, 1)] and M.ranges(b"aXXb", b"aYYb", 0, 2) == [(1, 1)] and M.ranges(b"XX", b"YY", 1, 1) == []
    assert M.stats(b"aXXb" * 2, b"aYYb" * 2, 4, decoded={1}) == dict(frames=2, equal_compressed=1, decoded=1, content_bytes=4, ranges=2, listed=2, passes=1)
