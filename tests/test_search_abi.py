"""CPU tests of the search call's boundary (include/zra_hip.h: ZraHipSearchArchive, ZraHipGetSearchStats, ZraHipDebugSearchScanMs):
declared and exported, the Python binding exists, NULL arguments and bad pattern sizes are refused before anything touches a device, no
CPU result without a GPU, the search kernels compiled without scratch, and the model the GPU tests use as their yardstick
(tests/search_model.py) agrees with a naive double loop."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import search_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH_CALLS = ["ZraHipSearchArchive", "ZraHipGetSearchStats", "ZraHipDebugSearchScanMs"]
MAXU64 = (1 << 64) - 1


def test_search_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in SEARCH_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_SEARCH_MAX_PATTERN\s+256u", txt)
    assert zra.SEARCH_MAX_PATTERN == 256


def test_search_binding_exists(zra):
    assert callable(zra.Engine.search) and callable(zra.Engine.search_stats)
    assert zra.SEARCH_STATS == ("frames", "decoded", "content_bytes", "matches", "listed", "passes")


def test_search_refuses_null_arguments_and_bad_pattern_sizes(zra):
    """{ZStdError, 42}; *nMatches is zeroed and the match array left alone. Without an engine every combination of the other arguments
    is refused alike (the remaining cases need an engine: tests/test_gpu_search.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    pat = ctypes.create_string_buffer(b"\x07" * 300)
    for pattern, m in ((pat, 8), (pat, 0), (pat, 257), (pat, 256), (None, 8), (None, 0)):
        for args in ((None, 0), (P(64), 100), (None, 100)):
            arr = (ctypes.c_uint64 * 4)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n = ctypes.c_uint64(0x1234)
            assert L.ZraHipSearchArchive(None, *args, pattern, m, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), (m, args)
            assert n.value == 0 and bytes(arr) == b"\xEE" * 32
            assert L.ZraHipSearchArchive(None, *args, pattern, m, 0, MAXU64, 0, None, 0, None).tup() == (1, 42), (m, args)
            assert L.ZraHipSearchArchive(None, *args, pattern, m, 0, MAXU64, 0, None, 4, ctypes.byref(n)).tup() == (1, 42), (m, args)
    assert L.ZraHipDebugSearchScanMs(None) == 0.0


def test_search_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetSearchStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetSearchStats(None, None)                                         # no-op


def test_search_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_search.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).search(64, 100, b"abc")                                  # no engine without a GPU: never a CPU result


def test_search_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    kernels = [k for k in res if k.startswith("zra_search_")]
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_search.hip")).read()
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_search_\w+)\s*\(", src))) and len(kernels) >= 3, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_search.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])


def test_model_agrees_with_a_naive_double_loop():
    rng = np.random.RandomState(5)
    some = overlaps = ranged = 0
    for case in range(400):
        k = int(rng.randint(2, 4))
        data = bytes(rng.randint(0, k, size=int(rng.randint(0, 40))).astype(np.uint8))
        m = int(rng.randint(1, 7))
        pat = bytes(rng.randint(0, k, size=m).astype(np.uint8))
        if case % 2:
            pat = (pat[:1 + case % 4 // 2] * m)[:m]                             # period 1 or 2: occurrences that overlap
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        end = len(data) if hi is None else hi
        want = [p for p in range(lo, end - m + 1) if all(data[p + i] == pat[i] for i in range(m))]
        got = M.matches(data, pat, lo, hi)
        assert got == want, (data, pat, lo, hi)
        some += bool(want); ranged += bool(want) and hi is not None
        overlaps += any(b - a < m for a, b in zip(want, want[1:]))
    assert some > 100 and overlaps > 20 and ranged > 40, (some, overlaps, ranged)   # (what the cases cover)
    assert M.matches(b"\0" * 1000, b"\0\0\0") == list(range(998))
    assert M.matches(b"abcabc", b"abc", 1) == [3] and M.matches(b"abcabc", b"abc", 0, 5) == [0] and M.matches(b"abc", b"abcd") == []
