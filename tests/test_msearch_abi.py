"""CPU tests of the multi-pattern search's boundary (include/zra_hip.h: ZraHipSearchArchiveMulti, ZraHipGetSearchMultiStats,
ZraHipDebugSearchMultiScanMs): declared, exported and bound, every rule-1 refusal before anything touches a device, no CPU result
without a GPU, the zra_msearch_* kernels compiled inside their budget with the zra_search_* set as it was, and the model the GPU tests
use as their yardstick (tests/msearch_model.py) agrees with a naive triple loop."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import msearch_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipSearchArchiveMulti", "ZraHipGetSearchMultiStats", "ZraHipDebugSearchMultiScanMs"]
MAXU64 = (1 << 64) - 1


def test_msearch_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_SEARCH_MAX_PATTERNS\s+64u", txt)
    assert re.search(r"#define\s+ZRA_HIP_SEARCH_MAX_PATTERN_BYTES\s+4096u", txt)
    assert re.search(r"typedef struct ZraHipPatternMatch \{ uint64_t offset; uint32_t pattern; uint32_t reserved; \}", txt)
    assert (zra.SEARCH_MAX_PATTERNS, zra.SEARCH_MAX_PATTERN_BYTES) == (64, 4096)
    assert ctypes.sizeof(zra.ZraHipPatternMatch) == 16
    assert callable(zra.Engine.search_multi) and callable(zra.Engine.search_multi_stats) and callable(zra.Engine.search_multi_scan_ms)
    assert zra.SEARCH_MULTI_STATS == ("frames", "decoded", "content_bytes", "matches", "listed", "passes", "patterns", "survivors")


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_msearch_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nMatches is zeroed, the match array and the per-pattern array are left alone. (The same cases with an engine:
    tests/test_gpu_msearch.py.)"""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 5000)
    cases = [(pats, _sizes(3, 4), 2), (pats, _sizes(3, 0), 2), (pats, _sizes(257), 1), (pats, _sizes(256), 1), (pats, _sizes(*([1] * 65)), 65),
             (pats, _sizes(*([256] * 17)), 17), (pats, _sizes(3), 0), (None, _sizes(3), 1), (pats, None, 1)]
    for hp, hs, k in cases:
        for arc in ((None, 0), (P(64), 100), (None, 100)):
            arr = (zra.ZraHipPatternMatch * 4)()
            per = (ctypes.c_uint64 * 65)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr)); ctypes.memset(per, 0xEE, ctypes.sizeof(per))
            n = ctypes.c_uint64(0x1234)
            assert L.ZraHipSearchArchiveMulti(None, *arc, hp, hs, k, 0, MAXU64, 0, arr, 4, ctypes.byref(n), per).tup() == (1, 42), (k, arc)
            assert n.value == 0 and bytes(arr) == b"\xEE" * 64 and bytes(per) == b"\xEE" * 520
            assert L.ZraHipSearchArchiveMulti(None, *arc, hp, hs, k, 0, MAXU64, 0, None, 0, None, None).tup() == (1, 42), (k, arc)
            assert L.ZraHipSearchArchiveMulti(None, *arc, hp, hs, k, 0, MAXU64, 0, None, 4, ctypes.byref(n), per).tup() == (1, 42), (k, arc)
    assert L.ZraHipDebugSearchMultiScanMs(None) == 0.0


def test_msearch_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetSearchMultiStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetSearchMultiStats(None, None)                                    # no-op


def test_msearch_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_msearch.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).search_multi(64, 100, [b"abc", b"d"])                    # no engine without a GPU: never a CPU result


def test_msearch_kernels_stay_inside_their_budget_and_leave_the_search_kernels_alone():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_msearch.hip")).read()
    kernels = [k for k in res if k.startswith("zra_msearch_")]
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_msearch_\w+)\s*\(", src))) and len(kernels) >= 2, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_msearch.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes"] <= 32768, (k, res[k])                       # four 256-lane workgroups fit a CU's 160 KiB
    ssrc = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_search.hip")).read()
    search = sorted(k for k in res if k.startswith("zra_search_"))
    assert search == sorted(set(re.findall(r"__global__.*?\b(zra_search_\w+)\s*\(", ssrc)))
    assert search == ["zra_search_carry_kernel", "zra_search_count_kernel", "zra_search_fill_kernel", "zra_search_jobs_kernel", "zra_search_scan_kernel"]


def test_model_agrees_with_a_naive_triple_loop():
    rng = np.random.RandomState(15)
    some = shared = mixed = ranged = last = 0
    for case in range(400):
        k = int(rng.randint(2, 4))
        data = bytes(rng.randint(0, k, size=int(rng.randint(0, 40))).astype(np.uint8))
        pats = [bytes(rng.randint(0, k, size=int(rng.randint(1, 7))).astype(np.uint8)) for _ in range(int(rng.randint(1, 6)))]
        if case % 2 and len(pats) < 5:
            pats.append(pats[0][:1 + case % 3])                                 # a prefix of pattern 0, or its equal: they share offsets
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        end = len(data) if hi is None else hi
        want = []
        for p in range(lo, end):
            for i, pat in enumerate(pats):
                if p + len(pat) <= end and all(data[p + j] == pat[j] for j in range(len(pat))):
                    want.append((p, i))
        got = MM.matches_multi(data, pats, lo, hi)
        assert got == want, (data, pats, lo, hi)
        surv = 0
        if end - lo >= min(len(p) for p in pats):
            for p in range(lo, end):
                surv += any(pat[0] == data[p] and ((len(pat) == 1) if p + 1 >= end else (len(pat) == 1 or pat[1] == data[p + 1])) for pat in pats)
        assert MM.survivors(data, pats, lo, hi) == surv, (data, pats, lo, hi)
        assert surv >= len({p for p, _ in want})                               # (every matching position passed the filter)
        some += bool(want); ranged += bool(want) and hi is not None
        shared += any(a[0] == b[0] for a, b in zip(want, want[1:]))
        mixed += len({len(pats[i]) for _, i in want}) > 1
        last += any(p == end - 1 for p, _ in want)
    assert some > 100 and shared > 50 and mixed > 50 and ranged > 40 and last > 20, (some, shared, mixed, ranged, last)   # (what the cases cover)
    assert MM.matches_multi(b"\0" * 5, [b"\0", b"\0\0", b"\0"]) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1),
                                                                    (3, 2), (4, 0), (4, 2)]
    assert MM.survivors(b"abab", [b"ab", b"b"]) == 4 and MM.survivors(b"abab", [b"ab"]) == 2 and MM.survivors(b"aba", [b"ab"], 0, 1) == 0
    assert MM.survivors(b"abab", [b"ab"], 2, 3) == 0 and MM.survivors(b"abab", [b"ab", b"a"], 2, 3) == 1
