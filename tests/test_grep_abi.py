"""CPU tests of the grep's boundary (include/zra_hip.h: ZraHipGrepArchive, ZraHipGetGrepStats, ZraHipDebugGrepScanMs): declared,
exported and bound, every rule-1 refusal before anything touches a device, no CPU result without a GPU, the zra_grep_* kernels compiled
inside their budget, and the model the GPU tests use as their yardstick (tests/grep_model.py) agrees with a naive per-position loop,
with bytes.split and with answers pinned by hand."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import grep_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipGrepArchive", "ZraHipGetGrepStats", "ZraHipDebugGrepScanMs"]
MAXU64 = (1 << 64) - 1


def test_grep_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_GREP_INVERT\s+1u", txt)
    assert zra.GREP_INVERT == 1
    assert zra.GREP_STATS == ("frames", "decoded", "content_bytes", "records", "selected", "listed", "passes", "matches")
    assert callable(zra.Engine.grep) and callable(zra.Engine.grep_stats) and callable(zra.Engine.grep_scan_ms)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_grep_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords is zeroed and the record array is left alone. (The same cases with an engine: tests/test_gpu_grep.py.)"""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 5000)
    nl = ctypes.create_string_buffer(b"ab\ncd")
    # (patterns, sizes, count, delimiter, mode)
    cases = [(pats, _sizes(3), 1, 10, 2), (pats, _sizes(3), 1, 10, 3), (pats, _sizes(3), 1, 10, 0x80000000),    # mode bits
             (nl, _sizes(5), 1, 10, 0), (nl, _sizes(2, 3), 2, 10, 1), (pats, _sizes(3), 1, 7, 0),                # a pattern holds the delimiter
             (pats, _sizes(3, 4), 2, 7, 0),
             (pats, _sizes(3, 0), 2, 10, 0), (pats, _sizes(257), 1, 10, 0), (pats, _sizes(*([1] * 65)), 65, 10, 0),   # the multi search's
             (pats, _sizes(*([256] * 17)), 17, 10, 0), (pats, _sizes(3), 0, 10, 0), (None, _sizes(3), 1, 10, 0), (pats, None, 1, 10, 0)]
    for hp, hs, k, delim, mode in cases:
        for arc in ((None, 0), (P(64), 100), (None, 100)):
            arr = (ctypes.c_uint64 * 8)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n = ctypes.c_uint64(0x1234)
            assert L.ZraHipGrepArchive(None, *arc, hp, hs, k, delim, mode, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), (k, delim, mode, arc)
            assert n.value == 0 and bytes(arr) == b"\xEE" * 64
            assert L.ZraHipGrepArchive(None, *arc, hp, hs, k, delim, mode, 0, MAXU64, 0, None, 0, None).tup() == (1, 42), (k, delim, mode, arc)
            assert L.ZraHipGrepArchive(None, *arc, hp, hs, k, delim, mode, 0, MAXU64, 0, None, 4, ctypes.byref(n)).tup() == (1, 42), (k, delim, mode, arc)
    assert L.ZraHipDebugGrepScanMs(None) == 0.0


def test_grep_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetGrepStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetGrepStats(None, None)                                           # no-op


def test_grep_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_grep.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep(64, 100, [b"abc", b"d"])                            # no engine without a GPU: never a CPU result


def test_grep_kernels_stay_inside_their_budget():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_grep.hip")).read()
    kernels = [k for k in res if k.startswith("zra_grep_")]
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_grep_\w+)\s*\(", src))) and len(kernels) >= 3, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_grep.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes"] <= 32768, (k, res[k])


def _naive(data, pats, delim, invert, lo, end):
    """(records, selected, matches) of [lo, end), one position at a time"""
    recs, sel, matches = [], [], 0
    start, hit = lo, False
    for p in range(lo, end):
        if data[p] == delim:
            recs.append((start, p - start))
            if hit != invert:
                sel.append((start, p - start))
            start, hit = p + 1, False
            continue
        for pat in pats:
            if p + len(pat) <= end and all(data[p + j] == pat[j] for j in range(len(pat))):
                hit = True
                matches += 1
    if start < end:
        recs.append((start, end - start))
        if hit != invert:
            sel.append((start, end - start))
    return recs, sel, matches


def test_model_agrees_with_a_naive_per_position_loop():
    rng = np.random.RandomState(18)
    empty = first_cut = last_cut = ends_delim = twice = inverted = 0
    for case in range(600):
        k = int(rng.randint(3, 5))
        delim = k - 1                                                          # one symbol of the alphabet is the delimiter
        data = bytes(rng.randint(0, k, size=int(rng.randint(0, 41))).astype(np.uint8))
        pats = [bytes(rng.randint(0, k - 1, size=int(rng.randint(1, 4))).astype(np.uint8)) for _ in range(int(rng.randint(1, 4)))]
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        end = len(data) if hi is None else hi
        invert = bool(case & 1)
        want = _naive(data, pats, delim, invert, lo, end)
        got = GM.grep(data, pats, delim, invert, lo, hi)
        assert got == want, (data, pats, delim, invert, lo, hi, got, want)
        recs, sel, matches = want
        assert sel == [r for r in recs if r in set(sel)] and len(set(recs)) == len(recs)
        assert all(delim not in data[o:o + n] for o, n in recs)
        other = _naive(data, pats, delim, not invert, lo, end)
        assert sorted(sel + other[1]) == recs and other[2] == matches         # the two modes split the records; matches does not depend on the mode
        empty += any(n == 0 for _, n in recs)
        first_cut += bool(recs) and lo > 0 and data[lo - 1] != delim
        last_cut += bool(recs) and end < len(data) and data[end] != delim and data[end - 1] != delim
        ends_delim += end > lo and data[end - 1] == delim
        inverted += invert and bool(sel)
        for o, n in recs:
            twice += sum(1 for p in range(o, o + n) for pat in pats if p + len(pat) <= end and data[p:p + len(pat)] == pat) >= 2
    assert min(empty, first_cut, last_cut, ends_delim, inverted) > 60 and twice > 200, (empty, first_cut, last_cut, ends_delim, twice, inverted)


def test_model_agrees_with_bytes_split():
    rng = np.random.RandomState(19)
    for case in range(100):
        data = bytes(rng.choice([10, 10, 97, 98, 99], size=int(rng.randint(0, 60))).astype(np.uint8))
        parts = data.split(b"\n")
        if parts[-1] == b"":
            parts.pop()                                                        # (no trailing empty record; b"" has none at all)
        recs = GM.records(data)
        assert [data[o:o + n] for o, n in recs] == parts, data
        assert all(o == 0 or data[o - 1] == 10 for o, _ in recs) and all(o + n == len(data) or data[o + n] == 10 for o, n in recs)
        _, sel, _ = GM.grep(data, [b"ab", b"c"])
        assert [data[o:o + n] for o, n in sel] == [x for x in parts if b"ab" in x or b"c" in x], data


def test_answers_pinned_by_hand():
    d = b"ab\ncd\n\nab"
    assert GM.records(d) == [(0, 2), (3, 2), (6, 0), (7, 2)]
    assert GM.grep(d, [b"ab"])[1] == [(0, 2), (7, 2)]
    assert GM.grep(d, [b"ab"], invert=True)[1] == [(3, 2), (6, 0)]
    assert GM.grep(d, [b"ab"], lo=0, hi=8)[1] == [(0, 2)]
    assert GM.grep(d, [b"ab"], invert=True, lo=0, hi=8)[1] == [(3, 2), (6, 0), (7, 1)]
    assert GM.grep(d, [b"ab"], lo=1, hi=9)[1] == [(7, 2)]
    assert GM.records(b"ab\n") == [(0, 2)]
    assert GM.records(b"") == [] and GM.records(b"\n") == [(0, 0)] and GM.records(b"x", lo=1) == []
