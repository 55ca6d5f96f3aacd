"""CPU tests of the extract with a record predicate (include/zra_hip.h: ZraHipExtractRecordsWhere, ZraHipArchiveExtractRecordsWhere):
declared, exported and bound; every rule-1 refusal before anything touches a device; no CPU result without a GPU; the model the GPU
tests use as their yardstick (tests/extract_where_model.py) against answers pinned by hand; the inputs of the GPU tests
(tests/extract_where_shapes.py) held to the seams they are built for; the kernels' 48-byte summary and its combine() restated in
Python, associative and equal to the model in `sel` and in `bytes`; and the zra_extractw_* kernels compiled inside their bounds."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import extract_where_model as XWM
import extract_where_shapes as SH
import grep_model as GM
import msearch_model
import where_model as WM
from test_grep_where_abi import CLAUSE_CASES, _clauses, _random_clauses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipExtractRecordsWhere", "ZraHipArchiveExtractRecordsWhere"]
MAXU64 = (1 << 64) - 1
NL = 10


def test_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert "where" in inspect.signature(zra.Engine.extract).parameters and "where" in inspect.signature(zra.Archive.extract).parameters
    assert "zra_extract_where.hip" in open(os.path.join(ROOT, "zra_amd", "build.py")).read()
    # the bring-up accessor the handle test finds the arena with: without a handle it answers NULL and 0, and null outputs are a no-op
    assert "ZraHipDebugArchiveArena" in declared and "ZraHipDebugArchiveArena" in zra.HIP_ABI_SYMBOLS and callable(zra.Archive.arena_range)
    base, n = ctypes.c_void_p(5), ctypes.c_size_t(5)
    L.ZraHipDebugArchiveArena(None, ctypes.byref(base), ctypes.byref(n))
    assert (base.value, n.value) == (None, 0)
    L.ZraHipDebugArchiveArena(None, None, None)


def test_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords and *dataSize are zeroed, the record array is left alone and dData is never touched (it is not even
    memory here), whatever the clauses are: the refused lists and, for want of an engine or an archive, the accepted ones; every mode
    word, and the null combinations."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 400)
    sizes = (ctypes.c_uint32 * 64)(*([3] * 64))
    arr = (ctypes.c_uint64 * 8)()
    for cl, k, good in CLAUSE_CASES + [(None, 4, False)]:
        hc = None if cl is None else _clauses(cl)
        nc = 1 if cl is None else len(cl)
        for mode in (0, 1, 2, 3, 1 << 31):
            for arc in ((None, 0), (P(64), 100)):
                for dd in ((None, 0), (P(4096), 64), (None, 64)):
                    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
                    tag = (cl and cl[:2], nc, k, mode, arc, dd)
                    st = L.ZraHipExtractRecordsWhere(None, *arc, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, arr, 4, ctypes.byref(n), *dd, ctypes.byref(ds)).tup()
                    assert st == (1, 42) and (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64, tag
                    assert L.ZraHipExtractRecordsWhere(None, *arc, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, None, 0, None, *dd, None).tup() == (1, 42), tag
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
            st = L.ZraHipArchiveExtractRecordsWhere(None, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, arr, 4, ctypes.byref(n), P(4096), 64, ctypes.byref(ds)).tup()
            assert st == (1, 42) and (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64, (cl and cl[:2], nc, k, mode)
            assert L.ZraHipArchiveExtractRecordsWhere(None, None, None, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, None, 4, None, None, 64, None).tup() == (1, 42)
    # the clause checks are ZraHipCheckRecordClauses', which the call shares with the grep
    for cl, k, good in CLAUSE_CASES:
        assert L.ZraHipCheckRecordClauses(_clauses(cl), len(cl), k).tup() == ((0, 0) if good else (1, 42)), (cl[:3], len(cl), k)


def test_fails_loudly_without_gpu(zra):
    """no engine, no result: the new entry points themselves refuse a null engine and a null handle with zeroed words (on any machine),
    and without a GPU Engine.extract(where=...) has no engine to run on: never a CPU answer"""
    L = zra.load()
    sizes = (ctypes.c_uint32 * 2)(3, 1)
    n, ds = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.ZraHipExtractRecordsWhere(None, None, 0, b"abcd", sizes, 2, 0, NL, 0, _clauses([(1, 0, 2)]), 1, 0, MAXU64, 0, None, 0, ctypes.byref(n), None, 0,
                                       ctypes.byref(ds)).tup() == (1, 42) and (n.value, ds.value) == (0, 0)
    n.value = ds.value = 7
    assert L.ZraHipArchiveExtractRecordsWhere(None, b"abcd", sizes, 2, 0, NL, 0, _clauses([(1, 0, 2)]), 1, 0, MAXU64, 0, None, 0, ctypes.byref(n), None, 0,
                                              ctypes.byref(ds)).tup() == (1, 42) and (n.value, ds.value) == (0, 0)
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_extract_where.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).extract(64, 100, [b"abc", b"d"], 0, 0, where=[(1, 0, 2)])


# ---- the model
def test_answers_pinned_by_hand():
    d = b"A B\nA\nB C\n\nA B C\nC"
    pats = [b"A", b"B", b"C"]
    A, B, C = 1, 2, 4

    def text(clauses, inv=False, **kw):
        return XWM.extract_where(d, pats, clauses, NL, inv, **kw)[3]

    assert text([(A | B, 0, 0)]) == b"A B\nA B C\n"
    assert text([(A | B, 0, 0)], True) == b"A\nB C\n\nC\n"
    assert text([(A, 0, C)]) == b"A B\nA\n"
    assert text([(A | B, 0, 0), (0, 0, C)]) == b"A B\nA\n\nA B C\n"
    assert text([(0, A | C, B)]) == b"A\nC\n"                                   # (the record hi ends gets its delimiter)
    assert text([(B, 0, A)], lo=2, hi=13) == b"B\nB C\n" and text([(0, 0, 0)], lo=3, hi=3) == b""
    got = XWM.extract_where(d, pats, [(A, 0, C)])
    assert got[:3] == (GM.records(d), [(0, 3), (4, 1)], 9) and XWM.starts(got[1]) == [0, 4]
    # the list that is not monotone: {0, 0, C}, {A | C, 0, 0} on records whose sets are {}, {C}, {A} and {A, C}
    turn = [(0, 0, C), (A | C, 0, 0)]
    d2 = b"x\nC\nA\nC A\nA C"
    assert WM.hit_sets(GM.records(d2), msearch_model.matches_multi(d2, pats)) == [0, C, A, A | C, A | C]
    assert XWM.extract_where(d2, pats, turn)[1] == [(0, 1), (4, 1), (6, 3), (10, 3)]
    assert XWM.extract_where(d2, pats, turn)[3] == b"x\nA\nC A\nA C\n" and XWM.extract_where(d2, pats, turn, invert=True)[3] == b"C\n"
    assert XWM.prefix_selection(b"..C..A.", pats, turn) == [True, True, True, False, False, False, True, True]
    assert XWM.prefix_selection(b"..C..A.", pats, turn, True) == [False, False, False, True, True, True, False, False]


def test_packing_is_the_extract_models():
    """under the plain predicate the model is tests/extract_model.py's, byte for byte"""
    import extract_model as XM
    rng = np.random.RandomState(31)
    for case in range(100):
        data = bytes(rng.choice(list(b"abc\n"), size=int(rng.randint(0, 60))).astype(np.uint8))
        pats = [bytes(rng.choice(list(b"abc"), size=int(rng.randint(1, 4))).astype(np.uint8)) for _ in range(int(rng.randint(1, 5)))]
        lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        for inv in (False, True):
            assert XWM.extract_where(data, pats, [(0, WM.full(len(pats)), 0)], NL, inv, lo, hi) == XM.extract(data, pats, NL, inv, lo, hi)
            assert XWM.extract_where(data, pats, [(0, 0, WM.full(len(pats)))], NL, not inv, lo, hi) == XM.extract(data, pats, NL, inv, lo, hi)


# ---- the inputs of the GPU tests reach their seams (conditions on the model, not measurements)
def _both(c, where, lo=0, hi=None):
    a, b = SH.model(c, where, False, lo, hi), SH.model(c, where, True, lo, hi)
    assert sorted(a[1] + b[1]) == a[0]
    return a, b


def _turns(flags):
    return sum(1 for x, y in zip(flags, flags[1:]) if x != y)


def test_shape_frame_size_4():
    c = SH.frame_size_4()
    data, pats = c["data"], c["pats"]
    recs = GM.records(data)
    assert c["late"] in recs and c["turn"] in recs and c["long_line"] in recs and len(data) > 1000
    for k, where in enumerate(SH.TINY_WHERE):
        a, b = _both(c, where)
        assert (a[1] and b[1]) or k == 3, k
    late = data[c["late"][0]:sum(c["late"])]
    # selected by an `all` that completes 31 bytes (seven passes of one frame) behind its first term
    flags = XWM.prefix_selection(late, pats, SH.TINY_WHERE[0])
    assert flags.index(True) >= 32 and flags[-1] and c["late"] in SH.model(c, SH.TINY_WHERE[0], False)[1]
    # selected from its second byte on, and unselected by a `none` pattern 31 bytes later
    flags = XWM.prefix_selection(late, pats, SH.TINY_WHERE[1])
    assert flags[1] and flags[31] and not flags[-1] and flags.index(False, 1) >= 32 and c["late"] not in SH.model(c, SH.TINY_WHERE[1], False)[1]
    turn = data[c["turn"][0]:sum(c["turn"])]
    flags = XWM.prefix_selection(turn, pats, SH.TINY_WHERE[4])
    assert flags[0] and flags[-1] and _turns(flags) == 2 and c["turn"] in SH.model(c, SH.TINY_WHERE[4], False)[1]
    changes = [i for i in range(len(flags) - 1) if flags[i] != flags[i + 1]]
    assert changes[1] - changes[0] > 16 and changes[0] > 8                     # passes apart


@pytest.mark.parametrize("dist", [64, 2048, 8192, 16384])
def test_shape_seams(dist):
    for has_a, has_b in ((True, True), (False, True), (True, False)):
        c = SH.seam(dist, has_a, has_b)
        S, big = c["S"], c["big"]
        assert big in GM.records(c["data"]) and c["c_left"] in GM.records(c["data"]) and c["c_right"] in GM.records(c["data"])
        assert (S + 50) // 64 != (S + 50 + dist) // 64
        if dist >= 2048:
            assert (S + 50) // 2048 != (S + 50 + dist) // 2048
        if dist >= 8192:
            assert (S + 50) // 8192 != (S + 50 + dist) // 8192 and (S + 50) // (2 * SH.FS) != (S + 50 + dist) // (2 * SH.FS)
        if dist == 16384:
            assert (S + 50 + dist) // 8192 == (S + 50) // 8192 + 2              # a whole tile without a delimiter in between
            assert NL not in c["data"][((S + 50) // 8192 + 1) * 8192:((S + 50) // 8192 + 2) * 8192]
        a, b = _both(c, [(0b011, 0, 0)])
        assert a[1] and b[1] and (big in a[1]) == (has_a and has_b)
        assert (big in SH.model(c, [(0b001, 0, 0b010)], False)[1]) == (has_a and not has_b)
        no_c = SH.model(c, [(0, 0, 0b100)], False)[1]
        assert big in no_c and c["c_left"] not in no_c and c["c_right"] not in no_c


def test_shape_seam_turns():
    for has_c, has_a in ((True, True), (True, False), (False, False)):
        c = SH.seam_turns(has_c, has_a)
        S, big = c["S"], c["big"]
        a, b = _both(c, SH.NONMONO)
        assert a[1] and b[1] and (big in a[1]) == (has_a or not has_c)
        flags = XWM.prefix_selection(c["data"][S:S + big[1]], c["pats"], SH.NONMONO)
        assert _turns(flags) == has_c + has_a and flags[0]
        if has_c and has_a:
            t1, t2 = [i for i in range(len(flags) - 1) if flags[i] != flags[i + 1]]
            assert (S + t1) // 8192 == S // 8192 + 1 and (S + t2) // 8192 == S // 8192 + 2   # a tile each: the early bytes, C, A


def test_shape_one_trip():
    c = SH.one_trip()
    data, pats, half = c["data"], c["pats"], c["half"]
    hit = bytearray(len(data))
    for p, _ in msearch_model.matches_multi(data, pats):
        hit[p] = 1
    dense = [sum(hit[t:t + 64]) for t in range(0, half - 64, 64)]
    sparse = [sum(hit[t:t + 64]) for t in range(half + 64, len(data) - 64, 64)]
    assert min(dense) >= 8 and all(hit[p] or data[p] == NL for p in range(half - 64))   # the segmented scan (from 8 hitting lanes)
    assert sum(1 for n in sparse if 1 <= n < 8) > len(sparse) * 3 // 4                   # the per-pattern ballots
    assert all(3 <= n <= 10 for _, n in GM.records(data)[:-1])
    sizes = {len(SH.model(c, w, False)[1]) for w in c["wheres"]}
    assert len(c["wheres"]) == 12 and len(sizes) > 4
    assert any(SH.model(c, w, False)[1] and SH.model(c, w, True)[1] for w in c["wheres"])


def test_shape_wide():
    c = SH.wide()
    assert len(c["pats"]) == 64 and len(set(c["pats"])) == 64
    recs = GM.records(c["data"])
    starts = {o for o, _ in recs}
    (lo1, hi1), (lo2, hi2) = c["ranges"][1], c["ranges"][2]
    assert lo1 not in starts and lo2 not in starts and c["data"][hi1 - 1] != NL and c["data"][hi1] != NL   # the ranges cut records
    assert c["ranges"][4][0] == c["ranges"][4][1] and c["ranges"][5][1] - c["ranges"][5][0] == 1
    assert all((w[0][0] | w[0][1] | w[0][2]) >> 63 for w in c["wheres"])
    sizes = {len(SH.model(c, w, False, *c["ranges"][k % len(c["ranges"])])[1]) for k, w in enumerate(c["wheres"])}
    assert len(sizes) > 4
    where = [(0b11, 0, 0), (0, 0b1100, 0b10000)]                                # test_capacity's
    a, b = _both(c, where)
    assert len(a[1]) > 8 and len(b[1]) > 8


def test_shape_lanes():
    c = SH.lanes()
    U = len(c["data"])
    tiles = -(-U // SH.TILE)
    assert tiles == 1030 > SH.LANES and -(-tiles // SH.LANES) == 2 and U <= 4 << 30   # one pass at staging 0; a scan lane walks two tiles
    recs = set(GM.records(c["data"]))
    for (start, size), whole in zip(c["stretches"], (3, 4, 8)):
        assert (start, size) in recs
        first = -(-start // SH.TILE)
        assert (start + size) // SH.TILE - first >= whole and start % SH.TILE and (start + size) % SH.TILE   # whole tiles inside, bytes on either side
    g = c["stretches"][2]
    assert any(b % SH.GROUP == 0 and g[0] < b * SH.TILE and (b + SH.GROUP) * SH.TILE <= sum(g) for b in range(tiles))   # a whole group of 8 tiles
    a, b = _both(c, SH.LANES_WHERE[0])
    assert c["stretches"][0] in a[1] and c["stretches"][1] in b[1] and c["stretches"][2] in b[1] and len(a[1]) > 100 and len(b[1]) > 100
    a, b = _both(c, SH.LANES_WHERE[1])
    assert c["stretches"][0] in a[1] and c["stretches"][1] in a[1] and c["stretches"][2] in b[1]
    four = c["data"][c["stretches"][1][0]:sum(c["stretches"][1])]
    flags = XWM.prefix_selection(four, c["pats"], SH.LANES_WHERE[1])
    assert _turns(flags) == 2 and flags[0] and flags[-1]


def test_shape_delimiters():
    T = SH.TILE
    for kind, has, free in (("last", [0, 63, 2047, 8191], [64, 2048, 8192]), ("first", [64, 2048, 8192], [0, 63, 2047, 8191]), ("both", [0, 63, 64, 2047, 2048, 8191, 8192], [])):
        c = SH.delimiters(kind)
        data = c["data"]
        assert all(data[p] == NL for p in has) and all(data[p] != NL for p in free)
        assert (data[-1] == NL) == (kind != "first") and (data[0] == NL) == (kind != "first") and len(data) > 3 * T
        for where in SH.DELIM_WHERE:
            a, b = _both(c, where)
            assert a[1] and b[1]
    assert set(SH.delimiters("only")["data"]) == {NL} and NL not in SH.delimiters("none")["data"]
    assert len(GM.records(SH.delimiters("none")["data"])) == 1 and len(GM.records(SH.delimiters("only")["data"])) == 3 * T + 777


# ---- the kernels' summary (zra_extract_where.hip: XWSum, combine(), advance(), the scan's last lane), restated
def _leaf(pos, is_delim, m):
    """the summary of one position: (has, front, behind, first, last, sel, bytes)"""
    return (1, 0, 0, pos, pos + 1, 0, 0) if is_delim else (0, m, m, 0, 0, 0, 0)


def _combine(a, b, clauses, inv):
    ha, fa, ba, ia, la, sa, ya = a
    hb, fb, bb, ib, lb, sb, yb = b
    if not hb:
        return (1, fa, ba | fb, ia, la, sa, ya) if ha else (0, fa | fb, fa | fb, ia, la, sa, ya)
    if not ha:
        return (1, fa | fb, bb, ib, lb, sb, yb)
    s = int(WM.selected(clauses, ba | fb, inv))
    return (1, fa, bb, ia, lb, sa + sb + s, ya + yb + s * (ib - la + 1))


def _fold_random(rng, leaves, clauses, inv):
    if len(leaves) == 1:
        return leaves[0]
    k = int(rng.randint(1, len(leaves)))
    return _combine(_fold_random(rng, leaves[:k], clauses, inv), _fold_random(rng, leaves[k:], clauses, inv), clauses, inv)


def _finish(total, lo, hi, clauses, inv):
    """(selected, packed bytes) of the range from its summary, as the scan kernel's last lane does from the state {start = lo, set = 0,
    sel = 0, bytes = 0}: advance() over the summary, then the last pass's end"""
    has, front, behind, first, last, sel, nbytes = total
    start, H, idx, at = lo, 0, 0, 0
    if not has:
        H |= front
    else:
        s = int(WM.selected(clauses, H | front, inv))
        idx += sel + s
        at += nbytes + s * (first - start + 1)
        H, start = behind, last
    if start < hi and WM.selected(clauses, H, inv):
        idx += 1
        at += hi - start + 1
    return idx, at


def test_summary_algebra_is_associative_and_equals_the_model():
    rng = np.random.RandomState(33)
    for case in range(300):
        n = int(rng.randint(1, 70))
        lo = int(rng.randint(0, 1000))
        k = int(rng.randint(1, 7))
        is_delim = rng.rand(n) < (0.05, 0.2, 0.5)[case % 3]
        masks = [0 if is_delim[j] or rng.rand() < 0.6 else int(rng.randint(1, 1 << k)) for j in range(n)]
        clauses = _random_clauses(rng, k) if case % 5 else [(0, 0, 1), (1 | 1 << (k - 1), 0, 0)]   # (every fifth: the list that is not monotone)
        inv = bool(case & 1)
        leaves = [_leaf(lo + j, bool(is_delim[j]), masks[j]) for j in range(n)]
        left = leaves[0]
        for leaf in leaves[1:]:
            left = _combine(left, leaf, clauses, inv)
        for _ in range(4):
            assert _fold_random(rng, leaves, clauses, inv) == left, (case, leaves, clauses)
        # the model on the same stream: records from the delimiters, sets from the (p, i) pairs
        text = bytes(NL if is_delim[j] else 120 for j in range(n))
        recs = [(lo + o, s) for o, s in GM.records(text)]
        pairs = [(lo + j, i) for j in range(n) for i in range(k) if masks[j] >> i & 1]
        sel = [r for r, H in zip(recs, WM.hit_sets(recs, pairs)) if WM.selected(clauses, H, inv)]
        assert _finish(left, lo, lo + n, clauses, inv) == (len(sel), sum(s + 1 for _, s in sel)), (case, left, sel)
        has, front, behind = left[:3]
        assert has or front == behind


# ---- the kernels
# LDS: a workgroup of the count or the copy may not take more than one of a CU's two 64 KiB halves would leave to a second one (65,536);
# the scan is ONE workgroup and may take a whole CU's 160 KiB (163,840)
KERNELS = {"zra_extractw_count_kernel": 65536, "zra_extractw_count_class_kernel": 65536, "zra_extractw_scan_kernel": 163840, "zra_extractw_copy_kernel": 65536,
           "zra_extractw_copy_class_kernel": 65536}


def test_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_extractw_")) == sorted(KERNELS)
    for k, lds in KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_extract_where.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= lds, (k, r)
