"""CPU tests of the grep with a record predicate (include/zra_hip.h: ZraHipGrepArchiveWhere, ZraHipArchiveGrepWhere,
ZraHipCheckRecordClauses): declared, exported and bound; every rule-1 refusal of the clauses before anything touches a device; no CPU
result without a GPU; the model the GPU tests use as their yardstick (tests/where_model.py) against a naive per-record loop, against
tests/grep_model.py for the two plain predicates and against answers pinned by hand; the kernels' 32-byte summary and its combine()
restated in Python, associative and equal to the model; the host header's checker program under the host sanitizers; and the
zra_grepw_* kernels compiled inside their bounds."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import grep_model as GM
import where_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipGrepArchiveWhere", "ZraHipArchiveGrepWhere", "ZraHipCheckRecordClauses"]
CHECKER = os.path.join(ROOT, "tools", "model", "where_check.cpp")
MAXU64 = (1 << 64) - 1
NL = 10


def test_where_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_WHERE_MAX_CLAUSES\s+8\b", txt)
    assert re.search(r"typedef struct ZraHipRecordClause \{ uint64_t all, any, none; \} ZraHipRecordClause;", txt)
    assert zra.WHERE_MAX_CLAUSES == 8 and callable(zra.check_record_clauses)
    import inspect
    assert "where" in inspect.signature(zra.Engine.grep).parameters and "where" in inspect.signature(zra.Archive.grep).parameters


def _clauses(cl):
    return (ctypes.c_uint64 * max(3 * len(cl), 3))(*(w for c in cl for w in c))


# (clauses, nPatterns, accepted)
CLAUSE_CASES = [([(0, 0, 0)] * 8, 4, True), ([(0, 0, 0)] * 9, 4, False), ([], 4, False), ([(1, 2, 4)] * 8, 3, True), ([(1, 2, 4)] * 200, 3, False),
                ([(1 << 4, 0, 0)], 5, True), ([(1 << 5, 0, 0)], 5, False), ([(0, 1 << 4, 0)], 5, True), ([(0, 1 << 5, 0)], 5, False),
                ([(0, 0, 1 << 4)], 5, True), ([(0, 0, 1 << 5)], 5, False), ([(1, 0, 0), (0, 0, 1 << 5)], 5, False), ([(1 << 63, 0, 0)], 64, True),
                ([(1 << 63, 0, 0)], 63, False), ([(0, 1 << 62, 0)], 63, True), ([(MAXU64, 0, 0), (0, MAXU64, 0), (0, 0, MAXU64)], 64, True),
                ([(3, 0, 2)], 4, False), ([(0, 3, 1)], 4, False), ([(1, 2, 4), (0, 8, 8)], 4, False), ([(3, 3, 4)], 4, True),
                ([(0, 0, 0)], 0, False), ([(0, 0, 0)], 65, False), ([(0, 0, 0)], 1, True), ([(0, 1, 0)], 1, True), ([(0, 2, 0)], 1, False)]


def test_check_record_clauses(zra):
    L = zra.load()
    for cl, k, good in CLAUSE_CASES:
        assert L.ZraHipCheckRecordClauses(_clauses(cl), len(cl), k).tup() == ((0, 0) if good else (1, 42)), (cl[:3], len(cl), k)
        if good:
            zra.check_record_clauses(cl, k)
        else:
            with pytest.raises(zra.ZraError):
                zra.check_record_clauses(cl, k)
    assert L.ZraHipCheckRecordClauses(None, 1, 4).tup() == (1, 42)
    assert L.ZraHipCheckRecordClauses(None, 0, 4).tup() == (1, 42)
    # the Python terms: an int mask or an iterable of indices
    zra.check_record_clauses([([0, 1], (), {2}), (0b11, 0, 0b100)], 3)
    with pytest.raises(zra.ZraError):
        zra.check_record_clauses([([0, 3], (), ())], 3)
    with pytest.raises(ValueError):
        zra.check_record_clauses([([64], (), ())], 64)
    with pytest.raises(ValueError):
        zra.check_record_clauses([(1, 2)], 3)


def test_where_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords is zeroed and the record array is left alone, whatever the clauses are: the refused lists and, for
    want of an engine or an archive, the accepted ones."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 400)
    sizes = (ctypes.c_uint32 * 64)(*([3] * 64))
    for cl, k, good in CLAUSE_CASES + [(None, 4, False)]:
        hc = None if cl is None else _clauses(cl)
        nc = 1 if cl is None else len(cl)
        for mode in (0, 1):
            for arc in ((None, 0), (P(64), 100)):
                arr = (ctypes.c_uint64 * 8)()
                ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                n = ctypes.c_uint64(0x1234)
                tag = (cl and cl[:2], nc, k, mode, arc)
                assert L.ZraHipGrepArchiveWhere(None, *arc, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), tag
                assert n.value == 0 and bytes(arr) == b"\xEE" * 64, tag
                assert L.ZraHipGrepArchiveWhere(None, *arc, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, None, 0, None).tup() == (1, 42), tag
            n = ctypes.c_uint64(0x1234)
            assert L.ZraHipArchiveGrepWhere(None, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), tag
            assert n.value == 0 and bytes(arr) == b"\xEE" * 64, tag
            assert L.ZraHipArchiveGrepWhere(None, pats, sizes, k, 0, NL, mode, hc, nc, 0, MAXU64, 0, None, 4, None).tup() == (1, 42), tag


def test_where_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_grep_where.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep(64, 100, [b"abc", b"d"], where=[(1, 0, 2)])         # no engine without a GPU: never a CPU result


# ---- the model
def _naive(data, pats, clauses, delim, invert, lo, end):
    """the selected records of [lo, end), record by record: pattern i is in the set iff it occurs in the record's bytes. (An occurrence
    that ends behind `end` lies in no record: the last record is clipped at `end`, as the range is.)"""
    out = []
    for off, size in GM.records(data, delim, lo, end):
        rec = data[off:off + size]
        H = WM.mask(i for i, p in enumerate(pats) if p in rec)
        if any((H & a) == a and (y == 0 or H & y) and not H & n for a, y, n in clauses) != invert:
            out.append((off, size))
    return out


def _random_clauses(rng, k):
    out = []
    for _ in range(int(rng.randint(1, 9))):
        t = rng.randint(0, 4, size=k)
        out.append((WM.mask(i for i in range(k) if t[i] == 0), WM.mask(i for i in range(k) if t[i] == 1), WM.mask(i for i in range(k) if t[i] == 2)))
    return out


def test_model_agrees_with_a_naive_per_record_loop():
    rng = np.random.RandomState(27)
    empty = cut = inverted = both = 0
    for case in range(200):
        data = bytes(rng.choice(list(b"abcd\n"), p=[0.2, 0.2, 0.2, 0.15, 0.25], size=int(rng.randint(0, 80))).astype(np.uint8))
        pats = [bytes(rng.choice(list(b"abcd"), size=int(rng.randint(1, 4))).astype(np.uint8)) for _ in range(int(rng.randint(1, 7)))]
        clauses = _random_clauses(rng, len(pats))
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        end = len(data) if hi is None else hi
        invert = bool(case & 1)
        recs, sel, nm = WM.grep_where(data, pats, clauses, NL, invert, lo, hi)
        want = _naive(data, pats, clauses, NL, invert, lo, end)
        assert sel == want, (data, pats, clauses, invert, lo, hi, sel, want)
        assert recs == GM.records(data, NL, lo, hi) and nm == GM.grep(data, pats, NL, False, lo, hi)[2]
        other = WM.grep_where(data, pats, clauses, NL, not invert, lo, hi)[1]
        assert sorted(sel + other) == recs                                     # the two modes split the records
        empty += any(n == 0 for _, n in recs)
        cut += bool(recs) and lo > 0 and data[lo - 1] != NL
        inverted += invert and bool(sel)
        both += bool(sel) and bool(other)
    assert min(empty, cut, inverted, both) > 40, (empty, cut, inverted, both)


def test_the_plain_predicates_are_the_grep_model():
    rng = np.random.RandomState(28)
    for case in range(200):
        data = bytes(rng.choice(list(b"abc\n"), size=int(rng.randint(0, 60))).astype(np.uint8))
        pats = [bytes(rng.choice(list(b"abc"), size=int(rng.randint(1, 4))).astype(np.uint8)) for _ in range(int(rng.randint(1, 5)))]
        lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        full = WM.full(len(pats))
        for inv in (False, True):
            want = GM.grep(data, pats, NL, inv, lo, hi)
            assert WM.grep_where(data, pats, [(0, full, 0)], NL, inv, lo, hi) == want
            assert WM.grep_where(data, pats, [(0, 0, full)], NL, not inv, lo, hi) == want
        assert WM.grep_where(data, pats, [(0, 0, 0)], NL, False, lo, hi)[1] == GM.records(data, NL, lo, hi)


def test_answers_pinned_by_hand():
    d = b"A B\nA\nB C\n\nA B C\nC"
    pats = [b"A", b"B", b"C"]
    recs = [(0, 3), (4, 1), (6, 3), (10, 0), (11, 5), (17, 1)]
    assert GM.records(d) == recs
    A, B, C = 1, 2, 4

    def sel(clauses, inv=False, **kw):
        return WM.grep_where(d, pats, clauses, NL, inv, **kw)[1]

    assert sel([(A | B, 0, 0)]) == [(0, 3), (11, 5)]                           # A and B
    assert sel([(A | B, 0, 0)], True) == [(4, 1), (6, 3), (10, 0), (17, 1)]
    assert sel([(A, 0, C)]) == [(0, 3), (4, 1)]                                # A and not C
    assert sel([(A, 0, C)], True) == [(6, 3), (10, 0), (11, 5), (17, 1)]
    assert sel([(A | B, 0, 0), (0, 0, C)]) == [(0, 3), (4, 1), (10, 0), (11, 5)]   # (A and B) or (not C)
    assert sel([(A | B, 0, 0), (0, 0, C)], True) == [(6, 3), (17, 1)]
    assert sel([(0, A | C, B)]) == [(4, 1), (17, 1)]                           # (A or C) and not B
    assert sel([(A | B, 0, 0)], lo=2, hi=13) == [] and sel([(B, 0, A)], lo=2, hi=13) == [(2, 1), (6, 3)]   # the range clips records and matches
    assert WM.hit_sets(recs, [(0, 0), (2, 1), (4, 0), (6, 1), (8, 2), (11, 0), (13, 1), (15, 2), (17, 2)]) == [3, 1, 6, 0, 7, 4]


# ---- the kernels' summary (zra_grep_where.hip: SumW, combine(), the scan's walk), restated
def _leaf(pos, is_delim, m):
    """the summary of one position: (has a delimiter, front, behind, the position behind the last delimiter, sel)"""
    return (1, 0, 0, pos + 1, 0) if is_delim else (0, m, m, 0, 0)


def _combine(a, b, clauses, inv):
    ha, fa, ba, la, sa = a
    hb, fb, bb, lb, sb = b
    if not hb:
        return (1, fa, ba | fb, la, sa) if ha else (0, fa | fb, fa | fb, la, sa)
    if not ha:
        return (1, fa | fb, bb, lb, sb)
    return (1, fa, bb, lb, sa + sb + int(WM.selected(clauses, ba | fb, inv)))


def _fold_random(rng, leaves, clauses, inv):
    if len(leaves) == 1:
        return leaves[0]
    k = int(rng.randint(1, len(leaves)))
    return _combine(_fold_random(rng, leaves[:k], clauses, inv), _fold_random(rng, leaves[k:], clauses, inv), clauses, inv)


def _finish(total, lo, hi, clauses, inv):
    """the selected count of the range from its summary, as the scan kernel's last lane does from the state {start = lo, set = 0}"""
    has, front, behind, last, sel = total
    if not has:
        return int(lo < hi and WM.selected(clauses, front, inv))
    count = sel + int(WM.selected(clauses, front, inv))
    return count + int(last < hi and WM.selected(clauses, behind, inv))


def test_summary_algebra_is_associative_and_equals_the_model():
    rng = np.random.RandomState(29)
    for case in range(300):
        n = int(rng.randint(1, 70))
        lo = int(rng.randint(0, 1000))
        k = int(rng.randint(1, 7))
        is_delim = rng.rand(n) < (0.05, 0.2, 0.5)[case % 3]
        masks = [0 if is_delim[j] or rng.rand() < 0.6 else int(rng.randint(1, 1 << k)) for j in range(n)]
        clauses = _random_clauses(rng, k)
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
        want = sum(1 for H in WM.hit_sets(recs, pairs) if WM.selected(clauses, H, inv))
        assert _finish(left, lo, lo + n, clauses, inv) == want, (case, left, want)
        has, front, behind, last, _ = left
        assert has or front == behind


# ---- the host header under the sanitizers
def test_where_check_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "where_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "zra_amd", "csrc"),
                    CHECKER, "-o", exe], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert re.fullmatch(r"where_check: \d{5,} cases ok", r.stdout.strip().split("\n")[-1]), r.stdout[-500:]
    src = open(CHECKER).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["zra_where.h"]
    hdr = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_where.h")).read()
    assert not re.search(r'#include\s+"', hdr) and "hip" not in " ".join(re.findall(r"#include\s+<([^>]+)>", hdr))


# ---- the kernels
WHERE_KERNELS = {"zra_grepw_count_kernel": 32768, "zra_grepw_count_class_kernel": 32768, "zra_grepw_scan_kernel": 65536, "zra_grepw_fill_kernel": 32768,
                 "zra_grepw_fill_class_kernel": 32768}


def test_where_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_grepw_")) == sorted(WHERE_KERNELS)
    for k, lds in WHERE_KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_grep_where.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= lds, (k, r)
