"""GPU tests of ZraHipGrepArchiveRegexContext (include/zra_hip.h): the records the regex grep selects with `before` records in front of
and `after` records behind each of them. The yardstick everywhere is the plaintext the test generated itself, cut, matched and given
its context on the CPU (tests/regex_context_model.py, held against the system's grep in tests/test_regex_context_abi.py). Every case
compares the status, the three counts, the list with its selected bits and all eight stats; a run without context is also compared
with Engine.grep_regex. The inputs come from tests/regex_context_shapes.py, where a CPU test asserts that each reaches its seam."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import regex_context_model as RCM
import regex_context_shapes as SH
from test_gpu_grep import _stats
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
SEL = 1 << 63
ZERO = dict(frames=0, decoded=0, content_bytes=0, records=0, selected=0, listed=0, passes=0, matches=0)
FS = SH.FS


def _raw(eng, zra, d, size, pats, cap, after=0, before=0, delim=NL, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, null=False):
    """(status, (*nRecords, *nSelected, *nGroups), the bytes of a record array two entries longer than the capacity, 0xEE-filled)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ns, ng = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    eng._order()
    st = zra.load().ZraHipGrepArchiveRegexContext(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), syntax, delim, mode, before, after, offset, length, staging,
                                                  None if null else arr, cap, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(ng)).tup()
    return st, (n.value, ns.value, ng.value), bytes(arr)


def _call(eng, zra, d, size, pats, **kw):
    try:
        return ((0, 0),) + eng.grep_regex_context(d.data_ptr(), size, pats, **kw)
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, 0, 0, []


def _archive(eng, zra, c, level=3):
    arc = _compress(eng, zra, c["data"], level, c["fs"], True)
    return arc, _dev(arc)


def _check(eng, zra, d, size, c, pairs=None, lo=None, hi="case", stagings=None, modes=None):
    """one call per staging, pair and mode of the case against the model. Returns {(after, before, invert): (listed, |S|, groups)}."""
    data, fs, pats, delim = c["data"], c["fs"], c["pats"], c["delim"]
    lo = c["lo"] if lo is None else lo
    hi = c["hi"] if hi == "case" else hi
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    out = {}
    for staging in c["stagings"] if stagings is None else stagings:
        for inv in c["modes"] if modes is None else modes:
            for after, before in c["pairs"] if pairs is None else pairs:
                want, nsel, groups, recs, matches = SH.model(c, after, before, inv, lo, hi)
                tag = (c["name"], after, before, lo, hi, staging, inv)
                kw = dict(delimiter=delim, invert=inv, fold_case=c["fold"], offset=lo, length=length, staging_bytes=staging)
                got = _call(eng, zra, d, size, pats, before=before, after=after, **kw)
                assert got[:4] == ((0, 0), len(want), nsel, groups), (tag, got[:4], (len(want), nsel, groups))
                assert got[4] == want, (tag, sorted(set(got[4]) ^ set(want))[:10], got[4][:6], want[:6])
                s = eng.grep_stats()
                if end == lo:
                    assert s == dict(ZERO, frames=-(-U // fs)) and not want, (tag, s)    # nothing decoded
                else:
                    assert s == _stats(U, fs, lo, end, staging, len(recs), len(want), len(want), matches), (tag, s)
                if after == 0 and before == 0:
                    plain = eng.grep_regex(d.data_ptr(), size, pats, **kw)
                    assert (plain[0], plain[1]) == (len(want), [(o, n) for o, n, _ in want]) and all(b for _, _, b in want) and nsel == len(want), tag
                out[(after, before, inv)] = (want, nsel, groups)
    return out


# ---- 1
@pytest.mark.parametrize("staging", [1, 0])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging):
    c, long_line = SH.frame_size_4()
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c, stagings=(staging,))
    want, nsel, groups = res[(2, 3, False)]
    assert nsel > 5 and groups > 3 and any(not b for _, _, b in want)
    assert gpu_engine.grep_stats()["passes"] == (-(-len(c["data"]) // 4) if staging else 1)


# ---- 2
def test_pending_records_one_record_per_pass(zra, gpu_engine):
    c = SH.one_record_per_pass()
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c)
    assert res[(0, 3, False)][1:] == (6, 4)
    assert gpu_engine.grep_stats()["passes"] == -(-len(c["data"]) // 48)
    _check(gpu_engine, zra, d, len(arc), c, pairs=[(1, 3)], lo=16 * 3 + 5, hi=len(c["data"]) - 16 * 4 - 7, stagings=(1,))


# ---- 3
def test_first_record_of_a_tile_resolved_from_in_front(zra, gpu_engine):
    c = SH.first_record_of_a_tile()
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c)
    want, nsel, groups = res[(2, 3, False)]
    assert {o + n for o, n, b in want if b} == {t for t, _ in SH.SEAM_TARGETS} and len(want) > 5 * nsel


# ---- 4
def test_tiles_and_passes_without_a_delimiter(zra, gpu_engine):
    c, longs = SH.delimiter_free_tiles()
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c)
    assert sorted(n for _, n, _ in res[(2, 2, False)][0])[-3:] == [9000, 20480, 20480]
    _check(gpu_engine, zra, d, len(arc), c, pairs=[(2, 2)], stagings=(1,), modes=(False,))


# ---- 5
@pytest.mark.parametrize("after,before", SH.GAP_PAIRS)
def test_two_selected_records_a_gap_apart(zra, gpu_engine, after, before):
    c = SH.gaps(after, before)
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c)
    assert res[(after, before, False)][1:] == (8, 6)


# ---- 6
def test_more_tiles_than_scan_lanes(zra, gpu_engine):
    c = SH.more_tiles_than_scan_lanes()
    arc, d = _archive(gpu_engine, zra, c, level=1)
    for staging in c["stagings"]:
        res = _check(gpu_engine, zra, d, len(arc), c, stagings=(staging,))
        assert res[(64, 64, False)][1] == 16
        assert gpu_engine.grep_stats()["passes"] == (9 if staging else 1)
    _check(gpu_engine, zra, d, len(arc), c, pairs=[(1, 1)], stagings=(16 * c["fs"],), modes=(True,))


# ---- 7
def test_random_small_shapes(zra, gpu_engine):
    for c in SH.random_small_shapes():
        arc, d = _archive(gpu_engine, zra, c)
        _check(gpu_engine, zra, d, len(arc), c)


# ---- 8
@pytest.fixture(scope="module")
def text(zra, gpu_engine):
    c = SH.text()
    arc, d = _archive(gpu_engine, zra, c)
    return dict(c=c, data=c["data"], arc=arc, d=d, pats=c["pats"], U=len(c["data"]))


def test_capacity(zra, gpu_engine, text):
    c, arc, d, pats, U = text["c"], text["arc"], text["d"], text["pats"], text["U"]
    after, before = 1, 4
    want, nsel, groups, recs, matches = SH.model(c, after, before, False)
    total = len(want)
    inside = next(k for k in range(2, total - 2) if not want[k][2] and not want[k - 1][2] and not want[k + 1][2] and want[k + 2][2])   # in a run of before-context
    assert want[-1][0] + want[-1][1] == U                                      # the record open at hi is the last of O: capacity |O| lists it, |O| - 1 does not
    for cap in (0, 1, inside + 1, total - 1, total, total + 1, total + 5):
        for staging in (0, FS, 1):
            st, counts, mem = _raw(gpu_engine, zra, d, len(arc), pats, cap, after, before, staging=staging, null=cap == 0)
            k = min(total, cap)
            assert (st, counts) == ((0, 0), (total, nsel, groups)), (cap, staging, st, counts)
            got = np.frombuffer(mem[:16 * k], dtype="<u8").reshape(-1, 2)
            assert [(int(o), int(n) & ~SEL, bool(int(n) & SEL)) for o, n in got.tolist()] == want[:k], (cap, staging)
            assert mem[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), (cap, staging)
            assert gpu_engine.grep_stats() == _stats(U, FS, 0, U, staging, len(recs), total, k, matches), (cap, staging)


# ---- 9
def test_range_ends_inside_records(zra, gpu_engine, text):
    c, ranges = SH.clipped_ranges()
    for lo, hi in ranges:
        res = _check(gpu_engine, zra, text["d"], len(text["arc"]), c, lo=lo, hi=hi)
        want = res[(64, 64, True)][0]
        if hi > lo and want:
            assert want[0][0] == lo and want[-1][0] + want[-1][1] in (hi, hi - 1)      # context stops at both ends; the clipped record is reported clipped
    lo, hi = ranges[0]
    want = _check(gpu_engine, zra, text["d"], len(text["arc"]), c, pairs=[(2, 3)], lo=lo, hi=hi, stagings=(1,), modes=(False,))[(2, 3, False)][0]
    assert want[0] == (lo, want[0][1], True) and want[-1][2] and want[-1][0] + want[-1][1] == hi     # ^ and $ hold at the clip


# ---- 10
@pytest.mark.parametrize("name", ["everything", "nothing", "empties", "delimiter_0", "fold_case"])
def test_degenerate_selections(zra, gpu_engine, name):
    c = SH.degenerate()[name]
    arc, d = _archive(gpu_engine, zra, c)
    res = _check(gpu_engine, zra, d, len(arc), c)
    after, before = c["pairs"][0]
    if name == "everything":
        assert res[(after, before, False)][2] == 1 and res[(after, before, True)] == ([], 0, 0)
    if name == "nothing":
        assert res[(after, before, False)] == ([], 0, 0) and res[(after, before, True)][2] == 1


# ---- 11
def test_a_damaged_frame(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    pats = [b"^\\x01+|\\x02{2,}$", b"\\x03\\x04"]
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs, 1):
            st, counts, mem = _raw(gpu_engine, zra, db, len(bad), pats, 6, 2, 3, mode=mode, staging=staging)
            assert (st, counts, mem) == ((1, want[7]), (0, 0, 0), b"\xEE" * 128), (mode, staging, st, counts)
            assert gpu_engine.grep_stats() == ZERO
    c = SH.case("damaged_outside", data, fs, pats, pairs=[(2, 3)])
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), c, lo=lo, hi=hi)


# ---- 12
def test_refusals_with_an_engine(zra, gpu_engine, text):
    d, size, pats = text["d"], len(text["arc"]), text["pats"]
    for kw in (dict(before=65), dict(after=65), dict(before=65, after=65), dict(mode=2), dict(mode=3, before=1), dict(syntax=2), dict(syntax=5)):
        st, counts, mem = _raw(gpu_engine, zra, d, size, pats, 2, **kw)
        assert (st, counts, mem) == ((1, 42), (0, 0, 0), b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, kw
    for bad in ([b"a**"], [b"ne+dle", b"(pin"], [b"a\\nb"], [b"^.{70}$"]):       # a refused expression: reasons 2, 2, 3 and 4
        st, counts, mem = _raw(gpu_engine, zra, d, size, bad, 2, 1, 1)
        assert (st, counts, mem) == ((1, 42), (0, 0, 0), b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, bad
    sizes = (ctypes.c_uint32 * 2)(*(len(p) for p in pats))
    arr = (ctypes.c_uint64 * 8)()
    L = zra.load()
    assert L.ZraHipGrepArchiveRegexContext(gpu_engine.h, d.data_ptr(), size, b"".join(pats), sizes, 2, 0, NL, 0, 1, 1, 0, MAXU64, 0, arr, 4, None, None, None).tup() == (1, 42)
    n = ctypes.c_uint64(7)
    assert L.ZraHipGrepArchiveRegexContext(gpu_engine.h, d.data_ptr(), size, b"".join(pats), sizes, 2, 0, NL, 0, 1, 1, 0, MAXU64, 0, arr, 4, ctypes.byref(n), None,
                                           None).tup() == (0, 0)
    assert n.value == len(SH.model(text["c"], 1, 1, False)[0])                   # nSelected and nGroups may be NULL
    for lo, ln in ((text["U"] + 1, 0), (0, text["U"] + 1), (text["U"], 1)):     # rule 3
        st, counts, mem = _raw(gpu_engine, zra, d, size, pats, 2, 1, 1, offset=lo, length=ln)
        assert (st, counts, mem) == ((5, 0), (0, 0, 0), b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO


# ---- 13
def test_handle_twin_with_partly_resident_frames(zra, gpu_engine, text):
    """Frames 1, 4 and 5 of 7 are resident. The answers are the engine call's; the handle's scan counters move as Archive.grep_regex's
    (ZraHipArchiveGrepRegex) do on the same range, and a scan is not a read."""
    import torch
    c, arc, d, pats = text["c"], text["arc"], text["d"], text["pats"]
    CUM, LAST = ("scans", "staged_total", "decoded_total"), ("staged", "decoded", "passes")
    with zra.Archive(gpu_engine, d.data_ptr(), len(arc), 4 * FS) as h:
        out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        for f in (1, 4, 5):
            h.read(out.data_ptr(), [f * FS], [1], [0])
        cache = h.stats()
        assert cache["resident"] == 3
        for staging in (0, 2 * FS, 1):
            for lo, hi in ((0, None), (FS + 7, 5 * FS + 9)):
                length = None if hi is None else hi - lo
                s0 = h.scan_stats()
                h.grep_regex(pats, offset=lo, length=length, staging_bytes=staging)
                s1 = h.scan_stats()
                moved = {k: s1[k] - s0[k] for k in CUM}
                assert moved["scans"] == 1 and moved["staged_total"] > 0 and moved["decoded_total"] > 0
                for after, before in ((2, 3), (64, 64), (0, 0)):
                    for inv in (False, True):
                        kw = dict(before=before, after=after, invert=inv, offset=lo, length=length, staging_bytes=staging)
                        plain = _call(gpu_engine, zra, d, len(arc), pats, **kw)
                        want = SH.model(c, after, before, inv, lo, hi)
                        assert plain == ((0, 0), len(want[0]), want[1], want[2], want[0]), kw
                        ps = gpu_engine.grep_stats()
                        sa = h.scan_stats()
                        got = ((0, 0),) + h.grep_regex_context(pats, **kw)
                        sb = h.scan_stats()
                        assert got == plain, kw
                        hs = gpu_engine.grep_stats()
                        assert dict(hs, decoded=0, content_bytes=0) == dict(ps, decoded=0, content_bytes=0) and hs["decoded"] == s1["decoded"] < ps["decoded"], (hs, ps)
                        assert {k: sb[k] - sa[k] for k in CUM} == moved and {k: sb[k] for k in LAST} == {k: s1[k] for k in LAST}, (kw, sa, sb, s1)
        assert h.stats() == cache


# ---- 14
def test_cli_mode_glrc(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta\n\ngamma one two\ndelta\neps\nzeta\neta\ntheta one\niota" + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "glrc", str(p_arc)] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    def lines(want, nsel, groups):
        out = []
        for k, (o, n, b) in enumerate(want):
            if k and o != want[k - 1][0] + want[k - 1][1] + 1:
                out.append("--")
            out.append("%d\t%d%s" % (o, n, "\t*" if b else ""))
        return out + ["%d records, %d selected, %d groups" % (len(want), nsel, groups), ""]

    for args, pats, delim, inv, fold, after, before in ((("-A", 1, "one$"), [b"one$"], NL, False, False, 1, 0), (("-B", 1, "-v", "on+e", "^.?eta"), [b"on+e", b"^.?eta"], NL, True, False, 0, 1),
                                                        (("-C", 1, "^g(a|m)+ "), [b"^g(a|m)+ "], NL, False, False, 1, 1), (("-d", "3b", "-A", 2, "-B", 0, "^y$"), [b"^y$"], 0x3B, False, False, 2, 0),
                                                        (("-i", "ONE"), [b"ONE"], NL, False, True, 0, 0), (("-C", 64, "tw?o"), [b"tw?o"], NL, False, False, 64, 64),
                                                        (("-A", 1, "^$"), [b"^$"], NL, False, False, 1, 0)):
        want, nsel, groups = RCM.context(data, pats, delim, inv, fold, before, after)[:3]
        r = run(*args)
        assert r.returncode == 0 and r.stdout.split("\n") == lines(want, nsel, groups) and want, (args, r.stdout, r.stderr)
        assert r.stdout.count("--\n") == groups - 1
    r = run("-C", 3, "absent+")
    assert r.returncode == 1 and r.stdout == "0 records, 0 selected, 0 groups\n", (r.stdout, r.stderr)
    for args in (("-A", 65, "a"), ("-B", "x", "a"), ("-C",), ("-A", 1), (), ("a**",), ("-C", 1, "(a"), ("a\\nb",)):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)


# ---- 15
def _both(eng, zra, d, size, pats, **kw):
    """the literal call and the regex call on the same archive: they share zra_context_tile.h behind their selection bits"""
    lit = ((0, 0),) + eng.grep_context(d.data_ptr(), size, pats, **kw)
    rx = ((0, 0),) + eng.grep_regex_context(d.data_ptr(), size, pats, **kw)
    assert rx == lit, (kw, rx[:4], lit[:4], sorted(set(rx[4]) ^ set(lit[4]))[:10])
    return lit


@pytest.mark.parametrize("before,after", [(3, 2), (64, 64), (0, 0)])
def test_literal_and_regex_context_agree_at_frame_size_4(zra, gpu_engine, before, after):
    """39 records of 0 to 6 bytes over `abc` in frames of 4 bytes, one frame to a pass: most passes end at most one record, so the
    pending ranges are moved, kept and dropped pass by pass. `ab` as a literal pattern and as an expression selects the same
    records; the lists, |S|, |O| and the groups of the two kernel sets must be identical, and the model's."""
    data = SH.lines(np.random.RandomState(6), 150, b"abc", 6)
    c = SH.case("seam_frame_size_4", data, 4, [b"ab"])
    arc, d = _archive(gpu_engine, zra, c)
    for inv in (False, True):
        want, nsel, groups, recs, _ = SH.model(c, after, before, inv)
        assert len(recs) == 39 and 0 < nsel < 39 and len(want) > 3
        got = _both(gpu_engine, zra, d, len(arc), c["pats"], before=before, after=after, invert=inv, staging_bytes=1)
        assert got == ((0, 0), len(want), nsel, groups, want), (inv, got[:4])
        assert gpu_engine.grep_stats()["passes"] == -(-len(data) // 4)
        cap = len(want) - 3                                                     # a capacity below |O|: the counts stay, the list is cut
        got = _both(gpu_engine, zra, d, len(arc), c["pats"], before=before, after=after, invert=inv, staging_bytes=1, max_records=cap)
        assert got == ((0, 0), len(want), nsel, groups, want[:cap]), (inv, cap, got[:4])


def test_literal_and_regex_context_agree_with_more_tiles_than_scan_lanes(zra, gpu_engine):
    """1,030 tiles: a lane of either scan kernel walks two tiles forwards and context_scan_tail walks them back; in nine passes of 128
    tiles the carried state and the pending ranges cross the passes."""
    c = SH.more_tiles_than_scan_lanes()
    arc, d = _archive(gpu_engine, zra, c, level=1)
    pats = [b"status=503", b"timeout after"]
    for before, after, staging in ((64, 64, 16 * c["fs"]), (3, 2, 0)):
        got = _both(gpu_engine, zra, d, len(arc), pats, before=before, after=after, staging_bytes=staging)
        want, nsel, groups, _, _ = SH.model(c, after, before, False)         # (the literal patterns select what the case's expression does)
        assert nsel == 16 and got == ((0, 0), len(want), nsel, groups, want), got[:4]
