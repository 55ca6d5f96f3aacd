"""GPU test of the seven range scans as one family (include/zra_hip.h: ZraHipSearchArchive, ZraHipSearchArchiveMulti, ZraHipGrepArchive,
ZraHipExtractRecords, ZraHipGrepArchiveWhere, ZraHipGrepArchiveRegex, ZraHipExtractRecordsRegex): they run through one host driver,
the five that cut records through one call path as well, and share one scratch pair of an engine with three head layouts and per-tile
entries of 16, 32 and 32 + 64 bytes, so they are called in turn on ONE engine, forwards, backwards and once more after the scratch
was handed back. A table left over from another call, a pass seam or a ping-pong word read with the wrong parity would show in a
count, a list, the packed bytes or a counter. The yardsticks are the CPU models of the seven calls' own test files. The shape is the
smallest at which every seam exists: more than one tile of 8,192 positions, twelve frames of 1,024 bytes (the last one short), passes
of one, two, three and all frames, and patterns cut across a frame boundary that is a pass boundary for all of them. The grep with
clauses and the regex grep write the grep's counters and milliseconds, the regex extract the extract's: ROW."""
import ctypes

import numpy as np
import pytest

import extract_model as XM
import extract_regex_model as XRM
import grep_model as GM
import msearch_model as MM
import regex_model as RM
import search_model as SM
import test_gpu_extract as X
import test_gpu_grep as G
import test_gpu_msearch as MS
import test_gpu_search as S
import where_model as WM
from test_gpu_update import _compress, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
FS = 1024
NL = 10
SEAM = 6 * FS                                                                  # a pass boundary at one, two and three frames per pass
GETTERS = dict(extract="ZraHipGetExtractStats", search="ZraHipGetSearchStats", grep="ZraHipGetGrepStats", multi="ZraHipGetSearchMultiStats")
STAGING = dict(extract=0, search=FS, grep=3 * FS, multi=2 * FS, where=2 * FS, regex=FS, xregex=3 * FS)
ORDER = ("extract", "search", "grep", "multi", "where", "regex", "xregex")
ROW = dict(extract="extract", search="search", grep="grep", multi="multi", where="grep", regex="grep", xregex="extract")   # whose counters and ms a call writes
ROWS = ("extract", "search", "grep", "multi")


def _words(eng, which):
    a = (ctypes.c_uint64 * 8)()
    getattr(eng.L, GETTERS[ROW[which]])(eng.h, a)
    return [int(v) for v in a]


def _ms(eng, which):
    return dict(extract=eng.extract_ms, search=eng.search_scan_ms, grep=eng.grep_scan_ms, multi=eng.search_multi_scan_ms)[ROW[which]]()


@pytest.fixture(scope="module")
def family(zra, gpu_engine):
    """The content, its archive on the device, the patterns, and per call what the models say: the answer and the eight counters."""
    import test_gpu_grep_regex as R                                            # (imported here: that file imports this one's importer)
    U = 12 * FS - 100
    a = bytearray(G._lines(np.random.RandomState(77), U))
    a[SEAM - 17:SEAM + 23] = bytes(a[SEAM - 17:SEAM + 23]).replace(b"\n", b"c")   # one stretch of line across the boundary
    data = bytes(a)
    pats = [b"b", data[SEAM - 1:SEAM + 2], data[SEAM - 17:SEAM + 23], b"zz", b"ea"]
    assert len(data) == U > 8192 and [len(p) for p in pats] == [1, 3, 40, 2, 2] and NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    geo = {k: G._stats(U, FS, 0, U, STAGING[k], 0, 0, 0, 0) for k in ORDER}
    assert [geo[k]["passes"] for k in ORDER] == [1, 12, 4, 6, 6, 12, 4] and geo["search"]["decoded"] == 12
    head = {k: [geo[k]["frames"], geo[k]["decoded"], geo[k]["content_bytes"]] for k in ORDER}
    one = SM.matches(data, pats[1])
    multi = MM.matches_multi(data, pats)
    recs, inv_sel, matches = GM.grep(data, pats, NL, True)
    xrecs, sel, xmatches, packed = XM.extract(data, pats)
    assert SEAM - 1 in one and (SEAM - 17, 2) in multi and len(one) > 20 and len(inv_sel) > 20 and len(sel) > 20 and recs == xrecs and matches == len(multi)
    # the clauses and the expressions are over the same five patterns, and each selects the record that crosses SEAM
    clauses = [(WM.mask([1, 2]), 0, WM.mask([3])), (0, WM.mask([4]), WM.mask([0]))]
    exprs = [pats[1] + b"|" + pats[3], b"^(" + pats[4] + b"|" + pats[0] + b")", pats[2]]
    assert RM.check(exprs, False, NL)["why"] == 0
    crossing = [r for r in recs if r[0] < SEAM < r[0] + r[1]]
    wrecs, wsel, wmatches = WM.grep_where(data, pats, clauses, NL)
    rrecs, rsel, rmatched = RM.grep_regex(data, exprs, NL, matcher=R._Memo(exprs))
    _, xrsel, xrmatched, xrpacked = XRM.extract_regex(data, exprs, NL, matcher=R._Memo(exprs))
    assert len(crossing) == 1 and crossing[0] in wsel and crossing[0] in rsel and crossing[0] in xrsel
    assert wrecs == rrecs == recs and wmatches == matches and 20 < len(wsel) < len(recs) - 20 and 20 < len(rsel) < len(recs) - 20
    assert (xrsel, xrmatched) == (rsel, rmatched) and len(xrpacked) == sum(n + 1 for _, n in rsel)
    want = dict(search=(len(one), one), multi=(len(multi), multi, MS._per(multi, len(pats))), grep=(len(inv_sel), inv_sel), extract=(len(sel), len(packed), sel, packed),
                where=(len(wsel), wsel), regex=(len(rsel), rsel), xregex=(len(xrsel), len(xrpacked), xrsel, xrpacked))
    words = dict(search=head["search"] + [len(one), len(one), 12, 0, 0],
                 multi=head["multi"] + [len(multi), len(multi), 6, len(pats), MM.survivors(data, pats)],
                 grep=[G._stats(U, FS, 0, U, 3 * FS, len(recs), len(inv_sel), len(inv_sel), matches)[k] for k in zra.GREP_STATS],
                 extract=[X._stats(U, FS, 0, U, 0, len(recs), len(sel), len(packed), matches)[k] for k in zra.EXTRACT_STATS],
                 where=[G._stats(U, FS, 0, U, STAGING["where"], len(recs), len(wsel), len(wsel), matches)[k] for k in zra.GREP_STATS],
                 regex=[G._stats(U, FS, 0, U, STAGING["regex"], len(recs), len(rsel), len(rsel), rmatched)[k] for k in zra.GREP_STATS],
                 xregex=[X._stats(U, FS, 0, U, STAGING["xregex"], len(recs), len(xrsel), len(xrpacked), rmatched)[k] for k in zra.EXTRACT_STATS])
    return dict(data=data, arc=arc, d=_dev(arc), pats=pats, clauses=clauses, exprs=exprs, want=want, words=words)


def _call(eng, which, f):
    """one call of the family on the device archive: what it returned, with the packed bytes for the extract"""
    import torch
    P, size, pats = f["d"].data_ptr(), len(f["arc"]), f["pats"]
    if which == "search":
        return eng.search(P, size, pats[1], staging_bytes=STAGING[which])
    if which == "multi":
        return eng.search_multi(P, size, pats, staging_bytes=STAGING[which])
    if which == "grep":
        return eng.grep(P, size, pats, invert=True, staging_bytes=STAGING[which])
    if which == "where":
        return eng.grep(P, size, pats, where=f["clauses"], staging_bytes=STAGING[which])
    if which == "regex":
        return eng.grep_regex(P, size, f["exprs"], staging_bytes=STAGING[which])
    cap = len(f["data"]) + 64
    buf = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda:0")
    if which == "xregex":
        n, ds, sel = eng.extract_regex(P, size, f["exprs"], buf.data_ptr(), cap, staging_bytes=STAGING[which], max_records=f["want"][which][0] + 1)
    else:
        n, ds, sel = eng.extract(P, size, pats, buf.data_ptr(), cap, staging_bytes=STAGING[which], max_records=f["want"]["extract"][0] + 1)
    torch.cuda.synchronize()
    return n, ds, sel, buf[:ds].cpu().numpy().tobytes()


def _round(eng, f, order, seen):
    """the calls of `order`, each against its model: answer, all eight counters of its row, a time above zero, the other rows untouched"""
    for which in order:
        got = _call(eng, which, f)
        assert tuple(got) == f["want"][which], (which, got[0], f["want"][which][0])
        assert _words(eng, which) == f["words"][which], (which, _words(eng, which), f["words"][which])
        assert _ms(eng, which) > 0, which
        seen[ROW[which]] = f["words"][which]
        for other in ROWS:
            assert _words(eng, other) == seen[other], (which, other)


def test_seven_calls_take_turns_on_one_engine(zra, gpu_engine, family):
    seen = {k: _words(gpu_engine, k) for k in ROWS}
    _round(gpu_engine, family, ORDER, seen)
    _round(gpu_engine, family, ORDER[::-1], seen)
    gpu_engine.release_scratch()                                               # scratch handed back: the same answers
    _round(gpu_engine, family, ORDER, seen)


def test_a_damaged_frame_ends_all_seven_the_same_way(zra, gpu_engine, family):
    """One byte flipped in the middle of frame 6's compressed span: every call ends with the status a whole-frame read of that frame
    gives, its row's counters and time zero, the caller's arrays untouched; the counters of the rows it does not write stay."""
    import test_gpu_extract_regex as XR                                        # (imported here: these files import this one's importer)
    import test_gpu_grep_regex as R
    import test_gpu_grep_where as W
    arc, pats, clauses, exprs = family["arc"], family["pats"], family["clauses"], family["exprs"]
    bad = _flip_mid(arc, [6])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {6} and want[6] != 0, want
    status = (1, want[6])
    seen = {k: _words(gpu_engine, k) for k in ROWS}
    _round(gpu_engine, family, ORDER, seen)                                    # every row's counters and time are non-zero now
    for which in ORDER:
        _round(gpu_engine, family, [which], seen)                              # and the call's row and time are its own
        if which == "extract":
            st, n, ds, mem, _ = X._raw(gpu_engine, zra, db, len(bad), pats, 13 * FS, 4, staging=STAGING[which])
            assert (st, n, ds, mem) == (status, 0, 0, b"\xEE" * 96), (which, st, n, ds)
        elif which == "xregex":
            st, n, ds, mem, _ = XR._raw(gpu_engine, zra, db, len(bad), exprs, 13 * FS, 4, staging=STAGING[which])
            assert (st, n, ds, mem) == (status, 0, 0, b"\xEE" * 96), (which, st, n, ds)
        elif which == "where":
            st, n, mem = W._raw(gpu_engine, zra, db, len(bad), pats, clauses, 4, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 96), (which, st, n)
        elif which == "regex":
            st, n, mem = R._raw(gpu_engine, zra, db, len(bad), exprs, 4, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 96), (which, st, n)
        elif which == "search":
            st, n, mem = S._raw(gpu_engine, zra, db, len(bad), pats[1], 4, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 48), (which, st, n)
        elif which == "grep":
            st, n, mem = G._raw(gpu_engine, zra, db, len(bad), pats, 4, mode=1, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 96), (which, st, n)
        else:
            st, n, mem, per = MS._raw(gpu_engine, zra, db, len(bad), pats, 4, staging=STAGING[which])
            assert (st, n, mem, per) == (status, 0, b"\xEE" * 96, b"\xEE" * 48), (which, st, n)
        seen[ROW[which]] = [0] * 8
        assert _ms(gpu_engine, which) == 0, which
        for other in ROWS:
            assert _words(gpu_engine, other) == seen[other], (which, other)
