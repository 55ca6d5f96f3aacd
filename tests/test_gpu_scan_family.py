"""GPU test of the four range scans as one family (include/zra_hip.h: ZraHipSearchArchive, ZraHipSearchArchiveMulti, ZraHipGrepArchive,
ZraHipExtractRecords): they run through one host driver and share one scratch pair of an engine, so they are called in turn on ONE
engine, the call with the largest tables first and the one with the smallest behind it, forwards, backwards and once more after the
scratch was handed back. A table left over from another call, a pass seam or a ping-pong word read with the wrong parity would show
in a count, a list, the packed bytes or a counter. The yardsticks are the CPU models of the four calls' own test files. The shape is
the smallest at which every seam exists: more than one tile of 8,192 positions, twelve frames of 1,024 bytes (the last one short),
passes of one, two, three and all frames, and patterns cut across a frame boundary that is a pass boundary for all of them."""
import ctypes

import numpy as np
import pytest

import extract_model as XM
import grep_model as GM
import msearch_model as MM
import search_model as SM
import test_gpu_extract as X
import test_gpu_grep as G
import test_gpu_msearch as MS
import test_gpu_search as S
from test_gpu_update import _compress, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
FS = 1024
NL = 10
SEAM = 6 * FS                                                                  # a pass boundary at one, two and three frames per pass
GETTERS = dict(extract="ZraHipGetExtractStats", search="ZraHipGetSearchStats", grep="ZraHipGetGrepStats", multi="ZraHipGetSearchMultiStats")
STAGING = dict(extract=0, search=FS, grep=3 * FS, multi=2 * FS)
ORDER = ("extract", "search", "grep", "multi")


def _words(eng, which):
    a = (ctypes.c_uint64 * 8)()
    getattr(eng.L, GETTERS[which])(eng.h, a)
    return [int(v) for v in a]


def _ms(eng, which):
    return dict(extract=eng.extract_ms, search=eng.search_scan_ms, grep=eng.grep_scan_ms, multi=eng.search_multi_scan_ms)[which]()


@pytest.fixture(scope="module")
def family(zra, gpu_engine):
    """The content, its archive on the device, the patterns, and per call what the models say: the answer and the eight counters."""
    U = 12 * FS - 100
    a = bytearray(G._lines(np.random.RandomState(77), U))
    a[SEAM - 17:SEAM + 23] = bytes(a[SEAM - 17:SEAM + 23]).replace(b"\n", b"c")   # one stretch of line across the boundary
    data = bytes(a)
    pats = [b"b", data[SEAM - 1:SEAM + 2], data[SEAM - 17:SEAM + 23], b"zz", b"ea"]
    assert len(data) == U > 8192 and [len(p) for p in pats] == [1, 3, 40, 2, 2] and NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    geo = {k: G._stats(U, FS, 0, U, STAGING[k], 0, 0, 0, 0) for k in ORDER}
    assert [geo[k]["passes"] for k in ORDER] == [1, 12, 4, 6] and geo["search"]["decoded"] == 12
    head = {k: [geo[k]["frames"], geo[k]["decoded"], geo[k]["content_bytes"]] for k in ORDER}
    one = SM.matches(data, pats[1])
    multi = MM.matches_multi(data, pats)
    recs, inv_sel, matches = GM.grep(data, pats, NL, True)
    xrecs, sel, xmatches, packed = XM.extract(data, pats)
    assert SEAM - 1 in one and (SEAM - 17, 2) in multi and len(one) > 20 and len(inv_sel) > 20 and len(sel) > 20 and recs == xrecs and matches == len(multi)
    want = dict(search=(len(one), one), multi=(len(multi), multi, MS._per(multi, len(pats))), grep=(len(inv_sel), inv_sel), extract=(len(sel), len(packed), sel, packed))
    words = dict(search=head["search"] + [len(one), len(one), 12, 0, 0],
                 multi=head["multi"] + [len(multi), len(multi), 6, len(pats), MM.survivors(data, pats)],
                 grep=[G._stats(U, FS, 0, U, 3 * FS, len(recs), len(inv_sel), len(inv_sel), matches)[k] for k in zra.GREP_STATS],
                 extract=[X._stats(U, FS, 0, U, 0, len(recs), len(sel), len(packed), matches)[k] for k in zra.EXTRACT_STATS])
    return dict(data=data, arc=arc, d=_dev(arc), pats=pats, want=want, words=words)


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
    cap = len(f["data"]) + 64
    buf = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda:0")
    n, ds, sel = eng.extract(P, size, pats, buf.data_ptr(), cap, staging_bytes=STAGING[which], max_records=f["want"]["extract"][0] + 1)
    torch.cuda.synchronize()
    return n, ds, sel, buf[:ds].cpu().numpy().tobytes()


def _round(eng, f, order, seen):
    """the calls of `order`, each against its model: answer, all eight counters, a time above zero, the other calls' counters untouched"""
    for which in order:
        got = _call(eng, which, f)
        assert tuple(got) == f["want"][which], (which, got[0], f["want"][which][0])
        assert _words(eng, which) == f["words"][which], (which, _words(eng, which), f["words"][which])
        assert _ms(eng, which) > 0, which
        seen[which] = f["words"][which]
        for other in ORDER:
            assert _words(eng, other) == seen[other], (which, other)


def test_four_calls_take_turns_on_one_engine(zra, gpu_engine, family):
    seen = {k: _words(gpu_engine, k) for k in ORDER}
    _round(gpu_engine, family, ORDER, seen)
    _round(gpu_engine, family, ORDER[::-1], seen)
    gpu_engine.release_scratch()                                               # scratch handed back: the same answers
    _round(gpu_engine, family, ORDER, seen)


def test_a_damaged_frame_ends_all_four_the_same_way(zra, gpu_engine, family):
    """One byte flipped in the middle of frame 6's compressed span: every call ends with the status a whole-frame read of that frame
    gives, its counters and its time zero, the caller's arrays untouched; the counters of the calls that did not run stay."""
    arc, pats = family["arc"], family["pats"]
    bad = _flip_mid(arc, [6])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {6} and want[6] != 0, want
    status = (1, want[6])
    _round(gpu_engine, family, ORDER, {k: _words(gpu_engine, k) for k in ORDER})   # every call's counters and time are non-zero now
    seen = {k: family["words"][k] for k in ORDER}
    for which in ORDER:
        if which == "extract":
            st, n, ds, mem, _ = X._raw(gpu_engine, zra, db, len(bad), pats, 13 * FS, 4, staging=STAGING[which])
            assert (st, n, ds, mem) == (status, 0, 0, b"\xEE" * 96), (which, st, n, ds)
        elif which == "search":
            st, n, mem = S._raw(gpu_engine, zra, db, len(bad), pats[1], 4, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 48), (which, st, n)
        elif which == "grep":
            st, n, mem = G._raw(gpu_engine, zra, db, len(bad), pats, 4, mode=1, staging=STAGING[which])
            assert (st, n, mem) == (status, 0, b"\xEE" * 96), (which, st, n)
        else:
            st, n, mem, per = MS._raw(gpu_engine, zra, db, len(bad), pats, 4, staging=STAGING[which])
            assert (st, n, mem, per) == (status, 0, b"\xEE" * 96, b"\xEE" * 48), (which, st, n)
        seen[which] = [0] * 8
        assert _ms(gpu_engine, which) == 0, which
        for other in ORDER:
            assert _words(gpu_engine, other) == seen[other], (which, other)
