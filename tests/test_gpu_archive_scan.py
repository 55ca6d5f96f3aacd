"""GPU test of the range scans through an archive handle (include/zra_hip.h: ZraHipArchiveSearch, ZraHipArchiveSearchMulti,
ZraHipArchiveGrep, ZraHipArchiveExtractRecords): a pass takes its resident frames out of the handle's arena and decodes the others, and
the answer is the plain call's on the same bytes. The yardsticks are the plain engine calls and the CPU models of their test files.
The shape is the smallest in which every seam exists: 40 frames (the last one of 300 bytes), 12 of them resident in slots whose order
is not frame order, passes of all, one and three frames, so that a pass is resident-missing-resident, mixed, all resident, all missing,
mixed ending on a resident frame, or one short resident frame; 40-byte stretches without a newline lie across a resident -> missing, a
missing -> resident, a resident -> resident boundary, a pass seam and the boundary into the short last frame, and each is a pattern.
With a frame size of 1,000 the arena slots and the window slots are not co-aligned."""
import ctypes

import numpy as np
import pytest

import extract_model as XM
import grep_model as GM
import msearch_model as MM
import search_model as SM
import test_gpu_grep as G
import test_gpu_scan_family as F
from test_gpu_update import _compress, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
NL = 10
MAXU64 = (1 << 64) - 1
NF = 40
WARM = (39, 20, 6, 2, 14, 5, 27, 8, 7, 21, 38, 0)                              # read in this order: slot order is not frame order
CUTS = (3, 5, 7, 9, 39)                                                        # the frame boundaries a 40-byte stretch lies across
ORDER = ("extract", "search", "grep", "multi")
PASSES_WORD = dict(search=5, multi=5, grep=6, extract=6)
MAXREC = 8192


def _content(seed, fs):
    U = (NF - 1) * fs + 300
    a = bytearray(G._lines(np.random.RandomState(seed), U))
    for b in CUTS:
        a[b * fs - 17:b * fs + 23] = bytes(a[b * fs - 17:b * fs + 23]).replace(b"\n", b"c")
    data = bytes(a)
    long_ = [data[b * fs - 17:b * fs + 23] for b in CUTS]
    pats = long_ + [b"b", data[7 * fs - 1:7 * fs + 2], b"zz", b"ea"]
    assert len(data) == U and all(len(p) == 40 and NL not in p for p in long_) and NL not in b"".join(pats)
    return data, pats


def _flen(f, fs, U):
    return min(fs, U - f * fs)


def _open_warm(zra, eng, d, size, fs, U, warm=WARM, slots=12):
    h = zra.Archive(eng, d.data_ptr(), size, slots * fs)
    if slots:
        import torch
        out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        for f in warm:
            h.read(out.data_ptr(), [f * fs], [1], [0])
    return h


def _resident_ok(h, n=12):
    s = h.stats()
    assert (s["slots"], s["resident"], s["evictions"]) == (n, n, 0), s
    return s


@pytest.fixture(scope="module", params=[1024, 1000])
def shape(request, zra, gpu_engine):
    fs = request.param
    data, pats = _content(77, fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    h = _open_warm(zra, gpu_engine, d, len(arc), fs, len(data))
    _resident_ok(h)
    yield dict(fs=fs, U=len(data), data=data, pats=pats, arc=arc, d=d, h=h)
    h.close()


def _plain(eng, which, d, size, pats, one, lo, length, staging):
    """one call of the family on the device archive; the extract with its packed bytes"""
    import torch
    kw = dict(offset=lo, length=length, staging_bytes=staging)
    P = d.data_ptr()
    if which == "search":
        return eng.search(P, size, one, **kw)
    if which == "multi":
        return eng.search_multi(P, size, pats, **kw)
    if which == "grep":
        return eng.grep(P, size, pats, **kw)
    buf = torch.full((48 * 1024,), 0xEE, dtype=torch.uint8, device="cuda:0")
    n, ds, sel = eng.extract(P, size, pats, buf.data_ptr(), buf.numel(), max_records=MAXREC, **kw)
    torch.cuda.synchronize()
    return n, ds, sel, buf[:ds].cpu().numpy().tobytes()


def _through(h, which, pats, one, lo, length, staging):
    """the same call through the handle"""
    import torch
    kw = dict(offset=lo, length=length, staging_bytes=staging)
    if which == "search":
        return h.search(one, **kw)
    if which == "multi":
        return h.search_multi(pats, **kw)
    if which == "grep":
        return h.grep(pats, **kw)
    buf = torch.full((48 * 1024,), 0xEE, dtype=torch.uint8, device="cuda:0")
    n, ds, sel = h.extract(pats, buf.data_ptr(), buf.numel(), max_records=MAXREC, **kw)
    torch.cuda.synchronize()
    return n, ds, sel, buf[:ds].cpu().numpy().tobytes()


def _model(which, data, pats, one, lo, hi):
    if which == "search":
        m = SM.matches(data, one, lo, hi)
        return len(m), m
    if which == "multi":
        m = MM.matches_multi(data, pats, lo, hi)
        return len(m), m, [sum(1 for _, i in m if i == j) for j in range(len(pats))]
    if which == "grep":
        _, sel, _ = GM.grep(data, pats, NL, False, lo, hi)
        return len(sel), sel
    _, sel, _, packed = XM.extract(data, pats, NL, False, lo, hi)
    return len(sel), len(packed), sel, packed


def _split(warm, fs, U, lo, hi):
    """(frames staged from the cache, frames decoded, bytes decoded) of a scan of [lo, hi)"""
    fr = range(lo // fs, (hi - 1) // fs + 1)
    miss = [f for f in fr if f not in warm]
    return len(fr) - len(miss), len(miss), sum(_flen(f, fs, U) for f in miss)


# ---- 1
@pytest.mark.parametrize("sub", [False, True])
def test_four_calls_equal_the_plain_call_and_the_model(zra, gpu_engine, shape, sub):
    fs, U, data, pats, d, h, size = shape["fs"], shape["U"], shape["data"], shape["pats"], shape["d"], shape["h"], len(shape["arc"])
    lo, hi = (6 * fs + fs // 2, 10 * fs + fs // 2) if sub else (0, U)
    length = hi - lo if sub else None
    staged, decoded, dec_bytes = _split(WARM, fs, U, lo, hi)
    assert (staged, decoded) == ((3, 2) if sub else (12, 28))
    singles = pats[:5] if not sub else [pats[2], pats[3], pats[6]]               # 6|7 and 8|9 lie inside the sub-range
    before = _resident_ok(h)
    totals = h.scan_stats()
    for staging in (0, fs, 3 * fs):
        for which in ORDER:
            for one in (singles if which == "search" else [None]):
                tag = (fs, sub, staging, which, one)
                want = _model(which, data, pats, one, lo, hi)
                plain = _plain(gpu_engine, which, d, size, pats, one, lo, length, staging)
                pw = F._words(gpu_engine, which)
                got = _through(h, which, pats, one, lo, length, staging)
                hw = F._words(gpu_engine, which)
                assert tuple(plain) == tuple(want), (tag, plain[0], want[0])
                assert tuple(got) == tuple(plain), (tag, got[0], plain[0])
                assert want[0] > 0, tag
                assert hw[:1] + hw[3:] == pw[:1] + pw[3:], (tag, hw, pw)
                assert pw[1:3] == [staged + decoded, sum(_flen(f, fs, U) for f in range(lo // fs, (hi - 1) // fs + 1))], (tag, pw)
                assert hw[1:3] == [decoded, dec_bytes], (tag, hw)
                assert F._ms(gpu_engine, which) > 0, tag
                s = h.scan_stats()
                totals = dict(scans=totals["scans"] + 1, staged=staged, decoded=decoded, passes=pw[PASSES_WORD[which]],
                              staged_total=totals["staged_total"] + staged, decoded_total=totals["decoded_total"] + decoded)
                assert s == totals, (tag, s, totals)
                assert h.scan_stage_ms() > 0, tag
    assert h.stats() == before


def test_long_patterns_are_found_across_every_boundary(zra, gpu_engine, shape):
    """the five stretches, each found where it was cut, by the one-frame passes"""
    fs, pats, h = shape["fs"], shape["pats"], shape["h"]
    n, listed, per = h.search_multi(pats[:5], staging_bytes=fs)
    assert [(b * fs - 17, i) in listed for i, b in enumerate(CUTS)] == [True] * 5 and min(per) >= 1, (n, per)


# ---- 2
def test_scans_leave_the_cache_alone(zra, gpu_engine, shape):
    import torch
    fs, U, data, pats, h = shape["fs"], shape["U"], shape["data"], shape["pats"], shape["h"]
    before = _resident_ok(h)
    for which in ORDER:
        _through(h, which, pats, pats[0], 0, None, 3 * fs)
    assert h.stats() == before
    out = torch.full((fs,), 0xEE, dtype=torch.uint8, device="cuda:0")
    for k, f in enumerate(sorted(WARM)):
        n = min(fs, U - f * fs - 1)                                            # (the reads' bound: a query ends in front of the last byte)
        h.read(out.data_ptr(), [f * fs], [n], [0])
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().tobytes() == data[f * fs:f * fs + n], f
        s = h.stats()
        assert (s["hits"], s["misses"], s["evictions"], s["resident"]) == (before["hits"] + k + 1, before["misses"], 0, 12), (f, s)


# ---- 3
def test_an_all_resident_range_launches_no_decode(zra, gpu_engine, shape):
    fs, data, pats, h = shape["fs"], shape["data"], shape["pats"], shape["h"]
    lo, hi = 6 * fs, 9 * fs
    for which in ORDER:
        for staging in (0, fs):
            got = _through(h, which, pats, pats[2], lo, hi - lo, staging)
            assert tuple(got) == tuple(_model(which, data, pats, pats[2], lo, hi)), (which, staging)
            assert gpu_engine.kernel_stats()["dec_launches"] == 0, (which, staging)
            s = h.scan_stats()
            assert (s["staged"], s["decoded"], s["passes"]) == (3, 0, 3 if staging else 1), (which, staging, s)
            assert F._words(gpu_engine, which)[1:3] == [0, 0], which
            assert h.scan_stage_ms() > 0


# ---- 4
def test_a_handle_without_slots_is_the_plain_call(zra, gpu_engine, shape):
    fs, U, data, pats, d, size = shape["fs"], shape["U"], shape["data"], shape["pats"], shape["d"], len(shape["arc"])
    with zra.Archive(gpu_engine, d.data_ptr(), size, 0) as h0:
        for which in ORDER:
            for staging in (0, 3 * fs):
                plain = _plain(gpu_engine, which, d, size, pats, pats[1], 0, None, staging)
                pw = F._words(gpu_engine, which)
                got = _through(h0, which, pats, pats[1], 0, None, staging)
                assert tuple(got) == tuple(plain) and F._words(gpu_engine, which) == pw, (which, staging)
                s = h0.scan_stats()
                assert (s["staged"], s["decoded"], s["passes"], s["staged_total"]) == (0, NF, pw[PASSES_WORD[which]], 0), s
                assert h0.scan_stage_ms() == 0
        assert h0.stats()["reads"] == 0


# ---- 5
def test_after_an_update_the_scan_sees_the_new_bytes(zra, gpu_engine, shape):
    """A write inside resident frame 6, one inside missing frame 10 and an append into the resident short last frame: the stage takes
    the refreshed arena bytes, the decode the re-bound archive."""
    import torch
    fs, U, data, arc = shape["fs"], shape["U"], shape["data"], shape["arc"]
    marks = [b"MARK-IN-RESIDENT-SIX", b"MARK-IN-MISSING-TEN", b"MARK-APPENDED-BEHIND"]
    d = _dev(arc)
    h = _open_warm(zra, gpu_engine, d, len(arc), fs, U)
    _resident_ok(h)
    blob = _dev(marks[0] + marks[1])
    app = b"\n" + marks[2] + b" and a tail"
    d_app = _dev(app)
    cap = len(arc) + zra.GetOutputBufferSize(U + len(app), fs) + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    new_size = h.update(d_out.data_ptr(), cap, writes=([6 * fs + 100, 10 * fs + 100], [len(marks[0]), len(marks[1])], [0, len(marks[0])]),
                        d_data=blob.data_ptr(), d_append=d_app.data_ptr(), append_size=len(app))
    want = [(6 * fs + 100, 0), (10 * fs + 100, 1), (U + 1, 2)]
    for staging in (0, 3 * fs):
        plain = gpu_engine.search_multi(d_out.data_ptr(), new_size, marks, staging_bytes=staging)
        got = h.search_multi(marks, staging_bytes=staging)
        assert got == plain and got[1] == want and got[2] == [1, 1, 1], (staging, got, plain)
        s = h.scan_stats()
        assert (s["staged"], s["decoded"]) == (12, NF - 12), s
    _resident_ok(h)
    h.close()


# ---- 6
def _raw_through(zra, h, which, pats, one, cap, lo=0, length=MAXU64, staging=0):
    """(status, the output words, the bytes of the sentinel-filled host arrays and of dData) of one call through the handle"""
    import torch
    L = zra.load()
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    per = (ctypes.c_uint64 * (len(pats) + 1))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr)); ctypes.memset(per, 0xEE, ctypes.sizeof(per))
    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    buf = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
    h.engine._order()
    if which == "search":
        st = L.ZraHipArchiveSearch(h.h, one, len(one), lo, length, staging, arr, cap, ctypes.byref(n))
    elif which == "multi":
        st = L.ZraHipArchiveSearchMulti(h.h, b"".join(pats), sizes, len(pats), lo, length, staging, ctypes.cast(arr, ctypes.POINTER(zra.ZraHipPatternMatch)), cap,
                                        ctypes.byref(n), per)
    elif which == "grep":
        st = L.ZraHipArchiveGrep(h.h, b"".join(pats), sizes, len(pats), NL, 0, lo, length, staging, arr, cap, ctypes.byref(n))
    else:
        st = L.ZraHipArchiveExtractRecords(h.h, b"".join(pats), sizes, len(pats), NL, 0, lo, length, staging, arr, cap, ctypes.byref(n), buf.data_ptr(), 4096,
                                           ctypes.byref(ds))
    torch.cuda.synchronize()
    return st.tup(), n.value, ds.value, bytes(arr), bytes(per), buf.cpu().numpy().tobytes()


def test_a_damaged_missing_frame_ends_every_call_and_changes_nothing(zra, gpu_engine, shape):
    fs, U, data, pats, arc = shape["fs"], shape["U"], shape["data"], shape["pats"], shape["arc"]
    bad = _flip_mid(arc, [10])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, frames=[9, 10, 11], d_arc=db)
    assert set(want) == {10} and want[10] != 0, want
    h = _open_warm(zra, gpu_engine, db, len(bad), fs, U)                       # the same warmed set: frame 10 is not resident
    cache = _resident_ok(h)
    scans = h.scan_stats()
    for which in ORDER:
        _plain(gpu_engine, which, shape["d"], len(arc), pats, pats[0], 0, None, 0)  # the kind's counters and time are non-zero now
        for staging in (0, 3 * fs):
            st, n, ds, arr, per, mem = _raw_through(zra, h, which, pats, pats[0], 4, staging=staging)
            tag = (which, staging, st, n, ds)
            assert st == (1, want[10]) and n == 0 and ds == (0 if which == "extract" else 0x5678), tag
            assert arr == b"\xEE" * len(arr) and per == b"\xEE" * len(per), tag
            # (dData: untouched when the failing pass is the first one; the extract's passes in front of a failing one have packed their
            # records already, through the handle as in the plain call, whose header promises nothing for the bytes inside the capacity)
            assert mem == b"\xEE" * 4096 or (which == "extract" and staging), tag
            assert F._words(gpu_engine, which) == [0] * 8 and F._ms(gpu_engine, which) == 0, tag
            assert h.scan_stats() == scans and h.stats() == cache, tag
    k = 0
    for which in ORDER:                                                        # in front of the damage every call succeeds
        got = _through(h, which, pats, pats[0], 0, 9 * fs, 3 * fs)
        assert tuple(got) == tuple(_model(which, data, pats, pats[0], 0, 9 * fs)), which
        k += 1
        s = h.scan_stats()
        assert (s["scans"], s["staged"], s["decoded"], s["passes"]) == (scans["scans"] + k, 6, 3, 3), s
    assert h.stats() == cache
    h.close()


# ---- 7
def test_two_handles_take_turns_on_one_engine(zra, gpu_engine, shape):
    """another archive with another resident set on the same engine: the handles share the engine's scan scratch, and the answers stay right"""
    fs = 1024
    data2, pats2 = _content(78, fs)
    arc2 = _compress(gpu_engine, zra, data2, 3, fs, True)
    d2 = _dev(arc2)
    warm2 = (11, 1, 9, 3, 4, 10)
    h2 = _open_warm(zra, gpu_engine, d2, len(arc2), fs, len(data2), warm=warm2, slots=6)
    _resident_ok(h2, 6)
    a = dict(h=shape["h"], data=shape["data"], pats=shape["pats"], fs=shape["fs"], U=shape["U"], warm=WARM)
    b = dict(h=h2, data=data2, pats=pats2, fs=fs, U=len(data2), warm=warm2)
    want = {}
    for staging_frames in (3, 0):
        for which in ORDER:
            for x in (a, b, a):
                key = (id(x["h"]), which)
                if key not in want:
                    want[key] = tuple(_model(which, x["data"], x["pats"], x["pats"][1], 0, None))
                got = _through(x["h"], which, x["pats"], x["pats"][1], 0, None, staging_frames * x["fs"])
                assert tuple(got) == want[key], (which, staging_frames, x is a)
                s = x["h"].scan_stats()
                assert (s["staged"], s["decoded"]) == (len(x["warm"]), NF - len(x["warm"])), s
    h2.close()
