"""GPU tests of ZraHipExtractRecordsWhere and ZraHipArchiveExtractRecordsWhere (include/zra_hip.h): the records a predicate over the
patterns selects WITH their bytes, packed. The yardstick everywhere is tests/extract_where_model.py (where_model's selection,
extract_model's packing) on the inputs of tests/extract_where_shapes.py, which tests/test_extract_where_abi.py holds to the seams
they are built for. Archives are written on the device. dData is a 0xEE-filled buffer handed over 64 bytes in, with a capacity that
leaves 64 guard bytes behind it: after every call both guards are still 0xEE. Every check compares status, both words, the packed
bytes, the list (also with Engine.grep(where=...)'s), all eight extract stats, and the grep's and the searches' stats with what they
were; it runs in both modes and, unless it is about emptiness, asserts that both select something."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expr_model as EM
import extract_where_shapes as SH
import grep_model as GM
import test_gpu_archive_scan as AS
import test_gpu_extract as X
import where_model as WM
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
GUARD = 64
FS = SH.FS
ZERO, TOO_SMALL = X.ZERO, X.TOO_SMALL


def _raw(eng, zra, d, size, pats, where, data_cap, rec_cap, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, handle=None):
    """(status, *nRecords, *dataSize, the bytes of a record array two entries longer than the capacity, the first data_cap bytes of
    dData) of one call, through `handle` when there is one; both 0xEE-filled before it. Asserts that the guards in front of dData and
    behind its capacity are intact."""
    import torch
    buf = torch.full((GUARD + data_cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (2 * (rec_cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    cl = (ctypes.c_uint64 * max(3 * len(where), 3))(*(w for c in where for w in c))
    eng._order()
    tail = (b"".join(pats), sizes, len(pats), syntax, NL, mode, cl, len(where), offset, length, staging, arr if rec_cap else None, rec_cap, ctypes.byref(n),
            buf.data_ptr() + GUARD, data_cap, ctypes.byref(ds))
    if handle is None:
        st = zra.load().ZraHipExtractRecordsWhere(eng.h, d.data_ptr(), size, *tail).tup()
    else:
        st = zra.load().ZraHipArchiveExtractRecordsWhere(handle.h, *tail).tup()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().tobytes()
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + data_cap:] == b"\xEE" * GUARD, ("guard", st, data_cap, rec_cap, mode, offset, length, staging)
    return st, n.value, ds.value, bytes(arr), host[GUARD:GUARD + data_cap]


def _check(eng, zra, d, size, c, where, lo=0, hi=None, staging=0, modes=(False, True), syntax=0, matches=None, slack=5, nonempty=True, the_grep=True):
    """one extract per mode of [lo, hi) of the case against the model. Returns {invert: (selected, packed)}."""
    data, fs, pats = c["data"], c["fs"], c["pats"]
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    out = {}
    for inv in modes:
        recs, sel, nm, packed = SH.model(c, where, inv, lo, hi, matches=matches)
        tag = (c["name"], where, lo, hi, staging, inv)
        if the_grep:
            assert eng.grep(d.data_ptr(), size, pats, where=where, invert=inv, offset=lo, length=length, staging_bytes=staging, syntax=syntax) == (len(sel), sel), tag
        others = (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats())
        st, n, ds, mem, got = _raw(eng, zra, d, size, pats, where, len(packed) + slack, len(sel) + 1, int(inv), lo, MAXU64 if hi is None else hi - lo, staging, syntax)
        print("extract_where", tag, "status", st, "selected", n, "model", len(sel), "bytes", ds, "model", len(packed))
        assert (st, n, ds) == ((0, 0), len(sel), len(packed)), (tag, st, n, ds, len(sel), len(packed))
        if got[:ds] != packed:
            bad = next(i for i in range(ds) if got[i] != packed[i])
            raise AssertionError((tag, "first wrong byte", bad, got[max(0, bad - 8):bad + 8], packed[max(0, bad - 8):bad + 8]))
        assert X._pairs(mem, n) == sel and mem[16 * n:] == b"\xEE" * (16 * (len(sel) + 3 - n)), tag
        s = eng.extract_stats()
        shortest = min(len(p) for p in pats) if matches is None else 1
        if end == lo or (end - lo < shortest and not WM.selected(where, 0, inv)):
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == X._stats(U, fs, lo, end, staging, len(recs), len(sel), len(packed), nm), (tag, s)
        assert (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats()) == others, tag
        out[inv] = (sel, packed)
    if nonempty and len(modes) == 2:
        assert out[False][0] and out[True][0], (c["name"], where, lo, hi, "a test that selects nothing shows nothing")
    return out


def _arc(eng, zra, c, level=3):
    """the case's archive on the device, written once"""
    if "_arc" not in c:
        c["_arc"] = _compress(eng, zra, c["data"], level, c["fs"], True)
    return c["_arc"], _dev(c["_arc"])


# ---- 1
@pytest.mark.parametrize("k", range(len(SH.TINY_WHERE)))
def test_frame_size_4_one_slot_every_record_crosses_passes(zra, gpu_engine, k):
    """the set, the packed offset and the provisional tail travel in the carried words: one frame per pass, then the same as one pass"""
    c = SH.frame_size_4()
    arc, d = _arc(gpu_engine, zra, c)
    where = SH.TINY_WHERE[k]
    one = _check(gpu_engine, zra, d, len(arc), c, where, staging=1, slack=len(c["data"]), nonempty=k != 3)
    assert gpu_engine.extract_stats()["passes"] == -(-len(c["data"]) // 4)
    whole = _check(gpu_engine, zra, d, len(arc), c, where, staging=0, nonempty=k != 3)
    assert one == whole
    if k == 0:
        assert c["late"] in one[False][0]                                       # copied provisionally, selected passes later
    if k == 1:
        assert c["late"] in one[True][0] and c["late"] not in one[False][0]     # copied provisionally, unselected passes later
    if k == 3:
        assert one[False][0] == GM.records(c["data"]) and one[True] == ([], b"")
    if k == 4:
        assert c["turn"] in one[False][0]


# ---- 2
@pytest.mark.parametrize("dist,what", [(64, "next trip"), (2048, "next wave"), (8192, "next tile"), (16384, "across a delimiter-free tile")])
def test_sets_across_every_seam_with_bytes(zra, gpu_engine, dist, what):
    """The long record's early bytes lie in trips, waves, tiles and (at staging 2 * FS) passes in front of the one where its selection
    is decided: the packed text holds them iff the model does."""
    for has_a, has_b in ((True, True), (False, True), (True, False)):
        c = SH.seam(dist, has_a, has_b)
        arc, d = _arc(gpu_engine, zra, c)
        big = c["big"]
        for staging in (0, 2 * FS):
            both = _check(gpu_engine, zra, d, len(arc), c, [(0b011, 0, 0)], staging=staging, slack=len(c["data"]))
            assert (big in both[False][0]) == (has_a and has_b) and (big in both[True][0]) != (has_a and has_b), (what, staging, has_a, has_b)
            a_not_b = _check(gpu_engine, zra, d, len(arc), c, [(0b001, 0, 0b010)], staging=staging, modes=(False,), slack=len(c["data"]))
            assert (big in a_not_b[False][0]) == (has_a and not has_b), (what, staging, has_a, has_b)
            no_c = _check(gpu_engine, zra, d, len(arc), c, [(0, 0, 0b100)], staging=staging, modes=(False,), slack=len(c["data"]))
            assert big in no_c[False][0] and c["c_left"] not in no_c[False][0] and c["c_right"] not in no_c[False][0]


@pytest.mark.parametrize("has_c,has_a", [(True, True), (True, False), (False, False)])
def test_a_selection_that_turns_twice_is_decided_at_the_delimiter(zra, gpu_engine, has_c, has_a):
    c = SH.seam_turns(has_c, has_a)
    arc, d = _arc(gpu_engine, zra, c)
    for staging in (0, 2 * FS):
        out = _check(gpu_engine, zra, d, len(arc), c, SH.NONMONO, staging=staging, slack=len(c["data"]))
        assert (c["big"] in out[False][0]) == (has_a or not has_c) and (c["big"] in out[True][0]) != (has_a or not has_c), (staging, has_c, has_a)


# ---- 3
def test_several_records_and_patterns_inside_one_trip(zra, gpu_engine):
    c = SH.one_trip()
    arc, d = _arc(gpu_engine, zra, c)
    sizes = set()
    for k, where in enumerate(c["wheres"]):
        out = _check(gpu_engine, zra, d, len(arc), c, where, staging=(0, 3 * FS)[k & 1], nonempty=False)
        sizes.add(len(out[False][0]))
    assert len(sizes) > 4, sizes


# ---- 4
def test_64_patterns_random_predicates(zra, gpu_engine):
    c = SH.wide()
    arc, d = _arc(gpu_engine, zra, c)
    sizes = set()
    for k, where in enumerate(c["wheres"]):
        lo, hi = c["ranges"][k % len(c["ranges"])]
        out = _check(gpu_engine, zra, d, len(arc), c, where, lo, hi, staging=(0, 2 * c["fs"])[k & 1], nonempty=False)
        sizes.add(len(out[False][0]))
    assert len(sizes) > 4, sizes


# ---- 5
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_the_plain_predicates_are_the_plain_extract(zra, gpu_engine, which):
    import torch
    c = SH.frame_size_4() if which == "tiny" else SH.wide()
    arc, d = _arc(gpu_engine, zra, c)
    pats, fs = c["pats"], c["fs"]
    full = WM.full(len(pats))
    cap = len(c["data"]) + 64
    a, b = torch.empty(cap, dtype=torch.uint8, device="cuda:0"), torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    for staging in (0, fs):
        for inv in (False, True):
            plain = gpu_engine.extract(d.data_ptr(), len(arc), pats, a.data_ptr(), cap, invert=inv, staging_bytes=staging, max_records=1 << 16)
            ps = gpu_engine.extract_stats()
            assert ps["selected"] == plain[0] > 0
            # any pattern, with the call's own invert; no pattern, with the opposite one
            for where, winv in (([(0, full, 0)], inv), ([(0, 0, full)], not inv)):
                got = gpu_engine.extract(d.data_ptr(), len(arc), pats, b.data_ptr(), cap, invert=winv, staging_bytes=staging, max_records=1 << 16, where=where)
                assert got == plain and gpu_engine.extract_stats() == ps, (which, staging, inv, where, got[:2], plain[:2])
                assert torch.equal(a[:plain[1]], b[:plain[1]]), (which, staging, inv, where)


# ---- 6
@pytest.mark.parametrize("k", range(len(SH.LANES_WHERE)))
def test_look_ahead_beyond_one_scan_lanes_run(zra, gpu_engine, k):
    c = SH.lanes()
    arc, d = _arc(gpu_engine, zra, c, level=1)
    out = _check(gpu_engine, zra, d, len(arc), c, SH.LANES_WHERE[k])
    assert gpu_engine.extract_stats()["passes"] == 1
    three, four, group = c["stretches"]
    if k == 0:                                                                 # A and B without C, or D without C
        assert three in out[False][0] and four in out[True][0] and group in out[True][0]
    else:
        assert three in out[False][0] and four in out[False][0] and group in out[True][0]


# ---- 7
@pytest.mark.parametrize("kind", ["last", "first", "both", "only", "none"])
def test_delimiter_positions(zra, gpu_engine, kind):
    c = SH.delimiters(kind)
    arc, d = _arc(gpu_engine, zra, c)
    for where in SH.DELIM_WHERE:
        for staging in (0, 3 * FS):
            _check(gpu_engine, zra, d, len(arc), c, where, staging=staging, nonempty=kind in ("last", "first", "both"), slack=64)
    _check(gpu_engine, zra, d, len(arc), c, SH.DELIM_WHERE[1], 63, 2 * SH.TILE + 1, staging=FS, nonempty=False)


# ---- 8
def test_capacity(zra, gpu_engine):
    c = SH.wide()
    arc, d = _arc(gpu_engine, zra, c)
    pats, fs, U = c["pats"], c["fs"], len(c["data"])
    where = [(0b11, 0, 0), (0, 0b1100, 0b10000)]
    for mode in (0, 1):
        recs, sel, nm, packed = SH.model(c, where, bool(mode))
        total, size = len(sel), len(packed)
        assert total > 8 and gpu_engine.grep(d.data_ptr(), len(arc), pats, where=where, invert=bool(mode)) == (total, sel)
        for staging in (0, fs):
            # the sizing call, a list one entry short, data one byte short: what the call needs, nothing listed
            for dcap, rcap in ((0, 0), (size + 9, total - 1), (size - 1, total), (size - 1, 0)):
                st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, where, dcap, rcap, mode=mode, staging=staging)
                tag = (mode, staging, dcap, rcap)
                assert (st, n, ds) == (TOO_SMALL, total, size), (tag, st, n, ds)
                assert mem == b"\xEE" * (16 * (rcap + 2)), tag                   # hRecords untouched
                assert got[:min(dcap, size)] == packed[:min(dcap, size)] or dcap == 0, tag
                assert gpu_engine.extract_stats() == ZERO, tag
            # fitting: exactly, and without a list
            for dcap, rcap in ((size, total), (size, 0), (size + 100, total + 5)):
                st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, where, dcap, rcap, mode=mode, staging=staging)
                tag = (mode, staging, dcap, rcap)
                assert (st, n, ds) == ((0, 0), total, size) and got[:size] == packed, (tag, st, n, ds)
                assert X._pairs(mem, min(rcap, total) if rcap else 0) == (sel if rcap else []), tag
                assert mem[16 * (total if rcap else 0):] == b"\xEE" * (16 * (rcap + 2 - (total if rcap else 0))), tag
                assert gpu_engine.extract_stats() == X._stats(U, fs, 0, U, staging, len(recs), total, size, nm), tag


# ---- 9
def test_expressions(zra, gpu_engine):
    c = SH.expressions()
    arc, d = _arc(gpu_engine, zra, c)
    syntax = zra.PATTERN_FOLD_CASE | zra.PATTERN_CLASSES
    matches = EM.set_matches(c["data"], EM.compile(c["pats"], syntax, NL))
    assert len({i for _, i in matches}) == 3
    for where in ([(0b011, 0, 0)], [(0, 0b110, 0b001)]):
        for staging in (0, 2 * FS):
            out = _check(gpu_engine, zra, d, len(arc), c, where, staging=staging, syntax=syntax, matches=matches)
            assert len(out[False][0]) > 5 and len(out[True][0]) > 5


# ---- 10
def test_shortcut_and_statuses(zra, gpu_engine):
    import torch
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    p = next(q for q in range(5 * fs + 100, 6 * fs) if NL not in data[q - 3:q + 9])
    pats = [data[p:p + 6], b"\xFF\xFE\xFD"]
    c = SH.case("statuses", data, fs, pats)
    arc, d = _arc(gpu_engine, zra, c)
    for lo, hi in ((p, p + 2), (12 * fs - 1, 12 * fs)):
        for staging in (0, fs):
            out = _check(gpu_engine, zra, d, len(arc), c, [(0b01, 0, 0)], lo, hi, staging, nonempty=False)   # false on the empty set: not decoded; inverted: scanned
            assert out[False] == ([], b"") and out[True][0] == GM.records(data, NL, lo, hi) and gpu_engine.extract_stats()["decoded"] == 1
            _check(gpu_engine, zra, d, len(arc), c, [(0b01, 0, 0)], lo, hi, staging, modes=(False,))
            assert gpu_engine.extract_stats() == dict(ZERO, frames=12)
            out = _check(gpu_engine, zra, d, len(arc), c, [(0, 0, 0b01)], lo, hi, staging, modes=(False,))   # true on the empty set: scanned, every record
            assert out[False][0] == GM.records(data, NL, lo, hi) and gpu_engine.extract_stats()["decoded"] == 1
    _check(gpu_engine, zra, d, len(arc), c, [(0, 0, 0)], p, p, nonempty=False)
    assert gpu_engine.extract_stats() == dict(ZERO, frames=12)
    # a frame with a flipped byte: a status, nothing listed
    bad = _flip_mid(arc, [7])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs):
            st, n, ds, mem, _ = _raw(gpu_engine, zra, db, len(bad), pats, [(0b01, 0, 0b10)], 13 * fs, 6, mode=mode, staging=staging)
            assert (st, n, ds, mem) == ((1, want[7]), 0, 0, b"\xEE" * 128), (mode, staging, st, n, ds)
            assert gpu_engine.extract_stats() == ZERO
    _check(gpu_engine, zra, db, len(bad), c, [(0b01, 0, 0b10)], 0, 7 * fs, nonempty=False)       # the same damage outside the range
    # rule 1 with an engine: nothing decoded, nothing written
    for where in ([(0b100, 0, 0)], [(1, 0, 1)], [(0, 1, 1)], [(0, 0, 0)] * 9, []):
        st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, where, 64, 2)
        assert (st, n, ds, mem, got) == ((1, 42), 0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO, where
    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, [(1, 0, 0)], 64, 2, mode=2)
    assert (st, n, ds, mem, got) == ((1, 42), 0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO
    # rule 2: dData inside the archive, one byte of overlap at either end; the archive is only read
    whole = torch.full((512 + len(arc) + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
    whole[512:512 + len(arc)] = d
    P = whole.data_ptr() + 512
    L = zra.load()
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
    sizes = (ctypes.c_uint32 * 2)(6, 3)
    cl = (ctypes.c_uint64 * 3)(1, 0, 0)
    for dptr, dcap in ((P + 100, 50), (P - 256, len(arc) + 512), (P - 10, 11), (P + len(arc) - 1, 10)):
        n.value, ds.value = 0x1234, 0x5678
        st = L.ZraHipExtractRecordsWhere(gpu_engine.h, P, len(arc), b"".join(pats), sizes, 2, 0, NL, 0, cl, 1, 0, MAXU64, 0, None, 0, ctypes.byref(n), dptr, dcap, ctypes.byref(ds)).tup()
        assert (st, n.value, ds.value) == ((1, 42), 0, 0) and gpu_engine.extract_stats() == ZERO, (dptr - P, dcap)
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert host[:512] == b"\xEE" * 512 and host[512 + len(arc):] == b"\xEE" * 512 and host[512:512 + len(arc)] == arc


@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames of the range resident"""
    import torch
    fs = 1000
    data, pats = AS._content(77, fs)
    U = len(data)
    c = SH.case("handle", data, fs, pats)
    arc, d = _arc(gpu_engine, zra, c)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, U, warm, slots)
    out = torch.empty(U + 64, dtype=torch.uint8, device="cuda:0")
    try:
        where = [(0b100000, 0, 0b1000000), (0, 0b11111, 0)]
        for lo, hi in ((0, U), (6 * fs + fs // 2, 10 * fs + fs // 2)):
            for staging in (0, 3 * fs):
                kw = dict(offset=lo, length=hi - lo, staging_bytes=staging, max_records=AS.MAXREC)
                before = h.stats()
                s0 = h.scan_stats()
                plain = h.extract(pats, out.data_ptr(), U + 64, **kw)
                s1 = h.scan_stats()
                got = h.extract(pats, out.data_ptr(), U + 64, where=where, **kw)
                s2 = h.scan_stats()
                hs = gpu_engine.extract_stats()
                text = out[:got[1]].cpu().numpy().tobytes()
                recs, sel, nm, packed = SH.model(c, where, False, lo, hi)
                assert got == (len(sel), len(packed), sel) and text == packed and got[0] > 0 and plain[0] > 0, (slots, lo, staging)
                assert h.grep(pats, where=where, offset=lo, length=hi - lo, staging_bytes=staging) == (len(sel), sel), (slots, lo, staging)
                st, n, ds, mem, raw = _raw(gpu_engine, zra, d, len(arc), pats, where, len(packed) + 5, len(sel) + 1, 1, lo, hi - lo, staging, handle=h)
                inv = SH.model(c, where, True, lo, hi)
                assert (st, n, ds, raw[:ds], X._pairs(mem, n)) == ((0, 0), len(inv[1]), len(inv[3]), inv[3], inv[1]), (slots, lo, staging)
                gpu_engine.extract(d.data_ptr(), len(arc), pats, out.data_ptr(), U + 64, where=where, **kw)
                es = gpu_engine.extract_stats()
                staged, decoded, dec_bytes = AS._split(warm, fs, U, lo, hi)
                assert hs == dict(es, decoded=decoded, content_bytes=dec_bytes), (hs, es)
                # the handle's counters move as for the plain extract on the same range
                assert {k: s2[k] - s1[k] for k in s1 if k.endswith("total") or k == "scans"} == {k: s1[k] - s0[k] for k in s1 if k.endswith("total") or k == "scans"}
                assert (s2["staged"], s2["decoded"], s2["passes"]) == (s1["staged"], s1["decoded"], s1["passes"]) and (s2["staged"], s2["decoded"]) == (staged, decoded)
                assert h.stats() == before                                     # a scan is not a read
        with pytest.raises(zra.ZraError) as e:                                  # dData inside the archive
            h.extract(pats, d.data_ptr() + 8, 16, where=where)
        assert (e.value.zra, e.value.zstd) == (1, 42)
        # dData over the arena (ZraHipDebugArchiveArena tells where it lies): one byte into either end and all of it are refused before
        # anything is decoded or written; touching it at either end is no overlap, which rule 1 shows without handing such a buffer over
        base, size = h.arena_range()
        assert (base != 0, size) == (slots != 0, slots * fs)
        if slots:
            L = zra.load()
            sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
            cl = (ctypes.c_uint64 * 6)(*(w for c_ in where for w in c_))
            n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
            before, s0 = h.stats(), h.scan_stats()
            for dptr, dcap in ((base + size - 1, 64), (base - 63, 64), (base, size), (base + 8, 16), (base - 8, size + 16)):
                n.value, ds.value = 0x1234, 0x5678
                st = L.ZraHipArchiveExtractRecordsWhere(h.h, b"".join(pats), sizes, len(pats), 0, NL, 0, cl, 2, 0, MAXU64, 0, None, 0, ctypes.byref(n), dptr, dcap,
                                                        ctypes.byref(ds)).tup()
                assert (st, n.value, ds.value) == ((1, 42), 0, 0) and gpu_engine.extract_stats() == ZERO, (dptr - base, dcap)
            assert (h.stats(), h.scan_stats()) == (before, s0)
            # the arena was not written: the resident frames still stage the content
            recs, sel, nm, packed = SH.model(c, where, False, 0, U)
            assert h.extract(pats, out.data_ptr(), U + 64, where=where, max_records=AS.MAXREC) == (len(sel), len(packed), sel)
            assert out[:len(packed)].cpu().numpy().tobytes() == packed
    finally:
        h.close()


# ---- 11
def test_cli_mode_gxw(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta two\n\ngamma one two\ndelta" + b"\n" + b"x;y;one;z" * 3
    c = SH.case("cli", data, 16, [b"one", b"two"])
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc, p_out = tmp_path / "lines.zra", tmp_path / "out.txt"
    p_arc.write_bytes(arc)

    def run(mode, *args):
        return subprocess.run([TOOL, mode, str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    for args, pats, where, inv in ((("-w", "+0,-1", "one", "two"), [b"one", b"two"], [(1, 0, 2)], False),
                                   (("-v", "-w", "+0,-1", "one", "two"), [b"one", b"two"], [(1, 0, 2)], True),
                                   (("-w", "+0,+1", "-w", "?2", "-F", "one", "two", "hex:" + b"delta".hex()), [b"one", b"two", b"delta"], [(3, 0, 0), (0, 4, 0)], False),
                                   (("-i", "-w", "?0,?1,-2", "ALPHA", "b[a-e]ta", "z"), [b"alpha", b"beta", b"z"], [(0, 3, 4)], False)):
        packed = SH.model(c, where, inv, pats=pats)[3]
        r = run("gxw", *args)
        assert r.returncode == 0 and r.stdout == packed and packed, (args, r.stdout, r.stderr)
    assert SH.model(c, [(1, 0, 2)], False)[3] == b"alpha one\nx;y;one;zx;y;one;zx;y;one;z\n"
    # the plain predicate prints what gx prints; -o writes the same bytes to a file
    plain = run("gx", "one", "two")
    r = run("gxw", "-w", "?0,?1", "-o", p_out, "one", "two")
    assert plain.returncode == r.returncode == 0 and r.stdout == b"" and p_out.read_bytes() == plain.stdout != b""
    r = run("gxw", "-w", "+0,+1", "alpha", "beta")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    for args in (("-w", "+7", "one", "two"), ("-w", "+0,-0", "one"), ("-w", "0", "one"), ("-w", "+0,", "one"), ("-w", "+64", "one"), ("one",), ("-w", "+0"),
                 ["-w", "+0"] * 9 + ["one"]):
        r = run("gxw", *args)
        assert r.returncode == 2 and r.stdout == b"", (args, r.stdout, r.stderr)
