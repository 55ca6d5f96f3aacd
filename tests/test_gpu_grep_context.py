"""GPU tests of ZraHipGrepArchiveContext (include/zra_hip.h): the records the grep selects with `before` records in front of and
`after` records behind each of them. The yardstick everywhere is the plaintext the test generated itself, cut, scanned and given its
context on the CPU (tests/context_model.py, held against the system's grep in tests/test_context_abi.py). Every case compares the
status, the three counts, the list with its selected bits and all eight stats; a run without context is also compared with Engine.grep.
The shapes are the smallest at which each seam exists: the scan's trip is 64 positions, its wave 2,048, its tile 8,192; a pass is a
whole number of frames, one frame with staging_bytes=1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import context_model as CM
import grep_model as GM
from test_gpu_grep import _lines, _stats
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
SEL = 1 << 63
ZERO = dict(frames=0, decoded=0, content_bytes=0, records=0, selected=0, listed=0, passes=0, matches=0)
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (64, 64)]                            # (after, before)
FS = 1024


def _raw(eng, zra, d, size, pats, cap, after=0, before=0, delim=NL, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, null=False):
    """(status, (*nRecords, *nSelected, *nGroups), the bytes of a record array two entries longer than the capacity, 0xEE-filled)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ns, ng = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    eng._order()
    st = zra.load().ZraHipGrepArchiveContext(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), syntax, delim, mode, before, after, offset, length, staging,
                                             None if null else arr, cap, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(ng)).tup()
    return st, (n.value, ns.value, ng.value), bytes(arr)


def _call(eng, zra, d, size, pats, **kw):
    try:
        return ((0, 0),) + eng.grep_context(d.data_ptr(), size, pats, **kw)
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, 0, 0, []


def _check(eng, zra, d, size, data, fs, pats, pairs=PAIRS, lo=0, hi=None, staging=0, delim=NL, modes=(False, True), syntax=0, model_pats=None):
    """one call per pair and mode of [lo, hi) against the model. Returns {(after, before, invert): (listed, |S|, groups)}."""
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    out = {}
    for inv in modes:
        for after, before in pairs:
            want, nsel, groups, recs, matches = CM.context(data, model_pats or pats, delim, inv, before, after, lo, hi) if syntax == 0 or model_pats else (None,) * 5
            tag = (after, before, lo, hi, staging, inv)
            got = _call(eng, zra, d, size, pats, before=before, after=after, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging, syntax=syntax)
            assert got[:4] == ((0, 0), len(want), nsel, groups), (tag, got[:4], (len(want), nsel, groups))
            assert got[4] == want, (tag, sorted(set(got[4]) ^ set(want))[:10], got[4][:6], want[:6])
            s = eng.grep_stats()
            if end == lo or (not inv and end - lo < min(len(p) for p in (model_pats or pats))):
                assert s == dict(ZERO, frames=-(-U // fs)) and not want, (tag, s)    # nothing decoded
            else:
                assert s == _stats(U, fs, lo, end, staging, len(recs), len(want), len(want), matches), (tag, s)
            if after == 0 and before == 0:
                plain = eng.grep(d.data_ptr(), size, pats, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging, syntax=syntax)
                assert (plain[0], plain[1]) == (len(want), [(o, n) for o, n, _ in want]) and all(b for _, _, b in want) and nsel == len(want), tag
            out[(after, before, inv)] = (want, nsel, groups)
    return out


# ---- 1
@pytest.mark.parametrize("staging", [0, 1])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging):
    """About 260 frames of 4 bytes. With one slot a pass holds 4 bytes: many passes in a row end no record (the 60-byte line spans 15 of
    them) while records are pending in front of them."""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"acde"), size=60).astype(np.uint8))
    data = _lines(rng, 500) + b"\n" + long_line + b"\n" + _lines(rng, 480)
    pats = [b"bbc", b"cdae", long_line[5:45], b"zz"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    res = _check(gpu_engine, zra, _dev(arc), len(arc), data, 4, pats, staging=staging)
    want, nsel, groups = res[(2, 3, False)]
    assert (501, 60, True) in want and nsel > 5 and groups > 3 and len(want) > nsel + 10 and any(not b for _, _, b in want)
    assert gpu_engine.grep_stats()["passes"] == (-(-len(data) // 4) if staging else 1)


# ---- 2
def test_pending_records_one_record_per_pass(zra, gpu_engine):
    """Frames of 16 bytes, one per pass. Segments of whole frames: A one line of 15 bytes, B two of 7, C four of 3, D one of 47 (two
    passes that end no record); an X selects a line. before = 3: the pending set grows over passes without a selected record and is
    trimmed to the last 3 (5 A in front of the first X), is kept whole (an X alone in its pass), kept in part (B: one unselected
    record of the pass in front of its X), dropped whole (C: three in front), stays smaller than 3 (two A between two X), waits
    through D's passes, and is dropped by the last pass (6 A behind the last X)."""
    def seg(kind, *sel):
        n, m = dict(A=(1, 15), B=(2, 7), C=(4, 3), D=(1, 47))[kind]
        return b"".join((b"X" if k in sel else b"u") + b"v" * (m - 1) + b"\n" for k in range(n))

    parts = [seg("A")] * 5 + [seg("A", 0)] + [seg("A")] * 4 + [seg("B", 1)] + [seg("A")] * 4 + [seg("C", 3)] + [seg("A")] * 2 + [seg("A", 0)] + \
            [seg("A")] * 2 + [seg("D")] + [seg("A", 0)] + [seg("A"), seg("D"), seg("B"), seg("C", 0)] + [seg("A")] * 6
    data = b"".join(parts)
    assert len(data) % 16 == 0
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    d = _dev(arc)
    for staging in (1, 0, 48):
        res = _check(gpu_engine, zra, d, len(arc), data, 16, [b"X"], pairs=[(0, 3), (1, 3), (2, 3), (5, 3), (0, 1), (64, 64)], staging=staging)
        want, nsel, groups = res[(0, 3, False)]
        assert nsel == 6 and sum(1 for o, n, b in want if not b) == 3 + 3 + 3 + 2 + 3 + 3 and groups == 4
    assert gpu_engine.grep_stats()["passes"] == -(-len(data) // 48)
    _check(gpu_engine, zra, d, len(arc), data, 16, [b"X"], pairs=[(1, 3)], lo=16 * 3 + 5, hi=len(data) - 16 * 4 - 7, staging=1)


# ---- 3
def _with_delimiters_at(rng, targets, total):
    """short lines over `abc`; for every target offset a line that holds QQ and whose newline lies exactly there"""
    out = bytearray()
    for t in sorted(targets):
        while len(out) + 40 < t - 12:
            out += bytes(rng.choice(list(b"abc"), size=int(rng.randint(0, 13))).astype(np.uint8)) + b"\n"
        out += b"c" * (t - 12 - len(out) - 1) + b"\n" if t - 12 - len(out) >= 1 else b""
        out += b"QQ" + b"a" * (t - len(out) - 2) + b"\n"
        assert out[t] == NL and len(out) == t + 1
    while len(out) < total:
        out += bytes(rng.choice(list(b"abc"), size=int(rng.randint(0, 13))).astype(np.uint8)) + b"\n"
    return bytes(out[:total - 1]) + b"b"


def test_context_crosses_every_seam(zra, gpu_engine):
    """A selected record's delimiter at position 63, 2,047 and 8,191 of a tile (the last lane of a trip, of a wave, of a tile) and at
    the last byte of a pass of two frames (10,239; 16,383 is both), its context records on the far side in each direction."""
    targets = [63, 2047, 8191, 10239, 16383]
    data = _with_delimiters_at(np.random.RandomState(3), targets, 18 * FS + 77)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    for staging in (0, 2 * FS):
        res = _check(gpu_engine, zra, d, len(arc), data, FS, [b"QQ"], pairs=[(2, 3), (1, 0), (0, 1), (64, 64), (0, 0)], staging=staging)
        want, nsel, groups = res[(2, 3, False)]
        ends = {o + n for o, n, b in want if b}
        assert ends == set(targets) and nsel == 5 and groups == 5 and len(want) > 5 * 5


@pytest.mark.parametrize("after,before", [(2, 3), (64, 64), (0, 5), (5, 0)])
def test_two_selected_records_a_gap_apart(zra, gpu_engine, after, before):
    """after + before unselected records between two selected ones: one group, all of the gap; one more: two groups, one record left out."""
    g = after + before
    lines = [b"u%d" % k for k in range(70)] + [b"X"] + [b"g%d" % k for k in range(g)] + [b"X"] + [b"w%d" % k for k in range(140)] + [b"X"] + \
            [b"h%d" % k for k in range(g + 1)] + [b"X"] + [b"t%d" % k for k in range(70)]
    data = b"\n".join(lines) + b"\n"
    arc = _compress(gpu_engine, zra, data, 3, 256, True)
    for staging in (0, 1):
        res = _check(gpu_engine, zra, _dev(arc), len(arc), data, 256, [b"X"], pairs=[(after, before)], staging=staging, modes=(False,))
        want, nsel, groups = res[(after, before, False)]
        assert nsel == 4 and groups == 3 and len(want) == 4 + 2 * g + 2 * (after + before)


# ---- 4
def test_a_tile_and_a_pass_without_a_delimiter(zra, gpu_engine):
    """A selected record, a record of 20,000 bytes (whole tiles, and with two frames to a pass whole passes, without a delimiter), short
    records: the long record is after-context. Then the same the other way round: it is before-context, pending while its passes go by."""
    rng = np.random.RandomState(9)
    body = _data(rng, 20000).replace(b"\n", b"\x0B").replace(b"Q", b"q")
    short = lambda n: _lines(rng, n, b"abc")[:-1] + b"\n"
    data = short(300) + b"QQ one\n" + body + b"\n" + short(200) + body[:9000] + b"\n" + b"two QQ\n" + short(150) + b"end"
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    for staging in (0, 2 * FS, 1):
        res = _check(gpu_engine, zra, d, len(arc), data, FS, [b"QQ"], pairs=[(2, 2), (1, 0), (0, 1), (64, 64)], staging=staging)
        want = res[(2, 2, False)][0]
        assert sorted(n for _, n, _ in want)[-2:] == [9000, 20000]


# ---- 4b
def test_more_tiles_than_scan_lanes(zra, gpu_engine):
    """8.4 MiB in frames of 64 KiB: 1,030 tiles, so a lane of the one-workgroup scan walks two tiles forwards and backwards and a
    workgroup's eight tiles are one of 129 groups; with passes of 16 frames the same content takes nine passes of 128 tiles. Lines of
    200 bytes or so, one stretch of 100,000 bytes without a newline (whole tiles without a delimiter) with a match in it."""
    fs = 65536
    U = 1029 * 8192 + 5000
    rng = np.random.RandomState(67)
    a = rng.randint(32, 127, size=U).astype(np.uint8)
    a[rng.randint(0, U, size=U // 200)] = NL
    a[3000000:3100000][a[3000000:3100000] == NL] = 32
    data = a.tobytes()
    pats = [data[123456:123459], data[3050000:3050012], data[8000000:8000004]]
    assert NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 1, fs, True)
    d = _dev(arc)
    for staging in (0, 16 * fs):
        res = _check(gpu_engine, zra, d, len(arc), data, fs, pats, pairs=[(2, 3), (64, 64)], staging=staging, modes=(False,))
        want, nsel, groups = res[(64, 64, False)]
        assert any(n >= 100000 and b for _, n, b in want) and nsel == 15 and groups == 15 and len(want) == 15 * 129
        assert gpu_engine.grep_stats()["passes"] == (9 if staging else 1)
    _check(gpu_engine, zra, d, len(arc), data, fs, pats, pairs=[(1, 1)], staging=16 * fs, modes=(True,))


def test_random_small_shapes(zra, gpu_engine):
    """Forty small archives: lines of 0 to 12 bytes over four letters, frames of 64 bytes, one, three or all frames to a pass, a range
    that begins and ends anywhere, every context width up to 64 and a selection density from a record in two to one in sixty."""
    rng = np.random.RandomState(71)
    for case in range(40):
        n = int(rng.randint(200, 3000))
        data = _lines(rng, n, b"abcd", 12)
        pats = [b"ab", b"ca"][:1 + case % 2] if case % 4 else [b"abcd", b"dcba"]
        arc = _compress(gpu_engine, zra, data, 3, 64, True)
        lo = int(rng.randint(0, n // 3)) if case % 3 else 0
        hi = int(rng.randint(2 * n // 3, n + 1)) if case % 3 == 2 else None
        pair = (int(rng.randint(0, 65)), int(rng.randint(0, 65))) if case % 2 else (int(rng.randint(0, 5)), int(rng.randint(0, 5)))
        _check(gpu_engine, zra, _dev(arc), len(arc), data, 64, pats, pairs=[pair], lo=lo, hi=hi, staging=(1, 192, 0)[case % 3], modes=(bool(case & 1),))


# ---- 5
@pytest.fixture(scope="module")
def text(zra, gpu_engine):
    """6 frames of 1,024 bytes and a last one of 300: lines of _data's alphabet, no newline at the end"""
    U = 6 * FS + 300
    a = bytearray(_data(np.random.RandomState(33), U))
    a[U - 1] = 2
    data = bytes(a)
    pats = [data[700:703], data[5 * FS + 40:5 * FS + 42]]
    assert NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    return dict(data=data, arc=arc, d=_dev(arc), pats=pats, U=U)


def test_capacity(zra, gpu_engine, text):
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
    after, before = 1, 4
    want, nsel, groups, recs, matches = CM.context(data, pats, NL, False, before, after)
    total = len(want)
    inside = next(k for k in range(2, total) if not want[k][2] and not want[k - 1][2] and not want[k + 1][2] and want[k + 2][2])   # in a run of before-context
    assert total > 12 and groups > 2
    for cap in (0, 1, inside + 1, total - 1, total, total + 5):
        for staging in (0, FS, 1):
            st, counts, mem = _raw(gpu_engine, zra, d, len(arc), pats, cap, after, before, staging=staging, null=cap == 0)
            k = min(total, cap)
            assert (st, counts) == ((0, 0), (total, nsel, groups)), (cap, staging, st, counts)
            got = np.frombuffer(mem[:16 * k], dtype="<u8").reshape(-1, 2)
            assert [(int(o), int(n) & ~SEL, bool(int(n) & SEL)) for o, n in got.tolist()] == want[:k], (cap, staging)
            assert mem[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), (cap, staging)
            assert gpu_engine.grep_stats() == _stats(U, FS, 0, U, staging, len(recs), total, k, matches), (cap, staging)


# ---- 6
def test_range_ends_inside_records(zra, gpu_engine, text):
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
    nl = [p for p in range(U) if data[p] == NL]
    hit = data.find(pats[0])
    for staging in (0, FS, 1):
        for lo, hi in ((nl[3] + 2, nl[-4] - 1), (hit - 30, hit + 60), (hit + 1, hit + 200), (nl[10], nl[40] + 1), (nl[10] + 1, nl[40]), (5, 5), (U - 1, U), (hit, hit + 2)):
            res = _check(gpu_engine, zra, d, len(arc), data, FS, pats, pairs=[(2, 3), (64, 64), (0, 0)], lo=lo, hi=hi, staging=staging)
            want = res[(64, 64, True)][0]
            if hi > lo and want:
                assert want[0][0] == lo and want[-1][0] + want[-1][1] in (hi, hi - 1)      # context stops at both ends; the clipped record is reported clipped


# ---- 7
def test_degenerate_selections(zra, gpu_engine):
    rng = np.random.RandomState(12)
    data = _lines(rng, 3000) + b"\n\n\n" + _lines(rng, 2500, b"ab") + b"\n" * 70 + _lines(rng, 600)
    arc = _compress(gpu_engine, zra, data, 3, 512, True)
    d = _dev(arc)
    recs = GM.records(data)
    for staging in (0, 1):
        res = _check(gpu_engine, zra, d, len(arc), data, 512, [b"\xFF\xFE"], pairs=[(2, 3), (64, 64)], staging=staging)   # nothing selected; inverted: everything
        assert res[(2, 3, False)] == ([], 0, 0) and res[(2, 3, True)] == ([(o, n, True) for o, n in recs], len(recs), 1)
        res = _check(gpu_engine, zra, d, len(arc), data, 512, [b"a", b"b", b"c", b"d", b"e"], pairs=[(1, 1), (0, 64)], staging=staging)   # inverted: the empty records
        assert all(n == 0 for _, n, b in res[(1, 1, True)][0] if b) and res[(1, 1, True)][1] > 70
    zdata = data.replace(b"\n", b"\x00")
    arc = _compress(gpu_engine, zra, zdata, 3, 512, True)
    _check(gpu_engine, zra, _dev(arc), len(arc), zdata, 512, [b"bb", b"cda"], pairs=[(2, 3)], delim=0, staging=512 * 3)


def test_fold_case_and_classes(zra, gpu_engine):
    lines = [b"alpha", b"Beta 17", b"gamma", b"delta", b"BETA 2x", b"eps", b"zeta", b"beta 99", b"eta"] * 40
    data = b"\n".join(lines) + b"\n"
    arc = _compress(gpu_engine, zra, data, 3, 256, True)
    d = _dev(arc)
    # `beta [0-9][0-9]` folded: the lines Beta 17 and beta 99, as literal patterns for the model
    for staging in (0, 256):
        got = _call(gpu_engine, zra, d, len(arc), [b"beta [0-9][0-9]"], before=1, after=2, staging_bytes=staging, syntax=zra.PATTERN_FOLD_CASE | zra.PATTERN_CLASSES)
        want, nsel, groups, recs, _ = CM.context(data, [b"Beta 17", b"beta 99"], NL, False, 1, 2)
        assert got == ((0, 0), len(want), nsel, groups, want) and nsel == 80
        assert gpu_engine.grep_stats() == _stats(len(data), 256, 0, len(data), staging, len(recs), len(want), len(want), 80)


# ---- 8
def test_a_damaged_frame(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    pats = [data[5 * fs + 100:5 * fs + 103].replace(b"\n", b"\x01"), data[9 * fs + 50:9 * fs + 52].replace(b"\n", b"\x01")]
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs, 1):
            st, counts, mem = _raw(gpu_engine, zra, db, len(bad), pats, 6, 2, 3, mode=mode, staging=staging)
            assert (st, counts, mem) == ((1, want[7]), (0, 0, 0), b"\xEE" * 128), (mode, staging, st, counts)
            assert gpu_engine.grep_stats() == ZERO
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), data, fs, pats, pairs=[(2, 3)], lo=lo, hi=hi)


def test_refusals_with_an_engine(zra, gpu_engine, text):
    d, size, pats = text["d"], len(text["arc"]), text["pats"]
    for kw in (dict(before=65), dict(after=65), dict(mode=2), dict(mode=3, before=1), dict(delim=pats[0][1]), dict(syntax=4)):
        st, counts, mem = _raw(gpu_engine, zra, d, size, pats, 2, **kw)
        assert (st, counts, mem) == ((1, 42), (0, 0, 0), b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, kw
    sizes = (ctypes.c_uint32 * 2)(*(len(p) for p in pats))
    arr = (ctypes.c_uint64 * 8)()
    L = zra.load()
    assert L.ZraHipGrepArchiveContext(gpu_engine.h, d.data_ptr(), size, b"".join(pats), sizes, 2, 0, NL, 0, 1, 1, 0, MAXU64, 0, arr, 4, None, None, None).tup() == (1, 42)
    n = ctypes.c_uint64(7)
    assert L.ZraHipGrepArchiveContext(gpu_engine.h, d.data_ptr(), size, b"".join(pats), sizes, 2, 0, NL, 0, 1, 1, 0, MAXU64, 0, arr, 4, ctypes.byref(n), None, None).tup() == (0, 0)
    assert n.value == len(CM.context(text["data"], pats, NL, False, 1, 1)[0])     # nSelected and nGroups may be NULL
    for lo, ln in ((text["U"] + 1, 0), (0, text["U"] + 1), (text["U"], 1)):     # rule 3
        st, counts, mem = _raw(gpu_engine, zra, d, size, pats, 2, 1, 1, offset=lo, length=ln)
        assert (st, counts, mem) == ((5, 0), (0, 0, 0), b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO


# ---- 9
def test_handle_twin_with_partly_resident_frames(zra, gpu_engine, text):
    """Frames 1, 4 and 5 of 7 are resident. The answers are the engine call's; the handle's scan counters move as Archive.grep's
    (ZraHipArchiveGrepExpr) do on the same range, and a scan is not a read."""
    import torch
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
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
                h.grep(pats, offset=lo, length=length, staging_bytes=staging, syntax=zra.PATTERN_FOLD_CASE)
                s1 = h.scan_stats()
                moved = {k: s1[k] - s0[k] for k in CUM}
                assert moved["scans"] == 1 and moved["staged_total"] > 0 and moved["decoded_total"] > 0
                for after, before in ((2, 3), (64, 64), (0, 0)):
                    for inv in (False, True):
                        kw = dict(before=before, after=after, invert=inv, offset=lo, length=length, staging_bytes=staging)
                        plain = _call(gpu_engine, zra, d, len(arc), pats, **kw)
                        want = CM.context(data, pats, NL, inv, before, after, lo, hi)
                        assert plain == ((0, 0), len(want[0]), want[1], want[2], want[0]), kw
                        ps = gpu_engine.grep_stats()
                        sa = h.scan_stats()
                        got = ((0, 0),) + h.grep_context(pats, **kw)
                        sb = h.scan_stats()
                        assert got == plain, kw
                        hs = gpu_engine.grep_stats()
                        assert dict(hs, decoded=0, content_bytes=0) == dict(ps, decoded=0, content_bytes=0) and hs["decoded"] == s1["decoded"] < ps["decoded"], (hs, ps)
                        assert {k: sb[k] - sa[k] for k in CUM} == moved and {k: sb[k] for k in LAST} == {k: s1[k] for k in LAST}, (kw, sa, sb, s1)
        assert h.stats() == cache


# ---- 10
def test_cli_mode_glc(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta\n\ngamma one two\ndelta\neps\nzeta\neta\ntheta one\niota" + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "glc", str(p_arc)] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    def lines(want, nsel, groups):
        out = []
        for k, (o, n, b) in enumerate(want):
            if k and o != want[k - 1][0] + want[k - 1][1] + 1:
                out.append("--")
            out.append("%d\t%d%s" % (o, n, "\t*" if b else ""))
        return out + ["%d records, %d selected, %d groups" % (len(want), nsel, groups), ""]

    for args, pats, delim, inv, after, before in ((("-A", 1, "one"), [b"one"], NL, False, 1, 0), (("-B", 1, "-v", "one", "hex:" + b"eta".hex()), [b"one", b"eta"], NL, True, 0, 1),
                                                  (("-C", 1, "-F", "gamma"), [b"gamma"], NL, False, 1, 1), (("-d", "3b", "-A", 2, "-B", 0, "y"), [b"y"], 0x3B, False, 2, 0),
                                                  (("-i", "ONE"), [b"one"], NL, False, 0, 0), (("-C", 64, "two"), [b"two"], NL, False, 64, 64)):
        want, nsel, groups = CM.context(data, pats, delim, inv, before, after)[:3]
        r = run(*args)
        assert r.returncode == 0 and r.stdout.split("\n") == lines(want, nsel, groups) and want, (args, r.stdout, r.stderr)
        assert r.stdout.count("--\n") == groups - 1
    r = run("-C", 3, "absent")
    assert r.returncode == 1 and r.stdout == "0 records, 0 selected, 0 groups\n", (r.stdout, r.stderr)
    for args in (("-A", 65, "a"), ("-B", "x", "a"), ("-C",), ("-A", 1), (), ("a\nb",)):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
