"""GPU tests of ZraHipGrepArchive (include/zra_hip.h): the records of a content range of a device-resident archive, cut at a delimiter
byte, in which one of several byte patterns occurs, or, inverted, none. The yardstick everywhere is the plaintext the test generated
itself, cut and scanned on the CPU (tests/grep_model.py, cross-checked in tests/test_grep_abi.py); `matches` is also held against
Engine.search_multi on the same range; for a frame that does not decode, the status ZraHipDecompressRABatch gives under
ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it. Archives are written on the device. The shapes are the smallest at which each seam
exists: the scan's trip is 64 positions, its wave 2,048, its tile 8,192; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grep_model as GM
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
ZERO = dict(frames=0, decoded=0, content_bytes=0, records=0, selected=0, listed=0, passes=0, matches=0)


def _grep(eng, zra, d, size, pats, **kw):
    """((zra, zstd), n_records, [(offset, size)]) of one grep"""
    try:
        n, recs = eng.grep(d.data_ptr(), size, pats, **kw)
        return (0, 0), n, recs
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, []


def _raw(eng, zra, d, size, pats, cap, delim=NL, mode=0, offset=0, length=MAXU64, staging=0):
    """(status, *nRecords, the bytes of a record array two entries longer than the capacity, 0xEE-filled before the call)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n = ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    eng._order()
    st = zra.load().ZraHipGrepArchive(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), delim, mode, offset, length, staging, arr if cap else None, cap,
                                      ctypes.byref(n)).tup()
    return st, n.value, bytes(arr)


def _stats(U, fs, lo, end, staging, records, selected, listed, matches):
    """the eight counters of a grep of [lo, end) that decoded"""
    f0, f1 = lo // fs, (end - 1) // fs
    slots = max(1, min(65536, (staging or 4 << 30) // fs))
    return dict(frames=-(-U // fs), decoded=f1 - f0 + 1, content_bytes=min(U, (f1 + 1) * fs) - f0 * fs, records=records, selected=selected, listed=listed,
                passes=-(-(f1 - f0 + 1) // slots), matches=matches)


def _check(eng, zra, d, size, data, fs, pats, lo=0, hi=None, staging=0, delim=NL, modes=(False, True)):
    """one grep per mode of [lo, hi) against the model: status, count, list and all eight stats; `matches` also against the multi
    search of the same range. Returns {invert: selected}."""
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    nm, _, _ = eng.search_multi(d.data_ptr(), size, pats, offset=lo, length=length, staging_bytes=staging, max_matches=0)
    out = {}
    for inv in modes:
        recs, sel, matches = GM.grep(data, pats, delim, inv, lo, hi)
        tag = (lo, hi, staging, inv)
        got = _grep(eng, zra, d, size, pats, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging)
        assert got[:2] == ((0, 0), len(sel)), (tag, got[:2], len(sel))
        assert got[2] == sel, (tag, sorted(set(got[2]) ^ set(sel))[:10], got[2][:6], sel[:6])
        s = eng.grep_stats()
        if end == lo or (not inv and end - lo < min(len(p) for p in pats)):
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == _stats(U, fs, lo, end, staging, len(recs), len(sel), len(sel), matches), (tag, s)
        assert matches == nm, (tag, matches, nm)
        out[inv] = sel
    return out


def _lines(rng, n, alphabet=b"abcde", longest=30):
    """about n bytes of short lines over `alphabet`, some empty, the last one without its newline"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(list(alphabet), size=int(rng.randint(0, longest + 1))).astype(np.uint8)) + b"\n"
    return bytes(out[:n - 1]) + b"e"


# ---- 1
@pytest.mark.parametrize("staging", [0, 1])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging):
    """About 260 frames of 4 bytes. With one slot a pass holds 4 bytes: shorter than M - 1 = 39, shorter than most records, and many
    passes in a row hold no delimiter (the 60-byte line spans 15 of them)."""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"acde"), size=60).astype(np.uint8))
    data = _lines(rng, 500) + b"\n" + long_line + b"\n" + _lines(rng, 480)
    pats = [b"b", b"cda", long_line[5:45], b"zz", b"ea"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    sel = _check(gpu_engine, zra, _dev(arc), len(arc), data, 4, pats, staging=staging)
    assert (501, 60) in sel[False] and len(sel[False]) > 20 and len(sel[True]) > 10 and any(n == 0 for _, n in sel[True])
    assert gpu_engine.grep_stats()["passes"] == (-(-len(data) // 4) if staging else 1)


# ---- 2
FS = 1024
NEEDLE = b"\xF0NEEDLE\xF1"


@pytest.fixture(scope="module")
def filler():
    """32 KiB without a delimiter and without a byte of NEEDLE: the body of the long record"""
    return _data(np.random.RandomState(5), 32 << 10).replace(b"\n", b"\x0B")


@pytest.mark.parametrize("dist,what", [(64, "next trip"), (2048, "next wave"), (8192, "next tile"), (16384, "two tiles on"), (20000, "about 20 KiB")])
def test_hit_is_carried_across_every_seam(zra, gpu_engine, filler, dist, what):
    """Short records, then one long record whose only match lies 50 bytes behind its start and whose ending delimiter lies `dist`
    positions behind the match, then short records. In one pass position p is lane p % 64 of trip p / 64 % 32 of wave p / 2048 % 4 of
    tile p / 8192, so the hit bit travels to the next trip, the next wave, the next tile, across a tile without a delimiter; with
    passes of two frames it travels through the state carried between passes as well. Then the same with the match removed: the
    record flips sides in both modes."""
    rng = np.random.RandomState(dist)
    head = _lines(rng, 300)[:-1] + b"\n"
    S = len(head)
    body = bytearray(filler[:50 + dist])
    body[50:50 + len(NEEDLE)] = NEEDLE
    tail = b"\n" + _lines(rng, 200, b"abc") + b"\n" + NEEDLE + b"\nlast"
    big = (S, 50 + dist)
    for with_match in (True, False):
        if not with_match:
            body[50:50 + len(NEEDLE)] = filler[50:50 + len(NEEDLE)]
        data = head + bytes(body) + tail
        assert (S + 50) // 64 != (S + 50 + dist) // 64 and len(data) % FS                  # (another trip at least; a short last frame)
        if dist == 16384:
            assert (S + 50 + dist) // 8192 == (S + 50) // 8192 + 2
        arc = _compress(gpu_engine, zra, data, 3, FS, True)
        d = _dev(arc)
        for staging in (0, 2 * FS):
            sel = _check(gpu_engine, zra, d, len(arc), data, FS, [NEEDLE, b"\xF2\xF3"], staging=staging)
            assert (big in sel[False], big in sel[True]) == (with_match, not with_match), (what, staging, with_match)
            assert sel[False][-1] == (len(data) - 5 - len(NEEDLE), len(NEEDLE)) and sel[True][-1] == (len(data) - 4, 4)


# ---- 3
@pytest.fixture(scope="module")
def text(zra, gpu_engine):
    """6 frames of 1,024 bytes and a last one of 300: lines of _data's alphabet (a newline every 24 bytes or so), no newline at the
    end. Delimiters are forced at the last byte of frame 0, the first byte of frame 2 and the first byte of frame 4 (the first byte of
    a pass of two frames, the byte in front of it not one), and a run of 300 of them crosses the boundary of frames 2 and 3."""
    U = 6 * FS + 300
    a = bytearray(_data(np.random.RandomState(33), U))
    a[FS - 1] = NL; a[2 * FS] = NL; a[4 * FS] = NL; a[4 * FS - 1] = 1; a[U - 1] = 2
    a[3 * FS - 100:3 * FS + 200] = b"\n" * 300
    data = bytes(a)
    pats = [data[700:703], data[5 * FS + 40:5 * FS + 42], data[5 * FS - 9:5 * FS + 9]]                  # 3, 2 and 18 bytes, the last across frames
    assert NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    return dict(data=data, arc=arc, d=_dev(arc), pats=pats, U=U)


def test_delimiter_positions(zra, gpu_engine, text):
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
    nl = [p for p in range(U) if data[p] == NL]
    a, b = nl[5], nl[-3]
    ranges = [(0, None), (a, b + 1), (a, b), (a + 1, b + 1), (0, FS), (FS - 1, 2 * FS + 1), (2 * FS, 4 * FS + 1), (4 * FS, U), (4 * FS - 1, 4 * FS + 1),
              (3 * FS - 100, 3 * FS + 200), (3 * FS - 101, 3 * FS + 201), (3 * FS - 50, 3 * FS + 50)]
    for staging in (0, 2 * FS, 1):
        for lo, hi in ranges:
            sel = _check(gpu_engine, zra, d, len(arc), data, FS, pats, lo, hi, staging)
            if (lo, hi) == (3 * FS - 100, 3 * FS + 200):
                assert sel[True] == [(p, 0) for p in range(lo, hi)] and sel[False] == []   # 300 delimiters: 300 empty records, no tail
            if (lo, hi) == (3 * FS - 101, 3 * FS + 201):
                assert len([r for r in sel[True] if r[1] == 0]) == 299                   # the first one ends the byte in front
    assert data[a] == NL and data[b] == NL and data[a + 1] != NL


def test_delimiters_only_and_no_delimiter(zra, gpu_engine):
    only = b"\n" * 2500
    arc = _compress(gpu_engine, zra, only, 3, FS, True)
    for staging in (0, 1):
        sel = _check(gpu_engine, zra, _dev(arc), len(arc), only, FS, [b"a", b"bc"], staging=staging)
        assert sel[True] == [(p, 0) for p in range(2500)] and sel[False] == []
    none = _data(np.random.RandomState(8), 9000).replace(b"\n", b"\x0B")
    arc = _compress(gpu_engine, zra, none, 3, FS, True)
    d = _dev(arc)
    for staging in (0, 3 * FS):
        assert _check(gpu_engine, zra, d, len(arc), none, FS, [none[8500:8504]], staging=staging) == {False: [(0, 9000)], True: []}
        assert _check(gpu_engine, zra, d, len(arc), none, FS, [b"\xFF\xFE"], staging=staging) == {False: [], True: [(0, 9000)]}
        assert _check(gpu_engine, zra, d, len(arc), none, FS, [none[10:14]], 11, 8999, staging)[True] == [(11, 8988)]   # the match begins in front of lo


# ---- 4
def test_range_ends(zra, gpu_engine, text):
    data, arc, d, U = text["data"], text["arc"], text["d"], text["U"]
    # an occurrence of 6 bytes inside one record, away from the forced places
    p = next(q for q in range(5 * FS + 100, U) if NL not in data[q - 3:q + 9])
    pat = data[p:p + 6]
    start = data.rfind(b"\n", 0, p) + 1
    other = [b"\xFF\xFE\xFD"]
    for staging in (0, FS):
        for hi in (p + 3, p + 5, p + 6, p + 7):                                # inside the occurrence, exactly behind it, one byte behind it
            sel = _check(gpu_engine, zra, d, len(arc), data, FS, [pat] + other, start - 40, hi, staging)
            assert ((start, hi - start) in sel[False]) == (hi >= p + 6) and ((start, hi - start) in sel[True]) == (hi < p + 6), hi
        # lo inside the record, behind the start of its match: the clipped record holds no match
        sel = _check(gpu_engine, zra, d, len(arc), data, FS, [pat] + other, p + 1, p + 400, staging)
        assert sel[True][0][0] == p + 1 and (not sel[False] or sel[False][0][0] > p + 1)
        # shorter than the shortest pattern: without INVERT nothing is decoded; inverted the range is scanned and every record selected
        for lo, hi in ((p, p + 2), (start - 1, start + 1), (U - 1, U), (U, U), (0, 0)):
            sel = _check(gpu_engine, zra, d, len(arc), data, FS, [pat, b"\xFF\xFE\xFD"], lo, hi, staging)
            assert sel[False] == [] and sel[True] == GM.records(data, NL, lo, hi)
            assert gpu_engine.grep_stats()["decoded"] == (1 if hi > lo else 0)       # (the inverted call ran last)
    assert _check(gpu_engine, zra, d, len(arc), data, FS, [pat], start - 1, start + 1)[True] == [(start - 1, 0), (start, 1)]


# ---- 5
def test_capacity(zra, gpu_engine, text):
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
    for mode in (0, 1):
        recs, sel, matches = GM.grep(data, pats, NL, bool(mode))
        total = len(sel)
        assert total > 5
        for cap in (0, 1, total - 1, total + 5):
            for staging in (0, FS):
                st, n, mem = _raw(gpu_engine, zra, d, len(arc), pats, cap, mode=mode, staging=staging)
                k = min(total, cap)
                assert (st, n) == ((0, 0), total), (mode, cap, staging, st, n)
                got = np.frombuffer(mem[:16 * k], dtype="<u8").reshape(-1, 2)
                assert [tuple(r) for r in got.tolist()] == sel[:k], (mode, cap, staging)
                assert mem[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), (mode, cap, staging)
                assert gpu_engine.grep_stats() == _stats(U, FS, 0, U, staging, len(recs), total, k, matches), (mode, cap, staging)


# ---- 6
def test_short_last_frame_unterminated_last_record_and_several_matches_in_one_record(zra, gpu_engine):
    data = b"xx ab ab cd\n" * 100 + b"\n" + b"q" * 900 + b"\nab, cd and ab again, no newline behind"
    assert len(data) % FS and not data.endswith(b"\n")
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    pats = [b"ab", b"cd", b"b a"]
    for staging in (0, FS):
        sel = _check(gpu_engine, zra, _dev(arc), len(arc), data, FS, pats, staging=staging)
        assert len(sel[False]) == 101 and sel[False][-1] == (len(data) - 38, 38) and sel[True] == [(1200, 0), (1201, 900)]
        assert gpu_engine.grep_stats()["matches"] == 101 * 4                    # every (p, i) pair; a record counts once


# ---- 6b
def test_more_than_one_workgroup_and_more_tiles_than_scan_lanes(zra, gpu_engine):
    """8.6 MiB in frames of 64 KiB: 1,101 tiles, so a workgroup's eight tiles are one of 138 groups and a lane of the one-workgroup scan
    walks two tiles; with passes of 16 frames the same content takes nine passes of 128 tiles. Lines of 200 bytes or so, two stretches
    of 100,000 and 20,000 bytes without a newline (whole tiles and a whole group without a delimiter), one of them with a match."""
    fs = 65536
    U = 1100 * 8192 + 5000
    rng = np.random.RandomState(66)
    a = rng.randint(32, 127, size=U).astype(np.uint8)
    a[rng.randint(0, U, size=U // 200)] = NL
    a[3000000:3100000][a[3000000:3100000] == NL] = 32
    quiet = a[7000000:7020000]                                                 # (a view: no newline, and no first byte of the 2-byte pattern)
    quiet[quiet == NL] = 32
    quiet[quiet == a[123456]] = 33 if a[123456] == 32 else 32
    data = a.tobytes()
    pats = [data[123456:123458], data[3050000:3050012], data[8000000:8000004], b"\x01\x02"]
    assert NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 1, fs, True)
    d = _dev(arc)
    for staging in (0, 16 * fs):
        sel = _check(gpu_engine, zra, d, len(arc), data, fs, pats, staging=staging)
        assert any(n >= 100000 for _, n in sel[False]) and any(20000 <= n < 100000 for _, n in sel[True])
        assert len(sel[False]) > 100 and len(sel[True]) > 10000
        assert gpu_engine.grep_stats()["passes"] == (9 if staging else 1)
    _check(gpu_engine, zra, d, len(arc), data, fs, pats, 3050005, 8000003, 16 * fs)


# ---- 7
@pytest.fixture(scope="module")
def damaged(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    return dict(data=data, arc=arc, bad=_flip_mid(arc, [7]), fs=fs)


def test_a_damaged_frame(zra, gpu_engine, damaged):
    data, bad, fs = damaged["data"], damaged["bad"], damaged["fs"]
    pats = [data[5 * fs + 100:5 * fs + 103].replace(b"\n", b"\x01"), data[9 * fs + 50:9 * fs + 52].replace(b"\n", b"\x01")]
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs, 1):
            st, n, mem = _raw(gpu_engine, zra, db, len(bad), pats, 6, mode=mode, staging=staging)
            assert (st, n, mem) == ((1, want[7]), 0, b"\xEE" * 128), (mode, staging, st, n)
            assert gpu_engine.grep_stats() == ZERO
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), data, fs, pats, lo, hi)
    assert _grep(gpu_engine, zra, db, len(bad), pats, offset=8 * fs - 1) == ((1, want[7]), 0, [])


# ---- 8
def test_refusals_with_an_engine(zra, gpu_engine, damaged):
    L = zra.load()
    arc = damaged["arc"]
    d = _dev(arc)
    P, size = d.data_ptr(), len(arc)
    buf = ctypes.create_string_buffer(b"\x03" * 5000)
    nlb = ctypes.create_string_buffer(b"ab\ncd")
    arr = (ctypes.c_uint64 * 4)()
    n = ctypes.c_uint64(0)
    nn = ctypes.byref(n)

    def sz(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    # (dArchive, size, hPatterns, hPatternSizes, nPatterns, delimiter, mode, offset, size, staging, hRecords, capacity, nRecords)
    for args in ((None, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, None, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, None, 1, NL, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, None, 2, nn),
                 (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, None), (P, size, buf, sz(3), 0, NL, 0, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, sz(*[1] * 65), 65, NL, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, buf, sz(3, 0), 2, NL, 0, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, sz(3, 257), 2, NL, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, buf, sz(*[256] * 17), 17, NL, 0, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, sz(3), 1, NL, 2, 0, MAXU64, 0, arr, 2, nn), (P, size, buf, sz(3), 1, NL, 3, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, sz(3), 1, 3, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, nlb, sz(2, 3), 2, NL, 1, 0, MAXU64, 0, arr, 2, nn),
                 (P, size, buf, sz(3), 1, 3, 0, size * 99, 5, 0, arr, 2, nn)):   # also in front of a range outside the content
        n.value = 0x1234
        ctypes.memset(arr, 0xEE, 32)
        assert L.ZraHipGrepArchive(gpu_engine.h, *args).tup() == (1, 42), args[3:7]
        assert n.value == (0x1234 if args[12] is None else 0) and bytes(arr) == b"\xEE" * 32
        assert gpu_engine.grep_stats() == ZERO
    pats = [b"\x01\x02"]
    for cut in (0, 10, 38, 42):                                                # rule 2: truncated archives
        st, got, mem = _raw(gpu_engine, zra, d, cut, pats, 2)
        assert (st, got, mem) == ((5, 0), 0, b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, cut
    U = len(damaged["data"])
    for lo, ln in ((U + 1, 0), (0, U + 1), (5, MAXU64 - 1), (MAXU64, 1), (U, 1)):   # rule 3: outside the content
        for mode in (0, 1):
            st, got, mem = _raw(gpu_engine, zra, d, len(arc), pats, 2, mode=mode, offset=lo, length=ln)
            assert (st, got, mem) == ((5, 0), 0, b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, (lo, ln)


# ---- 9
def test_a_grep_leaves_the_search_stats_alone(zra, gpu_engine, text):
    data, arc, d, pats = text["data"], text["arc"], text["d"], text["pats"]
    gpu_engine.search(d.data_ptr(), len(arc), pats[0], staging_bytes=2 * FS)
    gpu_engine.search_multi(d.data_ptr(), len(arc), pats, staging_bytes=3 * FS)
    s1, sm = gpu_engine.search_stats(), gpu_engine.search_multi_stats()
    assert s1["passes"] == 4 and sm["passes"] == 3
    a = _check(gpu_engine, zra, d, len(arc), data, FS, pats, staging=FS, modes=(False,))
    sg = gpu_engine.grep_stats()
    assert sg["passes"] == 7 and gpu_engine.grep_scan_ms() > 0
    assert gpu_engine.search_stats() == s1
    gpu_engine.search_multi(d.data_ptr(), len(arc), pats, staging_bytes=3 * FS)
    gpu_engine.search(d.data_ptr(), len(arc), pats[0], staging_bytes=2 * FS)
    assert gpu_engine.grep_stats() == sg and gpu_engine.search_multi_stats() == sm
    gpu_engine.release_scratch()                                               # scratch handed back: the same answer
    assert _check(gpu_engine, zra, d, len(arc), data, FS, pats, staging=FS, modes=(False,)) == a and gpu_engine.grep_stats() == sg


# ---- 10
def test_cli_mode_gl(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta two\n\ngamma one two\ndelta" + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc, p_junk = tmp_path / "lines.zra", tmp_path / "junk.zra"
    p_arc.write_bytes(arc); p_junk.write_bytes(b"\x01" * 100)

    def run(*args):
        return subprocess.run([TOOL, "gl", str(p_arc)] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    def lines(sel):
        return ["%d\t%d" % r for r in sel] + ["%d records" % len(sel), ""]

    for args, pats, delim, inv in ((("one",), [b"one"], NL, False), (("-v", "one", "hex:" + b"two".hex()), [b"one", b"two"], NL, True),
                                   (("-d", "3b", "-v", "one"), [b"one"], 0x3B, True), (("-v", "-d", "3B", "y", "z"), [b"y", b"z"], 0x3B, True)):
        sel = GM.grep(data, pats, delim, inv)[1]
        r = run(*args)
        assert r.returncode == 0 and r.stdout.split("\n") == lines(sel) and sel, (args, r.stdout, r.stderr)
    assert GM.grep(data, [b"one", b"two"], NL, True)[1] == [(19, 0), (34, 5)]
    r = run("absent", "hex:fffe")
    assert r.returncode == 1 and r.stdout == "0 records\n", (r.stdout, r.stderr)
    r = run("-v", "a", "e", "x")
    assert r.returncode == 0 and r.stdout == "19\t0\n1 records\n", (r.stdout, r.stderr)
    for args in (("a\nb",), ("-d", "61", "alpha"), ("-d", "100", "a"), ("-d",), ("-v",), (), ("a", "hex:0"), ["a"] * 65):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
    r = subprocess.run([TOOL, "gl", str(p_junk), "a"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "", (r.stdout, r.stderr)
