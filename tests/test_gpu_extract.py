"""GPU tests of ZraHipExtractRecords (include/zra_hip.h): the grep's selected records WITH their bytes, packed into a device buffer, each
followed by the delimiter. The yardstick everywhere is the plaintext the test generated itself, cut, scanned and joined on the CPU
(tests/extract_model.py, cross-checked in tests/test_extract_abi.py); the list and the count are also held against Engine.grep on the
same arguments; for a frame that does not decode, the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query
inside it. Archives are written on the device. dData is a 0xEE-filled buffer, handed over 257 bytes in (odd alignment) with a capacity
that leaves 256 guard bytes behind it: after every call both guards are still 0xEE. The shapes are the grep's seams: the scan's trip is
64 positions, its wave 2,048, its tile 8,192; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import extract_model as XM
import grep_model as GM
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
FRONT, BACK = 257, 256
ZERO = dict(frames=0, decoded=0, content_bytes=0, records=0, selected=0, packed_bytes=0, passes=0, matches=0)
TOO_SMALL = (6, 0)                                                             # OutputBufferTooSmall


def _raw(eng, zra, d, size, pats, data_cap, rec_cap, delim=NL, mode=0, offset=0, length=MAXU64, staging=0):
    """(status, *nRecords, *dataSize, the bytes of a record array two entries longer than the capacity, the first data_cap bytes of
    dData) of one call; both 0xEE-filled before it. Asserts that the guards in front of dData and behind its capacity are intact."""
    import torch
    buf = torch.full((FRONT + data_cap + BACK,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (2 * (rec_cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    eng._order()
    st = zra.load().ZraHipExtractRecords(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), delim, mode, offset, length, staging,
                                         arr if rec_cap else None, rec_cap, ctypes.byref(n), buf.data_ptr() + FRONT, data_cap, ctypes.byref(ds)).tup()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().tobytes()
    assert host[:FRONT] == b"\xEE" * FRONT and host[FRONT + data_cap:] == b"\xEE" * BACK, ("guard", st, data_cap, rec_cap, mode, offset, length, staging)
    return st, n.value, ds.value, bytes(arr), host[FRONT:FRONT + data_cap]


def _stats(U, fs, lo, end, staging, records, selected, packed, matches):
    """the eight counters of an extract of [lo, end) that decoded"""
    f0, f1 = lo // fs, (end - 1) // fs
    slots = max(1, min(65536, (staging or 4 << 30) // fs))
    return dict(frames=-(-U // fs), decoded=f1 - f0 + 1, content_bytes=min(U, (f1 + 1) * fs) - f0 * fs, records=records, selected=selected, packed_bytes=packed,
                passes=-(-(f1 - f0 + 1) // slots), matches=matches)


def _pairs(mem, k):
    return [tuple(r) for r in np.frombuffer(mem[:16 * k], dtype="<u8").reshape(-1, 2).tolist()]


def _check(eng, zra, d, size, data, fs, pats, lo=0, hi=None, staging=0, delim=NL, modes=(False, True), slack=5):
    """one extract per mode of [lo, hi) against the model: status, both words, the packed bytes, the list, all eight stats; the list
    and the count also against Engine.grep. Returns {invert: (selected, packed)}. (The model is computed once: the records a mode
    does not select are the ones the other mode selects, which tests/test_extract_abi.py holds.)"""
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    recs, hits, matches = GM.grep(data, pats, delim, False, lo, hi)
    hitset = set(hits)
    out = {}
    for inv in modes:
        sel = [r for r in recs if (r in hitset) != inv]
        packed = b"".join(data[o:o + n] + bytes([delim]) for o, n in sel)
        tag = (lo, hi, staging, inv)
        gn, glist = eng.grep(d.data_ptr(), size, pats, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging, max_records=len(recs) + 1)
        assert (gn, glist) == (len(sel), sel), (tag, gn, len(sel))
        st, n, ds, mem, got = _raw(eng, zra, d, size, pats, len(packed) + slack, len(sel) + 1, delim, int(inv), lo, MAXU64 if hi is None else hi - lo, staging)
        assert (st, n, ds) == ((0, 0), len(sel), len(packed)), (tag, st, n, ds, len(sel), len(packed))
        if got[:ds] != packed:
            bad = next(i for i in range(ds) if got[i] != packed[i])
            raise AssertionError((tag, "first wrong byte", bad, got[max(0, bad - 8):bad + 8], packed[max(0, bad - 8):bad + 8]))
        assert _pairs(mem, n) == sel and mem[16 * n:] == b"\xEE" * (16 * (len(sel) + 3 - n)), tag
        s = eng.extract_stats()
        if end == lo or (not inv and end - lo < min(len(p) for p in pats)):
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == _stats(U, fs, lo, end, staging, len(recs), len(sel), len(packed), matches), (tag, s)
        out[inv] = (sel, packed)
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
    """About 260 frames of 4 bytes (tests/test_gpu_grep.py's first corpus). With one slot a pass holds 4 bytes: shorter than M - 1 =
    39, so a pass owns positions only inside the carry area, and the 60-byte line is copied provisionally by 15 passes in a row."""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"acde"), size=60).astype(np.uint8))
    data = _lines(rng, 500) + b"\n" + long_line + b"\n" + _lines(rng, 480)
    pats = [b"b", b"cda", long_line[5:45], b"zz", b"ea"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    out = _check(gpu_engine, zra, _dev(arc), len(arc), data, 4, pats, staging=staging)
    assert (501, 60) in out[False][0] and long_line + b"\n" in out[False][1] and len(out[False][0]) > 20
    assert len(out[True][0]) > 10 and any(n == 0 for _, n in out[True][0]) and b"\n\n" in out[True][1]
    assert gpu_engine.extract_stats()["passes"] == (-(-len(data) // 4) if staging else 1)


# ---- 2
FS = 1024
NEEDLE = b"\xF0NEEDLE\xF1"


@pytest.fixture(scope="module")
def filler():
    """32 KiB without a delimiter and without a byte of NEEDLE: the body of the long record"""
    return _data(np.random.RandomState(5), 32 << 10).replace(b"\n", b"\x0B")


@pytest.mark.parametrize("dist", [64, 2048, 8192, 16384, 20000])
def test_provisional_tail(zra, gpu_engine, filler, dist):
    """Short records, some selected, then one long record whose only match lies 50 bytes behind its start and whose ending delimiter
    lies `dist` positions behind the match, then short records, some selected. With passes of two frames the long record is open at
    the end of up to ten passes in a row and copied provisionally by each. (a) It is selected: the parts must line up at one packed
    offset. (b) The match is removed: the selected short records behind it must overwrite what two or more passes left. (c) No
    selected record lies behind it either: what they left lies behind *dataSize. A capacity of the whole content lets every provisional
    byte land inside the buffer."""
    rng = np.random.RandomState(dist)
    head = _lines(rng, 300)[:-1] + b"\n" + NEEDLE + b" in front\n" + _lines(rng, 60)[:-1] + b"\n"
    S = len(head)
    with_match = bytearray(filler[:50 + dist])
    with_match[50:50 + len(NEEDLE)] = NEEDLE
    without = filler[:50 + dist]
    tail_sel = b"\n" + _lines(rng, 200, b"abc") + b"\n" + NEEDLE + b"\nlast"
    tail_none = b"\n" + _lines(rng, 200, b"abc") + b"\nlast"
    big = (S, 50 + dist)
    for body, tail, what in ((bytes(with_match), tail_sel, "a"), (without, tail_sel, "b"), (without, tail_none, "c")):
        data = head + body + tail
        data += b"!" * (len(data) % FS == 0)                                   # (a short last frame)
        arc = _compress(gpu_engine, zra, data, 3, FS, True)
        d = _dev(arc)
        for staging in (0, 2 * FS):
            out = _check(gpu_engine, zra, d, len(arc), data, FS, [NEEDLE, b"\xF2\xF3"], staging=staging, slack=len(data))
            assert (big in out[False][0], big in out[True][0]) == (what == "a", what != "a"), (what, staging)
            want = {"a": 3, "b": 2, "c": 1}[what]
            assert len(out[False][0]) == want and out[False][1].startswith(NEEDLE + b" in front\n"), (what, staging, out[False][0])
            if what == "b":
                assert out[False][1] == NEEDLE + b" in front\n" + NEEDLE + b"\n"
            if staging and dist >= 8192:
                assert gpu_engine.extract_stats()["passes"] >= 5


# ---- 3
@pytest.fixture(scope="module")
def text(zra, gpu_engine):
    """6 frames of 1,024 bytes and a last one of 300: lines of _data's alphabet (a newline every 24 bytes or so), no newline at the
    end. Delimiters are forced at the last byte of frame 0, the first byte of frame 2 and the first byte of frame 4 (the first byte of
    a pass of two frames, the byte in front of it not one), 5 bytes in front of the end of frame 1 (inside the last M - 1 = 17 bytes of
    a pass of two frames: evaluated from the carry area), and a run of 300 of them crosses the boundary of frames 2 and 3."""
    U = 6 * FS + 300
    a = bytearray(_data(np.random.RandomState(33), U))
    a[FS - 1] = NL; a[2 * FS] = NL; a[4 * FS] = NL; a[4 * FS - 1] = 1; a[U - 1] = 2; a[2 * FS - 5] = NL
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
              (2 * FS - 30, 2 * FS + 30), (3 * FS - 100, 3 * FS + 200), (3 * FS - 101, 3 * FS + 201), (3 * FS - 50, 3 * FS + 50)]
    for staging in (0, 2 * FS, 1):
        for lo, hi in ranges:
            out = _check(gpu_engine, zra, d, len(arc), data, FS, pats, lo, hi, staging)
            if (lo, hi) == (3 * FS - 100, 3 * FS + 200):
                assert out[True][1] == b"\n" * 300 and out[False][1] == b""        # 300 delimiters: 300 empty records, 300 bytes
    assert data[a] == NL and data[b] == NL and data[a + 1] != NL


def test_delimiters_only_and_no_delimiter(zra, gpu_engine):
    only = b"\n" * 2500
    arc = _compress(gpu_engine, zra, only, 3, FS, True)
    for staging in (0, 1):
        out = _check(gpu_engine, zra, _dev(arc), len(arc), only, FS, [b"a", b"bc"], staging=staging)
        assert out[True][1] == only and out[False][1] == b""
    none = _data(np.random.RandomState(8), 9000).replace(b"\n", b"\x0B")
    arc = _compress(gpu_engine, zra, none, 3, FS, True)
    d = _dev(arc)
    for staging in (0, 3 * FS):
        out = _check(gpu_engine, zra, d, len(arc), none, FS, [none[8500:8504]], staging=staging)
        assert out[False][1] == none + b"\n" and out[True][1] == b""          # one record plus one added delimiter
        out = _check(gpu_engine, zra, d, len(arc), none, FS, [b"\xFF\xFE"], staging=staging)
        assert out[True][1] == none + b"\n" and out[False][1] == b""
        assert _check(gpu_engine, zra, d, len(arc), none, FS, [none[10:14]], 11, 8999, staging)[True][1] == none[11:8999] + b"\n"


# ---- 4
def test_range_ends(zra, gpu_engine, text):
    data, arc, d, U = text["data"], text["arc"], text["d"], text["U"]
    # an occurrence of 6 bytes inside one record, away from the forced places
    p = next(q for q in range(5 * FS + 100, U) if NL not in data[q - 3:q + 9])
    pat = data[p:p + 6]
    start = data.rfind(b"\n", 0, p) + 1
    nxt = data.find(b"\n", p)
    other = [b"\xFF\xFE\xFD"]
    for staging in (0, FS):
        for hi in (p + 3, p + 5, p + 6, p + 7):                                # inside the occurrence, exactly behind it, one byte behind it
            out = _check(gpu_engine, zra, d, len(arc), data, FS, [pat] + other, start - 40, hi, staging)
            clipped = data[start:hi] + b"\n"                                   # the clipped last record gets its delimiter
            assert out[False][1].endswith(clipped) == (hi >= p + 6) and out[True][1].endswith(clipped) == (hi < p + 6), hi
        for hi in (nxt, nxt + 1):                                              # hi on a delimiter, and one behind it: the same last record
            out = _check(gpu_engine, zra, d, len(arc), data, FS, [pat] + other, start - 40, hi, staging)
            assert out[False][1].endswith(data[start:nxt] + b"\n") and out[False][0][-1] == (start, nxt - start), hi
        # lo inside the record, behind the start of its match: the clipped record holds no match
        out = _check(gpu_engine, zra, d, len(arc), data, FS, [pat] + other, p + 1, p + 400, staging)
        assert out[True][0][0][0] == p + 1 and out[True][1].startswith(data[p + 1:nxt] + b"\n")
        # the two shortcuts: the empty range, and without INVERT a range shorter than the shortest pattern (inverted it is scanned)
        for lo, hi in ((p, p + 2), (start - 1, start + 1), (U - 1, U), (U, U), (0, 0)):
            out = _check(gpu_engine, zra, d, len(arc), data, FS, [pat, b"\xFF\xFE\xFD"], lo, hi, staging)
            assert out[False] == ([], b"") and out[True][0] == GM.records(data, NL, lo, hi)
            assert gpu_engine.extract_stats()["decoded"] == (1 if hi > lo else 0)    # (the inverted call ran last)
    assert _check(gpu_engine, zra, d, len(arc), data, FS, [pat], start - 1, start + 1)[True][1] == b"\n" + data[start:start + 1] + b"\n"


# ---- 5
def test_capacity(zra, gpu_engine, text):
    data, arc, d, pats, U = text["data"], text["arc"], text["d"], text["pats"], text["U"]
    for mode in (0, 1):
        recs, sel, matches, packed = XM.extract(data, pats, NL, bool(mode))
        total, size = len(sel), len(packed)
        assert total > 5
        for dcap in (0, 1, size - 1, size, size + 5):
            for rcap in (0, total - 1, total):
                for staging in (0, FS):
                    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, dcap, rcap, mode=mode, staging=staging)
                    tag = (mode, dcap, rcap, staging, st, n, ds)
                    fits = dcap >= size and (rcap == 0 or rcap >= total)
                    assert (st, n, ds) == ((0, 0) if fits else TOO_SMALL, total, size), tag
                    if fits:
                        assert got[:size] == packed, tag
                        assert _pairs(mem, rcap) == sel[:rcap] and mem[16 * rcap:] == b"\xEE" * 32, tag
                        assert gpu_engine.extract_stats() == _stats(U, FS, 0, U, staging, len(recs), total, size, matches), tag
                    else:
                        assert mem == b"\xEE" * (16 * (rcap + 2)), tag           # hRecords untouched
                        assert gpu_engine.extract_stats() == ZERO, tag


# ---- 6
def test_more_than_one_workgroup_and_more_tiles_than_scan_lanes(zra, gpu_engine):
    """tests/test_gpu_grep.py's 8.6 MiB in frames of 64 KiB: 1,101 tiles, so a workgroup's eight tiles are one of 138 groups and a lane
    of the one-workgroup scan walks two tiles; with passes of 16 frames the same content takes nine passes of 128 tiles. Two stretches
    of 100,000 and 20,000 bytes without a newline (whole tiles and a whole group whose bytes are selected by a delimiter far behind),
    the first with a match. Inverted, about the whole content is copied."""
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
        out = _check(gpu_engine, zra, d, len(arc), data, fs, pats, staging=staging)
        assert any(n >= 100000 for _, n in out[False][0]) and any(20000 <= n < 100000 for _, n in out[True][0])
        assert len(out[False][0]) > 100 and len(out[True][0]) > 10000 and len(out[True][1]) > U * 9 // 10
        assert gpu_engine.extract_stats()["passes"] == (9 if staging else 1)
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
            st, n, ds, mem, _ = _raw(gpu_engine, zra, db, len(bad), pats, 13 * fs, 6, mode=mode, staging=staging)
            assert (st, n, ds, mem) == ((1, want[7]), 0, 0, b"\xEE" * 128), (mode, staging, st, n, ds)
            assert gpu_engine.extract_stats() == ZERO
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), data, fs, pats, lo, hi)
    st, n, ds, _, _ = _raw(gpu_engine, zra, db, len(bad), pats, 13 * fs, 0, offset=8 * fs - 1)
    assert (st, n, ds) == ((1, want[7]), 0, 0)


# ---- 8
def test_refusals_with_an_engine(zra, gpu_engine, damaged):
    import torch
    L = zra.load()
    arc = damaged["arc"]
    size = len(arc)
    # one allocation: 512 bytes, the archive, 512 bytes; and a buffer of its own
    whole = torch.full((512 + size + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
    whole[512:512 + size] = _dev(arc)
    P = whole.data_ptr() + 512
    out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
    D = out.data_ptr()
    buf = ctypes.create_string_buffer(b"\x03" * 5000)
    nlb = ctypes.create_string_buffer(b"ab\ncd")
    arr = (ctypes.c_uint64 * 4)()
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
    nn, dd = ctypes.byref(n), ctypes.byref(ds)

    def sz(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    def refused(args, status):
        n.value, ds.value = 0x1234, 0x5678
        ctypes.memset(arr, 0xEE, 32)
        assert L.ZraHipExtractRecords(gpu_engine.h, *args).tup() == status, args[3:7]
        assert n.value == (0x1234 if args[12] is None else 0) and ds.value == (0x5678 if args[15] is None else 0) and bytes(arr) == b"\xEE" * 32
        assert gpu_engine.extract_stats() == ZERO

    # (dArchive, size, hPatterns, hPatternSizes, nPatterns, delimiter, mode, offset, size, staging, hRecords, capacity, nRecords, dData, capacity, dataSize)
    T = (arr, 2, nn, D, 4096, dd)
    for args in ((None, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0) + T, (P, size, None, sz(3), 1, NL, 0, 0, MAXU64, 0) + T,
                 (P, size, buf, None, 1, NL, 0, 0, MAXU64, 0) + T, (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, None, 2, nn, D, 4096, dd),
                 (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, None, D, 4096, dd), (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, nn, D, 4096, None),
                 (P, size, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, nn, None, 4096, dd), (P, size, buf, sz(3), 0, NL, 0, 0, MAXU64, 0) + T,
                 (P, size, buf, sz(*[1] * 65), 65, NL, 0, 0, MAXU64, 0) + T, (P, size, buf, sz(3, 0), 2, NL, 0, 0, MAXU64, 0) + T,
                 (P, size, buf, sz(3, 257), 2, NL, 0, 0, MAXU64, 0) + T, (P, size, buf, sz(*[256] * 17), 17, NL, 0, 0, MAXU64, 0) + T,
                 (P, size, buf, sz(3), 1, NL, 2, 0, MAXU64, 0) + T, (P, size, buf, sz(3), 1, NL, 3, 0, MAXU64, 0) + T,
                 (P, size, buf, sz(3), 1, 3, 0, 0, MAXU64, 0) + T, (P, size, nlb, sz(2, 3), 2, NL, 1, 0, MAXU64, 0) + T,
                 (P, size, buf, sz(3), 1, 3, 0, size * 99, 5, 0) + T,          # also in front of a range outside the content
                 (P, size, buf, sz(3), 1, 3, 0, 0, MAXU64, 0, arr, 2, nn, P + 100, 50, dd)):   # rule 1 in front of rule 2
        refused(args, (1, 42))
    # rule 2: dData inside the archive, the archive inside dData, one byte of overlap at either end; in front of a truncated header
    for dptr, dcap, asize in ((P + 100, 50, size), (P - 256, size + 512, size), (P - 10, 11, size), (P + size - 1, 10, size), (P + 5, 1, 10)):
        refused((P, asize, buf, sz(3), 1, NL, 0, 0, MAXU64, 0, arr, 2, nn, dptr, dcap, dd), (1, 42))
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert host[:512] == b"\xEE" * 512 and host[512 + size:] == b"\xEE" * 512 and host[512:512 + size] == arc   # the archive is only read
    # touching is no overlap: the buffer ends where the archive begins, begins where it ends
    data, fs = damaged["data"], damaged["fs"]
    want = XM.extract(data, [b"\x01\x02"])
    for dptr in (P - 512, P + size):
        n.value = ds.value = 0
        st = L.ZraHipExtractRecords(gpu_engine.h, P, size, b"\x01\x02", sz(2), 1, NL, 0, 0, MAXU64, 0, None, 0, nn, dptr, 512, dd).tup()
        assert (st, n.value, ds.value) == ((0, 0) if len(want[3]) <= 512 else TOO_SMALL, len(want[1]), len(want[3]))
    whole[:512] = 0xEE
    whole[512 + size:] = 0xEE
    pats = [b"\x01\x02"]
    d = whole[512:]
    for cut in (0, 10, 38, 42):                                                # rule 3: truncated archives
        st, got, sz_, mem, _ = _raw(gpu_engine, zra, d, cut, pats, 64, 2)
        assert (st, got, sz_, mem) == ((5, 0), 0, 0, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO, cut
    U = len(data)
    for lo, ln in ((U + 1, 0), (0, U + 1), (5, MAXU64 - 1), (MAXU64, 1), (U, 1)):   # rule 4: outside the content
        for mode in (0, 1):
            st, got, sz_, mem, _ = _raw(gpu_engine, zra, d, size, pats, 64, 2, mode=mode, offset=lo, length=ln)
            assert (st, got, sz_, mem) == ((5, 0), 0, 0, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO, (lo, ln)


# ---- 9
def test_an_extract_leaves_the_other_stats_alone(zra, gpu_engine, text):
    data, arc, d, pats = text["data"], text["arc"], text["d"], text["pats"]
    gpu_engine.search(d.data_ptr(), len(arc), pats[0], staging_bytes=2 * FS)
    gpu_engine.search_multi(d.data_ptr(), len(arc), pats, staging_bytes=3 * FS)
    gpu_engine.grep(d.data_ptr(), len(arc), pats, staging_bytes=4 * FS)
    s1, sm, sg = gpu_engine.search_stats(), gpu_engine.search_multi_stats(), gpu_engine.grep_stats()
    assert (s1["passes"], sm["passes"], sg["passes"]) == (4, 3, 2)
    want = XM.extract(data, pats)

    def once():
        st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, len(want[3]), len(want[1]), staging=FS)
        assert (st, n, ds) == ((0, 0), len(want[1]), len(want[3])) and got == want[3] and _pairs(mem, n) == want[1]
        return gpu_engine.extract_stats()

    sx = once()
    assert sx["passes"] == 7 and gpu_engine.extract_ms() > 0
    assert (gpu_engine.search_stats(), gpu_engine.search_multi_stats(), gpu_engine.grep_stats()) == (s1, sm, sg)
    gpu_engine.grep(d.data_ptr(), len(arc), pats, staging_bytes=4 * FS)
    gpu_engine.search_multi(d.data_ptr(), len(arc), pats, staging_bytes=3 * FS)
    gpu_engine.search(d.data_ptr(), len(arc), pats[0], staging_bytes=2 * FS)
    assert gpu_engine.extract_stats() == sx
    gpu_engine.release_scratch()                                               # scratch handed back: the same answer
    assert once() == sx
    # the Python layer: the sizing call carries what is needed, the call returns the triple
    import torch
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.extract(d.data_ptr(), len(arc), pats, 0, 0)
    assert (e.value.zra, e.value.needed_records, e.value.needed_data) == (6, len(want[1]), len(want[3]))
    out = torch.empty(e.value.needed_data, dtype=torch.uint8, device="cuda:0")
    assert gpu_engine.extract(d.data_ptr(), len(arc), pats, out.data_ptr(), out.numel(), max_records=e.value.needed_records) == (len(want[1]), len(want[3]), want[1])
    assert out.cpu().numpy().tobytes() == want[3]
    assert gpu_engine.extract(d.data_ptr(), len(arc), pats, out.data_ptr(), out.numel(), invert=True, length=0) == (0, 0, [])


# ---- 10
def test_cli_mode_gx(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta two\n\ngamma one two\ndelta" + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc, p_junk, p_out = tmp_path / "lines.zra", tmp_path / "junk.zra", tmp_path / "out.txt"
    p_arc.write_bytes(arc); p_junk.write_bytes(b"\x01" * 100)

    def run(*args):
        return subprocess.run([TOOL, "gx", str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    for args, pats, delim, inv in ((("one",), [b"one"], NL, False), (("-v", "one", "hex:" + b"two".hex()), [b"one", b"two"], NL, True),
                                   (("-d", "3b", "-v", "one"), [b"one"], 0x3B, True), (("-v", "-d", "3B", "y", "z"), [b"y", b"z"], 0x3B, True)):
        packed = XM.extract(data, pats, delim, inv)[3]
        r = run(*args)
        assert r.returncode == 0 and r.stdout == packed and packed, (args, r.stdout, r.stderr)
        r = run("-o", p_out, *args)
        assert r.returncode == 0 and r.stdout == b"" and p_out.read_bytes() == packed, (args, r.stdout, r.stderr)
        p_out.unlink()
    assert XM.extract(data, [b"one"])[3] == b"alpha one\ngamma one two\nx;y;one;zx;y;one;zx;y;one;z\n"
    r = run("absent", "hex:fffe")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    r = run("-o", p_out, "absent")
    assert r.returncode == 1 and r.stdout == b"" and not p_out.exists(), (r.stdout, r.stderr)
    r = run("-v", "a", "e", "x")
    assert r.returncode == 0 and r.stdout == b"\n", (r.stdout, r.stderr)
    for args in (("a\nb",), ("-d", "61", "alpha"), ("-d", "100", "a"), ("-d",), ("-v",), (), ("a", "hex:0"), ["a"] * 65, ("-o",), ("-o", p_out)):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"", (args, r.stdout, r.stderr)
    r = subprocess.run([TOOL, "gx", str(p_junk), "a"], capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stdout == b"", (r.stdout, r.stderr)
