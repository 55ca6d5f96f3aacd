"""GPU tests of ZraHipSearchArchiveMulti (include/zra_hip.h): every (content offset, pattern index) at which one of several byte
patterns occurs inside a content range of a device-resident archive, ascending, in one decode of the range. The yardstick everywhere is
the plaintext the test generated itself, scanned on the CPU (tests/msearch_model.py, cross-checked in tests/test_msearch_abi.py); for a
frame that does not decode, the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it. Archives
are written on the device. The shapes are the smallest at which each seam exists: patterns of different lengths across passes shorter
than the longest, several patterns at one offset under a capacity, range ends inside and next to an occurrence, a short last frame."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import msearch_model as MM
import search_model as M
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
CAP = 1 << 17
ENTRY = np.dtype([("offset", "<u8"), ("pattern", "<u4"), ("reserved", "<u4")])


def _multi(eng, zra, d, size, pats, **kw):
    """((zra, zstd), n_matches, [(offset, pattern)], per_pattern) of one multi search"""
    kw.setdefault("max_matches", CAP)
    try:
        n, at, per = eng.search_multi(d.data_ptr(), size, pats, **kw)
        return (0, 0), n, at, per
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, [], []


def _raw(eng, zra, d, size, pats, cap, offset=0, length=MAXU64, staging=0):
    """(status, *nMatches, the bytes of a match array two entries longer than the capacity, the bytes of a per-pattern array one entry
    longer than the patterns; both 0xEE-filled before the call)"""
    arr = (zra.ZraHipPatternMatch * (cap + 2))()
    per = (ctypes.c_uint64 * (len(pats) + 1))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr)); ctypes.memset(per, 0xEE, ctypes.sizeof(per))
    n = ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    eng._order()
    st = zra.load().ZraHipSearchArchiveMulti(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), offset, length, staging, arr if cap else None, cap,
                                             ctypes.byref(n), per).tup()
    return st, n.value, bytes(arr), bytes(per)


def _per(want, k):
    return [sum(1 for _, i in want if i == j) for j in range(k)]


def _check(eng, zra, d, size, data, pats, lo=0, hi=None, staging=0):
    """one search of [lo, hi) against the model: status, count, list, per-pattern totals, matches / listed / patterns / survivors"""
    want = MM.matches_multi(data, pats, lo, hi)
    got = _multi(eng, zra, d, size, pats, offset=lo, length=None if hi is None else hi - lo, staging_bytes=staging)
    tag = (lo, hi, staging)
    assert got[:2] == ((0, 0), len(want)), (tag, got[:2], len(want))
    assert got[2] == want, (tag, sorted(set(got[2]) ^ set(want))[:10], got[2][:6], want[:6])
    assert got[3] == _per(want, len(pats)), (tag, got[3])
    s = eng.search_multi_stats()
    assert (s["matches"], s["listed"], s["patterns"], s["survivors"]) == (len(want), len(want), len(pats), MM.survivors(data, pats, lo, hi)), (tag, s)
    return want, s


# ---- 1
@pytest.mark.parametrize("staging,passes", [(0, 1), (1, 250)])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging, passes):
    """250 frames of 4 bytes, patterns of 1 to 256 bytes together, a duplicate and one that never matches. With one slot a pass holds 4
    bytes and the carry is shorter than M - 1 for 64 passes; the 256-byte match at p is owned 63 passes later than `a` at p + 10 would
    be under last-byte ownership, and the list must still ascend."""
    data = b"abcdefghij" * 100
    pats = [b"a", b"cdefg", b"abcdefghijab", data[:256], b"ja", b"abd", b"a"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    want, s = _check(gpu_engine, zra, _dev(arc), len(arc), data, pats, staging=staging)
    assert s == dict(frames=250, decoded=250, content_bytes=1000, matches=len(want), listed=len(want), passes=passes, patterns=7,
                     survivors=MM.survivors(data, pats)), s
    assert _per(want, 7) == [100, 100, 99, 75, 99, 0, 100] and s["survivors"] == 299                 # a., cd, ja
    assert want[:6] == [(0, 0), (0, 2), (0, 3), (0, 6), (2, 1), (9, 4)]
    assert want.index((0, 3)) < want.index((10, 0)) < want.index((10, 3))


# ---- 2
def test_several_patterns_at_one_offset_and_the_capacity_cut(zra, gpu_engine):
    fs = 1024
    U = 3 * fs + 5
    data = b"\0" * U
    pats = [b"\0", b"\0\0", b"\0\0\0", b"\0"]
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    want = MM.matches_multi(data, pats)
    total = 4 * U - 3
    assert len(want) == total and want[8:12] == [(2, 0), (2, 1), (2, 2), (2, 3)]                       # 10 and 11 cut inside offset 2's group
    wper = b"".join(int(v).to_bytes(8, "little") for v in (U, U - 1, U - 2, U)) + b"\xEE" * 8
    for cap in (0, 10, 11, total + 5):
        for staging in (0, 1):
            st, got, mem, per = _raw(gpu_engine, zra, d, len(arc), pats, cap, staging=staging)
            k = min(total, cap)
            assert (st, got, per) == ((0, 0), total, wper), (cap, st, got)
            e = np.frombuffer(mem[:16 * k], dtype=ENTRY)
            assert list(zip(e["offset"].tolist(), e["pattern"].tolist())) == want[:k], cap
            assert not e["reserved"].any() and mem[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), cap
            s = gpu_engine.search_multi_stats()
            assert s == dict(frames=4, decoded=4, content_bytes=U, matches=total, listed=k, passes=4 if staging else 1, patterns=4, survivors=U), s


# ---- 3
FS3 = 1024
PLACES = [0] + [k * FS3 - j for k in (1, 16, 17, 32) for j in (255, 128, 1)]


@pytest.fixture(scope="module")
def seams(zra, gpu_engine):
    """70 frames of 1,024 bytes and a last one of 700 (the shape of test_gpu_search.py's fixture, built afresh). A 256-byte pattern of
    bytes the alphabet does not hold lies at the content's start, 255, 128 and 1 bytes in front of the frame boundaries 1, 16, 17 and
    32 and at the content's end; a 2-byte pattern of alphabet bytes lies every 23 bytes; one 1-byte pattern is the content's last byte
    (the long pattern's last), another one a byte of the alphabet. `stale`: a longer archive of the same frame size whose plaintext is
    made of the four patterns."""
    U = 70 * FS3 + 700
    a = bytearray(_data(np.random.RandomState(3), U))
    short = bytes([5, 17])
    for p in range(7, U - 2, 23):
        a[p:p + 2] = short
    big = bytes(200 + (i % 127) % 50 for i in range(256))
    places = PLACES + [U - 256]
    for p in places:
        a[p:p + 256] = big
    data = bytes(a)
    one, common = data[U - 1:], bytes([9])
    assert set(places) <= set(M.matches(data, big)) and len(M.matches(data, short)) > 2000 and len(M.matches(data, common)) > 500
    arc = _compress(gpu_engine, zra, data, 3, FS3, True)
    filler = ((big + short * 32 + one * 32 + common * 32) * 200)[:75 * FS3]
    stale = _compress(gpu_engine, zra, filler, 3, FS3, True)
    return dict(data=data, arc=arc, d=_dev(arc), pats=[big, short, one, common], U=U, filler=filler, stale=stale, d_stale=_dev(stale))


def test_range_ends(zra, gpu_engine, seams):
    data, arc, d, pats, U = seams["data"], seams["arc"], seams["d"], seams["pats"], seams["U"]
    # the window holds other plaintext, made of the patterns, in every slot and behind the 700 bytes of the last one
    _check(gpu_engine, zra, seams["d_stale"], len(seams["stale"]), seams["filler"], pats)
    ranges = [(0, None), (0, U), (U - 256 - 5, U), (U - 256, U), (U - 255, U), (U - 2, U), (U - 1, U), (69 * FS3 + 5, U - 1)]
    for p in (16 * FS3 - 128, 17 * FS3 - 1):                                   # a long occurrence across a pass boundary of 16 slots
        ranges += [(p - 2100, p + k) for k in (1, 2, 255, 256)]                # hi behind its first byte: 1, 2, 255 and all 256 bytes inside
        ranges += [(p - 2100, p + 256 + k) for k in (1, 2, 255, 256)]          # hi behind its last byte
        ranges += [(p + 1, p + 600), (p + 255, p + 600), (p, p + 256)]         # lo inside it; exactly it
    for staging, slots in ((0, 71), (16 * FS3, 16), (3 * FS3, 3), (1, 1)):
        for lo, hi in ranges:
            want, s = _check(gpu_engine, zra, d, len(arc), data, pats, lo, hi, staging)
            end = U if hi is None else hi
            f0, f1 = lo // FS3, (end - 1) // FS3
            assert (s["frames"], s["decoded"], s["content_bytes"], s["passes"]) == (71, f1 - f0 + 1, min(U, (f1 + 1) * FS3) - f0 * FS3,
                                                                                   -(-(f1 - f0 + 1) // slots)), (lo, hi, staging, s)
            if end == U:
                assert want[-1] == (U - 1, 2)                                  # the 1-byte pattern at the content's last byte
    big_at = [p for p, i in MM.matches_multi(data, pats) if i == 0]
    assert set(PLACES + [U - 256]) <= set(big_at)


# ---- 4
def test_limits(zra, gpu_engine):
    fs = 4096
    rng = np.random.RandomState(44)
    data = _data(rng, 16 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for k, m in ((64, 64), (16, 256)):                                         # 4,096 bytes in all
        pats = [data[o:o + m] for o in rng.randint(0, len(data) - m, size=k - 2)] + [data[:m - 1] + b"\xFF", data[len(data) - m:]]
        want, s = _check(gpu_engine, zra, d, len(arc), data, pats, staging=5 * fs)
        assert len(want) >= k - 1 and want[-1][0] == len(data) - m and s["passes"] == 4, (k, m, len(want), s)
    pats = [bytes([b]) for b in range(64)]                                     # every byte of the alphabet is a pattern
    want, s = _check(gpu_engine, zra, d, len(arc), data, pats)
    assert len(want) == len(data) == s["survivors"]


# ---- 5
@pytest.fixture(scope="module")
def damaged20(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    return dict(data=data, arc=arc, bad=_flip_mid(arc, [7]), fs=fs)


def test_refusals_in_order(zra, gpu_engine, damaged20):
    L = zra.load()
    data, arc, bad, fs = damaged20["data"], damaged20["arc"], damaged20["bad"], damaged20["fs"]
    U = len(data)
    d = _dev(arc)
    P, size = d.data_ptr(), len(arc)
    buf = ctypes.create_string_buffer(b"\x03" * 5000)
    arr = (zra.ZraHipPatternMatch * 2)()
    per = (ctypes.c_uint64 * 65)()
    n = ctypes.c_uint64(0)
    nn = ctypes.byref(n)

    def sz(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    # rule 1, also in front of a range outside the content
    for args in ((None, size, buf, sz(3), 1, 0, MAXU64, 0, arr, 2, nn, per), (P, size, None, sz(3), 1, 0, MAXU64, 0, arr, 2, nn, per),
                 (P, size, buf, None, 1, 0, MAXU64, 0, arr, 2, nn, per), (P, size, buf, sz(3), 1, 0, MAXU64, 0, None, 2, nn, per),
                 (P, size, buf, sz(3), 1, 0, MAXU64, 0, arr, 2, None, per), (P, size, buf, sz(3), 0, 0, MAXU64, 0, arr, 2, nn, per),
                 (P, size, buf, sz(*[1] * 65), 65, 0, MAXU64, 0, arr, 2, nn, per), (P, size, buf, sz(3, 0), 2, 0, MAXU64, 0, arr, 2, nn, per),
                 (P, size, buf, sz(3, 257), 2, 0, MAXU64, 0, arr, 2, nn, per), (P, size, buf, sz(*[256] * 17), 17, 0, MAXU64, 0, arr, 2, nn, per),
                 (P, size, buf, sz(0), 1, size * 99, 5, 0, arr, 2, nn, per)):
        n.value = 0x1234
        ctypes.memset(arr, 0xEE, 32); ctypes.memset(per, 0xEE, 520)
        assert L.ZraHipSearchArchiveMulti(gpu_engine.h, *args).tup() == (1, 42), args[3:6]
        assert n.value == (0x1234 if args[10] is None else 0) and bytes(arr) == b"\xEE" * 32 and bytes(per) == b"\xEE" * 520
        assert set(gpu_engine.search_multi_stats().values()) == {0}
    assert L.ZraHipSearchArchiveMulti(gpu_engine.h, P, size, buf, sz(*[256] * 16), 16, 0, MAXU64, 0, arr, 2, nn, None).tup() == (0, 0) and n.value == 0
    pats = [data[5 * fs + 100:5 * fs + 103], data[9 * fs + 50:9 * fs + 52]]
    # rule 2: truncated archives
    for cut in (0, 10, 38, 42):
        st, got, mem, pm = _raw(gpu_engine, zra, d, cut, pats, 2)
        assert (st, got, mem, pm) == ((5, 0), 0, b"\xEE" * 64, b"\xEE" * 24), cut
        assert set(gpu_engine.search_multi_stats().values()) == {0}
    # rule 3: outside the content
    for lo, ln in ((U + 1, 0), (0, U + 1), (5, MAXU64 - 1), (MAXU64, 1), (U, 1)):
        st, got, mem, pm = _raw(gpu_engine, zra, d, len(arc), pats, 2, lo, ln)
        assert (st, got, mem, pm) == ((5, 0), 0, b"\xEE" * 64, b"\xEE" * 24), (lo, ln, st)
        assert set(gpu_engine.search_multi_stats().values()) == {0}
    # a range shorter than the shortest pattern: Success, nothing decoded, the per-pattern totals zeroed; one byte more is searched
    for lo, ln in ((U, 0), (U, MAXU64), (9 * fs + 50, 1)):
        st, got, mem, pm = _raw(gpu_engine, zra, d, len(arc), pats, 2, lo, ln)
        assert (st, got, mem, pm) == ((0, 0), 0, b"\xEE" * 64, b"\0" * 16 + b"\xEE" * 8), (lo, ln, st)
        assert gpu_engine.search_multi_stats() == dict(frames=20, decoded=0, content_bytes=0, matches=0, listed=0, passes=0, patterns=2, survivors=0)
    assert _multi(gpu_engine, zra, d, len(arc), pats, offset=9 * fs + 50, length=2)[:3] == ((0, 0), 1, [(9 * fs + 50, 1)])
    assert gpu_engine.search_multi_stats()["decoded"] == 1
    # rule 5: a frame with a flipped byte, refused by the decoder's own checks
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for staging in (0, 4 * fs, 1):
        st, got, mem, pm = _raw(gpu_engine, zra, db, len(bad), pats, 6, staging=staging)
        assert (st, got, mem, pm) == ((1, want[7]), 0, b"\xEE" * 128, b"\xEE" * 24), (staging, st, got)
        assert set(gpu_engine.search_multi_stats().values()) == {0}
    # damage outside the range does not disturb the search; one byte of the damaged frame inside does
    for lo, hi in ((0, 7 * fs), (8 * fs, U), (8 * fs - 1, U)):
        ref = MM.matches_multi(data, pats, lo, hi)
        got = _multi(gpu_engine, zra, db, len(bad), pats, offset=lo, length=hi - lo)
        if lo == 8 * fs - 1:
            assert got == ((1, want[7]), 0, [], []), (lo, hi, got[:2])
        else:
            assert got == ((0, 0), len(ref), ref, _per(ref, 2)) and len(ref) > 0, (lo, hi, got[:2])
    # a flipped bit in the seek table, the stored CRC-32 left alone: no complaint about the CRC, the frames decode or they do not
    tb = bytearray(arc); tb[38 + 5 * 7] ^= 1; tb = bytes(tb)
    dt = _dev(tb)
    failing = _frame_status(gpu_engine, zra, tb, d_arc=dt)
    assert set(failing) <= {6, 7}
    ref = MM.matches_multi(data, pats)
    got = _multi(gpu_engine, zra, dt, len(tb), pats)
    assert got == (((1, failing[min(failing)]), 0, [], []) if failing else ((0, 0), len(ref), ref, _per(ref, 2))), got[:2]
    ref = MM.matches_multi(data, pats, 8 * fs)
    assert _multi(gpu_engine, zra, dt, len(tb), pats, offset=8 * fs) == ((0, 0), len(ref), ref, _per(ref, 2)) and len(ref) > 0


# ---- 6
def test_independent_of_the_single_search(zra, gpu_engine, damaged20):
    data, arc, fs = damaged20["data"], damaged20["arc"], damaged20["fs"]
    d = _dev(arc)
    pats = [data[5 * fs + 100:5 * fs + 103], data[9 * fs + 50:9 * fs + 52], data[3 * fs - 20:3 * fs + 20]]
    ref1, refm = M.matches(data, pats[0]), MM.matches_multi(data, pats)

    def single():
        n, at = gpu_engine.search(d.data_ptr(), len(arc), pats[0], staging_bytes=6 * fs)
        assert (n, at) == (len(ref1), ref1)
        return gpu_engine.search_stats()

    s1 = single()
    m1, _ = _check(gpu_engine, zra, d, len(arc), data, pats, staging=3 * fs)
    ms = gpu_engine.search_multi_stats()
    assert gpu_engine.search_stats() == s1 and s1["passes"] == 4 and ms["passes"] == 7
    assert single() == s1 and gpu_engine.search_multi_stats() == ms
    assert gpu_engine.search_multi_scan_ms() > 0
    gpu_engine.release_scratch()                                               # scratch handed back: the same answers from both
    m2, _ = _check(gpu_engine, zra, d, len(arc), data, pats, staging=3 * fs)
    assert m1 == m2 == refm and gpu_engine.search_multi_stats() == ms and single() == s1


# ---- 7
def test_cli_mode_gm(zra, gpu_engine, tmp_path):
    fs = 1024
    a = bytearray(_data(np.random.RandomState(9), 40 * fs + 5))
    needle, other = b"NEEDLE-42", b"E-4"
    places = [3, 7 * fs - 4, 40 * fs - 6]
    for p in places:
        a[p:p + len(needle)] = needle
    data = bytes(a)
    clean = _compress(gpu_engine, zra, data, 3, fs, True)
    p_clean, p_junk = tmp_path / "clean.zra", tmp_path / "junk.zra"
    p_clean.write_bytes(clean); p_junk.write_bytes(b"\x01" * 100)

    def run(*args):
        return subprocess.run([TOOL, "gm"] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    want = MM.matches_multi(data, [needle, other, needle[:1]])
    assert [w for w in want if w[1] < 2] == sorted([(p, 0) for p in places] + [(p + 5, 1) for p in places])
    r = run(p_clean, needle.decode(), "hex:" + other.hex(), "N")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split("\n") == ["%d\t%d" % w for w in want] + ["%d matches" % len(want), ""], r.stdout
    r = run(p_clean, "absent", "hex:fffe")
    assert r.returncode == 1 and r.stdout == "0 matches\n", (r.stdout, r.stderr)
    for args in ((p_junk, "a"), (tmp_path / "missing.zra", "a"), (p_clean, "a", "hex:0"), (p_clean, "a", ""), (p_clean,), [p_clean] + ["a"] * 65):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
