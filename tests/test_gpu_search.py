"""GPU tests of ZraHipSearchArchive (include/zra_hip.h): every content offset at which a byte pattern occurs inside a content range of
a device-resident archive, ascending, without an output buffer. The yardstick everywhere is the plaintext the test generated itself,
scanned on the CPU (tests/search_model.py, cross-checked in tests/test_search_abi.py); for a frame that does not decode, the status
ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it (existing code). Archives are written on the
device. The shapes are the smallest at which each seam exists: occurrences across frames, across passes, across passes shorter than
the pattern, behind a short last frame, at both ends of a range."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import search_model as M
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
CAP = 1 << 16


def _search(eng, zra, d, size, pat, **kw):
    """((zra, zstd), n_matches, [offsets]) of one search"""
    kw.setdefault("max_matches", CAP)
    try:
        n, at = eng.search(d.data_ptr(), size, pat, **kw)
        return (0, 0), n, at
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, []


def _raw(eng, zra, d, size, pat, cap, offset=0, length=MAXU64, staging=0):
    """(status, *nMatches, the bytes of a match array two entries longer than the capacity, 0xEE-filled before the call)"""
    arr = (ctypes.c_uint64 * (cap + 2))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n = ctypes.c_uint64(0x1234)
    eng._order()
    st = zra.load().ZraHipSearchArchive(eng.h, d.data_ptr(), size, pat, len(pat), offset, length, staging, arr if cap else None, cap, ctypes.byref(n)).tup()
    return st, n.value, bytes(arr)


def _listed(mem, k):
    return [int(v) for v in np.frombuffer(mem[:8 * k], dtype=np.uint64)]


# ---- 1
@pytest.mark.parametrize("staging,passes", [(0, 1), (1, 250)])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging, passes):
    """250 frames of 4 bytes: a pattern of 5 bytes straddles two frames, one of 12 spans four, one of 256 spans 64; with one slot the
    carry grows over many passes shorter than m - 1."""
    data = b"abcdefghij" * 100
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    d = _dev(arc)
    for pat in (b"a", b"cdefg", b"abcdefghijab", data[:256], b"ja", b"abd", b"x" * 7):
        want = M.matches(data, pat)
        st, n, at = _search(gpu_engine, zra, d, len(arc), pat, staging_bytes=staging)
        assert (st, n) == ((0, 0), len(want)) and at == want, (pat[:16], st, n, at[:8], want[:8])
        s = gpu_engine.search_stats()
        assert s == dict(frames=250, decoded=250, content_bytes=1000, matches=len(want), listed=len(want), passes=passes), s
    assert M.matches(data, b"a") == list(range(0, 1000, 10)) and M.matches(data, data[:256]) == list(range(0, 750, 10))
    assert M.matches(data, b"abd") == []


# ---- 2
def test_overlaps_and_capacity(zra, gpu_engine):
    fs = 1024
    U = 3 * fs + 5
    arc = _compress(gpu_engine, zra, b"\0" * U, 3, fs, True)
    d = _dev(arc)
    n = U - 2
    for cap in (10, n + 5):
        st, got, mem = _raw(gpu_engine, zra, d, len(arc), b"\0\0\0", cap)
        k = min(n, cap)
        assert (st, got) == ((0, 0), n), (cap, st, got)
        assert _listed(mem, k) == list(range(k)) and mem[8 * k:] == b"\xEE" * (8 * (cap + 2 - k)), cap
        s = gpu_engine.search_stats()
        assert (s["matches"], s["listed"], s["decoded"], s["content_bytes"]) == (n, k, 4, U), s
    st, got, mem = _raw(gpu_engine, zra, d, len(arc), b"\0\0\0", 0)                # NULL array with capacity 0: count only
    assert (st, got, mem) == ((0, 0), n, b"\xEE" * 16)
    assert gpu_engine.search_stats()["listed"] == 0
    assert _search(gpu_engine, zra, d, len(arc), b"\0\0\0", staging_bytes=1) == ((0, 0), n, list(range(n)))


# ---- 3
FS3 = 1024
PLACES = [0] + [k * FS3 - j for k in (1, 16, 17, 32) for j in (255, 128, 1)]


@pytest.fixture(scope="module")
def seams(zra, gpu_engine):
    """70 frames of 1,024 bytes and a last one of 700. A 256-byte pattern of bytes the alphabet does not hold lies at the content's
    start, 255, 128 and 1 bytes in front of the frame boundaries 1, 16, 17 and 32 (period 127: the three copies at one boundary
    overlap and agree) and at the content's end; a 2-byte pattern of alphabet bytes lies every 23 bytes."""
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
    found = M.matches(data, big)
    assert set(places) <= set(found) and len(M.matches(data, short)) > 2000
    arc = _compress(gpu_engine, zra, data, 3, FS3, True)
    return dict(data=data, arc=arc, d=_dev(arc), big=big, short=short, places=places, U=U)


def test_seams_between_frames_and_passes(zra, gpu_engine, seams):
    data, arc, d = seams["data"], seams["arc"], seams["d"]
    want = {k: M.matches(data, seams[k]) for k in ("big", "short")}

    def check():
        for staging, passes in ((0, 1), (16 * FS3, 5), (3 * FS3, 24), (1, 71)):     # 16 slots: the boundaries 16 and 32 lie between passes
            for k in ("big", "short"):
                st, n, at = _search(gpu_engine, zra, d, len(arc), seams[k], staging_bytes=staging)
                assert (st, n) == ((0, 0), len(want[k])), (k, staging, st, n, len(want[k]))
                assert at == want[k], (k, staging, sorted(set(at) ^ set(want[k]))[:10])
                s = gpu_engine.search_stats()
                assert s == dict(frames=71, decoded=71, content_bytes=seams["U"], matches=n, listed=n, passes=passes), (k, staging, s)

    check()
    gpu_engine.release_scratch()                                               # scratch handed back in between: the same answers
    check()


# ---- 4
def test_stale_bytes_are_never_matched(zra, gpu_engine):
    """One slot: the short last frame lands on the plaintext of frame 4, whose bytes from 300 on stay where they were."""
    fs = 1024
    U = 5 * fs + 300
    a = bytearray(_data(np.random.RandomState(4), U))
    marker = bytes(range(230, 246))
    for o in (290, 500, 1000):                                                 # 290: across the place where the last frame's content will end
        a[4 * fs + o:4 * fs + o + 16] = marker
    data = bytes(a)
    seam = data[U - 8:] + data[4 * fs + 300:4 * fs + 308]                      # occurs only where stale bytes follow the last frame
    assert M.matches(data, seam) == [] and M.matches(data, marker) == [4 * fs + 290, 4 * fs + 500, 4 * fs + 1000]
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for staging, passes in ((1, 6), (5 * fs, 2), (0, 1)):
        assert _search(gpu_engine, zra, d, len(arc), marker, staging_bytes=staging) == ((0, 0), 3, M.matches(data, marker)), staging
        assert gpu_engine.search_stats()["passes"] == passes
        assert _search(gpu_engine, zra, d, len(arc), seam, staging_bytes=staging) == ((0, 0), 0, []), staging
        # the last frame's own tail is found where it is
        tail = M.matches(data, data[U - 8:])
        assert tail[-1] == U - 8
        assert _search(gpu_engine, zra, d, len(arc), data[U - 8:], staging_bytes=staging) == ((0, 0), len(tail), tail), staging


# ---- 5
def test_ranges(zra, gpu_engine, seams):
    data, arc, d, big, short, U = seams["data"], seams["arc"], seams["d"], seams["big"], seams["short"], seams["U"]

    def both(pat, lo, hi, **kw):
        """the search of [lo, hi) and the model's answer"""
        got = _search(gpu_engine, zra, d, len(arc), pat, offset=lo, length=None if hi is None else hi - lo, **kw)
        want = M.matches(data, pat, lo, hi)
        return got, ((0, 0), len(want), want)

    for p in (16 * FS3 - 128, 17 * FS3 - 1):
        for staging in (0, 16 * FS3, 1):
            got, want = both(big, p, p + 256, staging_bytes=staging)           # exactly the occurrence
            assert got == want == ((0, 0), 1, [p]), (p, staging, got)
            got, want = both(big, p + 1, U, staging_bytes=staging)             # cut at its first byte
            assert got == want and p not in got[2] and got[1] > 0, (p, staging, got)
            got, want = both(big, 0, p + 255, staging_bytes=staging)           # cut at its last byte
            assert got == want and p not in got[2] and got[1] > 0, (p, staging, got)
            got, want = both(big, p, p + 255, staging_bytes=staging)           # a range shorter than the pattern
            assert got == want == ((0, 0), 0, []), (p, staging, got)
            assert gpu_engine.search_stats() == dict(frames=71, decoded=0, content_bytes=0, matches=0, listed=0, passes=0)
    # inside one frame
    got, want = both(short, 3 * FS3 + 10, 3 * FS3 + 510)
    assert got == want and got[1] > 10, got
    s = gpu_engine.search_stats()
    assert (s["decoded"], s["content_bytes"], s["passes"]) == (1, FS3, 1), s
    # from the middle of frame 20 to the middle of frame 40
    for pat in (short, big):
        for staging in (0, 4 * FS3):
            got, want = both(pat, 20 * FS3 + 512, 40 * FS3 + 512, staging_bytes=staging)
            assert got == want, (staging, got[:2], want[:2])
            s = gpu_engine.search_stats()
            assert (s["decoded"], s["content_bytes"], s["passes"]) == (21, 21 * FS3, 1 if not staging else 6), s
    # to the end
    got, want = both(big, 31 * FS3 + 5, None, staging_bytes=8 * FS3)
    assert got == want and got[2][-1] == U - 256, got
    s = gpu_engine.search_stats()
    assert (s["decoded"], s["content_bytes"]) == (40, U - 31 * FS3), s
    got, want = both(short, U - 2, None)
    assert got == want
    # nothing to search
    for length in (0, None):
        assert _search(gpu_engine, zra, d, len(arc), short, offset=U, length=length) == ((0, 0), 0, [])
        assert gpu_engine.search_stats()["decoded"] == 0
    # outside the content
    for lo, ln in ((U + 1, 0), (0, U + 1), (5, MAXU64 - 1), (MAXU64, 1), (U, 1)):
        st, n, mem = _raw(gpu_engine, zra, d, len(arc), short, 4, lo, ln)
        assert (st, n, mem) == ((5, 0), 0, b"\xEE" * 48), (lo, ln, st, n)
        assert set(gpu_engine.search_stats().values()) == {0}


# ---- 6
@pytest.mark.parametrize("level", [1, 3, 9])
@pytest.mark.parametrize("ck", [True, False])
@pytest.mark.parametrize("fs,nfr", [(65536, 9), (262144, 4)])
def test_real_frame_sizes(zra, gpu_engine, fs, nfr, ck, level):
    U = nfr * fs + fs // 3 + 1
    a = bytearray(_data(np.random.RandomState(fs + level), U))
    planted = bytes([201, 202, 203, 204, 205, 206, 207, 208])
    for k in range(1, nfr + 1):
        a[k * fs - 4:k * fs + 4] = planted                                      # across every frame boundary
    data = bytes(a)
    arc = _compress(gpu_engine, zra, data, level, fs, ck)
    d = _dev(arc)
    common = data[1000:1003]
    for pat in (common, planted):
        want = M.matches(data, pat)
        st, n, at = _search(gpu_engine, zra, d, len(arc), pat)
        assert (st, n) == ((0, 0), len(want)) and at == want, (st, n, len(want))
        s = gpu_engine.search_stats()
        assert s == dict(frames=nfr + 1, decoded=nfr + 1, content_bytes=U, matches=n, listed=n, passes=1), s
    assert M.matches(data, planted) == [k * fs - 4 for k in range(1, nfr + 1)] and len(M.matches(data, common)) > 20
    assert gpu_engine.kernel_stats()["dec_launches"] >= 1 and gpu_engine.search_scan_ms() > 0


# ---- 7
@pytest.fixture(scope="module")
def damaged20(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    return dict(data=data, arc=arc, bad=_flip_mid(arc, [7]), fs=fs)


def test_damaged_frames(zra, gpu_engine, damaged20):
    data, arc, bad, fs = damaged20["data"], damaged20["arc"], damaged20["bad"], damaged20["fs"]
    U = len(data)
    pat = data[5 * fs + 100:5 * fs + 103]
    d = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=d)
    assert set(want) == {7} and want[7] != 0, want
    for staging in (0, 4 * fs, 1):
        st, n, mem = _raw(gpu_engine, zra, d, len(bad), pat, 6, staging=staging)
        assert (st, n, mem) == ((1, want[7]), 0, b"\xEE" * 64), (staging, st, n)
        assert set(gpu_engine.search_stats().values()) == {0}
    # the frames outside the range are not touched
    for lo, hi in ((0, 7 * fs), (8 * fs, U), (8 * fs - 1, U)):
        ref = M.matches(data, pat, lo, hi)
        got = _search(gpu_engine, zra, d, len(bad), pat, offset=lo, length=hi - lo)
        if lo == 8 * fs - 1:
            assert got == ((1, want[7]), 0, []), (lo, hi, got[:2])             # one byte of the damaged frame is inside
        else:
            assert got == ((0, 0), len(ref), ref) and len(ref) > 0, (lo, hi, got[:2])
    # two damaged frames in different passes: the lower one's status, and the call stops behind its pass
    bad2 = _flip_mid(arc, [7, 15])
    d2 = _dev(bad2)
    want2 = _frame_status(gpu_engine, zra, bad2, d_arc=d2)
    assert set(want2) == {7, 15}
    assert _search(gpu_engine, zra, d2, len(bad2), pat, staging_bytes=4 * fs) == ((1, want2[7]), 0, [])
    assert _search(gpu_engine, zra, d2, len(bad2), pat, offset=8 * fs, staging_bytes=4 * fs) == ((1, want2[15]), 0, [])
    # and the sound archive answers
    ref = M.matches(data, pat)
    assert _search(gpu_engine, zra, _dev(arc), len(arc), pat) == ((0, 0), len(ref), ref)


# ---- 8
def test_refusals_and_header_statuses(zra, gpu_engine, damaged20):
    L = zra.load()
    data, arc, fs = damaged20["data"], damaged20["arc"], damaged20["fs"]
    d = _dev(arc)
    P, size = d.data_ptr(), len(arc)
    pat = ctypes.create_string_buffer(b"\x03" * 300)
    arr = (ctypes.c_uint64 * 2)()
    ctypes.memset(arr, 0xEE, 16)
    n = ctypes.c_uint64(0x1234)
    nn = ctypes.byref(n)
    for args in ((None, size, pat, 3, 0, MAXU64, 0, arr, 2, nn), (P, size, None, 3, 0, MAXU64, 0, arr, 2, nn), (P, size, pat, 3, 0, MAXU64, 0, None, 2, nn),
                 (P, size, pat, 0, 0, MAXU64, 0, arr, 2, nn), (P, size, pat, 257, 0, MAXU64, 0, arr, 2, nn), (P, size, pat, 3, 0, MAXU64, 0, arr, 2, None),
                 (P, size, pat, 0, size * 99, 5, 0, arr, 2, nn)):                   # (rule 1 comes before the range)
        n.value = 0x1234
        assert L.ZraHipSearchArchive(gpu_engine.h, *args).tup() == (1, 42), args[2:6]
        assert n.value == (0x1234 if args[-1] is None else 0) and bytes(arr) == b"\xEE" * 16
        assert set(gpu_engine.search_stats().values()) == {0}
    assert L.ZraHipSearchArchive(gpu_engine.h, P, size, pat, 256, 0, MAXU64, 0, arr, 2, nn).tup() == (0, 0) and n.value == 0   # 256 is allowed
    # truncated archives
    for cut in (0, 10, 38, 42):
        st, got, mem = _raw(gpu_engine, zra, d, cut, b"\x03\x04", 2)
        assert (st, got, mem) == ((5, 0), 0, b"\xEE" * 32), cut
    # a flipped bit in the seek table, the stored CRC-32 left alone: no complaint about the CRC, the frames decode or they do not
    bad = bytearray(arc); bad[38 + 5 * 7] ^= 1; bad = bytes(bad)
    db = _dev(bad)
    pat2 = data[9 * fs + 50:9 * fs + 53]
    failing = _frame_status(gpu_engine, zra, bad, d_arc=db)
    print("seek-table bit: frames that do not decode", failing)
    assert set(failing) <= {6, 7}
    ref = M.matches(data, pat2)
    got = _search(gpu_engine, zra, db, len(bad), pat2)
    assert got == (((1, failing[min(failing)]), 0, []) if failing else ((0, 0), len(ref), ref)), got[:2]
    ref = M.matches(data, pat2, 8 * fs)
    assert _search(gpu_engine, zra, db, len(bad), pat2, offset=8 * fs) == ((0, 0), len(ref), ref) and len(ref) > 0


# ---- 9
def test_cli_mode_g(zra, gpu_engine, damaged20, tmp_path):
    fs = 1024
    a = bytearray(_data(np.random.RandomState(9), 40 * fs + 5))
    needle = b"NEEDLE-42"
    places = [3, 7 * fs - 4, 40 * fs - 6]
    for p in places:
        a[p:p + len(needle)] = needle
    clean = _compress(gpu_engine, zra, bytes(a), 3, fs, True)
    p_clean, p_bad, p_junk = tmp_path / "clean.zra", tmp_path / "bad.zra", tmp_path / "junk.zra"
    p_clean.write_bytes(clean); p_bad.write_bytes(damaged20["bad"]); p_junk.write_bytes(b"\x01" * 100)

    def run(*args):
        return subprocess.run([TOOL, "g"] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    r = run(p_clean, needle.decode())
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split("\n") == [str(p) for p in places] + ["3 matches", ""], r.stdout
    h = run(p_clean, "hex:" + needle.hex())
    assert h.returncode == 0 and h.stdout == r.stdout, (h.stdout, h.stderr)
    r = run(p_clean, "absent")
    assert r.returncode == 1 and r.stdout == "0 matches\n", (r.stdout, r.stderr)
    for args in ((p_junk, "a"), (p_bad, "a"), (tmp_path / "missing.zra", "a"), (p_clean, "hex:0"), (p_clean, "")):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
