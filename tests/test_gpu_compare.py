"""GPU tests of ZraHipCompareArchives (include/zra_hip.h): the maximal runs of content positions at which two device-resident archives
differ, ascending, without an output buffer. The yardstick everywhere is the pair of plaintexts the test generated itself, compared on
the CPU (tests/compare_model.py, cross-checked in tests/test_compare_abi.py); for a frame that does not decode, the status
ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it (existing code). Archives are written on the
device. The shapes are the smallest at which each seam exists: runs across frames, across passes, next to frames that are not decoded,
behind a short last frame, at both ends of a range."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compare_model as M
from test_gpu_update import _compress, _data, _dev, _update
from test_gpu_verify import _flip_mid, _frame_status
import verify_model as VM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
ZERO = dict.fromkeys(("frames", "equal_compressed", "decoded", "content_bytes", "ranges", "listed", "passes"), 0)


def _cmp(eng, zra, a, b, **kw):
    """((zra, zstd), n_ranges, differing_bytes, [(offset, size)]) of one compare of the archives a and b = (device tensor, size)"""
    try:
        n, nb, at = eng.compare(a[0].data_ptr(), a[1], b[0].data_ptr(), b[1], **kw)
        return (0, 0), n, nb, at
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, 0, []


def _raw(eng, zra, a, b, cap, mode=0, offset=0, length=MAXU64, staging=0):
    """(status, *nRanges, *differingBytes, the bytes of a range array two entries longer than the capacity, 0xEE-filled before)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, nb = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
    eng._order()
    st = zra.load().ZraHipCompareArchives(eng.h, a[0].data_ptr(), a[1], b[0].data_ptr(), b[1], mode, offset, length, staging, arr if cap else None, cap,
                                          ctypes.byref(n), ctypes.byref(nb)).tup()
    return st, n.value, nb.value, bytes(arr)


def _listed(mem, k):
    v = np.frombuffer(mem[:16 * k], dtype=np.uint64)
    return [(int(v[2 * i]), int(v[2 * i + 1])) for i in range(k)]


def _pair(eng, zra, data, fs, level=3, ck=True):
    arc = _compress(eng, zra, data, level, fs, ck)
    return (_dev(arc), len(arc)), arc


def _want(a, b, lo=0, hi=None):
    r = M.ranges(a, b, lo, hi)
    return (0, 0), len(r), sum(s for _, s in r), r


def _break_magic(arc, frames):
    """the first byte of the frames' compressed spans changed: another failure, and another code, than _flip_mid's"""
    hs, e = VM.fields(arc)[0], VM.entries(arc)
    a = bytearray(arc)
    for k in frames:
        a[hs + e[k]] ^= 1
    return bytes(a)


def _changed(a, b, fs):
    """the frames of the common content whose bytes differ, or whose lengths do"""
    c = min(len(a), len(b))
    return {f for f in range(-(-c // fs)) if a[f * fs:(f + 1) * fs] != b[f * fs:(f + 1) * fs]}


# ---- 1
RUNS4 = [(0, 1), (2, 1),              # two runs one equal byte apart inside a frame, the first at the content's start
         (13, 1),                     # a run of 1 byte
         (40, 4),                     # exactly frame 10
         (83, 9),                     # the last byte of frame 20, frames 21 and 22
         (118, 2),                    # ends on the boundary 30, frame 30 equal
         (200, 2),                    # starts on the boundary 50, frame 49 equal
         (298, 2), (301, 2),          # one equal byte apart across the boundary 75
         (396, 12),                   # three whole frames
         (998, 2)]                    # to the content's end


@pytest.mark.parametrize("staging,passes", [(0, 1), (1, 250)])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging, passes):
    """250 frames of 4 bytes, in one pass and in 250: every run shape against frames that are decoded and frames that are not."""
    a = b"abcdefghij" * 100
    b = bytearray(a)
    for off, n in RUNS4:
        b[off:off + n] = a[off:off + n].upper()
    b = bytes(b)
    assert M.ranges(a, b) == RUNS4
    A, _ = _pair(gpu_engine, zra, a, 4)
    B, _ = _pair(gpu_engine, zra, b, 4)
    changed = _changed(a, b, 4)
    assert len(changed) == 14
    for decode_all in (False, True):
        got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging, decode_all=decode_all)
        assert got == _want(a, b), (decode_all, got)
        s = gpu_engine.compare_stats()
        want = M.stats(a, b, 4, decoded=None if decode_all else changed, slots=None if passes == 1 else 1)
        assert s == want and s["passes"] == passes, (decode_all, s, want)
        assert gpu_engine.compare_sizes() == (1000, 1000)
    got = _cmp(gpu_engine, zra, B, A, staging_bytes=staging)                   # the other way round
    assert got == _want(a, b), got


# ---- 2
FS2 = 1024


@pytest.fixture(scope="module")
def updated(zra, gpu_engine):
    """64 frames of 1,024 bytes and a last one of 700; an update writes inside frame 5 and across the boundary between the 16th and the
    17th frame (frames 15 and 16), and appends 300 bytes."""
    from test_gpu_update import _patched
    rng = np.random.RandomState(2)
    old = _data(rng, 64 * FS2 + 700)
    writes = [(5 * FS2 + 100, rng.randint(128, 256, size=50).astype(np.uint8).tobytes()),
              (16 * FS2 - 20, rng.randint(128, 256, size=40).astype(np.uint8).tobytes())]
    app = rng.randint(128, 256, size=300).astype(np.uint8).tobytes()
    arc = _compress(gpu_engine, zra, old, 3, FS2, True)
    st, out, size = _update(gpu_engine, zra, arc, writes, app)
    assert st == (0, 0)
    new_arc = out[:size]
    new = _patched(old, writes, app)
    return dict(old=old, new=new, A=(_dev(arc), len(arc)), B=(_dev(new_arc), len(new_arc)))


def test_update_is_the_producer(zra, gpu_engine, updated):
    """The update carries every untouched frame over byte for byte: those are equal by their compressed bytes. Decoded are the three
    written frames 5, 15 and 16, and a fourth pair: the append grows the last frame from 700 to 1,000 bytes, it is encoded again and
    lies inside the common content (and holds no range). A range that ends in front of the last frame decodes the three."""
    old, new, A, B = updated["old"], updated["new"], updated["A"], updated["B"]
    want = _want(old, new)
    assert want[1] == 2 and want[3][1][0] == 16 * FS2 - 20 and want[3][1][1] == 40

    def check():
        for staging, passes, slots in ((0, 1, None), (2 * 16 * FS2, 5, 16), (1, 65, 1)):   # 16 slots: the boundary 16 lies between passes
            got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging)
            assert got == want, (staging, got)
            s = gpu_engine.compare_stats()
            assert s == M.stats(old, new, FS2, decoded={5, 15, 16, 64}, slots=slots), (staging, s)
            assert (s["decoded"], s["equal_compressed"], s["passes"]) == (4, 61, passes), s
            assert gpu_engine.compare_sizes() == (len(old), len(new))
            got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging, length=64 * FS2)      # without the last frame: the three written ones
            assert got == want and gpu_engine.compare_stats()["decoded"] == 3, (staging, got)
            assert _cmp(gpu_engine, zra, A, B, staging_bytes=staging, decode_all=True) == want, staging
            assert gpu_engine.compare_stats()["decoded"] == 65

    check()
    gpu_engine.release_scratch()                                               # scratch handed back in between: the same answers
    check()


# ---- 3
def test_same_content_at_two_levels(zra, gpu_engine):
    import torch
    fs = 4096
    data = _data(np.random.RandomState(3), 20 * fs)
    A, _ = _pair(gpu_engine, zra, data, fs, 3)
    B, _ = _pair(gpu_engine, zra, data, fs, 9)
    assert _cmp(gpu_engine, zra, A, B) == ((0, 0), 0, 0, [])
    s = gpu_engine.compare_stats()
    print("level 3 against level 9:", s)
    assert s["decoded"] + s["equal_compressed"] == s["frames"] == 20 and s["ranges"] == 0, s
    A2 = (A[0].clone(), A[1])                                                  # an archive against a device copy of itself
    torch.cuda.synchronize()
    assert _cmp(gpu_engine, zra, A, A2) == ((0, 0), 0, 0, [])
    s = gpu_engine.compare_stats()
    assert s == dict(ZERO, frames=20, equal_compressed=20, passes=1), s
    assert gpu_engine.kernel_stats()["dec_launches"] == 0
    assert _cmp(gpu_engine, zra, A, A2, decode_all=True) == ((0, 0), 0, 0, [])
    s = gpu_engine.compare_stats()
    assert s == dict(ZERO, frames=20, decoded=20, content_bytes=20 * fs, passes=1), s
    assert gpu_engine.kernel_stats()["dec_launches"] >= 1


# ---- 4
def test_stale_bytes_are_never_reported(zra, gpu_engine):
    """One slot per half: the short last frame lands on the plaintext of frame 4, whose bytes from 300 on stay where they were, and
    differ between the halves."""
    fs = 1024
    U = 5 * fs + 300
    a = bytearray(_data(np.random.RandomState(4), U))
    b = bytearray(a)
    for p in list(range(4 * fs + 296, 5 * fs)) + [5 * fs + 7, U - 2, U - 1]:   # frame 4 from 296 on; the last frame's last two bytes
        b[p] = a[p] ^ 0x80
    a, b = bytes(a), bytes(b)
    A, _ = _pair(gpu_engine, zra, a, fs)
    B, _ = _pair(gpu_engine, zra, b, fs)
    want = _want(a, b)
    assert want[3] == [(4 * fs + 296, fs - 296), (5 * fs + 7, 1), (U - 2, 2)]
    for staging, passes in ((1, 6), (2 * 5 * fs, 2), (0, 1)):
        for decode_all in (False, True):
            got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging, decode_all=decode_all)
            assert got == want, (staging, decode_all, got)
            assert gpu_engine.compare_stats()["passes"] == passes
    got = _cmp(gpu_engine, zra, A, B, staging_bytes=1, offset=5 * fs + 8)
    assert got == ((0, 0), 1, 2, [(U - 2, 2)]), got


# ---- 5
def test_capacity(zra, gpu_engine):
    fs = 1024
    U = 3 * fs + 5
    a = bytes(U)
    b = bytes(1 if p % 2 == 0 else 0 for p in range(U))
    A, _ = _pair(gpu_engine, zra, a, fs)
    B, _ = _pair(gpu_engine, zra, b, fs)
    n = (U + 1) // 2
    ref = M.ranges(a, b)
    assert len(ref) == n and ref[:2] == [(0, 1), (2, 1)] and ref[-1] == (U - 1, 1)
    for cap in (10, n + 5):
        for staging in (0, 1):
            st, got, nb, mem = _raw(gpu_engine, zra, A, B, cap, staging=staging)
            k = min(n, cap)
            assert (st, got, nb) == ((0, 0), n, n), (cap, st, got, nb)
            assert _listed(mem, k) == ref[:k] and mem[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), cap
            s = gpu_engine.compare_stats()
            assert (s["ranges"], s["listed"], s["decoded"], s["content_bytes"]) == (n, k, 4, U), s
    st, got, nb, mem = _raw(gpu_engine, zra, A, B, 0)                          # NULL array with capacity 0: count only
    assert (st, got, nb, mem) == ((0, 0), n, n, b"\xEE" * 32)
    assert gpu_engine.compare_stats()["listed"] == 0


# ---- 6
FS6 = 1024


@pytest.fixture(scope="module")
def seams(zra, gpu_engine):
    """70 frames of 1,024 bytes and a last one of 700 against a copy with runs of 30 bytes inside frames 3, 20, 30 and 40, runs of 40
    bytes across the boundaries 16, 17 and 32, and 300 bytes more at the end."""
    U = 70 * FS6 + 700
    a = _data(np.random.RandomState(6), U)
    b = bytearray(a)
    runs = [(3 * FS6 + 10, 30), (16 * FS6 - 20, 40), (17 * FS6 - 20, 40), (20 * FS6 + 700, 30), (30 * FS6 + 5, 30), (32 * FS6 - 20, 40), (40 * FS6 + 100, 30)]
    for p, n in runs:
        for q in range(p, p + n):
            b[q] = a[q] ^ 0x80
    b = bytes(b) + bytes(range(200, 250)) * 6
    assert M.ranges(a, b) == runs
    return dict(a=a, b=b, A=_pair(gpu_engine, zra, a, FS6)[0], B=_pair(gpu_engine, zra, b, FS6)[0], U=U, runs=runs)


def test_ranges(zra, gpu_engine, seams):
    a, b, A, B, U = seams["a"], seams["b"], seams["A"], seams["B"], seams["U"]

    def both(lo, hi, **kw):
        return _cmp(gpu_engine, zra, A, B, offset=lo, length=None if hi is None else hi - lo, **kw), _want(a, b, lo, hi)

    for staging in (0, 2 * 16 * FS6, 1):
        got, want = both(0, None, staging_bytes=staging)
        assert got == want and got[1] == 7, (staging, got)
        assert gpu_engine.compare_sizes() == (U, U + 300)
        p = 16 * FS6 - 20
        got, want = both(p + 10, p + 30, staging_bytes=staging)               # a run cut at lo and at hi, across a boundary
        assert got == want == ((0, 0), 1, 20, [(p + 10, 20)]), (staging, got)
        got, want = both(p + 39, U, staging_bytes=staging)                    # its last byte
        assert got == want and got[3][0] == (p + 39, 1), (staging, got)
        got, want = both(0, p + 1, staging_bytes=staging)                     # its first byte
        assert got == want and got[3][-1] == (p, 1), (staging, got)
        got, want = both(p + 40, 17 * FS6 - 20, staging_bytes=staging)        # between two runs
        assert got == want == ((0, 0), 0, 0, []), (staging, got)
    # inside one frame
    p = 20 * FS6 + 700
    got, want = both(p + 10, p + 20)
    assert got == want == ((0, 0), 1, 10, [(p + 10, 10)]), got
    s = gpu_engine.compare_stats()
    assert s == dict(frames=1, equal_compressed=0, decoded=1, content_bytes=10, ranges=1, listed=1, passes=1), s
    # from the middle of frame 20 to the middle of frame 40
    for staging, passes in ((0, 1), (2 * 4 * FS6, 6)):
        got, want = both(20 * FS6 + 512, 40 * FS6 + 512, staging_bytes=staging)
        assert got == want and got[1] == 4, (staging, got)
        s = gpu_engine.compare_stats()
        assert (s["frames"], s["decoded"], s["equal_compressed"], s["passes"]) == (21, 5, 16, passes) and s["decoded"] <= 21, s
        got, want = both(20 * FS6 + 512, 40 * FS6 + 512, staging_bytes=staging, decode_all=True)
        assert got == want
        s = gpu_engine.compare_stats()
        assert (s["decoded"], s["content_bytes"], s["passes"]) == (21, 20 * FS6, passes), s
    # nothing to compare
    for length in (0, None):
        assert _cmp(gpu_engine, zra, A, B, offset=U, length=length) == ((0, 0), 0, 0, [])
        assert gpu_engine.compare_stats() == ZERO and gpu_engine.kernel_stats()["dec_launches"] == 0
        assert gpu_engine.compare_sizes() == (U, U + 300)
    # outside the common content: UA < UB, the bound is UA whichever side is the shorter one
    for x, y in ((A, B), (B, A)):
        for lo, ln in ((U + 1, 0), (0, U + 1), (5, MAXU64 - 1), (MAXU64, 1), (U, 1), (U + 1, MAXU64)):
            st, n, nb, mem = _raw(gpu_engine, zra, x, y, 4, offset=lo, length=ln)
            assert (st, n, nb, mem) == ((5, 0), 0, 0, b"\xEE" * 96), (lo, ln, st, n)
            assert gpu_engine.compare_stats() == ZERO and gpu_engine.compare_sizes() == (0, 0)
    got = _cmp(gpu_engine, zra, B, A)
    assert got == _want(a, b) and gpu_engine.compare_sizes() == (U + 300, U)


# ---- 7
@pytest.mark.parametrize("level", [1, 3, 9])
@pytest.mark.parametrize("fs,nfr", [(65536, 9), (262144, 4)])
def test_real_frame_sizes(zra, gpu_engine, fs, nfr, level):
    U = nfr * fs + fs // 3 + 1
    a = _data(np.random.RandomState(fs + level), U)
    b = bytearray(a)
    for k in range(1, nfr + 1):
        for q in range(k * fs - 4, k * fs + 4):                                # 8 bytes across every frame boundary
            b[q] = a[q] ^ 0x80
    for k in range(nfr + 1):
        q = k * fs + 1000 + 1031 * k                                           # and one byte per frame, at changing alignments
        b[q] = a[q] ^ 0x80
    b = bytes(b)
    A, _ = _pair(gpu_engine, zra, a, fs, level)
    B, _ = _pair(gpu_engine, zra, b, fs, 3)
    want = _want(a, b)
    assert want[1] == 2 * nfr + 1 and want[2] == 9 * nfr + 1
    for decode_all in (False, True):
        got = _cmp(gpu_engine, zra, A, B, decode_all=decode_all)
        assert got == want, (decode_all, got)
        s = gpu_engine.compare_stats()
        assert s == M.stats(a, b, fs), s
    assert gpu_engine.kernel_stats()["dec_launches"] >= 1 and gpu_engine.compare_ms() > 0
    # the same content on both sides: at the same level every frame is equal by its compressed bytes
    B2, _ = _pair(gpu_engine, zra, a, fs, 3)
    assert _cmp(gpu_engine, zra, A, B2) == ((0, 0), 0, 0, [])
    s = gpu_engine.compare_stats()
    assert s["decoded"] + s["equal_compressed"] == nfr + 1 and (level != 3 or s["decoded"] == 0), s


# ---- 8
@pytest.fixture(scope="module")
def damaged20(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    return dict(data=data, arc=arc, fs=fs)


def test_damaged_frames(zra, gpu_engine, damaged20):
    data, arc, fs = damaged20["data"], damaged20["arc"], damaged20["fs"]
    U = len(data)
    bad = _flip_mid(arc, [7])
    G, D = (_dev(arc), len(arc)), (_dev(bad), len(bad))
    want = _frame_status(gpu_engine, zra, bad, d_arc=D[0])
    assert set(want) == {7} and want[7] != 0, want
    for x, y in ((D, G), (G, D)):                                              # frame 7 flipped in A only, in B only: its spans differ, it is decoded
        for staging in (0, 2 * 4 * fs, 1):
            st, n, nb, mem = _raw(gpu_engine, zra, x, y, 6, staging=staging)
            assert (st, n, nb, mem) == ((1, want[7]), 0, 0, b"\xEE" * 128), (staging, st, n)
            assert gpu_engine.compare_stats() == ZERO and gpu_engine.compare_sizes() == (0, 0)
    # ranges that avoid frame 7
    for lo, hi in ((0, 7 * fs), (8 * fs, U)):
        assert _cmp(gpu_engine, zra, D, G, offset=lo, length=hi - lo) == ((0, 0), 0, 0, []), (lo, hi)
        assert _cmp(gpu_engine, zra, D, G, offset=lo, length=hi - lo, decode_all=True) == ((0, 0), 0, 0, []), (lo, hi)
    assert _cmp(gpu_engine, zra, D, G, offset=8 * fs - 1)[0] == (1, want[7])   # one byte of the damaged frame is inside
    # two frames damaged in different ways, in different passes: the lower one's status, and the call stops behind its pass
    bad2 = _break_magic(bad, [15])
    D2 = (_dev(bad2), len(bad2))
    want2 = _frame_status(gpu_engine, zra, bad2, d_arc=D2[0])
    assert set(want2) == {7, 15} and want2[7] == want[7] and want2[15] not in (0, want[7]), want2
    assert _cmp(gpu_engine, zra, D2, G, staging_bytes=2 * 4 * fs)[0] == (1, want2[7])
    assert _cmp(gpu_engine, zra, D2, G, offset=8 * fs, staging_bytes=2 * 4 * fs)[0] == (1, want2[15])
    # the lowest frame index wins whichever side it is on: 15 in A, 7 in B, one pass
    bad15 = _break_magic(arc, [15])
    D15 = (_dev(bad15), len(bad15))
    assert _cmp(gpu_engine, zra, D15, D)[0] == (1, want[7])
    assert _cmp(gpu_engine, zra, D, D15)[0] == (1, want[7])
    assert _cmp(gpu_engine, zra, D15, G)[0] == (1, want2[15]) and _cmp(gpu_engine, zra, G, D15)[0] == (1, want2[15])
    # the same frame failing on both sides, in different ways: A before B
    other7 = _break_magic(arc, [7])
    O7 = (_dev(other7), len(other7))
    code7 = _frame_status(gpu_engine, zra, other7, d_arc=O7[0])[7]
    assert code7 not in (0, want[7])
    assert _cmp(gpu_engine, zra, D, O7)[0] == (1, want[7]) and _cmp(gpu_engine, zra, O7, D)[0] == (1, code7)
    assert _cmp(gpu_engine, zra, D, O7, decode_all=True, staging_bytes=1)[0] == (1, want[7])
    # the same flip on both sides: equal without being decoded (the documented limit), frame 7's status when everything is decoded
    Dc = (_dev(bad), len(bad))
    assert _cmp(gpu_engine, zra, D, Dc) == ((0, 0), 0, 0, [])
    s = gpu_engine.compare_stats()
    assert s == dict(ZERO, frames=20, equal_compressed=20, passes=1), s
    assert _cmp(gpu_engine, zra, D, Dc, decode_all=True)[0] == (1, want[7])
    assert gpu_engine.compare_stats() == ZERO
    # and the sound archive answers
    assert _cmp(gpu_engine, zra, G, (_dev(arc), len(arc)), decode_all=True) == ((0, 0), 0, 0, [])


# ---- 9
def test_refusals_in_order(zra, gpu_engine, damaged20):
    L = zra.load()
    arc, fs = damaged20["arc"], damaged20["fs"]
    d = _dev(arc)
    P, size = d.data_ptr(), len(arc)
    arr = (ctypes.c_uint64 * 4)()
    ctypes.memset(arr, 0xEE, 32)
    n, nb = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
    nn, bb = ctypes.byref(n), ctypes.byref(nb)
    for args in ((None, size, P, size, 0, 0, MAXU64, 0, arr, 2, nn, bb), (P, size, None, size, 0, 0, MAXU64, 0, arr, 2, nn, bb),
                 (P, size, P, size, 0, 0, MAXU64, 0, None, 2, nn, bb), (P, size, P, size, 2, 0, MAXU64, 0, arr, 2, nn, bb),
                 (P, size, P, size, 0x80000001, 0, MAXU64, 0, arr, 2, nn, bb), (P, size, P, size, 0, 0, MAXU64, 0, arr, 2, None, bb),
                 (P, size, P, size, 4, size * 99, 5, 0, arr, 2, nn, bb),           # (rule 1 comes before the range)
                 (P, 10, P, size, 4, 0, MAXU64, 0, arr, 2, nn, bb)):               # (and before the headers)
        n.value = nb.value = 0x1234
        assert L.ZraHipCompareArchives(gpu_engine.h, *args).tup() == (1, 42), args[4:8]
        assert n.value == (0x1234 if args[-2] is None else 0) and nb.value == 0 and bytes(arr) == b"\xEE" * 32
        assert gpu_engine.compare_stats() == ZERO
    assert L.ZraHipCompareArchives(gpu_engine.h, P, size, P, size, 1, 0, MAXU64, 0, arr, 2, nn, None).tup() == (0, 0) and n.value == 0   # differingBytes may be NULL
    A = (d, size)
    # truncated A, then truncated B; A's header comes first
    for cut in (0, 10, 38, 42):
        assert _raw(gpu_engine, zra, (d, cut), A, 2) == ((5, 0), 0, 0, b"\xEE" * 64), cut
        assert _raw(gpu_engine, zra, A, (d, cut), 2) == ((5, 0), 0, 0, b"\xEE" * 64), cut
    junk = bytearray(arc); junk[8] ^= 1                                         # (another magic: HeaderInvalid)
    J = (_dev(junk), len(junk))
    assert _raw(gpu_engine, zra, J, A, 2) == ((3, 0), 0, 0, b"\xEE" * 64) and _raw(gpu_engine, zra, A, J, 2) == ((3, 0), 0, 0, b"\xEE" * 64)
    assert _cmp(gpu_engine, zra, J, (d, 10))[0] == (3, 0) and _cmp(gpu_engine, zra, (d, 10), J)[0] == (5, 0)   # A's problem before B's
    nofs = bytearray(arc); nofs[30:34] = bytes(4)                               # a frame size of 0, on either side
    Z = (_dev(nofs), len(nofs))
    assert _cmp(gpu_engine, zra, Z, A)[0] == (3, 0) and _cmp(gpu_engine, zra, A, Z)[0] == (3, 0) and _cmp(gpu_engine, zra, Z, Z)[0] == (3, 0)
    # frame sizes 1,024 against 2,048, before the range
    data = damaged20["data"][:8192]
    X, _ = _pair(gpu_engine, zra, data, 1024)
    Y, _ = _pair(gpu_engine, zra, data, 2048)
    assert _raw(gpu_engine, zra, X, Y, 2) == ((1, 40), 0, 0, b"\xEE" * 64)
    assert _raw(gpu_engine, zra, X, Y, 2, offset=1 << 40) == ((1, 40), 0, 0, b"\xEE" * 64)
    assert gpu_engine.compare_stats() == ZERO
    assert _raw(gpu_engine, zra, X, X, 2, offset=1 << 40)[0] == (5, 0)


# ---- 10
def test_cli_mode_cmp(zra, gpu_engine, damaged20, tmp_path):
    fs = 1024
    a = _data(np.random.RandomState(10), 40 * fs + 5)
    b = bytearray(a)
    runs = [(3, 2), (7 * fs - 4, 9), (40 * fs + 4, 1)]
    for p, n in runs:
        for q in range(p, p + n):
            b[q] = a[q] ^ 0x80
    b = bytes(b)
    files = dict(a=_compress(gpu_engine, zra, a, 3, fs, True), a9=_compress(gpu_engine, zra, a, 9, fs, True), b=_compress(gpu_engine, zra, b, 3, fs, True),
                 longer=_compress(gpu_engine, zra, a + b"xyz", 3, fs, True), other=_compress(gpu_engine, zra, a, 3, 2 * fs, True),
                 bad=_flip_mid(_compress(gpu_engine, zra, a, 3, fs, True), [7]), junk=b"\x01" * 100)
    path = {}
    for k, v in files.items():
        path[k] = tmp_path / (k + ".zra")
        path[k].write_bytes(v)

    def run(x, y):
        return subprocess.run([TOOL, "cmp", str(x), str(y)], capture_output=True, text=True, timeout=120)

    for y in ("a", "a9"):
        r = run(path["a"], path[y])
        assert (r.returncode, r.stdout) == (0, "0 ranges, 0 bytes differ\n"), (y, r.stdout, r.stderr)
    r = run(path["a"], path["b"])
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stdout == "".join("%d %d\n" % x for x in runs) + "3 ranges, 12 bytes differ\n", r.stdout
    r = run(path["a"], path["longer"])
    assert (r.returncode, r.stdout) == (1, "0 ranges, 0 bytes differ\nsizes differ: %d %d\n" % (len(a), len(a) + 3)), (r.stdout, r.stderr)
    for x, y in (("junk", "a"), ("a", "junk"), ("bad", "a"), ("a", "bad"), ("a", "other"), ("a", "missing"), ("missing", "a")):
        r = run(path.get(x, tmp_path / "missing.zra"), path.get(y, tmp_path / "missing.zra"))
        assert r.returncode == 2 and r.stdout == "", (x, y, r.stdout, r.stderr)
    r = subprocess.run([TOOL, "cmp", str(path["a"])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == ""
