"""GPU tests of ZraHipDiffArchives (include/zra_hip.h): the writes and the packed bytes that give one device-resident archive the
content of another, in the shape ZraHipUpdateArchive takes. The yardstick everywhere is the pair of plaintexts the test generated
itself, run through tests/diff_model.py (cross-checked in tests/test_diff_abi.py); for a frame that does not decode, the status
ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it (existing code). Archives are written on the
device. The shapes are the smallest at which each seam exists: misaligned slots, short last grains, runs of dirty grains across tiles,
frames and passes and next to frames that are not decoded, a tail that starts inside a frame. Every call's data buffer is followed by
a sentinel that no call may touch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compare_model as CM
import diff_model as M
from test_gpu_update import _compress, _data, _dev, _patched, _update
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
ZERO = dict.fromkeys(("frames", "equal_compressed", "decoded", "tail_decoded", "writes", "dirty_bytes", "passes", "dirty_grains"), 0)
SENT = 0xA5
TOO_SMALL = (6, 0)


def _arc(eng, zra, data, fs, level=3, ck=True):
    arc = _compress(eng, zra, data, level, fs, ck)
    return (_dev(arc), len(arc))


def _raw(eng, zra, A, B, wcap, dcap, grain=1, mode=0, staging=0, d_data=None):
    """One ZraHipDiffArchives with a data buffer of dcap bytes and 64 sentinel bytes behind it, and host arrays two entries longer than
    wcap, 0xEE-filled. dict: st, n, data_size, append_offset, append_size, arrays (the three arrays' bytes), data (the dcap bytes),
    sentinel_ok."""
    import torch
    buf = torch.full((dcap + 64,), SENT, dtype=torch.uint8, device="cuda:0") if d_data is None else None
    torch.cuda.synchronize()
    arrs = [(ctypes.c_uint64 * (wcap + 2))() for _ in range(3)]
    for x in arrs:
        ctypes.memset(x, 0xEE, ctypes.sizeof(x))
    w = [ctypes.c_uint64(0x1234) for _ in range(4)]
    eng._order()
    st = zra.load().ZraHipDiffArchives(eng.h, A[0].data_ptr() if A[0] is not None else None, A[1], B[0].data_ptr() if B[0] is not None else None, B[1],
                                       mode, grain, staging, *(arrs if wcap else (None, None, None)), wcap, ctypes.byref(w[0]),
                                       (buf.data_ptr() if dcap else None) if d_data is None else d_data, dcap, ctypes.byref(w[1]), ctypes.byref(w[2]),
                                       ctypes.byref(w[3])).tup()
    out = buf.cpu().numpy().tobytes() if buf is not None else b""
    return dict(st=st, n=w[0].value, data_size=w[1].value, append_offset=w[2].value, append_size=w[3].value, arrays=[bytes(x) for x in arrs],
                data=out[:dcap], sentinel_ok=out[dcap:] == bytes([SENT]) * 64 if buf is not None else True)


def _untouched(r, wcap):
    return all(x == b"\xEE" * (8 * (wcap + 2)) for x in r["arrays"])


def _diff(eng, zra, A, B, a, b, fs, grain=1, **kw):
    """One diff with capacities that fit, checked against the model of the plaintexts a and b: statuses, writes, data offsets, packed
    data, tail, the untouched rest of the host arrays and the sentinel. Returns the model's (writes, data, append_offset, append_size)."""
    want = M.patch(a, b, fs, grain)
    writes, data, ao, asz = want
    wcap, dcap = len(writes) + 3, len(data) + 5
    r = _raw(eng, zra, A, B, wcap, dcap, grain, **kw)
    assert r["st"] == (0, 0), (grain, kw, r["st"])
    assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (len(writes), len(data), ao, asz), (grain, kw, r["n"], len(writes))
    off, size, doff = (np.frombuffer(x, dtype=np.uint64) for x in r["arrays"])
    k = len(writes)
    assert [(int(o), int(s)) for o, s in zip(off[:k], size[:k])] == writes, (grain, kw)
    assert [int(x) for x in doff[:k]] == [int(x) for x in np.cumsum([0] + [s for _, s in writes])[:k]], (grain, kw)
    assert all(x[8 * k:] == b"\xEE" * (8 * (wcap + 2 - k)) for x in r["arrays"]), (grain, kw)
    assert r["data"][:len(data)] == data, (grain, kw)
    assert r["data"][len(data):] == bytes([SENT]) * 5 and r["sentinel_ok"], (grain, kw)
    return want


def _pair(eng, zra, a, b, fs, level=3, ck=True):
    return _arc(eng, zra, a, fs, level, ck), _arc(eng, zra, b, fs, level, ck)


def _changed(a, b, fs):
    c = min(len(a), len(b))
    return {f for f in range(-(-c // fs)) if a[f * fs:(f + 1) * fs] != b[f * fs:(f + 1) * fs]}


# ---- 1
RUNS4 = [(0, 1), (2, 1), (13, 1), (40, 4), (83, 9), (118, 2), (200, 2), (298, 2), (301, 2), (396, 12), (998, 2)]   # tests/test_gpu_compare.py


@pytest.mark.parametrize("staging,passes", [(0, 1), (1, 250)])
def test_known_answers_at_frame_size_4(zra, gpu_engine, staging, passes):
    """250 frames of 4 bytes, in one pass and in 250, grain 1: the writes are the compare's ranges, the data B's bytes of them."""
    a = b"abcdefghij" * 100
    b = bytearray(a)
    for off, n in RUNS4:
        b[off:off + n] = a[off:off + n].upper()
    b = bytes(b)
    assert CM.ranges(a, b) == RUNS4
    A, B = _pair(gpu_engine, zra, a, b, 4)
    changed = _changed(a, b, 4)
    for decode_all in (False, True):
        writes, data, ao, asz = _diff(gpu_engine, zra, A, B, a, b, 4, 1, staging=staging, mode=1 if decode_all else 0)
        assert writes == RUNS4 and data == b"".join(b[o:o + n] for o, n in RUNS4) and (ao, asz) == (38, 0)
        s = gpu_engine.diff_stats()
        want = M.stats(a, b, 4, 1, decoded=None if decode_all else changed, slots=None if passes == 1 else 1)
        assert s == want and s["passes"] == passes and s["dirty_grains"] == 38, (decode_all, s, want)


# ---- 2
FS2 = 1000


@pytest.fixture(scope="module")
def misaligned(zra, gpu_engine):
    """20 frames of 1,000 bytes (slots that are not 16-byte aligned) and a last one of 700, against a copy that differs at: the first
    and the last byte of frame 3; the last byte of frame 5 (the short last grain); the bytes on both sides of the boundaries 8 (a frame
    boundary inside a pass of 3) and 9 (a pass boundary of passes of 3); the last byte of frame 12, frame 13 equal (an end in front of an
    equal-flagged frame), and of frame 14, frame 15 equal (the same across a pass boundary); the first byte of frame 17 behind the equal
    frame 16; a byte in the middle; the last byte of C."""
    U = 20 * FS2 + 700
    a = _data(np.random.RandomState(21), U)
    b = bytearray(a)
    at = [3000, 3999, 5999, 7999, 8000, 8999, 9000, 12999, 14999, 17000, 18500, U - 1]
    for p in at:
        b[p] = a[p] ^ 0x80
    b = bytes(b)
    A, B = _pair(gpu_engine, zra, a, b, FS2)
    return dict(a=a, b=b, A=A, B=B, at=at)


@pytest.mark.parametrize("grain", [1, 2, 4, 16, 64, 1024, 8192])
def test_grain_sweep_at_frame_size_1000(zra, gpu_engine, misaligned, grain):
    a, b, A, B = (misaligned[k] for k in ("a", "b", "A", "B"))
    changed = _changed(a, b, FS2)
    assert changed == {3, 5, 7, 8, 9, 12, 14, 17, 18, 20}
    for staging, slots in ((1, 1), (2 * 3 * FS2, 3), (0, None)):
        writes, data, ao, asz = _diff(gpu_engine, zra, A, B, a, b, FS2, grain, staging=staging)
        s = gpu_engine.diff_stats()
        assert s == M.stats(a, b, FS2, grain, decoded=changed, slots=slots), (staging, s)
        if grain == 1:
            assert writes == [(3000, 1), (3999, 1), (5999, 1), (7999, 2), (8999, 2), (12999, 1), (14999, 1), (17000, 1), (18500, 1), (20699, 1)]
        if grain == 64:
            assert (5960, 40) in writes and (7960, 104) in writes and (12960, 40) in writes and (17000, 64) in writes and (20640, 60) in writes, writes
        if grain == 8192:                                                      # one grain per frame: whole frames, neighbours merged
            assert writes == [(3000, 1000), (5000, 1000), (7000, 3000), (12000, 1000), (14000, 1000), (17000, 2000), (20000, 700)]
    _diff(gpu_engine, zra, A, B, a, b, FS2, grain, staging=2 * 3 * FS2, mode=1)     # every frame decoded: the same patch
    assert gpu_engine.diff_stats()["decoded"] == 21


# ---- 3
@pytest.mark.parametrize("grain", [1, 64])
def test_three_tiles_per_frame(zra, gpu_engine, grain):
    """4 frames of 20,000 bytes: runs of dirty grains across positions 8,192 and 16,384 of a frame, and single bytes on either side."""
    fs = 20000
    a = _data(np.random.RandomState(31), 4 * fs)
    b = bytearray(a)
    at = [8191, fs + 8192, fs + 16383] + list(range(2 * fs + 8188, 2 * fs + 8197)) + list(range(2 * fs + 16380, 2 * fs + 16390)) + \
        list(range(3 * fs + 8100, 3 * fs + 8300)) + [3 * fs + 16384, 4 * fs - 1]
    for p in at:
        b[p] = a[p] ^ 0x80
    b = bytes(b)
    A, B = _pair(gpu_engine, zra, a, b, fs)
    for staging in (0, 2 * fs):
        writes, _, _, _ = _diff(gpu_engine, zra, A, B, a, b, fs, grain, staging=staging)
        s = gpu_engine.diff_stats()
        assert s == M.stats(a, b, fs, grain, slots=None if staging == 0 else 1), s
    if grain == 64:
        assert (2 * fs + 8128, 128) in writes and (2 * fs + 16320, 128) in writes and (3 * fs + 8064, 256) in writes, writes
        assert (8128, 64) in writes and (fs + 8192, 64) in writes and (fs + 16320, 64) in writes and writes[-1] == (4 * fs - 32, 32), writes


# ---- 4
FS4 = 1024


@pytest.mark.parametrize("ua,ub", [(6 * FS4 + 100, 6 * FS4 + 100), (4 * FS4, 6 * FS4 + 10), (3 * FS4 + 300, 5 * FS4 + 20), (FS4, 5 * FS4)])
def test_round_trip_through_the_update(zra, gpu_engine, ua, ub):
    """update(A, diff(A, B)) is byte for byte the archive ZraHipCompressBuffer writes from B's plaintext, at the level and checksum flag
    B was written with: equal sizes; a tail behind a whole number of frames; a tail that starts inside a frame and reaches into two new
    ones; one frame grown to five."""
    import torch
    rng = np.random.RandomState(ua + ub)
    b = _data(rng, ub)
    a = bytearray(b[:ua])
    for p, n in ((5, 3), (FS4 - 2, 4), (ua - 1, 1), (ua // 2, 70)):
        for q in range(p, min(ua, p + n)):
            a[q] = b[q] ^ 0x80
    a = bytes(a)
    for level, ck in ((3, True), (1, False)):
        A, B = _pair(gpu_engine, zra, a, b, FS4, level, ck)
        arc_b = _compress(gpu_engine, zra, b, level, FS4, ck)
        for grain in (1, 64):
            writes, data, ao, asz = M.patch(a, b, FS4, grain)
            d_data = torch.full((len(data) + 64,), SENT, dtype=torch.uint8, device="cuda:0")
            w, got_ao, got_asz, got_size = gpu_engine.diff(A[0].data_ptr(), A[1], B[0].data_ptr(), B[1], d_data.data_ptr(), len(data), grain=grain,
                                                           staging_bytes=2 * 2 * FS4)
            assert (got_ao, got_asz, got_size) == (ao, asz, len(data)) and [(int(o), int(n)) for o, n in zip(w[0], w[1])] == writes
            assert all(x.dtype == np.uint64 for x in w)
            s = gpu_engine.diff_stats()
            assert s == M.stats(a, b, FS4, grain, decoded=_changed(a, b, FS4), slots=2, tail_slots=4), (grain, s)
            cap = len(arc_b) + 4096
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            size = gpu_engine.update(A[0].data_ptr(), A[1], d_out.data_ptr(), cap, writes=w, d_data=d_data.data_ptr(),
                                     d_append=d_data.data_ptr() + got_ao if got_asz else 0, append_size=got_asz, level=level, checksum=ck)
            assert d_out[:size].cpu().numpy().tobytes() == arc_b, (ua, ub, level, grain)
            assert d_data[len(data):].cpu().numpy().tobytes() == bytes([SENT]) * 64


# ---- 5
def test_update_is_the_producer(zra, gpu_engine):
    """A -> update -> B as tests/test_gpu_compare.py builds it: at grain 1 the writes are exactly the changed bytes and the tail is the
    append; the pairs decoded are the ones the compare decodes for the same pair."""
    fs = 1024
    rng = np.random.RandomState(2)
    old = _data(rng, 64 * fs + 700)
    writes = [(5 * fs + 100, rng.randint(128, 256, size=50).astype(np.uint8).tobytes()),
              (16 * fs - 20, rng.randint(128, 256, size=40).astype(np.uint8).tobytes())]
    app = rng.randint(128, 256, size=300).astype(np.uint8).tobytes()
    arc = _compress(gpu_engine, zra, old, 3, fs, True)
    st, out, size = _update(gpu_engine, zra, arc, writes, app)
    assert st == (0, 0)
    new = _patched(old, writes, app)
    A, B = (_dev(arc), len(arc)), (_dev(out[:size]), size)
    for staging, slots, tslots in ((0, None, None), (2 * 16 * fs, 16, 32), (1, 1, 1)):
        w, data, ao, asz = _diff(gpu_engine, zra, A, B, old, new, fs, 1, staging=staging)
        assert w == [(o, len(x)) for o, x in writes] and data == writes[0][1] + writes[1][1] + app and (ao, asz) == (90, 300)
        s = gpu_engine.diff_stats()
        assert s == M.stats(old, new, fs, 1, decoded={5, 15, 16, 64}, slots=slots, tail_slots=tslots), (staging, s)
        n, nb, _ = gpu_engine.compare(A[0].data_ptr(), A[1], B[0].data_ptr(), B[1], staging_bytes=staging)
        assert (n, nb) == (2, 90) and gpu_engine.compare_stats()["decoded"] == s["decoded"] == 4
        assert gpu_engine.diff_stats() == s                                    # a compare does not touch the diff stats


# ---- 6
def test_capacities(zra, gpu_engine):
    fs = 1024
    ua, ub = 3 * fs + 5, 4 * fs + 9
    a = bytes(ua)
    b = bytes(1 if p % 4 == 0 else 0 for p in range(ub))
    A, B = _pair(gpu_engine, zra, a, b, fs)
    writes, data, ao, asz = M.patch(a, b, fs, 2)
    n, need = len(writes), len(data)
    assert n == (ua + 3) // 4 and ao == 2 * n - 1 and asz == ub - ua           # (the last grain is clipped to C: one byte)
    for staging in (0, 1):
        for wcap, dcap in ((n - 1, need), (n, need - 1), (0, 0), (n + 2, ao), (1, 1)):
            r = _raw(gpu_engine, zra, A, B, wcap, dcap, 2, staging=staging)
            assert r["st"] == TOO_SMALL, (wcap, dcap, r["st"])
            assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (n, need, ao, asz), (wcap, dcap)
            assert _untouched(r, wcap) and r["sentinel_ok"], (wcap, dcap)
            assert gpu_engine.diff_stats() == ZERO
        r = _raw(gpu_engine, zra, A, B, n, need, 2, staging=staging)           # the sizing call's numbers fit exactly
        assert r["st"] == (0, 0) and r["data"] == data and r["sentinel_ok"] and (r["n"], r["data_size"]) == (n, need)
        assert all(x[8 * n:] == b"\xEE" * 16 for x in r["arrays"])
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.diff(A[0].data_ptr(), A[1], B[0].data_ptr(), B[1], 0, 0, grain=2, max_writes=0)
    assert (e.value.zra, e.value.needed_writes, e.value.needed_data) == (6, n, need)


# ---- 7
def test_refusals_in_order(zra, gpu_engine):
    import torch
    fs = 1024
    data = _data(np.random.RandomState(7), 8 * fs)
    A, B = _pair(gpu_engine, zra, data, data + b"more", fs)
    buf = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda:0")

    def st(X, Y, grain=1, mode=0, wcap=2, dcap=64, d_data=None):
        r = _raw(gpu_engine, zra, X, Y, wcap, dcap, grain, mode=mode, d_data=d_data)
        assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0) and _untouched(r, wcap) and r["sentinel_ok"]
        assert gpu_engine.diff_stats() == ZERO
        return r["st"]

    junk = bytearray(_compress(gpu_engine, zra, data, 3, fs, True)); junk[8] ^= 1   # (another magic: HeaderInvalid)
    J = (_dev(junk), len(junk))
    cut = (A[0], 10)
    other = _arc(gpu_engine, zra, data, 2 * fs)
    # rule 1, in front of the headers
    for grain in (0, 3, 16384, 8193, 1 << 31):
        assert st(A, B, grain=grain) == (1, 42) and st(cut, J, grain=grain) == (1, 42), grain
    for mode in (2, 3, 0x80000000):
        assert st(A, B, mode=mode) == (1, 42) and st(cut, J, mode=mode) == (1, 42), mode
    assert st((None, A[1]), B) == (1, 42) and st(A, (None, B[1])) == (1, 42)
    assert st(A, B, dcap=64, d_data=0) == (1, 42)                              # dData NULL with a capacity
    # rule 2, in front of the headers: the data buffer inside A, inside B
    assert st(J, B, d_data=J[0].data_ptr() + 8, dcap=16) == (1, 42) and st(A, J, d_data=J[0].data_ptr() + J[1] - 1, dcap=16) == (1, 42)
    assert st(A, B, d_data=A[0].data_ptr() - 0 + A[1] - 1, dcap=1) == (1, 42)
    # rule 3: A's header before B's, and before the frame sizes
    assert st(cut, J) == (5, 0) and st(J, cut) == (3, 0) and st(J, other) == (3, 0) and st(other, J) == (3, 0)
    # rules 4 and 5
    assert st(A, other) == (1, 40) and st(other, A) == (1, 40)
    assert st(B, A) == (1, 40)                                                 # UB < UA: no patch
    assert _raw(gpu_engine, zra, A, B, 2, 64, d_data=buf.data_ptr())["st"] == (0, 0)   # and the pair itself is fine
    assert gpu_engine.diff_stats() == dict(ZERO, frames=8, equal_compressed=8, tail_decoded=1, passes=2)
    assert buf[:4].cpu().numpy().tobytes() == b"more" and buf[4:].cpu().numpy().tobytes() == bytes([SENT]) * 4092


# ---- 8
def test_damaged_frames(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(8), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    G, D, Dc = (_dev(arc), len(arc)), (_dev(bad), len(bad)), (_dev(bad), len(bad))
    want = _frame_status(gpu_engine, zra, bad, d_arc=D[0])
    assert set(want) == {7} and want[7] != 0, want

    def failed(r, code):
        return r["st"] == (1, code) and (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0) and _untouched(r, 6) and \
            r["sentinel_ok"] and gpu_engine.diff_stats() == ZERO and gpu_engine.diff_ms() == 0

    for staging in (0, 2 * 4 * fs, 1):                                         # frame 7 flipped in B only: its spans differ, it is decoded
        assert failed(_raw(gpu_engine, zra, G, D, 6, 4096, staging=staging), want[7]), staging
    assert failed(_raw(gpu_engine, zra, D, G, 6, 4096), want[7])               # in A only
    # the same flip on both sides: clean without being decoded (the documented limit), frame 7's status when everything is decoded
    r = _raw(gpu_engine, zra, D, Dc, 6, 4096)
    assert r["st"] == (0, 0) and (r["n"], r["data_size"]) == (0, 0) and gpu_engine.diff_stats() == dict(ZERO, frames=20, equal_compressed=20, passes=1)
    assert failed(_raw(gpu_engine, zra, D, Dc, 6, 4096, mode=1), want[7])
    # a damaged tail frame of B: A is the first 10 frames and a half
    short = _arc(gpu_engine, zra, data[:10 * fs + 100], fs)
    bad15 = _flip_mid(arc, [15])
    D15 = (_dev(bad15), len(bad15))
    code15 = _frame_status(gpu_engine, zra, bad15, d_arc=D15[0])[15]
    for staging in (0, 2 * fs):
        assert failed(_raw(gpu_engine, zra, short, D15, 6, 10 * fs, staging=staging), code15), staging
    r = _raw(gpu_engine, zra, short, G, 6, 10 * fs)                            # and the sound pair answers
    assert r["st"] == (0, 0) and (r["n"], r["append_offset"], r["append_size"]) == (0, 0, 10 * fs - 100) and r["data"][:10 * fs - 100] == data[10 * fs + 100:]


# ---- 9
def test_identical_archives(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(9), 20 * fs)
    A = _arc(gpu_engine, zra, data, fs)
    A2 = (A[0].clone(), A[1])
    for grain in (1, 8192):
        r = _raw(gpu_engine, zra, A, A2, 4, 64, grain)
        assert r["st"] == (0, 0) and (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0)
        assert _untouched(r, 4) and r["data"] == bytes([SENT]) * 64 and r["sentinel_ok"]
        assert gpu_engine.diff_stats() == dict(ZERO, frames=20, equal_compressed=20, passes=1)
        assert gpu_engine.kernel_stats()["dec_launches"] == 0
    r = _raw(gpu_engine, zra, A, A2, 0, 0, 1, mode=1)                          # decoded everywhere: still nothing to write
    assert r["st"] == (0, 0) and gpu_engine.diff_stats() == dict(ZERO, frames=20, decoded=20, passes=1) and gpu_engine.kernel_stats()["dec_launches"] >= 1


# ---- 10
def test_interleaved_with_the_other_archive_calls(zra, gpu_engine):
    """One engine, one staging window: a diff between a search, a verify and a compare, on archives of two frame sizes, forwards and,
    after the scratch was handed back, in reverse."""
    pairs = []
    for fs, seed in ((1000, 41), (4096, 42)):
        ua = 9 * fs + fs // 3
        a = bytearray(_data(np.random.RandomState(seed), ua))
        a[2 * fs + 7:2 * fs + 15] = b"NEEDLE!!"
        a = bytes(a)
        b = bytearray(a + _data(np.random.RandomState(seed + 10), fs + 50))
        for p in (0, 3 * fs - 1, 3 * fs, 7 * fs + 100, ua - 1):
            b[p] ^= 0x80
        b = bytes(b)
        A, B = _pair(gpu_engine, zra, a, b, fs)
        pairs.append((a, b, A, B, fs))

    def search(a, b, A, B, fs):
        assert gpu_engine.search(A[0].data_ptr(), A[1], b"NEEDLE!!", staging_bytes=3 * fs) == (1, [2 * fs + 7])

    def verify(a, b, A, B, fs):
        assert gpu_engine.verify(B[0].data_ptr(), B[1], staging_bytes=2 * fs)[0] == 0

    def compare(a, b, A, B, fs):
        r = CM.ranges(a, b)
        assert gpu_engine.compare(A[0].data_ptr(), A[1], B[0].data_ptr(), B[1], staging_bytes=2 * 2 * fs) == (len(r), sum(n for _, n in r), r)

    def diff(a, b, A, B, fs):
        for grain, staging in ((1, 2 * 2 * fs), (64, 0)):
            _diff(gpu_engine, zra, A, B, a, b, fs, grain, staging=staging)

    steps = [(f, p) for p in pairs for f in (search, diff, verify, diff, compare, diff)]
    for f, p in steps:
        f(*p)
    gpu_engine.release_scratch()
    for f, p in reversed(steps):
        f(*p)


# ---- 10b
def test_a_refused_sign_call_leaves_the_diff_counters_alone(zra, gpu_engine):
    """Every call's counters and milliseconds are a row of one table: a row belongs to one call. After a sign call that succeeded and a
    diff that succeeded, a sign call refused for its grain (3: not a power of two) zeroes the sign's row and leaves the diff's row,
    counters and milliseconds, as it was."""
    from test_gpu_sign import SIGN_ZERO, _sign_raw
    fs = 1000
    a = _data(np.random.RandomState(5), 5 * fs + 17)
    b = bytearray(a + _data(np.random.RandomState(6), fs))
    b[fs + 3] ^= 1
    b[4 * fs] ^= 1
    b = bytes(b)
    A, B = _pair(gpu_engine, zra, a, b, fs)
    assert _sign_raw(gpu_engine, zra, A, 64)["st"] == (0, 0) and gpu_engine.sign_stats()["signed"] == 6
    _diff(gpu_engine, zra, A, B, a, b, fs, 64, staging=2 * 2 * fs)
    stats, ms = gpu_engine.diff_stats(), zra.load().ZraHipDebugDiffMs(gpu_engine.h)
    assert stats == M.stats(a, b, fs, 64, decoded=_changed(a, b, fs), slots=2, tail_slots=4) and ms > 0, (stats, ms)
    r = _sign_raw(gpu_engine, zra, A, 3, cap=64)
    assert r["st"] == (1, 42) and r["info"] == (0,) * 6, r["st"]
    assert gpu_engine.sign_stats() == SIGN_ZERO and gpu_engine.sign_ms() == 0
    assert gpu_engine.diff_stats() == stats and zra.load().ZraHipDebugDiffMs(gpu_engine.h) == ms


# ---- 11
def test_cli_mode_diff(zra, gpu_engine, tmp_path):
    fs = 1024
    a = _data(np.random.RandomState(11), 10 * fs + 5)
    b = bytearray(a)
    for p, n in ((3, 2), (7 * fs - 4, 9), (10 * fs + 4, 1)):
        for q in range(p, p + n):
            b[q] = a[q] ^ 0x80
    b = bytes(b) + b"tail bytes"
    files = dict(a=_compress(gpu_engine, zra, a, 3, fs, True), a9=_compress(gpu_engine, zra, a, 9, fs, True), b=_compress(gpu_engine, zra, b, 3, fs, True),
                 other=_compress(gpu_engine, zra, a, 3, 2 * fs, True), junk=b"\x01" * 100)
    path = {}
    for k, v in files.items():
        path[k] = tmp_path / (k + ".zra")
        path[k].write_bytes(v)

    def run(*args):
        return subprocess.run([TOOL, "diff"] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    for y in ("a", "a9"):
        r = run(path["a"], path[y])
        assert (r.returncode, r.stdout) == (0, "append 0\n0 writes, 0 bytes written, 0 bytes of patch data\n"), (y, r.stdout, r.stderr)
    for grain in (1, 64):
        w, data, ao, asz = M.patch(a, b, fs, grain)
        r = run(path["a"], path["b"], "-g", grain) if grain != 1 else run(path["a"], path["b"])
        assert r.returncode == 1, (r.stdout, r.stderr)
        assert r.stdout == "".join("%d %d\n" % x for x in w) + "append %d\n%d writes, %d bytes written, %d bytes of patch data\n" % (asz, len(w), ao, len(data)), r.stdout
    for args in ((path["junk"], path["a"]), (path["a"], path["junk"]), (path["a"], path["other"]), (path["b"], path["a"]), (path["a"], tmp_path / "missing.zra"),
                 (path["a"], path["b"], "-g", 3), (path["a"], path["b"], "-g"), (path["a"],)):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
