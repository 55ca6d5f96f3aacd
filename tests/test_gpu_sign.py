"""GPU tests of ZraHipSignArchive and ZraHipDiffSignature (include/zra_hip.h): the content signature of a device-resident archive,
and the diff of an archive against the signature of a replica. The yardsticks are the plaintexts the test generated itself, run through
tests/sign_model.py (cross-checked in tests/test_sign_abi.py) and tests/diff_model.py, with `slots` and `tail_slots` both
stagingBytes / frameSize; for a frame that does not decode, the status ZraHipDecompressRABatch gives under
ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it. The shapes are the smallest at which each seam exists. Every device buffer is
followed by a sentinel that no call may touch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compare_model as CM
import diff_model as M
import sign_model as SM
from test_gpu_diff import RUNS4, _changed, _pair, _raw, _untouched
from test_gpu_update import _compress, _data, _dev, _patched, _update
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
ZERO = dict.fromkeys(("frames", "equal_compressed", "decoded", "tail_decoded", "writes", "dirty_bytes", "passes", "dirty_grains"), 0)
SIGN_ZERO = dict.fromkeys(("frames", "signed", "grain_words", "content_bytes", "compressed_bytes", "passes"), 0)
SENT = 0xA5
SENTW = int.from_bytes(bytes([SENT]) * 8, "little")
TOO_SMALL = (6, 0)
ALL = 0xFFFFFFFFFFFFFFFF
SEED2 = 0x9E3779B97F4A7C15
EXTRA = 4                                                                      # sentinel words behind a signature buffer


def _sigbuf(words):
    import torch
    return torch.full((8 * (words + EXTRA),), SENT, dtype=torch.uint8, device="cuda:0")


def _words(buf):
    return [int(x) for x in np.frombuffer(buf.cpu().numpy().tobytes(), dtype="<u8")]


def _sign_raw(eng, zra, A, grain, seed=0, first=0, count=ALL, staging=0, cap=None, buf=None, d_sig=None):
    """One ZraHipSignArchive into a buffer of `cap` words (None: what the archive needs, from its header) with EXTRA sentinel words
    behind it. dict: st, info (the six fields), words (all cap + EXTRA words afterwards), buf."""
    import torch
    if cap is None:
        raw = A[0][:38].cpu().numpy().tobytes()
        cap = SM.words(int.from_bytes(raw[18:26], "little"), int.from_bytes(raw[30:34], "little"), grain)
    if buf is None:
        buf = _sigbuf(cap)
    torch.cuda.synchronize()
    info = zra.ZraHipSignature(1, 2, 3, 4, 5, 6)
    eng._order()
    st = zra.load().ZraHipSignArchive(eng.h, A[0].data_ptr() if A[0] is not None else None, A[1], grain, seed, first, count, staging,
                                      (buf.data_ptr() if cap else None) if d_sig is None else d_sig, cap, ctypes.byref(info)).tup()
    return dict(st=st, info=(info.contentSize, info.frameSize, info.grain, info.seed, info.frames, info.words), words=_words(buf), buf=buf, cap=cap)


def _signed(eng, zra, A, arc, plain, fs, grain, seed=0, staging=0):
    """sign() of the whole archive, checked word for word against the model; returns (Signature, buffer, words)."""
    want = SM.signature(arc, plain, fs, grain, seed)
    r = _sign_raw(eng, zra, A, grain, seed, staging=staging)
    assert r["st"] == (0, 0), (grain, staging, r["st"])
    assert r["info"] == (len(plain), fs, grain, seed, -(-len(plain) // fs), len(want)), r["info"]
    bad = [i for i, (x, y) in enumerate(zip(r["words"], want)) if x != y]
    assert not bad, (grain, staging, seed, bad[:8], len(bad))
    assert r["words"][len(want):] == [SENTW] * EXTRA
    return zra.Signature(*r["info"]), r["buf"], want


def _sd_raw(eng, zra, sig, buf, B, wcap, dcap, mode=0, staging=0, d_data=None, sig_words=None, d_sig=None):
    """One ZraHipDiffSignature, shaped as test_gpu_diff._raw."""
    import torch
    dbuf = torch.full((dcap + 64,), SENT, dtype=torch.uint8, device="cuda:0") if d_data is None else None
    torch.cuda.synchronize()
    arrs = [(ctypes.c_uint64 * (wcap + 2))() for _ in range(3)]
    for x in arrs:
        ctypes.memset(x, 0xEE, ctypes.sizeof(x))
    w = [ctypes.c_uint64(0x1234) for _ in range(4)]
    info = zra.ZraHipSignature(*sig) if sig is not None else None
    eng._order()
    st = zra.load().ZraHipDiffSignature(eng.h, ctypes.byref(info) if info is not None else None,
                                        (buf.data_ptr() if buf is not None else None) if d_sig is None else d_sig,
                                        (sig[5] if sig is not None else 0) if sig_words is None else sig_words,
                                        B[0].data_ptr() if B[0] is not None else None, B[1], mode, staging, *(arrs if wcap else (None, None, None)), wcap,
                                        ctypes.byref(w[0]), (dbuf.data_ptr() if dcap else None) if d_data is None else d_data, dcap, ctypes.byref(w[1]),
                                        ctypes.byref(w[2]), ctypes.byref(w[3])).tup()
    out = dbuf.cpu().numpy().tobytes() if dbuf is not None else b""
    return dict(st=st, n=w[0].value, data_size=w[1].value, append_offset=w[2].value, append_size=w[3].value, arrays=[bytes(x) for x in arrs],
                data=out[:dcap], sentinel_ok=out[dcap:] == bytes([SENT]) * 64 if dbuf is not None else True)


def _sigdiff(eng, zra, sig, buf, B, a, b, fs, **kw):
    """One signature diff with capacities that fit, checked against diff_model.patch of the plaintexts at the signature's grain."""
    grain = sig.grain
    want = M.patch(a, b, fs, grain)
    writes, data, ao, asz = want
    wcap, dcap = len(writes) + 3, len(data) + 5
    r = _sd_raw(eng, zra, sig, buf, B, wcap, dcap, **kw)
    assert r["st"] == (0, 0), (grain, kw, r["st"])
    assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (len(writes), len(data), ao, asz), (grain, kw, r["n"], len(writes))
    off, size, doff = (np.frombuffer(x, dtype=np.uint64) for x in r["arrays"])
    k = len(writes)
    assert [(int(o), int(s)) for o, s in zip(off[:k], size[:k])] == writes, (grain, kw)
    assert [int(x) for x in doff[:k]] == [int(x) for x in np.cumsum([0] + [s for _, s in writes])[:k]], (grain, kw)
    assert all(x[8 * k:] == b"\xEE" * (8 * (wcap + 2 - k)) for x in r["arrays"]), (grain, kw)
    assert r["data"][:len(data)] == data, (grain, kw)
    assert r["data"][len(data):] == bytes([SENT]) * 5 and r["sentinel_ok"], (grain, kw)
    assert _words(buf)[sig.words:] == [SENTW] * EXTRA
    return want, r


def _arcs(eng, zra, a, b, fs, level=3, ck=True):
    """(archive bytes of a, (device, size) of it, the same of b)"""
    xa, xb = _compress(eng, zra, a, level, fs, ck), _compress(eng, zra, b, level, fs, ck)
    return xa, (_dev(xa), len(xa)), xb, (_dev(xb), len(xb))


# ---- 1
@pytest.mark.parametrize("staging,passes", [(0, 1), (1, 250)])
def test_frame_size_4(zra, gpu_engine, staging, passes):
    """250 frames of 4 bytes at grain 64: one grain per frame, every grain clipped to its frame; in one pass and in 250."""
    a = b"abcdefghij" * 100
    b = bytearray(a)
    for off, n in RUNS4:
        b[off:off + n] = a[off:off + n].upper()
    b = bytes(b)
    xa, A, xb, B = _arcs(gpu_engine, zra, a, b, 4)
    sig, buf, want = _signed(gpu_engine, zra, A, xa, a, 4, 64, staging=staging)
    assert sig.words == 500 == zra.signature_words(1000, 4, 64)
    s = gpu_engine.sign_stats()
    assert s == dict(frames=250, signed=250, grain_words=250, content_bytes=1000, compressed_bytes=_span_bytes(xa), passes=passes), s
    changed = _changed(a, b, 4)
    assert changed == {f for o, n in RUNS4 for f in range(o // 4, (o + n - 1) // 4 + 1)}
    for decode_all in (False, True):
        (writes, data, ao, asz), _ = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, 4, staging=staging, mode=1 if decode_all else 0)
        assert sorted(f for o, n in writes for f in range(o // 4, (o + n) // 4)) == sorted(changed) and ao == 4 * len(changed)
        s = gpu_engine.diff_signature_stats()
        slots = None if passes == 1 else 1
        assert s == M.stats(a, b, 4, 64, decoded=None if decode_all else changed, slots=slots, tail_slots=slots) and s["passes"] == passes, (decode_all, s)


def _span_bytes(arc):
    """the compressed bytes of all frames: the last seek-table entry"""
    t = 38 + int.from_bytes(arc[34:38], "little")
    F = int.from_bytes(arc[26:30], "little") - 1
    return int.from_bytes(arc[t + 5 * F:t + 5 * F + 5], "little")


# ---- 2
FS2 = 1000


@pytest.fixture(scope="module")
def misaligned(zra, gpu_engine):
    """The pair of tests/test_gpu_diff.py::misaligned: 20 frames of 1,000 bytes (slots that are not 8-byte aligned) and a last one of
    700, against a copy that differs at the first and last byte of frames, on both sides of frame and pass boundaries, next to equal
    frames, in the middle and at the last byte of C."""
    U = 20 * FS2 + 700
    a = _data(np.random.RandomState(21), U)
    b = bytearray(a)
    for p in [3000, 3999, 5999, 7999, 8000, 8999, 9000, 12999, 14999, 17000, 18500, U - 1]:
        b[p] = a[p] ^ 0x80
    b = bytes(b)
    xa, A, xb, B = _arcs(gpu_engine, zra, a, b, FS2)
    return dict(a=a, b=b, A=A, B=B, xa=xa, xb=xb)


@pytest.mark.parametrize("grain", [64, 128, 1024, 8192])
def test_grain_sweep_at_frame_size_1000(zra, gpu_engine, misaligned, grain):
    a, b, A, B, xa = (misaligned[k] for k in ("a", "b", "A", "B", "xa"))
    changed = _changed(a, b, FS2)
    assert changed == {3, 5, 7, 8, 9, 12, 14, 17, 18, 20}
    gpf = -(-FS2 // grain)
    for staging, slots in ((1, 1), (3 * FS2, 3), (0, None)):
        sig, buf, want = _signed(gpu_engine, zra, A, xa, a, FS2, grain, staging=staging)
        assert want[20 * (1 + gpf) + 1 + -(-700 // grain):] == [0] * (gpf - -(-700 // grain))      # no byte behind the short frame's last grain
        s = gpu_engine.sign_stats()
        assert s == dict(frames=21, signed=21, grain_words=20 * gpf + -(-700 // grain), content_bytes=len(a), compressed_bytes=_span_bytes(xa),
                         passes=21 if slots == 1 else 7 if slots == 3 else 1), (staging, s)
        (writes, data, ao, asz), r = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, FS2, staging=staging)
        s = gpu_engine.diff_signature_stats()
        assert s == M.stats(a, b, FS2, grain, decoded=changed, slots=slots, tail_slots=slots), (staging, s)
        if grain == 64:
            assert (5960, 40) in writes and (7960, 104) in writes and (12960, 40) in writes and (17000, 64) in writes and (20640, 60) in writes, writes
        if grain >= 1024:                                                      # one grain per frame: whole frames, neighbours merged
            assert writes == [(3000, 1000), (5000, 1000), (7000, 3000), (12000, 1000), (14000, 1000), (17000, 2000), (20000, 700)]
    _, r_all = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, FS2, staging=3 * FS2, mode=1)   # every frame decoded: the same patch
    assert gpu_engine.diff_signature_stats()["decoded"] == 21
    # word for word and byte for byte what the diff of the two archives gives at this grain
    wcap, dcap = len(writes) + 3, len(data) + 5
    d = _raw(gpu_engine, zra, A, B, wcap, dcap, grain)
    assert d["st"] == (0, 0)
    for k in ("n", "data_size", "append_offset", "append_size", "arrays", "data"):
        assert d[k] == r[k] == r_all[k], k


# ---- 3
@pytest.mark.parametrize("grain", [64, 8192])
def test_three_tiles_per_frame(zra, gpu_engine, grain):
    """4 frames of 20,000 bytes: a 32-byte last grain at grain 64, a 3,616-byte one at 8,192; the dirty positions of the diff's test."""
    fs = 20000
    a = _data(np.random.RandomState(31), 4 * fs)
    b = bytearray(a)
    at = [8191, fs + 8192, fs + 16383] + list(range(2 * fs + 8188, 2 * fs + 8197)) + list(range(2 * fs + 16380, 2 * fs + 16390)) + \
        list(range(3 * fs + 8100, 3 * fs + 8300)) + [3 * fs + 16384, 4 * fs - 1]
    for p in at:
        b[p] = a[p] ^ 0x80
    b = bytes(b)
    xa, A, xb, B = _arcs(gpu_engine, zra, a, b, fs)
    for staging, slots in ((0, None), (fs, 1)):
        sig, buf, _ = _signed(gpu_engine, zra, A, xa, a, fs, grain, staging=staging)
        (writes, _, _, _), _ = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, fs, staging=staging)
        s = gpu_engine.diff_signature_stats()
        assert s == M.stats(a, b, fs, grain, slots=slots, tail_slots=slots), s
    if grain == 64:
        assert (2 * fs + 8128, 128) in writes and (2 * fs + 16320, 128) in writes and (3 * fs + 8064, 256) in writes, writes
        assert (8128, 64) in writes and (fs + 8192, 64) in writes and (fs + 16320, 64) in writes and writes[-1] == (4 * fs - 32, 32), writes
    else:
        assert writes == [(0, 8192), (fs + 8192, 8192), (2 * fs, 2 * fs)], writes   # grains of 8,192, 8,192 and 3,616 bytes per frame


# ---- 4
FS4 = 1024


@pytest.mark.parametrize("ua,ub", [(6 * FS4 + 100, 6 * FS4 + 100), (4 * FS4, 6 * FS4 + 10), (3 * FS4 + 300, 5 * FS4 + 20), (FS4, 5 * FS4)])
def test_round_trip_through_the_update(zra, gpu_engine, ua, ub):
    """update(A, diff_signature(sign(A), B)) is byte for byte the archive ZraHipCompressBuffer writes from B's plaintext."""
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
        for grain in (64, 1024):
            nw = zra.signature_words(ua, FS4, grain)
            d_sig = _sigbuf(nw)
            sig = gpu_engine.sign(A[0].data_ptr(), A[1], d_sig.data_ptr(), nw, grain=grain, staging_bytes=2 * FS4)
            assert sig == (ua, FS4, grain, 0, -(-ua // FS4), nw)
            writes, data, ao, asz = M.patch(a, b, FS4, grain)
            d_data = torch.full((len(data) + 64,), SENT, dtype=torch.uint8, device="cuda:0")
            w, got_ao, got_asz, got_size = gpu_engine.diff_signature(sig, d_sig.data_ptr(), nw, B[0].data_ptr(), B[1], d_data.data_ptr(), len(data),
                                                                     staging_bytes=2 * FS4)
            assert (got_ao, got_asz, got_size) == (ao, asz, len(data)) and [(int(o), int(n)) for o, n in zip(w[0], w[1])] == writes
            assert all(x.dtype == np.uint64 for x in w)
            s = gpu_engine.diff_signature_stats()
            assert s == M.stats(a, b, FS4, grain, decoded=_changed(a, b, FS4), slots=2, tail_slots=2), (grain, s)
            cap = len(arc_b) + 4096
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            size = gpu_engine.update(A[0].data_ptr(), A[1], d_out.data_ptr(), cap, writes=w, d_data=d_data.data_ptr(),
                                     d_append=d_data.data_ptr() + got_ao if got_asz else 0, append_size=got_asz, level=level, checksum=ck)
            assert d_out[:size].cpu().numpy().tobytes() == arc_b, (ua, ub, level, grain)
            assert d_data[len(data):].cpu().numpy().tobytes() == bytes([SENT]) * 64
            assert _words(d_sig)[nw:] == [SENTW] * EXTRA


# ---- 5
def test_incremental_signing(zra, gpu_engine):
    """A -> update -> B: two writes and an append that grows the last frame and adds one. The old signature, copied into a buffer of
    B's size and re-signed in the touched frames only, is B's signature."""
    fs, grain = 1024, 128
    rng = np.random.RandomState(5)
    old = _data(rng, 64 * fs + 700)
    writes = [(5 * fs + 100, rng.randint(128, 256, size=50).astype(np.uint8).tobytes()),
              (16 * fs - 20, rng.randint(128, 256, size=40).astype(np.uint8).tobytes())]
    app = rng.randint(128, 256, size=600).astype(np.uint8).tobytes()
    arc = _compress(gpu_engine, zra, old, 3, fs, True)
    st, out, size = _update(gpu_engine, zra, arc, writes, app)
    assert st == (0, 0)
    new, arc_b = _patched(old, writes, app), out[:size]
    assert -(-len(new) // fs) == 66
    A, B = (_dev(arc), len(arc)), (_dev(arc_b), size)
    sig_a, buf_a, words_a = _signed(gpu_engine, zra, A, arc, old, fs, grain)
    sig_b, buf_b, words_b = _signed(gpu_engine, zra, B, arc_b, new, fs, grain)
    nb = zra.signature_words(len(new), fs, grain)
    assert nb == sig_b.words == 66 * 9 and sig_a.words == 65 * 9
    inc = _sigbuf(nb)
    inc[:8 * sig_a.words] = buf_a[:8 * sig_a.words]
    signed = 0
    for first, count in ((5, 1), (15, 2), (64, None)):
        got = gpu_engine.sign(B[0].data_ptr(), B[1], inc.data_ptr(), nb, grain=grain, first_frame=first, frame_count=count, staging_bytes=fs)
        assert got == sig_b
        s = gpu_engine.sign_stats()
        n = 66 - first if count is None else count
        assert (s["frames"], s["signed"], s["passes"]) == (66, n, n), s
        signed += s["signed"]
    assert signed == 5
    w = _words(inc)
    assert w[:nb] == words_b and w[nb:] == [SENTW] * EXTRA
    stride = 9
    for f in range(64):
        if f not in (5, 15, 16):
            assert w[f * stride:(f + 1) * stride] == words_a[f * stride:(f + 1) * stride], f    # byte for byte the old records
    assert w[64 * stride:65 * stride] != words_a[64 * stride:65 * stride]
    # and the incremental signature is good for the next diff: B against itself
    r = _sd_raw(gpu_engine, zra, sig_b, inc, B, 2, 64)
    assert r["st"] == (0, 0) and r["n"] == 0 and gpu_engine.diff_signature_stats() == dict(ZERO, frames=66, equal_compressed=66, passes=1)


# ---- 6
def test_seeds(zra, gpu_engine, misaligned):
    a, b, A, B, xa = (misaligned[k] for k in ("a", "b", "A", "B", "xa"))
    sig0, buf0, w0 = _signed(gpu_engine, zra, A, xa, a, FS2, 64, seed=0)
    sig1, buf1, w1 = _signed(gpu_engine, zra, A, xa, a, FS2, 64, seed=SEED2)
    assert all(x != y for x, y in zip(w0, w1) if (x, y) != (0, 0)) and sig1.seed == SEED2
    (p0, r0), (p1, r1) = _sigdiff(gpu_engine, zra, sig0, buf0, B, a, b, FS2), _sigdiff(gpu_engine, zra, sig1, buf1, B, a, b, FS2)
    assert p0 == p1 and r0["arrays"] == r1["arrays"] and r0["data"] == r1["data"]
    # the words of one seed under the other's description: every frame word and every grain word differs
    _, r = (None, _sd_raw(gpu_engine, zra, sig1, buf0, B, 4, len(a) + 8))
    assert r["st"] == (0, 0) and r["n"] == 1 and r["data_size"] == len(a) and r["data"][:len(a)] == b


# ---- 7
def test_capacities(zra, gpu_engine):
    import torch
    fs, grain = 1024, 64
    ua, ub = 3 * fs + 5, 4 * fs + 9
    a = bytes(ua)
    b = bytes(1 if (p % fs // grain) % 2 == 0 and p % grain == 0 else 0 for p in range(ub))
    xa, A, xb, B = _arcs(gpu_engine, zra, a, b, fs)
    words = zra.signature_words(ua, fs, grain)
    assert words == 4 * 17
    # the sign sizing call: header arithmetic, no decode, nothing written
    for cap in (0, 1, words - 1):
        assert gpu_engine.verify(A[0].data_ptr(), A[1])[0] == 0 and gpu_engine.kernel_stats()["dec_launches"] >= 1   # (a decode in between)
        r = _sign_raw(gpu_engine, zra, A, grain, 3, cap=cap)
        assert r["st"] == TOO_SMALL and r["info"] == (ua, fs, grain, 3, 4, words), (cap, r["st"], r["info"])
        assert r["words"] == [SENTW] * (cap + EXTRA) and gpu_engine.kernel_stats()["dec_launches"] == 0
        assert gpu_engine.sign_stats() == SIGN_ZERO and gpu_engine.sign_ms() == 0
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.sign(A[0].data_ptr(), A[1], 0, 0, grain=grain)
    assert (e.value.zra, e.value.needed_words) == (6, words)
    sig, buf, _ = _signed(gpu_engine, zra, A, xa, a, fs, grain)                # `words` words fit exactly
    assert gpu_engine.kernel_stats()["dec_launches"] >= 1
    # the diff's capacity matrix
    writes, data, ao, asz = M.patch(a, b, fs, grain)
    n, need = len(writes), len(data)
    assert n == 3 * 8 + 1 and ao == 24 * grain + 5 and asz == ub - ua          # (the last grain is clipped to C: five bytes)
    for staging in (0, 1):
        for wcap, dcap in ((n - 1, need), (n, need - 1), (0, 0), (n + 2, ao), (1, 1)):
            r = _sd_raw(gpu_engine, zra, sig, buf, B, wcap, dcap, staging=staging)
            assert r["st"] == TOO_SMALL, (wcap, dcap, r["st"])
            assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (n, need, ao, asz), (wcap, dcap)
            assert _untouched(r, wcap) and r["sentinel_ok"], (wcap, dcap)
            assert gpu_engine.diff_signature_stats() == ZERO
        r = _sd_raw(gpu_engine, zra, sig, buf, B, n, need, staging=staging)    # the sizing call's numbers fit exactly
        assert r["st"] == (0, 0) and r["data"] == data and r["sentinel_ok"] and (r["n"], r["data_size"]) == (n, need)
        assert all(x[8 * n:] == b"\xEE" * 16 for x in r["arrays"])
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.diff_signature(sig, buf.data_ptr(), sig.words, B[0].data_ptr(), B[1], 0, 0, max_writes=0)
    assert (e.value.zra, e.value.needed_writes, e.value.needed_data) == (6, n, need)


# ---- 8
def test_refusals_in_order(zra, gpu_engine):
    import torch
    fs, grain = 1024, 64
    data = _data(np.random.RandomState(7), 8 * fs)
    xa, A, xb, B = _arcs(gpu_engine, zra, data, data + b"more", fs)
    junk = bytearray(xa); junk[8] ^= 1                                         # (another magic: HeaderInvalid)
    J = (_dev(junk), len(junk))
    cut = (A[0], 10)
    nofs = bytearray(xa); nofs[30:34] = bytes(4)                               # a frame size of 0
    Z = (_dev(nofs), len(nofs))
    bad = _flip_mid(xa, [2])
    D = (_dev(bad), len(bad))
    words = zra.signature_words(len(data), fs, grain)

    # ---- sign
    def sg(X, cap=words, decodes=False, **kw):
        r = _sign_raw(gpu_engine, zra, X, kw.pop("grain", grain), cap=cap, **kw)
        if r["st"] not in ((0, 0), TOO_SMALL):                                 # (a failing frame leaves the words of the range undefined)
            assert r["info"] == (0,) * 6 and (decodes or r["words"] == [SENTW] * (cap + EXTRA)), r
        if r["st"] != (0, 0):
            assert gpu_engine.sign_stats() == SIGN_ZERO and gpu_engine.sign_ms() == 0
        return r["st"]

    # rule 1, in front of the header and of the range
    for g in (0, 1, 32, 63, 96, 16384, 1 << 31):
        assert sg(J, grain=g, first=100) == (1, 42), g
    assert sg((None, J[1])) == (1, 42) and sg(J, d_sig=0) == (1, 42)           # dSig NULL with a capacity
    # rule 2, in front of the header: the signature inside the archive, and reaching into its first byte
    assert sg(J, d_sig=J[0].data_ptr() + 8, cap=2) == (1, 42) and sg(J, d_sig=J[0].data_ptr() - 8 * words + 1) == (1, 42)
    # rule 3, in front of the range
    assert sg(J, first=100) == (3, 0) and sg(cut, first=100) == (5, 0) and sg(Z, first=100) == (3, 0)
    # rule 4, in front of the capacity; the empty range is Success whatever the capacity
    assert sg(A, first=9, cap=0) == (5, 0) and sg(A, first=3, count=6, cap=0) == (5, 0) and sg(A, first=0, count=ALL - 1, cap=0) == (5, 0)
    for first, count in ((8, ALL), (8, 0), (3, 0)):
        r = _sign_raw(gpu_engine, zra, A, grain, first=first, count=count, cap=0)
        assert r["st"] == (0, 0) and r["info"] == (len(data), fs, grain, 0, 8, words) and r["words"] == [SENTW] * EXTRA
        assert gpu_engine.sign_stats() == dict(SIGN_ZERO, frames=8)
    # rule 5, in front of a failing frame
    assert sg(D, cap=words - 1) == TOO_SMALL
    assert sg(D, decodes=True)[0] == 1 and sg(A) == (0, 0)

    # ---- signature diff
    sig, buf, _ = _signed(gpu_engine, zra, A, xa, data, fs, grain)
    xo = _compress(gpu_engine, zra, data + b"more and more", 3, 2 * fs, True)
    O = (_dev(xo), len(xo))
    sig_o, buf_o, _ = _signed(gpu_engine, zra, O, xo, data + b"more and more", 2 * fs, grain)
    sig_b, buf_b, _ = _signed(gpu_engine, zra, B, xb, data + b"more", fs, grain)
    dbuf = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda:0")

    def st(s, sb, Y, mode=0, wcap=2, dcap=64, **kw):
        r = _sd_raw(gpu_engine, zra, s, sb, Y, wcap, dcap, mode=mode, **kw)
        assert (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0) and _untouched(r, wcap) and r["sentinel_ok"]
        assert gpu_engine.diff_signature_stats() == ZERO and gpu_engine.diff_signature_ms() == 0
        return r["st"]

    # rule 1, in front of the header
    for mode in (2, 3, 0x80000000):
        assert st(sig, buf, J, mode=mode) == (1, 42), mode
    assert st(None, buf, J) == (1, 42) and st(sig, None, J) == (1, 42) and st(sig, buf, (None, B[1])) == (1, 42)
    assert st(sig, buf, J, dcap=64, d_data=0) == (1, 42)                       # dData NULL with a capacity
    for wrong in (sig._replace(grain=96), sig._replace(grain=32), sig._replace(grain=16384), sig._replace(frame_size=0), sig._replace(frames=sig.frames + 1),
                  sig._replace(words=sig.words + 1), sig._replace(content_size=sig.content_size + fs), sig._replace(grain=128)):
        assert st(wrong, buf, J, sig_words=sig.words + 1) == (1, 42), wrong
    assert st(sig, buf, J, sig_words=sig.words - 1) == (1, 42)
    # rule 2, in front of the header: the data buffer inside B, inside the signature
    assert st(sig, buf, J, d_data=J[0].data_ptr() + J[1] - 1, dcap=16) == (1, 42) and st(sig, buf, J, d_data=buf.data_ptr() + 8 * sig.words - 1, dcap=1) == (1, 42)
    # rule 3, in front of the frame size
    assert st(sig_o, buf_o, J) == (3, 0) and st(sig_o, buf_o, cut) == (5, 0) and st(sig, buf, Z) == (3, 0)
    # rule 4; rule 5, in front of a failing frame
    assert st(sig_o, buf_o, B) == (1, 40) and st(sig, buf, O) == (1, 40)
    assert st(sig_b, buf_b, A) == (1, 40) and st(sig_b, buf_b, D, mode=1) == (1, 40)   # UB < UA: no patch
    r = _sd_raw(gpu_engine, zra, sig, buf, B, 2, 64, d_data=dbuf.data_ptr())           # and the pair itself is fine
    assert r["st"] == (0, 0)
    assert gpu_engine.diff_signature_stats() == dict(ZERO, frames=8, equal_compressed=8, tail_decoded=1, passes=2)
    assert dbuf[:4].cpu().numpy().tobytes() == b"more" and dbuf[4:].cpu().numpy().tobytes() == bytes([SENT]) * 4092


# ---- 9
def test_damaged_frames(zra, gpu_engine):
    fs, grain = 4096, 1024
    data = _data(np.random.RandomState(8), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    G, D = (_dev(arc), len(arc)), (_dev(bad), len(bad))
    want = _frame_status(gpu_engine, zra, bad, d_arc=D[0])
    assert set(want) == {7} and want[7] != 0, want
    words, stride = zra.signature_words(len(data), fs, grain), 5
    # sign: frame 7's status, whatever the passes; outside the range's records and behind the capacity nothing is written
    for staging in (0, 4 * fs, 1):
        r = _sign_raw(gpu_engine, zra, D, grain, staging=staging)
        assert r["st"] == (1, want[7]) and r["info"] == (0,) * 6 and r["words"][words:] == [SENTW] * EXTRA, (staging, r["st"])
        assert gpu_engine.sign_stats() == SIGN_ZERO and gpu_engine.sign_ms() == 0
    r = _sign_raw(gpu_engine, zra, D, grain, first=5, count=3, staging=fs)
    assert r["st"] == (1, want[7])
    assert r["words"][:5 * stride] == [SENTW] * (5 * stride) and r["words"][8 * stride:] == [SENTW] * (words - 8 * stride + EXTRA)
    r = _sign_raw(gpu_engine, zra, D, grain, first=8)                          # the frames behind it sign
    assert r["st"] == (0, 0) and r["words"][:8 * stride] == [SENTW] * (8 * stride)
    assert r["words"][8 * stride:words] == SM.signature(arc, data, fs, grain)[8 * stride:]
    # signature diff: A sound, frame 7 flipped in B: its frame word differs, it is decoded. In front of the capacities (rule 7, rule 8)
    sig, buf, _ = _signed(gpu_engine, zra, G, arc, data, fs, grain)

    def failed(r, code):
        return r["st"] == (1, code) and (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0) and _untouched(r, r["wcap"]) and \
            r["sentinel_ok"] and gpu_engine.diff_signature_stats() == ZERO and gpu_engine.diff_signature_ms() == 0

    def run(s, sb, Y, wcap, dcap, **kw):
        return dict(_sd_raw(gpu_engine, zra, s, sb, Y, wcap, dcap, **kw), wcap=wcap)

    for staging in (0, 4 * fs, 1):
        assert failed(run(sig, buf, D, 6, 4096, staging=staging), want[7]), staging
    assert failed(run(sig, buf, D, 0, 0), want[7]) and failed(run(sig, buf, D, 6, 4096, mode=1), want[7])
    # a damaged tail frame of B: A is the first 10 frames and a half
    xs = _compress(gpu_engine, zra, data[:10 * fs + 100], 3, fs, True)
    S = (_dev(xs), len(xs))
    sig_s, buf_s, _ = _signed(gpu_engine, zra, S, xs, data[:10 * fs + 100], fs, grain)
    bad15 = _flip_mid(arc, [15])
    D15 = (_dev(bad15), len(bad15))
    code15 = _frame_status(gpu_engine, zra, bad15, d_arc=D15[0])[15]
    for staging in (0, 2 * fs):
        assert failed(run(sig_s, buf_s, D15, 6, 10 * fs, staging=staging), code15), staging
    r = _sd_raw(gpu_engine, zra, sig_s, buf_s, G, 6, 10 * fs)                  # and the sound pair answers
    assert r["st"] == (0, 0) and (r["n"], r["append_offset"], r["append_size"]) == (0, 0, 10 * fs - 100) and r["data"][:10 * fs - 100] == data[10 * fs + 100:]


# ---- 10
def test_identical_and_relevelled_archives(zra, gpu_engine):
    fs = 16384                                                                 # (of 4 KiB frames of this data, one has the same bytes at levels 3 and 9)
    data = _data(np.random.RandomState(9), 8 * fs)
    xa = _compress(gpu_engine, zra, data, 3, fs, True)
    x9 = _compress(gpu_engine, zra, data, 9, fs, True)
    A, A2, A9 = (_dev(xa), len(xa)), (_dev(xa), len(xa)), (_dev(x9), len(x9))
    for grain in (64, 8192):
        sig, buf, _ = _signed(gpu_engine, zra, A, xa, data, fs, grain)
        r = _sd_raw(gpu_engine, zra, sig, buf, A2, 4, 64)
        assert r["st"] == (0, 0) and (r["n"], r["data_size"], r["append_offset"], r["append_size"]) == (0, 0, 0, 0)
        assert _untouched(r, 4) and r["data"] == bytes([SENT]) * 64 and r["sentinel_ok"]
        assert gpu_engine.diff_signature_stats() == dict(ZERO, frames=8, equal_compressed=8, passes=1)
        assert gpu_engine.kernel_stats()["dec_launches"] == 0
        r = _sd_raw(gpu_engine, zra, sig, buf, A2, 0, 0, mode=1)               # decoded everywhere: still nothing to write
        assert r["st"] == (0, 0) and gpu_engine.diff_signature_stats() == dict(ZERO, frames=8, decoded=8, passes=1)
        assert gpu_engine.kernel_stats()["dec_launches"] >= 1
        # the same content at level 9: other compressed bytes in every frame, so every frame is decoded; no grain differs
        ea, e9 = _entries(xa), _entries(x9)
        assert all(xa[ea[0] + ea[1][f]:ea[0] + ea[1][f + 1]] != x9[e9[0] + e9[1][f]:e9[0] + e9[1][f + 1]] for f in range(8))
        r = _sd_raw(gpu_engine, zra, sig, buf, A9, 4, 64)
        assert r["st"] == (0, 0) and r["n"] == 0 and _untouched(r, 4) and r["data"] == bytes([SENT]) * 64
        assert gpu_engine.diff_signature_stats() == dict(ZERO, frames=8, decoded=8, passes=1)


def _entries(arc):
    """(header size, seek-table entries) of an archive"""
    hs, t = int.from_bytes(arc[4:8], "little") + 8, 38 + int.from_bytes(arc[34:38], "little")
    F = int.from_bytes(arc[26:30], "little") - 1
    return hs, [int.from_bytes(arc[t + 5 * i:t + 5 * i + 5], "little") for i in range(F + 1)]


# ---- 11
def test_interleaved_with_the_other_archive_calls(zra, gpu_engine):
    """One engine, one staging window: sign and signature diff between a search, a verify, a compare and a diff, on archives of two
    frame sizes, forwards and, after the scratch was handed back, in reverse."""
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
        xa, A, xb, B = _arcs(gpu_engine, zra, a, b, fs)
        pairs.append(dict(a=a, b=b, A=A, B=B, fs=fs, xa=xa, model={g: SM.signature(xa, a, fs, g) for g in (64, 1024)}))

    def search(p):
        assert gpu_engine.search(p["A"][0].data_ptr(), p["A"][1], b"NEEDLE!!", staging_bytes=3 * p["fs"]) == (1, [2 * p["fs"] + 7])

    def verify(p):
        assert gpu_engine.verify(p["B"][0].data_ptr(), p["B"][1], staging_bytes=2 * p["fs"])[0] == 0

    def compare(p):
        r = CM.ranges(p["a"], p["b"])
        assert gpu_engine.compare(p["A"][0].data_ptr(), p["A"][1], p["B"][0].data_ptr(), p["B"][1], staging_bytes=2 * 2 * p["fs"]) == (len(r), sum(n for _, n in r), r)

    def diff(p):
        want = M.patch(p["a"], p["b"], p["fs"], 64)
        r = _raw(gpu_engine, zra, p["A"], p["B"], len(want[0]), len(want[1]), 64, staging=2 * 2 * p["fs"])
        assert r["st"] == (0, 0) and r["data"] == want[1] and r["n"] == len(want[0])

    def sign(p):
        for grain, staging in ((64, 2 * p["fs"]), (1024, 0)):
            r = _sign_raw(gpu_engine, zra, p["A"], grain, staging=staging)
            assert r["st"] == (0, 0) and r["words"] == p["model"][grain] + [SENTW] * EXTRA
            p["sig", grain] = (zra.Signature(*r["info"]), r["buf"])

    def sigdiff(p):
        for grain, staging in ((64, 0), (1024, 2 * p["fs"])):
            _sigdiff(gpu_engine, zra, *p["sig", grain], p["B"], p["a"], p["b"], p["fs"], staging=staging)

    steps = [(f, p) for p in pairs for f in (sign, search, sigdiff, verify, sign, diff, sigdiff, compare, sigdiff)]
    for f, p in steps:
        f(p)
    gpu_engine.release_scratch()
    for f, p in reversed(steps):
        f(p)


# ---- 11b
def test_compare_and_signature_diff_share_one_scratch_group(zra, gpu_engine):
    """The compare and the signature diff keep their flags, tables and lists in ONE scratch group of the engine. At frame size 4 with
    four staging bytes (250 passes of one slot): a compare, a signature diff whose tables are larger (all 250 slots in one pass, a dirty
    flag per grain), the compare again: the group is reserved again at a larger size between two uses, and the third call's ranges
    and counters are the first call's. Then from empty scratch in the reverse order, the signature diff first."""
    a = b"abcdefghij" * 100
    b = bytearray(a)
    for off, n in RUNS4:
        b[off:off + n] = a[off:off + n].upper()
    b = bytes(b)
    xa, A, xb, B = _arcs(gpu_engine, zra, a, b, 4)
    sig, buf, _ = _signed(gpu_engine, zra, A, xa, a, 4, 64)

    def compare():
        r = gpu_engine.compare(A[0].data_ptr(), A[1], B[0].data_ptr(), B[1], staging_bytes=4)
        assert r == (len(RUNS4), sum(n for _, n in RUNS4), RUNS4), r
        s = gpu_engine.compare_stats()
        assert s["passes"] == 250, s
        return r, s

    def sigdiff():
        want, r = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, 4, staging=0)
        s = gpu_engine.diff_signature_stats()
        assert s["passes"] == 1, s
        return want, {k: v for k, v in r.items()}, s

    for order in ((compare, sigdiff, compare), (sigdiff, compare, sigdiff)):
        gpu_engine.release_scratch()
        got = [f() for f in order]
        assert got[2] == got[0], (got[0], got[2])


# ---- 12
def test_cli_modes_sign_and_sigdiff(zra, gpu_engine, tmp_path):
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

    def run(mode, *args):
        return subprocess.run([TOOL, mode] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    for grain, seed, opts in ((4096, 0, ()), (64, 0, ("-g", 64)), (1024, 77, ("-s", 77, "-g", 1024))):
        sigf = tmp_path / ("a.%d.sig" % grain)
        r = run("sign", path["a"], sigf, *opts)
        words = SM.signature(files["a"], a, fs, grain, seed)
        assert (r.returncode, r.stdout) == (0, "11 frames, %d words, grain %d\n" % (len(words), grain)), (r.stdout, r.stderr)
        raw = sigf.read_bytes()
        assert raw[:40] == len(a).to_bytes(8, "little") + fs.to_bytes(4, "little") + grain.to_bytes(4, "little") + seed.to_bytes(8, "little") + \
            (11).to_bytes(8, "little") + len(words).to_bytes(8, "little")
        assert raw[40:] == b"".join(w.to_bytes(8, "little") for w in words)
        for y in ("a", "a9"):
            r = run("sigdiff", sigf, path[y])
            assert (r.returncode, r.stdout) == (0, "append 0\n0 writes, 0 bytes written, 0 bytes of patch data\n"), (y, r.stdout, r.stderr)
        d = run("diff", path["a"], path["b"], "-g", grain)
        r = run("sigdiff", sigf, path["b"])
        w, data, ao, asz = M.patch(a, b, fs, grain)
        assert d.returncode == r.returncode == 1, (r.stdout, r.stderr)
        assert r.stdout == d.stdout == "".join("%d %d\n" % x for x in w) + "append %d\n%d writes, %d bytes written, %d bytes of patch data\n" % (asz, len(w), ao, len(data))
    sigf = tmp_path / "a.64.sig"
    sig_b = tmp_path / "b.sig"
    assert run("sign", path["b"], sig_b).returncode == 0
    (tmp_path / "short.sig").write_bytes(sigf.read_bytes()[:-8])
    (tmp_path / "odd.sig").write_bytes(sigf.read_bytes()[:39])
    for mode, args in (("sigdiff", (tmp_path / "junk.sig", path["a"])), ("sigdiff", (path["junk"], path["a"])), ("sigdiff", (sigf, path["junk"])),
                       ("sigdiff", (sigf, path["other"])), ("sigdiff", (sig_b, path["a"])), ("sigdiff", (sigf, tmp_path / "missing.zra")),
                       ("sigdiff", (tmp_path / "short.sig", path["a"])), ("sigdiff", (tmp_path / "odd.sig", path["a"])), ("sigdiff", (sigf,)),
                       ("sigdiff", (sigf, path["a"], "-g", 64)),
                       ("sign", (path["junk"], tmp_path / "x.sig")), ("sign", (path["a"], tmp_path / "x.sig", "-g", 3)), ("sign", (path["a"], tmp_path / "x.sig", "-g")),
                       ("sign", (path["a"], tmp_path / "x.sig", "-x", 3)), ("sign", (path["a"], tmp_path / "x.sig", "-s", "seed")), ("sign", (path["a"],)),
                       ("sign", (tmp_path / "missing.zra", tmp_path / "x.sig"))):
        r = run(mode, *args)
        assert r.returncode == 2 and r.stdout == "", (mode, args, r.stdout, r.stderr)
