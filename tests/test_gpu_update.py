"""GPU tests of ZraHipUpdateArchive (include/zra_hip.h): byte ranges of a device-resident archive overwritten and bytes appended.
The yardstick is a from-scratch compress of the patched content: frames are independent and the encoder is deterministic per
(content, level, checksum), so at the level the archive was written with the update must reproduce it byte for byte, header, seek
table and CRC-32 included. Counters pin that the work is proportional to the change; statuses are compared with the calls they are
specified by."""
import ctypes

import numpy as np
import pytest

import corpus as C
import oracle_lib as O

pytestmark = pytest.mark.gpu
SENT = 0xEE


def _data(rng, n):
    """Compressible bytes: a small alphabet with copied runs (tests/test_gpu_archive_cache.py::_data)."""
    a = rng.randint(0, 24, size=n).astype(np.uint8)
    for _ in range(n // 4096):
        src, ln = int(rng.randint(0, max(1, n - 600))), int(rng.randint(16, 512))
        dst = int(rng.randint(0, max(1, n - ln)))
        a[dst:dst + ln] = a[src:src + ln]
    return a.tobytes()


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) if len(b) else b"\0", dtype=np.uint8).copy()).to("cuda:0")


def _compress(eng, zra, data, level, fs, ck):
    import torch
    d_in = _dev(data)
    d_arc = torch.empty(zra.GetOutputBufferSize(len(data), fs) + 64, dtype=torch.uint8, device="cuda:0")
    asz = eng.compress(d_in.data_ptr(), len(data), d_arc.data_ptr(), level, fs, ck)
    return d_arc[:asz].cpu().numpy().tobytes()


def _patched(data, writes, append=b""):
    p = bytearray(data)
    for off, b in writes:
        p[off:off + len(b)] = b
    return bytes(p) + bytes(append)


def _update(eng, zra, arc, writes, append=b"", level=3, ck=True, cap=None, d_arc=None):
    """((zra, zstd), bytes of the output buffer, size reported) of one update; the output is pre-filled with the sentinel. writes =
    [(offset, bytes)]; their bytes lie in one device blob with gaps between them."""
    import torch
    blob, offs, sizes, doffs = bytearray(b"\x55" * 3), [], [], []
    for off, b in writes:
        offs.append(off); sizes.append(len(b)); doffs.append(len(blob))
        blob += b + b"\x55" * 5
    d_data = _dev(blob)
    d_app = _dev(append)
    if d_arc is None:
        d_arc = _dev(arc)
    if cap is None:
        U = int.from_bytes(arc[18:26], "little"); fs = int.from_bytes(arc[30:34], "little")
        cap = len(arc) + zra.GetOutputBufferSize(U + len(append), fs) + 64
    d_out = torch.full((cap + 16,), SENT, dtype=torch.uint8, device="cuda:0")
    try:
        size = eng.update(d_arc.data_ptr(), len(arc), d_out.data_ptr(), cap, writes=(offs, sizes, doffs), d_data=d_data.data_ptr(),
                          d_append=d_app.data_ptr() if len(append) else 0, append_size=len(append), level=level, checksum=ck)
        st = (0, 0)
    except zra.ZraError as e:
        st, size = (e.zra, e.zstd), e.needed
    return st, d_out.cpu().numpy().tobytes(), size


def _untouched(out, cap):
    return out == bytes([SENT]) * (cap + 16)


def _decompress(eng, arc):
    import torch
    U = int.from_bytes(arc[18:26], "little")
    d = _dev(arc)
    d_out = torch.empty(U + 64, dtype=torch.uint8, device="cuda:0")
    eng.decompress(d.data_ptr(), len(arc), d_out.data_ptr(), U)
    return d_out[:U].cpu().numpy().tobytes()


def _table(arc):
    """(header size, body offsets of the frames + the end) of an archive"""
    hs = int.from_bytes(arc[4:8], "little") + 8
    nt = int.from_bytes(arc[26:30], "little"); meta = int.from_bytes(arc[34:38], "little")
    t = 38 + meta
    return hs, [int.from_bytes(arc[t + 5 * i:t + 5 * i + 5], "little") for i in range(nt)]


def _frames(arc):
    hs, e = _table(arc)
    return [arc[hs + e[i]:hs + e[i + 1]] for i in range(len(e) - 1)]


def _touched(writes, append, U, fs):
    t = set()
    for off, b in writes:
        if len(b):
            t.update(range(off // fs, (off + len(b) - 1) // fs + 1))
    if len(append):
        t.update(range(U // fs, (U + len(append) - 1) // fs + 1))
    return t


def _random_writes(rng, n, fs):
    """non-overlapping writes of every size class, frame-aligned and not, in [0, n - 200), and one that ends exactly at n"""
    sizes = [1, 2, 100, fs - 1, fs, fs + 1, 3 * fs + 5]
    rng.shuffle(sizes)
    room = n - 200 - sum(sizes)
    gap = max(2, room // (len(sizes) + 1))
    writes, pos = [], 0
    for i, z in enumerate(sizes):
        pos += int(rng.randint(1, gap))
        if i % 2:
            al = (pos + fs - 1) // fs * fs
            if al + z + sum(sizes[i + 1:]) + gap * (len(sizes) - 1 - i) < n - 200:
                pos = al
        assert pos + z <= n - 200
        writes.append((pos, rng.randint(0, 256, size=z).astype(np.uint8).tobytes()))
        pos += z
    writes.append((n - 100, rng.randint(0, 256, size=100).astype(np.uint8).tobytes()))
    rng.shuffle(writes)
    return writes


# ---- 1
@pytest.mark.parametrize("level,ck", [(3, True), (1, False), (9, True)])
@pytest.mark.parametrize("fs", [4096, 65536, 10000])
def test_update_equals_compress_from_scratch(zra, gpu_engine, fs, level, ck):
    rng = np.random.RandomState(fs + level)
    nfr = 14 if fs == 65536 else 40
    for n in (nfr * fs, nfr * fs - fs // 2):
        data = _data(rng, n)
        arc = _compress(gpu_engine, zra, data, level, fs, ck)
        # appends: none; fs / 4 bytes (inside the short last frame, or a new short frame when n is a frame multiple); several new frames
        for app_n in (0, fs // 4, 2 * fs + 77):
            writes = _random_writes(rng, n, fs)
            append = _data(rng, app_n) if app_n else b""
            want_content = _patched(data, writes, append)
            want = _compress(gpu_engine, zra, want_content, level, fs, ck)
            st, out, size = _update(gpu_engine, zra, arc, writes, append, level, ck)
            assert st == (0, 0), (fs, level, n, app_n, st)
            assert size == len(want) and out[:size] == want, (fs, level, n, app_n)
            assert out[size:] == bytes([SENT]) * (len(out) - size)
            s = gpu_engine.update_stats()
            assert s["frames"] == (len(want_content) + fs - 1) // fs
            assert s["touched"] == s["compressed"] == len(_touched(writes, append, n, fs))
            assert s["content_bytes"] == sum(len(b) for _, b in writes) + app_n
            if level == 3 and len(want_content) <= (1 << 20):
                ost, oarc = O.zra_compress(want_content, 3, fs, ck)
                assert ost == (0, 0) and out[:size] == oarc, (fs, n, app_n)


# ---- 2
def test_untouched_frames_are_carried_touched_ones_encoded_again(zra, gpu_engine):
    rng = np.random.RandomState(2)
    fs = 4096
    n = 50 * fs + 1234
    data = _data(rng, n)
    backend = "zl" if O.have_libzstd() else "zo"
    foreign_frames = [O.compress_frame(data[o:o + fs], level=19, checksum=True, backend=backend) for o in range(0, n, fs)]
    foreign = zra.stitch_header([len(f) for f in foreign_frames], n, fs) + b"".join(foreign_frames)
    assert _decompress(gpu_engine, foreign) == data
    for arc in (_compress(gpu_engine, zra, data, 3, fs, True), foreign):
        writes = [(5 * fs + 17, b"\x01" * 40), (9 * fs - 3, b"\x02" * 9), (20 * fs, rng.randint(0, 256, size=2 * fs).astype(np.uint8).tobytes())]
        append = _data(rng, fs + 5)
        st, out, size = _update(gpu_engine, zra, arc, writes, append, level=1)
        assert st == (0, 0)
        new = out[:size]
        want_content = _patched(data, writes, append)
        assert _decompress(gpu_engine, new) == want_content
        touched = _touched(writes, append, n, fs)
        assert touched == {5, 8, 9, 20, 21, 50, 51}
        old_f, new_f = _frames(arc), _frames(new)
        assert len(new_f) == 52
        level1 = _frames(_compress(gpu_engine, zra, want_content, 1, fs, True))
        for f in range(52):
            if f in touched:
                assert new_f[f] == level1[f], f                                # encoded again, with the level of the update
            else:
                assert new_f[f] == old_f[f], f                                 # carried over byte for byte
        s = gpu_engine.update_stats()
        assert s["carried_bytes"] == sum(len(old_f[f]) for f in range(50) if f not in touched)
        assert s["encoded_bytes"] == sum(len(new_f[f]) for f in touched)
        assert (s["touched"], s["decoded"]) == (7, 4)                          # 20 and 21 are replaced whole, 51 is new


# ---- 3
def test_work_is_proportional_to_the_change(zra, gpu_engine):
    rng = np.random.RandomState(3)
    fs, nfr = 65536, 1024
    n = nfr * fs
    data = _data(rng, n)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d_arc = _dev(arc)
    hs, e = _table(arc)
    body = e[-1]
    K = ("frames", "touched", "decoded", "compressed", "passes")
    # one 4 KiB write inside a frame
    w = [(700 * fs + 1000, rng.randint(0, 256, size=4096).astype(np.uint8).tobytes())]
    st, out, size = _update(gpu_engine, zra, arc, w, d_arc=d_arc)
    s = gpu_engine.update_stats()
    assert st == (0, 0) and tuple(s[k] for k in K) == (nfr, 1, 1, 1, 1), s
    assert s["carried_bytes"] == body - (e[701] - e[700]) and s["content_bytes"] == 4096
    assert _decompress(gpu_engine, out[:size]) == _patched(data, w)
    # one write covering exactly frames 5..7: nothing to decode
    w = [(5 * fs, rng.randint(0, 256, size=3 * fs).astype(np.uint8).tobytes())]
    st, out, size = _update(gpu_engine, zra, arc, w, d_arc=d_arc)
    s = gpu_engine.update_stats()
    assert st == (0, 0) and tuple(s[k] for k in K) == (nfr, 3, 0, 3, 1), s
    assert s["carried_bytes"] == body - (e[8] - e[5])
    # append only, behind a whole number of frames
    app = _data(rng, 2 * fs + 10)
    st, out, size = _update(gpu_engine, zra, arc, [], app, d_arc=d_arc)
    s = gpu_engine.update_stats()
    assert st == (0, 0) and tuple(s[k] for k in K) == (nfr + 3, 3, 0, 3, 1), s
    assert s["carried_bytes"] == body
    assert out[:size] == _compress(gpu_engine, zra, data + app, 3, fs, True)
    # nothing at all (and a write of no bytes far outside the content): the same archive
    st, out, size = _update(gpu_engine, zra, arc, [(1 << 60, b"")], d_arc=d_arc)
    s = gpu_engine.update_stats()
    assert st == (0, 0) and tuple(s[k] for k in K) == (nfr, 0, 0, 0, 0), s
    assert out[:size] == arc and s["carried_bytes"] == body and s["encoded_bytes"] == 0
    # counters are zero after any other outcome
    st, out, size = _update(gpu_engine, zra, arc, [(n, b"\x01")], d_arc=d_arc)
    assert st == (5, 0) and set(gpu_engine.update_stats().values()) == {0}


# ---- 4
def test_empty_and_tiny_archives(zra, gpu_engine):
    rng = np.random.RandomState(4)
    fs = 4096
    empty = _compress(gpu_engine, zra, b"", 3, fs, True)
    assert len(empty) == 43
    app = _data(rng, 3 * fs + 9)
    st, out, size = _update(gpu_engine, zra, empty, [], app)
    assert st == (0, 0) and out[:size] == _compress(gpu_engine, zra, app, 3, fs, True)
    st, out, size = _update(gpu_engine, zra, empty, [])
    assert st == (0, 0) and out[:size] == empty
    one = _compress(gpu_engine, zra, b"a", 3, fs, True)
    st, out, size = _update(gpu_engine, zra, one, [], b"b")
    assert st == (0, 0) and out[:size] == _compress(gpu_engine, zra, b"ab", 3, fs, True)
    assert gpu_engine.update_stats()["decoded"] == 1
    st, out, size = _update(gpu_engine, zra, one, [(0, b"z")])
    assert st == (0, 0) and out[:size] == _compress(gpu_engine, zra, b"z", 3, fs, True)
    assert gpu_engine.update_stats()["decoded"] == 0


# ---- 5
def test_meta_section_is_kept(zra, gpu_engine):
    L = zra.load()
    rng = np.random.RandomState(5)
    fs = 16384
    data = _data(rng, 9 * fs + 1000)
    meta = bytes(rng.randint(0, 256, size=100).astype(np.uint8))
    c = ctypes.c_void_p()
    assert L.ZraCreateCompressor(ctypes.byref(c), len(data), 3, fs, True, ctypes.create_string_buffer(meta, len(meta)), len(meta)).tup() == (0, 0)
    body, pos = b"", 0
    while pos < len(data):
        chunk = data[pos:pos + 3 * fs]
        out = ctypes.create_string_buffer(L.ZraGetOutputBufferSizeWithCompressor(c, len(chunk)))
        osz = ctypes.c_size_t(0)
        assert L.ZraCompressWithCompressor(c, ctypes.create_string_buffer(chunk, len(chunk)), len(chunk), out, ctypes.byref(osz)).tup() == (0, 0)
        body += out.raw[:osz.value]; pos += len(chunk)
    hsz = L.ZraGetHeaderSizeWithCompressor(c)
    hb = ctypes.create_string_buffer(hsz)
    assert L.ZraGetHeaderWithCompressor(c, hb).tup() == (0, 0)
    L.ZraDeleteCompressor(c)
    arc = hb.raw[:hsz] + body
    assert arc[38:138] == meta
    writes = [(fs - 10, b"\x07" * 30), (len(data) - 5, b"\x08" * 5)]
    append = _data(rng, fs)
    st, out, size = _update(gpu_engine, zra, arc, writes, append)
    assert st == (0, 0)
    new = out[:size]
    assert _decompress(gpu_engine, new) == _patched(data, writes, append)
    plain = _compress(gpu_engine, zra, _patched(data, writes, append), 3, fs, True)
    assert _frames(new) == _frames(plain)
    L.ZraHipSetOptions(1)                                                      # header constructors verify the CRC-32
    try:
        h = ctypes.c_void_p()
        assert L.ZraCreateHeader2(ctypes.byref(h), ctypes.create_string_buffer(new, len(new)), len(new)).tup() == (0, 0)
        assert L.ZraGetMetadataSize(h) == 100 and L.ZraGetUncompressedSizeWithHeader(h) == len(data) + fs
        mbuf = ctypes.create_string_buffer(100)
        L.ZraGetMetadata(h, mbuf)
        assert mbuf.raw == meta
        L.ZraDeleteHeader(h)
        bad = bytearray(new); bad[50] ^= 1                                     # (the check does look: a changed meta byte fails it)
        assert L.ZraCreateHeader2(ctypes.byref(h), ctypes.create_string_buffer(bytes(bad), len(bad)), len(bad)).tup() != (0, 0)
    finally:
        L.ZraHipSetOptions(0)


# ---- 6
def test_refusals_leave_the_output_alone(zra, gpu_engine):
    import torch
    L = zra.load()
    rng = np.random.RandomState(6)
    fs = 4096
    n = 30 * fs + 77
    data = _data(rng, n)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    # the bound is inclusive: a write may reach the last byte, not the one behind it
    st, out, size = _update(gpu_engine, zra, arc, [(n - 9, b"\x01" * 10)])
    assert st == (5, 0) and _untouched(out, len(out) - 16)
    st, out, size = _update(gpu_engine, zra, arc, [(2 ** 64 - 4, b"\x01" * 10)])
    assert st == (5, 0) and _untouched(out, len(out) - 16)
    st, out, size = _update(gpu_engine, zra, arc, [(n - 10, b"\x01" * 10)])
    assert st == (0, 0) and out[:size] == _compress(gpu_engine, zra, data[:-10] + b"\x01" * 10, 3, fs, True)
    # overlapping writes
    st, out, size = _update(gpu_engine, zra, arc, [(100, b"\x01" * 10), (5000, b"\x03" * 10), (109, b"\x02" * 10)])
    assert st == (1, 42) and _untouched(out, len(out) - 16)
    st, out, size = _update(gpu_engine, zra, arc, [(100, b"\x01" * 10), (5000, b"\x03" * 10), (110, b"\x02" * 10)])
    assert st == (0, 0)
    # capacity: one byte short reports the size needed; exactly that size succeeds
    w = [(3 * fs + 1, b"\x05" * 999)]
    st, out, need = _update(gpu_engine, zra, arc, w)
    assert st == (0, 0)
    st, out2, size = _update(gpu_engine, zra, arc, w, cap=need - 1)
    assert st == (6, 0) and size == need and _untouched(out2, need - 1)
    st, out3, size = _update(gpu_engine, zra, arc, w, cap=need)
    assert st == (0, 0) and size == need and out3[:need] == out[:need] and out3[need:] == bytes([SENT]) * 16
    # output inside the archive buffer
    big = torch.full((len(arc) + 4096,), SENT, dtype=torch.uint8, device="cuda:0")
    big[:len(arc)] = _dev(arc)
    before = big.cpu().numpy().tobytes()
    osz = ctypes.c_size_t(0x1234)
    for d_out, cap in ((big.data_ptr() + len(arc) - 1, 4096), (big.data_ptr(), len(arc)), (big.data_ptr() + 10, 5)):
        st = L.ZraHipUpdateArchive(gpu_engine.h, big.data_ptr(), len(arc), None, None, None, None, 0, None, 0, d_out, cap, ctypes.byref(osz), 3, True)
        assert st.tup() == (1, 42) and osz.value == 0x1234
    assert big.cpu().numpy().tobytes() == before
    # NULL arguments behind a real engine
    d_arc = _dev(arc)
    d_out = torch.full((len(arc) + 8192,), SENT, dtype=torch.uint8, device="cuda:0")
    u64 = ctypes.c_uint64
    off, one, zero = (u64 * 1)(5), (u64 * 1)(1), (u64 * 1)(0)
    A, O_, D = d_arc.data_ptr(), d_out.data_ptr(), d_arc.data_ptr()
    cap = len(arc) + 8192
    for name, args in {
        "outSize": (A, len(arc), D, off, one, zero, 1, None, 0, O_, cap, None),
        "dOut": (A, len(arc), D, off, one, zero, 1, None, 0, None, cap, ctypes.byref(osz)),
        "dArchive": (None, len(arc), D, off, one, zero, 1, None, 0, O_, cap, ctypes.byref(osz)),
        "hOffsets": (A, len(arc), D, None, one, zero, 1, None, 0, O_, cap, ctypes.byref(osz)),
        "hSizes": (A, len(arc), D, off, None, zero, 1, None, 0, O_, cap, ctypes.byref(osz)),
        "hDataOffsets": (A, len(arc), D, off, one, None, 1, None, 0, O_, cap, ctypes.byref(osz)),
        "dData": (A, len(arc), None, off, one, zero, 1, None, 0, O_, cap, ctypes.byref(osz)),
        "dAppend": (A, len(arc), D, off, zero, zero, 1, None, 7, O_, cap, ctypes.byref(osz)),
    }.items():
        assert L.ZraHipUpdateArchive(gpu_engine.h, *args, 3, True).tup() == (1, 42), name
        assert osz.value == 0x1234, name
    assert d_out.cpu().numpy().tobytes() == bytes([SENT]) * cap
    # dData may be NULL when every write is empty
    assert L.ZraHipUpdateArchive(gpu_engine.h, A, len(arc), None, off, zero, zero, 1, None, 0, O_, cap, ctypes.byref(osz), 3, True).tup() == (0, 0)
    assert d_out[:osz.value].cpu().numpy().tobytes() == arc
    # header damage: the statuses of opening a handle on the same bytes
    h = ctypes.c_void_p()
    n_cmp = 0
    for case, a, _, _, _ in C.mutated_headers(321, 40, O.zra_compress):
        d = _dev(a)
        so = L.ZraHipArchiveOpen(gpu_engine.h, d.data_ptr(), len(a), 0, ctypes.byref(h)).tup()
        if so == (0, 0):
            L.ZraHipArchiveClose(h)
            continue
        st, out, size = _update(gpu_engine, zra, a, [], b"x", cap=len(a) + 100000, d_arc=d)
        assert st == so, (case, st, so)
        assert _untouched(out, len(a) + 100000)
        n_cmp += 1
    assert n_cmp > 0
    for size in (0, 10, 38, 42):
        st = L.ZraHipUpdateArchive(gpu_engine.h, A, size, None, None, None, None, 0, None, 0, O_, cap, ctypes.byref(osz), 3, True)
        assert st.tup() == (5, 0), size
    # an old seek table that runs backwards over a frame that is carried over
    hs, e = _table(arc)
    bad = bytearray(arc)
    bad[38 + 5 * 10:38 + 5 * 10 + 5] = (e[12] + 1).to_bytes(5, "little")       # entry 10 beyond entry 11: frame 10 is inverted
    bad = bytes(bad)
    st, out, size = _update(gpu_engine, zra, bad, [(0, b"\x01")])
    assert st == (1, 20) and _untouched(out, len(out) - 16)
    bad2 = bytearray(arc)
    bad2[38 + 5 * 30:38 + 5 * 30 + 5] = (e[31] + 1000).to_bytes(5, "little")   # the last frame ends beyond the body
    st, out, size = _update(gpu_engine, zra, bytes(bad2), [(0, b"\x01")])
    assert st == (1, 20) and _untouched(out, len(out) - 16)


# ---- 7
def test_damaged_frames(zra, gpu_engine):
    import torch
    L = zra.load()
    rng = np.random.RandomState(7)
    fs = 4096
    n = 20 * fs
    data = _data(rng, n)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    hs, e = _table(arc)

    def damage(a, k):
        b = bytearray(a)
        b[hs + (e[k] + e[k + 1]) // 2] ^= 0x10
        return bytes(b)

    def batch_status(a, off):
        d = _dev(a)
        d_out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        L.ZraHipSetOptions(8)                                                  # ZRA_HIP_OPT_RA_WHOLE_FRAMES
        try:
            gpu_engine.decompress_ra_batch(d.data_ptr(), len(a), d_out.data_ptr(), [off], [8], [0])
            return (0, 0)
        except zra.ZraError as x:
            return (x.zra, x.zstd)
        finally:
            L.ZraHipSetOptions(0)

    k = 7
    bad = damage(arc, k)
    want = batch_status(bad, k * fs + 100)
    assert want[0] == 1 and want[1] != 0
    # a partial write into the damaged frame: its status, nothing written
    st, out, size = _update(gpu_engine, zra, bad, [(k * fs + 100, b"\x01" * 50)])
    assert st == want and _untouched(out, len(out) - 16)
    assert set(gpu_engine.update_stats().values()) == {0}
    # a write that replaces the damaged frame whole: it is not decoded, and the result is sound
    w = [(k * fs, rng.randint(0, 256, size=fs).astype(np.uint8).tobytes())]
    st, out, size = _update(gpu_engine, zra, bad, w)
    assert st == (0, 0) and out[:size] == _compress(gpu_engine, zra, _patched(data, w), 3, fs, True)
    # a write elsewhere: the damaged bytes are carried as they are
    w = [(2 * fs + 5, b"\x02" * 10)]
    st, out, size = _update(gpu_engine, zra, bad, w)
    assert st == (0, 0)
    assert _frames(out[:size])[k] == _frames(bad)[k] != _frames(arc)[k]
    assert batch_status(out[:size], k * fs + 100) == want
    # two damaged frames, both partly written: the lower one's status. Frame 12 gets a damaged checksum (its last 4 bytes), frame 7 a
    # damaged block: two different statuses.
    b2 = bytearray(bad); b2[hs + e[13] - 1] ^= 0xFF; b2 = bytes(b2)
    s7, s12 = batch_status(b2, 7 * fs), batch_status(b2, 12 * fs)
    assert s12 == (1, 22)
    st, out, size = _update(gpu_engine, zra, b2, [(12 * fs + 9, b"\x03" * 9), (7 * fs + 1, b"\x04")])
    assert st == s7 and _untouched(out, len(out) - 16)
    st, out, size = _update(gpu_engine, zra, b2, [(12 * fs + 9, b"\x03" * 9)])
    assert st == s12


# ---- 8
def test_many_touched_frames_go_through_several_passes(zra, gpu_engine):
    import torch
    fs, nfr = 4096, 70000
    n = nfr * fs
    g = torch.Generator(device="cuda:0"); g.manual_seed(8)
    d_data = torch.randint(0, 20, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    d_data[fs:] = torch.where(d_data[fs:] < 12, d_data[:-fs], d_data[fs:])      # frames resemble their predecessor: compressible
    d_data = d_data.contiguous()
    cap = zra.GetOutputBufferSize(n, fs) + 64
    d_arc = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    asz = gpu_engine.compress(d_data.data_ptr(), n, d_arc.data_ptr(), 3, fs, True)
    # one write per frame: 16 bytes at in-frame offset 1000
    d_new = torch.randint(0, 256, (nfr * 16,), dtype=torch.uint8, device="cuda:0", generator=g)
    offs = np.arange(nfr, dtype=np.uint64) * fs + 1000
    d_out = torch.full((cap,), SENT, dtype=torch.uint8, device="cuda:0")
    size = gpu_engine.update(d_arc.data_ptr(), asz, d_out.data_ptr(), cap, writes=(offs, np.full(nfr, 16, dtype=np.uint64), np.arange(nfr, dtype=np.uint64) * 16),
                             d_data=d_new.data_ptr())
    s = gpu_engine.update_stats()
    assert (s["frames"], s["touched"], s["decoded"], s["compressed"]) == (nfr, nfr, nfr, nfr), s
    assert s["passes"] >= 2 and s["carried_bytes"] == 0 and s["content_bytes"] == 16 * nfr
    d_data.view(nfr, fs)[:, 1000:1016] = d_new.view(nfr, 16)
    d_ref = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    rsz = gpu_engine.compress(d_data.data_ptr(), n, d_ref.data_ptr(), 3, fs, True)
    assert size == rsz and torch.equal(d_out[:size], d_ref[:rsz])
    assert bool((d_out[size:] == SENT).all())


# ---- 9
def test_update_after_release_scratch_and_repeat(zra, gpu_engine):
    rng = np.random.RandomState(9)
    fs = 10000
    n = 33 * fs + 3
    data = _data(rng, n)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    w = [(4 * fs - 2, b"\x09" * 7), (30 * fs, b"\x0a" * fs)]
    app = _data(rng, 777)
    want = _compress(gpu_engine, zra, _patched(data, w, app), 3, fs, True)
    gpu_engine.release_scratch()
    st, out1, size1 = _update(gpu_engine, zra, arc, w, app)
    assert st == (0, 0) and out1[:size1] == want
    st, out2, size2 = _update(gpu_engine, zra, arc, w, app)
    assert st == (0, 0) and out2 == out1
    gpu_engine.release_scratch()
    st, out3, size3 = _update(gpu_engine, zra, arc, w, app)
    assert st == (0, 0) and out3 == out1
