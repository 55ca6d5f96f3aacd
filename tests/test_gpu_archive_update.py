"""GPU tests of ZraHipArchiveUpdate (include/zra_hip.h): an update through an archive handle, which takes old plaintext from the
handle's cache where it is resident, binds the handle to the result and keeps the cache coherent and warm. The yardsticks are never
the call itself: ZraHipUpdateArchive in a call of its own on the same old bytes, ZraHipCompressBuffer of the patched content, numpy
slices of the patched content, and a FRESH handle opened on the result."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENT = 0xEE
COUNTERS = ("reads", "hits", "misses", "evictions")


def _data(rng, n):
    """Compressible bytes: a small alphabet with copied runs (tests/test_gpu_update.py::_data)."""
    a = rng.randint(0, 24, size=n).astype(np.uint8)
    for _ in range(n // 4096):
        src, ln = int(rng.randint(0, max(1, n - 600))), int(rng.randint(16, 512))
        dst = int(rng.randint(0, max(1, n - ln)))
        a[dst:dst + ln] = a[src:src + ln]
    return a.tobytes()


def _rand(rng, n):
    """new bytes: outside _data's alphabet, so a written byte always differs from the original one"""
    return rng.randint(128, 256, size=n).astype(np.uint8).tobytes()


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) if len(b) else b"\0", dtype=np.uint8).copy()).to("cuda:0")


def _compress(eng, zra, data, fs, level=3, ck=True):
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


def _cap(zra, arc_len, U, fs, app_n):
    return arc_len + zra.GetOutputBufferSize(U + app_n, fs) + 64


def _update(call, writes, append, cap, d_out=None):
    """((zra, zstd), the output tensor, size reported) of call(d_out, cap, writes=, d_data=, d_append=, append_size=); the output
    (cap + 16 bytes) is pre-filled with the sentinel unless one is given. writes = [(offset, bytes)], their bytes in one device blob
    with gaps between them."""
    import torch
    import zra_amd
    blob, offs, sizes, doffs = bytearray(b"\x55" * 3), [], [], []
    for off, b in writes:
        offs.append(off); sizes.append(len(b)); doffs.append(len(blob))
        blob += b + b"\x55" * 5
    d_data, d_app = _dev(blob), _dev(append)
    if d_out is None:
        d_out = torch.full((cap + 16,), SENT, dtype=torch.uint8, device="cuda:0")
    try:
        size = call(d_out.data_ptr(), cap, writes=(offs, sizes, doffs), d_data=d_data.data_ptr(),
                    d_append=d_app.data_ptr() if len(append) else 0, append_size=len(append))
        st = (0, 0)
    except zra_amd.ZraError as e:
        st, size = (e.zra, e.zstd), e.needed
    torch.cuda.synchronize()
    return st, d_out, size


def _engine_update(eng, d_arc, asz, writes, append, cap, level=3, ck=True):
    """The yardstick: ZraHipUpdateArchive of the archive at d_arc in a call of its own -> (status, output bytes, size)."""
    st, d_out, size = _update(lambda o, c, **k: eng.update(d_arc.data_ptr(), asz, o, c, level=level, checksum=ck, **k), writes, append, cap)
    return st, d_out.cpu().numpy().tobytes(), size


def _handle_update(A, writes, append, cap, level=3, ck=True, d_out=None):
    return _update(lambda o, c, **k: A.update(o, c, level=level, checksum=ck, **k), writes, append, cap, d_out)


def _read(A, queries):
    """the answers of one read of queries [(offset, size)] through handle A"""
    import torch
    offs, sizes = [q[0] for q in queries], [q[1] for q in queries]
    oofs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
    d = torch.empty(int(sum(sizes)) + 16, dtype=torch.uint8, device="cuda:0")
    A.read(d.data_ptr(), offs, sizes, oofs)
    b = d.cpu().numpy().tobytes()
    return [b[int(o):int(o) + int(s)] for o, s in zip(oofs, sizes)]


def _want(content, queries):
    return [content[o:o + s] for o, s in queries]


def _frame_queries(frames, fs, U):
    """one query per frame: the whole frame, cut at the last readable byte (the reference's bound: offset + size < U)"""
    return [(f * fs, min(fs, U - 1 - f * fs)) for f in frames]


def _warm(A, frames, fs):
    _read(A, [(f * fs + 1, 1) for f in frames])


def _delta(after, before, keys=COUNTERS):
    return tuple(after[k] - before[k] for k in keys)


def _queries(rng, U, fs, nq):
    sizes = np.minimum(rng.choice([1, 2, 100, fs - 1, fs, fs + 1, 2 * fs + 3], size=nq), U - 2)
    return [(int(rng.randint(0, U - int(s) - 1)), int(s)) for s in sizes]


def _random_writes(rng, n, fs):
    """non-overlapping writes of every size class, frame-aligned and not, in [0, n - 200), and one that ends exactly at n
    (tests/test_gpu_update.py::_random_writes)"""
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
        writes.append((pos, _rand(rng, z)))
        pos += z
    writes.append((n - 100, _rand(rng, 100)))
    rng.shuffle(writes)
    return writes


RESIDENT = (2, 5, 6, 9, 14, 20, 27, 39)     # of 40 frames; 39 is the short last one


def _mixed_writes(rng, fs, n):
    """Every size class of tests/test_gpu_update.py over the frames RESIDENT and their neighbours -> (writes, frames partly written,
    frames written whole)."""
    w = [(2 * fs + 17, _rand(rng, 100)),                # wholly inside resident frame 2
         (6 * fs + fs - 50, _rand(rng, 100)),           # spans resident 6 and non-resident 7
         (9 * fs, _rand(rng, fs)),                      # replaces resident frame 9 whole
         (11 * fs + 5, _rand(rng, fs - 1)),             # non-resident 11 and 12
         (14 * fs + 1, _rand(rng, 1)),                  # resident 14
         (16 * fs + 7, _rand(rng, 2)),                  # non-resident 16
         (20 * fs - 3, _rand(rng, fs + 1)),             # non-resident 19 and resident 20
         (22 * fs + 9, _rand(rng, 3 * fs + 5)),         # 22 .. 25: 23 and 24 whole
         (n - 100, _rand(rng, 100))]                    # up to the last byte, in resident frame 39
    rng.shuffle(w)
    return w, {2, 6, 7, 11, 12, 14, 16, 19, 20, 22, 25, 39}, {9, 23, 24}


# ---- 1
@pytest.mark.parametrize("fs", [4096, 10000, 65536])
def test_equals_engine_update_and_compress_from_scratch(zra, gpu_engine, fs):
    rng = np.random.RandomState(fs)
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    arc = _compress(gpu_engine, zra, content, fs)
    d_arc = _dev(arc)
    A = zra.Archive(gpu_engine, d_arc.data_ptr(), len(arc), 8 * fs)
    try:
        _warm(A, RESIDENT, fs)
        assert A.stats()["resident"] == 8
        for rnd in range(2):
            U = len(content)
            if rnd == 0:
                writes, append = _mixed_writes(rng, fs, U)[0], _data(rng, 2 * fs + 77)
            else:
                writes, append = _random_writes(rng, U, fs), _data(rng, fs // 4)
            cap = _cap(zra, len(arc), U, fs, len(append))
            resident = A.stats()["resident"]                                   # round 1: whatever the 300 queries of round 0 left
            st_e, out_e, size_e = _engine_update(gpu_engine, d_arc, len(arc), writes, append, cap)
            assert st_e == (0, 0)
            st, d_out, size = _handle_update(A, writes, append, cap)
            assert st == (0, 0), (fs, rnd, st)
            out = d_out.cpu().numpy().tobytes()
            content = _patched(content, writes, append)
            assert size == size_e and out[:size] == out_e[:size], (fs, rnd)
            assert out[:size] == _compress(gpu_engine, zra, content, fs), (fs, rnd)      # header, table and CRC-32 included
            assert out[size:] == bytes([SENT]) * (len(out) - size)
            assert (A.d_archive, A.size) == (d_out.data_ptr(), size)
            U = len(content)
            s = A.stats()
            assert (s["uncompressed_size"], s["resident"]) == (U, resident)
            qs = _queries(rng, U, fs, 300)
            got = _read(A, qs)
            assert got == _want(content, qs), (fs, rnd)
            with zra.Archive(gpu_engine, d_out.data_ptr(), size, 8 * fs) as fresh:
                assert got == _read(fresh, qs), (fs, rnd)
            arc, d_arc = out[:size], d_out[:size]                               # (round 1 stages frames that round 0 refreshed)
    finally:
        A.close()


# ---- 2
def test_the_cache_survives(zra, gpu_engine):
    rng = np.random.RandomState(2)
    fs = 4096
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    arc = _compress(gpu_engine, zra, content, fs)
    d_arc = _dev(arc)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), len(arc), 8 * fs) as A:
        _warm(A, RESIDENT, fs)
        before = A.stats()
        assert before["resident"] == 8
        writes, part, whole = _mixed_writes(rng, fs, n)
        append = _data(rng, fs + 9)
        st, d_out, size = _handle_update(A, writes, append, _cap(zra, len(arc), n, fs, len(append)))
        assert st == (0, 0)
        new = _patched(content, writes, append)
        s1 = A.stats()
        assert s1["resident"] == 8 and _delta(s1, before) == (0, 0, 0, 0)
        # every frame resident before, the touched ones included (2, 6, 14, 20 partly, 9 whole, 39 grown by the append): hits only,
        # nothing decoded, the new bytes in the touched ones
        qs = _frame_queries(RESIDENT, fs, len(new))
        got = _read(A, qs)
        s2 = A.stats()
        assert _delta(s2, s1) == (1, 8, 0, 0), (s1, s2)
        assert gpu_engine.kernel_stats()["dec_launches"] == 0 and gpu_engine.decode_stage_stats()["small_launches"] == 0
        assert got == _want(new, qs)
        for f, (g, q) in zip(RESIDENT, zip(got, qs)):
            assert (g != content[q[0]:q[0] + q[1]]) == (f in part or f in whole), f
        # a touched frame that was not resident is a miss (7, 11: partly written; 23: replaced whole; 40: appended)
        qs = _frame_queries((7, 11, 23, 40), fs, len(new))
        assert _read(A, qs) == _want(new, qs)
        assert _delta(A.stats(), s2) == (1, 0, 4, 4)


# ---- 3
def test_counters(zra, gpu_engine):
    rng = np.random.RandomState(3)
    fs = 4096
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    arc = _compress(gpu_engine, zra, content, fs)
    d_arc = _dev(arc)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), len(arc), 8 * fs) as A:
        assert A.update_stats() == dict(updates=0, frames=40, archive_bytes=len(arc), staged=0, refreshed=0, staged_total=0, refreshed_total=0)
        _warm(A, RESIDENT, fs)
        before = A.stats()
        # K = 3 resident frames partly written (2, 5, 14), M = 2 non-resident partly written (3, 30), W = 2 resident written whole (9, 20)
        # and one non-resident written whole (33)
        w1 = [(2 * fs + 9, _rand(rng, 50)), (5 * fs, _rand(rng, fs - 1)), (14 * fs + 100, _rand(rng, 1)), (3 * fs + 1, _rand(rng, 7)),
              (30 * fs + fs - 8, _rand(rng, 8)), (9 * fs, _rand(rng, fs)), (20 * fs, _rand(rng, fs)), (33 * fs, _rand(rng, fs))]
        st, d1, size1 = _handle_update(A, w1, b"", _cap(zra, len(arc), n, fs, 0))
        assert st == (0, 0)
        e = gpu_engine.update_stats()
        assert (e["frames"], e["touched"], e["decoded"], e["compressed"], e["passes"]) == (40, 8, 2, 8, 1), e
        u = A.update_stats()
        assert u == dict(updates=1, frames=40, archive_bytes=size1, staged=3, refreshed=5, staged_total=3, refreshed_total=5), u
        assert _delta(A.stats(), before) == (0, 0, 0, 0) and A.stats()["resident"] == 8
        # second update, into another buffer: K = 1 (27), M = 1 (0), W = 0, and an append of two frames and a bit behind resident 39
        w2 = [(27 * fs + 5, _rand(rng, 5)), (0, _rand(rng, 3))]
        app = _data(rng, 2 * fs + 10)
        st, d2, size2 = _handle_update(A, w2, app, _cap(zra, size1, n, fs, len(app)))
        assert st == (0, 0)
        e = gpu_engine.update_stats()
        assert (e["frames"], e["touched"], e["decoded"], e["compressed"]) == (42, 5, 1, 5), e     # 0, 27, 39 .. 41; 27 and 39 from the cache
        u = A.update_stats()
        assert u == dict(updates=2, frames=42, archive_bytes=size2, staged=2, refreshed=2, staged_total=5, refreshed_total=7), u
        assert _delta(A.stats(), before) == (0, 0, 0, 0) and A.stats()["resident"] == 8
        new = _patched(_patched(content, w1), w2, app)
        assert d2[:size2].cpu().numpy().tobytes() == _compress(gpu_engine, zra, new, fs)
        # an update that touches nothing is accepted and counted
        st, d3, size3 = _handle_update(A, [], b"", size2 + 64, d_out=d1)
        assert st == (0, 0) and size3 == size2
        u = A.update_stats()
        assert u == dict(updates=3, frames=42, archive_bytes=size2, staged=0, refreshed=0, staged_total=5, refreshed_total=7), u


# ---- 4
@pytest.mark.parametrize("app_n,frames_after", [(3 * 4096, 43), (1000, 40)])
def test_append_behind_a_resident_short_last_frame(zra, gpu_engine, app_n, frames_after):
    """The old last frame (39) holds fs / 2 bytes and is resident. The append fills it and adds frames, or ends inside it."""
    rng = np.random.RandomState(4)
    fs = 4096
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    arc = _compress(gpu_engine, zra, content, fs)
    d_arc = _dev(arc)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), len(arc), 8 * fs) as A:
        assert _read(A, [(39 * fs, fs // 2 - 1)]) == [content[39 * fs:n - 1]]
        with pytest.raises(zra.ZraError) as e:
            _read(A, [(39 * fs, fs // 2)])                                     # the reference's ">=" at U
        assert (e.value.zra, e.value.zstd) == (5, 0)
        s0 = A.stats()
        assert s0["resident"] == 1
        app = _data(rng, app_n)
        st, d_out, size = _handle_update(A, [], app, _cap(zra, len(arc), n, fs, app_n))
        assert st == (0, 0)
        new = content + app
        U2 = len(new)
        assert d_out[:size].cpu().numpy().tobytes() == _compress(gpu_engine, zra, new, fs)
        u = A.update_stats()
        assert (u["frames"], u["archive_bytes"], u["staged"], u["refreshed"]) == (frames_after, size, 1, 1), u
        assert gpu_engine.update_stats()["decoded"] == 0
        s1 = A.stats()
        assert (s1["uncompressed_size"], s1["resident"]) == (U2, 1) and _delta(s1, s0) == (0, 0, 0, 0)
        # the grown frame 39 is a hit with its new length
        q = (39 * fs, min(fs, U2 - 1 - 39 * fs))
        assert _read(A, [q]) == _want(new, [q])
        assert _delta(A.stats(), s1) == (1, 1, 0, 0)
        assert gpu_engine.kernel_stats()["dec_launches"] == 0
        # across the old end, and the bound at U'
        q = (n - 300, min(300 + app_n, U2 - 1 - (n - 300)))
        assert _read(A, [q]) == _want(new, [q])
        assert _read(A, [(U2 - 11, 10)]) == [new[U2 - 11:U2 - 1]]
        with pytest.raises(zra.ZraError) as e:
            _read(A, [(U2 - 10, 10)])
        assert (e.value.zra, e.value.zstd) == (5, 0)
        with zra.Archive(gpu_engine, d_out.data_ptr(), size, 8 * fs) as fresh:
            qs = _frame_queries(range(38, frames_after), fs, U2)
            assert _read(A, qs) == _read(fresh, qs) == _want(new, qs)


# ---- 5
def test_refusals_change_nothing(zra, gpu_engine):
    import torch
    L = zra.load()
    rng = np.random.RandomState(5)
    fs = 4096
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    good = _compress(gpu_engine, zra, content, fs)
    hs = int.from_bytes(good[4:8], "little") + 8
    ent = [int.from_bytes(good[38 + 5 * i:43 + 5 * i], "little") for i in range(41)]
    bad = bytearray(good)
    for k in (7, 31):                                                          # 7 will be written partly, 31 never: both not resident
        bad[hs + (ent[k] + ent[k + 1]) // 2] ^= 0x10
    bad = bytes(bad)
    d_arc = torch.full((len(bad) + 4096,), SENT, dtype=torch.uint8, device="cuda:0")
    d_arc[:len(bad)] = _dev(bad)

    def batch_status(d, size, off):
        """tests/test_gpu_update.py::test_damaged_frames: the batch call's status for a query inside the frame, whole frames verified"""
        d_o = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        L.ZraHipSetOptions(8)
        try:
            gpu_engine.decompress_ra_batch(d, size, d_o.data_ptr(), [off], [8], [0])
            return (0, 0)
        except zra.ZraError as x:
            return (x.zra, x.zstd)
        finally:
            L.ZraHipSetOptions(0)

    want7 = batch_status(d_arc.data_ptr(), len(bad), 7 * fs + 100)
    assert want7[0] == 1 and want7[1] != 0
    with zra.Archive(gpu_engine, d_arc.data_ptr(), len(bad), 8 * fs) as A:
        _warm(A, RESIDENT, fs)
        cap = _cap(zra, len(bad), n, fs, 0)
        ok_w = [(2 * fs + 5, _rand(rng, 40)), (12 * fs + 1, _rand(rng, 9))]
        st, _, need = _engine_update(gpu_engine, d_arc, len(bad), ok_w, b"", cap)
        assert st == (0, 0)
        s0, u0 = A.stats(), A.update_stats()
        cases = {
            "out of bounds": (dict(writes=[(n - 9, b"\x01" * 10)]), (5, 0)),
            "two writes share a byte": (dict(writes=[(2 * fs, b"\x01" * 10), (5000, b"\x03" * 10), (2 * fs + 9, b"\x02" * 10)]), (1, 42)),
            "one byte short": (dict(writes=ok_w, cap=need - 1), (6, 0)),
            "damaged touched frame": (dict(writes=[(2 * fs + 5, b"\x01" * 40), (7 * fs + 100, b"\x02" * 50)]), want7),
        }
        for name, (kw, want) in cases.items():
            c = kw.get("cap", cap)
            st, d_out, size = _handle_update(A, kw["writes"], b"", c)
            assert st == want, (name, st, want)
            if name == "one byte short":
                assert size == need
            assert d_out.cpu().numpy().tobytes() == bytes([SENT]) * (c + 16), name
            assert (A.stats(), A.update_stats()) == (s0, u0), name
            assert (A.d_archive, A.size) == (d_arc.data_ptr(), len(bad)), name
            qs = _frame_queries(RESIDENT, fs, n)
            assert _read(A, qs) == _want(content, qs), name                    # the old content, 2 * fs + 5 included
            assert _delta(A.stats(), s0) == (1, 8, 0, 0), name                 # with the old hits
            s0 = A.stats()
        # dOut overlapping the archive the handle is bound to
        before = d_arc.cpu().numpy().tobytes()
        osz = ctypes.c_size_t(0x1234)
        for d_o, c in ((d_arc.data_ptr() + len(bad) - 1, 4096), (d_arc.data_ptr(), len(bad)), (d_arc.data_ptr() + 10, 5)):
            st = L.ZraHipArchiveUpdate(A.h, None, None, None, None, 0, None, 0, d_o, c, ctypes.byref(osz), 3, True)
            assert st.tup() == (1, 42) and osz.value == 0x1234
        assert d_arc.cpu().numpy().tobytes() == before
        assert (A.stats(), A.update_stats()) == (s0, u0)
        # NULL arguments behind a real handle
        for args in ((None, None, None, None, 0, None, 0, None, cap, ctypes.byref(osz)),
                     (None, None, None, None, 0, None, 0, d_arc.data_ptr() + len(bad), 4096, None),
                     (None, None, None, None, 0, None, 7, d_arc.data_ptr() + len(bad), 4096, ctypes.byref(osz))):
            assert L.ZraHipArchiveUpdate(A.h, *args, 3, True).tup() == (1, 42)
        assert osz.value == 0x1234 and (A.stats(), A.update_stats()) == (s0, u0)
        # a damaged UNTOUCHED frame (7 and 31 now) is carried: reading it afterwards fails exactly as through a fresh handle
        st, d_out, size = _handle_update(A, ok_w, b"", cap)
        assert st == (0, 0) and size == need
        new = _patched(content, ok_w)
        with zra.Archive(gpu_engine, d_out.data_ptr(), size, 8 * fs) as fresh:
            for f in (7, 31):
                got = []
                for h in (A, fresh):
                    with pytest.raises(zra.ZraError) as e:
                        _read(h, [(f * fs + 3, 20)])
                    got.append((e.value.zra, e.value.zstd))
                assert got[0] == got[1] == batch_status(d_out.data_ptr(), size, f * fs + 3), (f, got)
            qs = _frame_queries((2, 12, 30), fs, n)
            assert _read(A, qs) == _read(fresh, qs) == _want(new, qs)


# ---- 6
def test_handle_without_slots(zra, gpu_engine):
    import torch
    rng = np.random.RandomState(6)
    fs = 4096
    n = 40 * fs - fs // 2
    content = _data(rng, n)
    arc = _compress(gpu_engine, zra, content, fs)
    d_arc = _dev(arc)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), len(arc), 0) as A:
        writes, _, _ = _mixed_writes(rng, fs, n)
        append = _data(rng, fs + 100)
        cap = _cap(zra, len(arc), n, fs, len(append))
        st_e, out_e, size_e = _engine_update(gpu_engine, d_arc, len(arc), writes, append, cap)
        st, d_out, size = _handle_update(A, writes, append, cap)
        assert st == st_e == (0, 0) and size == size_e and d_out.cpu().numpy().tobytes() == out_e
        u = A.update_stats()
        assert (u["updates"], u["frames"], u["archive_bytes"], u["staged"], u["refreshed"]) == (1, 41, size, 0, 0)
        s = A.stats()
        assert (s["slots"], s["resident"], s["uncompressed_size"]) == (0, 0, n + len(append))
        new = _patched(content, writes, append)
        qs = _queries(rng, len(new), fs, 100)
        offs, sizes = [q[0] for q in qs], [q[1] for q in qs]
        oofs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
        d_ref = torch.empty(int(sum(sizes)), dtype=torch.uint8, device="cuda:0")
        gpu_engine.decompress_ra_batch(d_out.data_ptr(), size, d_ref.data_ptr(), offs, sizes, oofs)
        ref = d_ref.cpu().numpy().tobytes()
        assert b"".join(_read(A, qs)) == ref == b"".join(_want(new, qs))


# ---- 7
def test_ping_pong_between_two_buffers(zra, gpu_engine):
    import torch
    rng = np.random.RandomState(7)
    fs = 10000
    n = 30 * fs + 3
    model = _data(rng, n)
    arc = _compress(gpu_engine, zra, model, fs)
    cap = _cap(zra, len(arc), n + 4 * (fs + 50), fs, 0)
    bufs = [torch.full((cap + 16,), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    bufs[0][:len(arc)] = _dev(arc)
    size = len(arc)
    with zra.Archive(gpu_engine, bufs[0].data_ptr(), size, 12 * fs) as A:
        for r in range(4):
            # the last frame and up to 10 others are resident, the rest is not: the write that ends at the last byte stages from the cache
            _read(A, [(len(model) - 50, 1)] + [(int(o), 1) for o in rng.randint(0, len(model) - 200, size=10)])
            writes = [w for w in _random_writes(rng, len(model), fs) if r % 2 == 0 or len(w[1]) < 3 * fs]
            append = _data(rng, fs + 50) if r != 2 else b""
            st, d_out, size = _handle_update(A, writes, append, cap, d_out=bufs[(r + 1) % 2])
            assert st == (0, 0), (r, st)
            model = _patched(model, writes, append)
            U = len(model)
            whole = [(o, min(8 * fs, U - 1 - o)) for o in range(0, U - 1, 8 * fs)]
            assert b"".join(_read(A, whole)) == model[:U - 1], r
            assert A.stats()["resident"] <= 12
        u = A.update_stats()
        assert (u["updates"], u["frames"], u["archive_bytes"]) == (4, (len(model) + fs - 1) // fs, size)
        assert u["refreshed_total"] >= u["staged_total"] >= 4
        assert bufs[0][:size].cpu().numpy().tobytes() == _compress(gpu_engine, zra, model, fs)
        assert gpu_engine.verify(bufs[0].data_ptr(), size, content=True) == (0, [])


# ---- 8
def test_several_passes_stage_from_the_cache(zra, gpu_engine):
    """The shape of tests/test_gpu_update.py::test_many_touched_frames_go_through_several_passes, with 256 resident frames at either end
    of the archive: both passes take frames from the cache."""
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
    d_new = torch.randint(0, 256, (nfr * 16,), dtype=torch.uint8, device="cuda:0", generator=g)
    writes = (np.arange(nfr, dtype=np.uint64) * fs + 1000, np.full(nfr, 16, dtype=np.uint64), np.arange(nfr, dtype=np.uint64) * 16)
    d_ref = torch.full((cap,), SENT, dtype=torch.uint8, device="cuda:0")
    rsz = gpu_engine.update(d_arc.data_ptr(), asz, d_ref.data_ptr(), cap, writes=writes, d_data=d_new.data_ptr())
    hot = list(range(256)) + list(range(nfr - 256, nfr))
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, 512 * fs) as A:
        _warm(A, hot, fs)
        s0 = A.stats()
        assert s0["resident"] == 512
        d_out = torch.full((cap,), SENT, dtype=torch.uint8, device="cuda:0")
        size = A.update(d_out.data_ptr(), cap, writes=writes, d_data=d_new.data_ptr())
        e, u = gpu_engine.update_stats(), A.update_stats()
        assert e["passes"] >= 2 and (e["touched"], e["decoded"], e["compressed"]) == (nfr, nfr - 512, nfr), e
        assert (u["staged"], u["refreshed"], u["frames"], u["archive_bytes"]) == (512, 512, nfr, size), u
        assert size == rsz and torch.equal(d_out, d_ref)                       # the sentinel tail included
        d_data.view(nfr, fs)[:, 1000:1016] = d_new.view(nfr, 16)
        d_got = torch.empty(512 * 64, dtype=torch.uint8, device="cuda:0")
        A.read(d_got.data_ptr(), [f * fs + 984 for f in hot], [64] * 512, [64 * i for i in range(512)])
        s1 = A.stats()
        assert _delta(s1, s0) == (1, 512, 0, 0) and gpu_engine.kernel_stats()["dec_launches"] == 0
        assert torch.equal(d_got.view(512, 64), d_data.view(nfr, fs)[hot, 984:1048])


# ---- 9
def test_two_handles_on_one_engine(zra, gpu_engine):
    rng = np.random.RandomState(9)
    fs = 4096
    n = 40 * fs - fs // 2
    contents = [_data(rng, n) for _ in range(2)]
    arcs = [_compress(gpu_engine, zra, c, fs) for c in contents]
    d_arcs = [_dev(a) for a in arcs]
    A, B = (zra.Archive(gpu_engine, d.data_ptr(), len(a), 8 * fs) for d, a in zip(d_arcs, arcs))
    with A, B:
        _warm(A, RESIDENT, fs)
        _warm(B, RESIDENT, fs)
        sB, uB = B.stats(), B.update_stats()
        writes, _, _ = _mixed_writes(rng, fs, n)
        st, d_out, size = _handle_update(A, writes, _data(rng, 100), _cap(zra, len(arcs[0]), n, fs, 100))
        assert st == (0, 0)
        assert (B.stats(), B.update_stats()) == (sB, uB)
        assert d_arcs[1].cpu().numpy().tobytes() == arcs[1]
        qs = _frame_queries(RESIDENT, fs, n)
        assert _read(B, qs) == _want(contents[1], qs)
        assert _delta(B.stats(), sB) == (1, 8, 0, 0)                           # B's residency is its own
        assert gpu_engine.kernel_stats()["dec_launches"] == 0
