"""GPU tests of the archive handle (include/zra_hip.h: ZraHipArchive*): a device-resident archive opened once, whole decoded frames
kept in a CLOCK-managed HBM arena. Answers are compared with the source and byte for byte with ZraHipDecompressRABatch (bytes outside
the answers included), statuses with ZraHipDecompressRABatch under ZRA_HIP_OPT_RA_WHOLE_FRAMES, counters with what Python computes."""
import ctypes

import numpy as np
import pytest

import corpus as C
import oracle_lib as O

pytestmark = pytest.mark.gpu
SENT = 0xEE


def _data(rng, n):
    """Compressible bytes: a small alphabet with copied runs (literals and matches for the decoder)."""
    a = rng.randint(0, 24, size=n).astype(np.uint8)
    for _ in range(n // 4096):
        src, ln = int(rng.randint(0, max(1, n - 600))), int(rng.randint(16, 512))
        dst = int(rng.randint(0, max(1, n - ln)))
        a[dst:dst + ln] = a[src:src + ln]
    return a.tobytes()


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to("cuda:0")


def _compress(eng, zra, data, fs):
    import torch
    d_in = _dev(data)
    d_arc = torch.empty(zra.GetOutputBufferSize(len(data), fs) + 64, dtype=torch.uint8, device="cuda:0")
    asz = eng.compress(d_in.data_ptr(), len(data), d_arc.data_ptr(), 3, fs, True)
    return d_arc, asz


def _layout(sizes, gap=3):
    """Answer offsets with `gap` untouched bytes between answers, and the buffer length (a sentinel tail included)."""
    oofs, at = [], gap
    for s in sizes:
        oofs.append(at); at += int(s) + gap
    return np.array(oofs, dtype=np.uint64), at + 16


def _expected(data, offs, sizes, oofs, n):
    e = bytearray([SENT]) * n
    for o, s, oo in zip(offs, sizes, oofs):
        e[int(oo):int(oo) + int(s)] = data[int(o):int(o) + int(s)]
    return bytes(e)


def _run(fn, d_out, offs, sizes, oofs):
    """(status, output bytes) of fn(d_out, offs, sizes, oofs) on an output pre-filled with the sentinel."""
    d_out.fill_(SENT)
    try:
        fn(d_out.data_ptr(), offs, sizes, oofs)
        st = (0, 0)
    except Exception as e:
        st = (e.zra, e.zstd)
    return st, d_out.cpu().numpy().tobytes()


def _distinct(offs, sizes, fs):
    f = set()
    for o, s in zip(offs, sizes):
        if s:
            f.update(range(int(o) // fs, (int(o) + int(s) - 1) // fs + 1))
    return len(f)


def _mix(rng, n, fs, nq):
    sizes = rng.choice([0, 1, 2, 100, fs - 1, fs, fs + 1, 3 * fs + 5], size=nq).astype(np.int64)
    sizes = np.minimum(sizes, n - 2)
    offs = np.array([rng.randint(0, n - int(s) - 1) for s in sizes], dtype=np.int64)
    k = nq // 10
    offs[:k] = offs[k:2 * k]; sizes[:k] = sizes[k:2 * k]                       # exact duplicates
    offs[2 * k:3 * k] = np.minimum(offs[3 * k:4 * k] + 7, n - sizes[2 * k:3 * k] - 1)   # overlaps
    return offs.astype(np.uint64), sizes.astype(np.uint64)


@pytest.mark.parametrize("fs", [4096, 65536, 10000])
def test_random_mixes_match_source_and_batch(zra, gpu_engine, fs):
    import torch
    rng = np.random.RandomState(fs)
    nfr = max(24, (3 << 20) // fs)
    n = nfr * fs - (fs // 3 if fs == 10000 else 0)                            # 10000: not a power of two, short last frame
    data = _data(rng, n)
    d_arc, asz = _compress(gpu_engine, zra, data, fs)
    frames = (n + fs - 1) // fs
    offs, sizes = _mix(rng, n, fs, 400)
    oofs, total = _layout(sizes)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    want = _expected(data, offs, sizes, oofs, total)
    st, ref = _run(lambda *a: gpu_engine.decompress_ra_batch(d_arc.data_ptr(), asz, *a), d_out, offs, sizes, oofs)
    assert st == (0, 0) and ref == want
    dist = _distinct(offs, sizes, fs)
    for slots in (0, 1, 7, frames):
        with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, slots * fs) as A:
            s0 = A.stats()
            assert (s0["slots"], s0["frame_size"], s0["uncompressed_size"]) == (slots, fs, n)
            for rep in range(2):
                st, got = _run(A.read, d_out, offs, sizes, oofs)
                assert st == (0, 0), (fs, slots, rep, st)
                assert got == ref, (fs, slots, rep)                          # answers, gaps and sentinel tail
            s = A.stats()
            assert s["reads"] == 2 and s["hits"] + s["misses"] == 2 * dist, (fs, slots, s)
            assert s["resident"] <= slots
            if slots == frames:
                # repeat read: every frame resident, nothing decoded
                before = A.stats()
                st, got = _run(A.read, d_out, offs, sizes, oofs)
                after = A.stats()
                assert st == (0, 0) and got == ref
                assert after["misses"] == before["misses"] and after["hits"] - before["hits"] == dist
                assert gpu_engine.kernel_stats()["dec_launches"] == 0
                assert gpu_engine.decode_stage_stats()["small_launches"] == 0


def test_counting_across_reads(zra, gpu_engine):
    import torch
    rng = np.random.RandomState(11)
    fs = 4096
    n = 600 * fs + 123
    data = _data(rng, n)
    d_arc, asz = _compress(gpu_engine, zra, data, fs)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, 40 * fs) as A:
        prev = A.stats()
        for r in range(6):
            offs, sizes = _mix(rng, n // (3 if r % 2 else 1), fs, 60)        # odd reads stay in the first third: some frames come back
            oofs, total = _layout(sizes)
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            st, got = _run(A.read, d_out, offs, sizes, oofs)
            assert st == (0, 0) and got == _expected(data, offs, sizes, oofs, total)
            s = A.stats()
            assert s["reads"] - prev["reads"] == 1
            assert (s["hits"] - prev["hits"]) + (s["misses"] - prev["misses"]) == _distinct(offs, sizes, fs), (r, s, prev)
            assert s["resident"] <= 40
            prev = s


def test_clock_keeps_the_hot_frame(zra, gpu_engine):
    """S = 64 slots, every read = hot frame H + K = 16 frames never touched before: H is a hit on every read after the first (FIFO or
    random replacement would evict it)."""
    import torch
    fs, S, K, R = 4096, 64, 16, 20
    rng = np.random.RandomState(5)
    n = (1 + K * R + 2) * fs
    data = _data(rng, n)
    d_arc, asz = _compress(gpu_engine, zra, data, fs)
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, S * fs) as A:
        prev = A.stats()
        for r in range(R):
            frames = [0] + [1 + r * K + k for k in range(K)]
            offs = np.array([f * fs + 17 for f in frames], dtype=np.uint64)
            sizes = np.full(len(frames), 100, dtype=np.uint64)
            oofs, total = _layout(sizes)
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            st, got = _run(A.read, d_out, offs, sizes, oofs)
            assert st == (0, 0) and got == _expected(data, offs, sizes, oofs, total)
            s = A.stats()
            hits, misses = s["hits"] - prev["hits"], s["misses"] - prev["misses"]
            assert (hits, misses) == ((0, K + 1) if r == 0 else (1, K)), (r, hits, misses)
            assert s["resident"] <= S
            prev = s
        assert A.stats()["evictions"] > 0


def test_overflow_read_decodes_in_passes(zra, gpu_engine):
    import torch
    fs, S = 4096, 16
    rng = np.random.RandomState(6)
    n = 200 * fs + 55
    data = _data(rng, n)
    d_arc, asz = _compress(gpu_engine, zra, data, fs)
    frames = rng.choice(199, size=3 * S, replace=False)
    offs = np.array([int(f) * fs + int(rng.randint(0, fs // 2)) for f in frames], dtype=np.uint64)
    sizes = np.array([int(rng.choice([1, 100, fs // 2, fs + 9])) for _ in frames], dtype=np.uint64)
    oofs, total = _layout(sizes)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, S * fs) as A:
        for rep in range(2):
            st, got = _run(A.read, d_out, offs, sizes, oofs)
            assert st == (0, 0) and got == _expected(data, offs, sizes, oofs, total), rep
        s = A.stats()
        assert s["resident"] <= S and s["evictions"] > 0 and s["hits"] + s["misses"] == 2 * _distinct(offs, sizes, fs), s


def _opts(zra, v):
    zra.load().ZraHipSetOptions(v)


@pytest.mark.parametrize("seed", range(2))
def test_damaged_archives_and_option_independence(zra, gpu_engine, seed):
    """Statuses on damaged frames: a handle with slots answers like the batch call with whole frames, whatever the process-wide
    option; a handle without slots follows the option like the batch call. After a failing read intact frames still read right, and the
    failing range fails again, decoded again (counted as misses)."""
    import torch
    checked = 0
    try:
        for case, a in C.mutated_archives(40000 + seed, 30, O.zra_compress):
            if not C.seek_table_consistent(a):
                continue
            U = int.from_bytes(a[18:26], "little"); fs = int.from_bytes(a[30:34], "little")
            if U < 2:
                continue
            frames = (U + fs - 1) // fs
            d_arc = _dev(a)
            rng = np.random.RandomState(seed * 1000 + case)
            qs = []
            for _ in range(3):
                off = int(rng.randint(0, U - 1))
                qs.append((off, max(1, min(int(rng.choice([1, 100, fs, 2 * fs + 3, U - off - 1])), U - off - 1))))
            qs.append((0, U - 1))
            d_out = torch.empty(U + 64, dtype=torch.uint8, device="cuda:0")
            batch = lambda *x: gpu_engine.decompress_ra_batch(d_arc.data_ptr(), len(a), *x)
            per_frame_ok = []
            for f in range(frames):
                o = f * fs; sz = min(fs, U - 1 - o)
                _opts(zra, 8)
                per_frame_ok.append(sz <= 0 or _run(batch, d_out, [o], [sz], [0])[0] == (0, 0))
                _opts(zra, 0)
            try:
                A, A0 = zra.Archive(gpu_engine, d_arc.data_ptr(), len(a), frames * fs), zra.Archive(gpu_engine, d_arc.data_ptr(), len(a), 0)
            except zra.ZraError as e:                                          # a header status: the batch call's
                _opts(zra, 8)
                assert (e.zra, e.zstd) == _run(batch, d_out, [0], [1], [0])[0], (seed, case)
                _opts(zra, 0)
                continue
            with A, A0:
                for off, sz in qs:
                    q = ([off], [sz], [0])
                    _opts(zra, 8)
                    want8 = _run(batch, d_out, *q)
                    _opts(zra, 0)
                    want0 = _run(batch, d_out, *q)
                    for opt, want in ((0, want0), (8, want8)):
                        _opts(zra, opt)
                        before = A.stats()
                        got = _run(A.read, d_out, *q)
                        assert got[0] == want8[0], (seed, case, opt, off, sz, got[0], want8[0])
                        if got[0] == (0, 0):
                            assert got[1] == want8[1]
                        else:
                            # fails again, decoded again: every frame of the range is a hit or a miss, the failing ones misses
                            again = _run(A.read, d_out, *q)
                            after = A.stats()
                            assert again[0] == got[0]
                            assert after["misses"] - before["misses"] >= 2
                            assert (after["hits"] - before["hits"]) + (after["misses"] - before["misses"]) == 2 * _distinct([off], [sz], fs)
                        got0 = _run(A0.read, d_out, *q)
                        assert got0[0] == want[0], (seed, case, opt, off, sz, got0[0], want[0])
                        if want[0] == (0, 0):
                            assert got0[1] == want[1]
                        _opts(zra, 0)
                        checked += 1
                # intact frames still read right after the failures
                for f in range(frames):
                    o = f * fs; sz = min(fs, U - 1 - o)
                    if sz > 0 and per_frame_ok[f]:
                        st, got = _run(A.read, d_out, [o], [sz], [0])
                        _opts(zra, 8)
                        st8, ref = _run(batch, d_out, [o], [sz], [0])
                        _opts(zra, 0)
                        assert st == st8 == (0, 0) and got == ref, (seed, case, f)
                assert A.stats()["resident"] <= frames
    finally:
        _opts(zra, 0)
    assert checked > 0


def test_open_errors_bounds_and_drop(zra, gpu_engine):
    import torch
    L = zra.load()
    h = ctypes.c_void_p()

    def open_status(d, size):
        st = L.ZraHipArchiveOpen(gpu_engine.h, d, size, 1 << 20, ctypes.byref(h)).tup()
        if st == (0, 0):
            L.ZraHipArchiveClose(h)
        return st

    def batch_status(d, size):
        d_out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        try:
            gpu_engine.decompress_ra_batch(d, size, d_out.data_ptr(), [], [], [])   # no query: the header checks alone
            return (0, 0)
        except zra.ZraError as e:
            return (e.zra, e.zstd)

    n_cmp = 0
    for case, a, _, _, _ in C.mutated_headers(321, 40, O.zra_compress):
        d = _dev(a)
        sb = batch_status(d.data_ptr(), len(a))
        so = open_status(d.data_ptr(), len(a))
        assert so == sb, (case, so, sb)
        n_cmp += sb != (0, 0)
    assert n_cmp > 0
    rng = np.random.RandomState(9)
    fs = 4096
    n = 40 * fs + 5
    data = _data(rng, n)
    d_arc, asz = _compress(gpu_engine, zra, data, fs)
    hs = int.from_bytes(d_arc[:8].cpu().numpy().tobytes()[4:8], "little") + 8
    for size in (0, 10, 38, hs - 1):
        assert open_status(d_arc.data_ptr(), size) == batch_status(d_arc.data_ptr(), size) == (5, 0), size
    assert L.ZraHipArchiveOpen(gpu_engine.h, None, 100, 0, ctypes.byref(h)).tup() == (1, 42)
    d_out = torch.empty(3 * fs, dtype=torch.uint8, device="cuda:0")
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, 8 * fs) as A:
        offs, sizes = [5, 3 * fs], [2 * fs, 10]
        A.read(d_out.data_ptr(), offs, sizes, [0, 2 * fs])
        s1 = A.stats()
        assert (s1["reads"], s1["hits"], s1["misses"], s1["resident"]) == (1, 0, 4, 4)
        with pytest.raises(zra.ZraError) as e:
            A.read(d_out.data_ptr(), [0, n - 10], [1, 10], [0, 1])                # offset + size == uncompressedSize: refused
        assert (e.value.zra, e.value.zstd) == (5, 0)
        assert A.stats() == s1
        A.read(d_out.data_ptr(), offs, sizes, [0, 2 * fs])
        s2 = A.stats()
        assert (s2["hits"] - s1["hits"], s2["misses"] - s1["misses"]) == (4, 0)
        A.drop_cache()
        assert A.stats()["resident"] == 0
        A.read(d_out.data_ptr(), offs, sizes, [0, 2 * fs])
        s3 = A.stats()
        assert (s3["hits"] - s2["hits"], s3["misses"] - s2["misses"]) == (0, 4)
        assert d_out[: 2 * fs].cpu().numpy().tobytes() == data[5:5 + 2 * fs]


def test_two_handles_on_one_engine(zra, gpu_engine):
    import torch
    rng = np.random.RandomState(12)
    arcs = []
    for fs in (4096, 16384):
        n = 100 * fs + 77
        data = _data(rng, n)
        arcs.append((fs, n, data) + _compress(gpu_engine, zra, data, fs))
    hs = [zra.Archive(gpu_engine, d.data_ptr(), asz, 10 * fs) for fs, n, data, d, asz in arcs]
    try:
        for r in range(6):
            k = r % 2
            fs, n, data, _, _ = arcs[k]
            offs, sizes = _mix(rng, n, fs, 30)
            oofs, total = _layout(sizes)
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            st, got = _run(hs[k].read, d_out, offs, sizes, oofs)
            assert st == (0, 0) and got == _expected(data, offs, sizes, oofs, total), (r, k)
    finally:
        for A in hs:
            A.close()


def test_arena_memory_is_returned_and_refused_when_too_large(zra, gpu_engine):
    import torch
    # header-only archives are enough for open: it reads and checks the header, it decodes nothing
    fs = 65536
    hdr = zra.stitch_header([0] * 4096, 4096 * fs, fs)                          # 4096 frames of 64 KiB: a 256 MiB arena
    d_hdr = _dev(hdr)

    def lifetime():
        A = zra.Archive(gpu_engine, d_hdr.data_ptr(), len(hdr), 256 << 20)
        assert A.stats()["slots"] == 4096
        A.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    free1 = lifetime()
    free2 = lifetime()
    assert abs(free1 - free2) < (2 << 20), (free1, free2)
    big_fs = 0xFFFFFFF0
    huge = zra.stitch_header([0] * 100, 100 * big_fs, big_fs)                  # 100 slots of ~4 GiB: beyond any device
    d_huge = _dev(huge)
    L = zra.load()
    h = ctypes.c_void_p(0)
    assert L.ZraHipArchiveOpen(gpu_engine.h, d_huge.data_ptr(), len(huge), 1 << 62, ctypes.byref(h)).tup() == (1, 64)
    assert h.value in (None, 0)
    # the engine is still usable
    rng = np.random.RandomState(3)
    data = _data(rng, 20 * 4096 + 1)
    d_arc, asz = _compress(gpu_engine, zra, data, 4096)
    d_out = torch.empty(100, dtype=torch.uint8, device="cuda:0")
    with zra.Archive(gpu_engine, d_arc.data_ptr(), asz, 4 * 4096) as A:
        A.read(d_out.data_ptr(), [5000], [100], [0])
    assert d_out.cpu().numpy().tobytes() == data[5000:5100]
