"""GPU tests at the sizes BASELINE.json names (C3, the one-GPU shard of C4, the one-GPU share of C5; C1 and C2 live in
test_gpu_parity.py). At these sizes the oracle cannot be run over everything, so parity is checked through properties the domain offers
(round trip, idempotence, seek-table invariants + CRC-32, random access == slices of the input) plus byte parity with the oracle on a
prefix / on the reference's anchor archives. Everything goes through the C ABI (ctypes); torch only holds the device buffers."""
import hashlib
import json
import os
import threading
import zlib

import numpy as np
import pytest

import corpus as C
import oracle_lib as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GiB = 1 << 30


def _entries(head, n):
    e = np.frombuffer(head[38:38 + 5 * n], dtype=np.uint8).reshape(n, 5).astype(np.int64)
    return e[:, 0] | (e[:, 1] << 8) | (e[:, 2] << 16) | (e[:, 3] << 24) | (e[:, 4] << 32)


def _check_header(head, N, fs, arc_size):
    nent = (N + fs - 1) // fs + 1
    assert int.from_bytes(head[18:26], "little") == N and int.from_bytes(head[26:30], "little") == nent and int.from_bytes(head[30:34], "little") == fs
    ent = _entries(head, nent)
    assert ent[0] == 0 and np.all(np.diff(ent) > 0) and ent[-1] == arc_size - (38 + 5 * nent)
    assert int.from_bytes(head[14:18], "little") == zlib.crc32(head[18:38 + 5 * nent], zlib.crc32(head[:14]))     # CalculateHash, zra.cpp:128-133
    return ent


@pytest.fixture(autouse=True)
def _free_device_memory(gpu_engine):
    """these tests each fill a large part of the 288 GB: start from an empty torch cache and an engine without scratch, and leave it so"""
    import torch
    gpu_engine.release_scratch()
    torch.cuda.empty_cache()
    yield
    gpu_engine.release_scratch()
    torch.cuda.empty_cache()


def _all_queries_equal(torch, d_ra, d_in, offs, qb, chunk=1 << 16):
    """every answer of a fixed-size query batch against the resident input, on the device"""
    dev = d_in.device
    ar = torch.arange(qb, device=dev, dtype=torch.int64)
    for i in range(0, len(offs), chunk):
        o = torch.from_numpy(offs[i:i + chunk].astype(np.int64)).to(dev)
        want = d_in[(o[:, None] + ar[None, :]).reshape(-1)]
        got = d_ra[i * qb:(i + len(o)) * qb]
        if not torch.equal(want, got):
            return False
    return True


def test_config_c3_16gib_1m_random_access_queries(zra, gpu_engine):
    """BASELINE config C3 (the metric's configuration): 16 GiB corpus, frameSize 64 KiB, level 3, 1,000,000 random DecompressRA(offset, 4 KiB)
    queries on one MI355X. ALL one million answers are compared with the input on the device."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    fs, N, Q, qb = 65536, 16 * GiB, 1_000_000, 4096
    base = bench.synth_corpus(64 << 20, seed=1)
    d_in = torch.from_numpy(base).to(dev).repeat(N // len(base))[:N].contiguous()
    bound = zra.GetOutputBufferSize(N, fs)
    d_arc = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    n1 = gpu_engine.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
    nent = N // fs + 1
    head = d_arc[: 38 + 5 * nent].cpu().numpy().tobytes()
    ent = _check_header(head, N, fs, n1)
    # the corpus repeats every 64 MiB = 1024 frames: so do the frame sizes (frames are independent, zra.cpp:216-225)
    sz = np.diff(ent)
    assert np.array_equal(sz[:1024], sz[1024:2048]) and np.array_equal(sz[:1024], sz[-1024:])
    # byte parity with the oracle on all 1,024 distinct frames of the corpus (the rest of the archive repeats them: the size check above)
    nchk = 1024
    st, ref = O.zra_compress(base[: nchk * fs].tobytes(), 3, fs, True)
    refbody = ref[38 + 5 * (nchk + 1):]
    assert d_arc[len(head): len(head) + len(refbody)].cpu().numpy().tobytes() == refbody
    # idempotence
    d_arc2 = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    n2 = gpu_engine.compress(d_in.data_ptr(), N, d_arc2.data_ptr(), 3, fs, True)
    assert n1 == n2 and torch.equal(d_arc[:n1], d_arc2[:n2])
    del d_arc2
    # round trip of the whole archive
    d_out = torch.empty(N, dtype=torch.uint8, device=dev)
    gpu_engine.decompress(d_arc.data_ptr(), n1, d_out.data_ptr(), N)
    assert torch.equal(d_out, d_in)
    del d_out
    # 1 M queries of 4 KiB, offsets from a fixed seed, every answer checked
    rng = np.random.RandomState(42)
    offs = rng.randint(0, N - qb - 1, size=Q).astype(np.uint64)
    sizes = np.full(Q, qb, dtype=np.uint64)
    oo = np.arange(Q, dtype=np.uint64) * qb
    d_ra = torch.zeros(Q * qb + 64, dtype=torch.uint8, device=dev)
    gpu_engine.decompress_ra_batch(d_arc.data_ptr(), n1, d_ra.data_ptr(), offs, sizes, oo)
    assert _all_queries_equal(torch, d_ra, d_in, offs, qb)
    # small batches (per-slice jobs, nothing proportional to the archive's 262,144 frames): 1, 64 and 4096 queries
    for k in (1, 64, 4096):
        d_ra[: k * qb].zero_()
        gpu_engine.decompress_ra_batch(d_arc.data_ptr(), n1, d_ra.data_ptr(), offs[1000:1000 + k], sizes[:k], oo[:k])
        assert _all_queries_equal(torch, d_ra, d_in, offs[1000:1000 + k], qb)
    # whole-frame mode (reference error behaviour: every touched frame decoded in full, checksums verified) returns the same bytes
    zra.load().ZraHipSetOptions(8)
    try:
        d_ra.zero_()
        gpu_engine.decompress_ra_batch(d_arc.data_ptr(), n1, d_ra.data_ptr(), offs[:200000], sizes[:200000], oo[:200000])
        assert _all_queries_equal(torch, d_ra, d_in, offs[:200000], qb)
    finally:
        zra.load().ZraHipSetOptions(0)


def test_config_c4_shard_8gib_level9_256k(zra, gpu_engine):
    """BASELINE config C4, the share of one GPU: 64 GiB of log-like data over 8 GPUs = 8 GiB per GPU, frameSize 256 KiB, level 9 (lazy2,
    two blocks per frame). The shard goes through ZraHipCompressFrames (what a rank runs) and through the whole-archive call; the
    reference's three level-9 / 256 KiB anchor archives are reproduced by the HIP path itself."""
    import torch
    dev = torch.device("cuda", 0)
    fs, N = 262144, 8 * GiB
    # (1) the reference's anchors at L9 / 256 KiB: archive size + sha256 recorded from the reference
    anc = json.load(open(os.path.join(GOLD, "anchors.json")))
    ci = anc["configs"].index([9, 262144])
    gens = {"A": C.gen_A, "B": C.gen_B, "C": C.gen_C, "D": C.gen_D, "E": C.gen_E}
    for name in ("C", "D", "E"):
        arc = zra.CompressBuffer(gens[name](anc["n"]), 9, fs, True)
        size, sha = anc["archives"][name][ci]
        assert len(arc) == size and hashlib.sha256(arc).hexdigest()[:16] == sha, name
    # (2) the 8 GiB shard
    base = np.frombuffer(C.gen_loglike(32 << 20, seed=4), dtype=np.uint8)
    d_in = torch.from_numpy(base.copy()).to(dev).repeat(N // len(base))[:N].contiguous()
    bound = zra.GetOutputBufferSize(N, fs)
    d_arc = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    n1 = gpu_engine.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 9, fs, True)
    nent = N // fs + 1
    head = d_arc[: 38 + 5 * nent].cpu().numpy().tobytes()
    ent = _check_header(head, N, fs, n1)
    nchk = 12                                        # 3 MiB through the oracle's lazy2 (slow on the CPU)
    st, ref = O.zra_compress(base[: nchk * fs].tobytes(), 9, fs, True)
    assert st == (0, 0)
    refbody = ref[38 + 5 * (nchk + 1):]
    assert d_arc[len(head): len(head) + len(refbody)].cpu().numpy().tobytes() == refbody
    # the rank-side call of the sharded path gives the same frames: packed body + sizes
    d_body = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    d_sizes = torch.empty(N // fs, dtype=torch.int64, device=dev)
    blen = gpu_engine.compress_frames(d_in.data_ptr(), N, d_body.data_ptr(), d_sizes.data_ptr(), 9, fs, True)
    assert blen == n1 - len(head) and torch.equal(d_body[:blen], d_arc[len(head):n1])
    assert np.array_equal(d_sizes.cpu().numpy(), np.diff(ent))
    assert zra.stitch_header(d_sizes.cpu().numpy().astype(np.uint64), N, fs) == head      # the stitched header is the archive's
    del d_body
    # round trip
    d_out = torch.empty(N, dtype=torch.uint8, device=dev)
    gpu_engine.decompress(d_arc.data_ptr(), n1, d_out.data_ptr(), N)
    assert torch.equal(d_out, d_in)


def test_config_c5_share_32gib_resident_concurrent_streams(zra, gpu_engine):
    """BASELINE config C5, the share of one GPU: 256 GiB archive over 8 GPUs = 32 GiB of original data per GPU, archive resident in HBM,
    concurrent random-access streams: two engines on two host threads answer different query batches against the same resident archive
    at the same time; every answer is checked."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    fs, N, qb = 65536, 32 * GiB, 4096
    base = bench.synth_corpus(64 << 20, seed=3)
    d_in = torch.from_numpy(base).to(dev).repeat(N // len(base))[:N].contiguous()
    bound = zra.GetOutputBufferSize(N, fs)
    d_arc = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    n1 = gpu_engine.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
    gpu_engine.release_scratch()                      # the compressor's scratch is not needed while serving
    engines = [gpu_engine, zra.Engine(0)]
    Q = 200000
    res, errs = [None, None], []

    def stream(k):
        try:
            rng = np.random.RandomState(100 + k)
            for it in range(3):
                offs = rng.randint(0, N - qb - 1, size=Q).astype(np.uint64)
                sizes = np.full(Q, qb, dtype=np.uint64)
                oo = np.arange(Q, dtype=np.uint64) * qb
                d_ra = torch.zeros(Q * qb + 64, dtype=torch.uint8, device=dev)
                engines[k].decompress_ra_batch(d_arc.data_ptr(), n1, d_ra.data_ptr(), offs, sizes, oo)
                res[k] = (d_ra, offs)
        except Exception as e:               # noqa: BLE001 (reported below, on the main thread)
            errs.append((k, repr(e)))

    th = [threading.Thread(target=stream, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        d_ra, offs = res[k]
        assert _all_queries_equal(torch, d_ra, d_in, offs, qb), k
    # a mixed batch on the resident archive: sizes from 1 byte to 1 MiB, crossing frame boundaries
    rng = np.random.RandomState(7)
    q = 20000
    sizes = rng.choice([1, 100, 4096, 65536, 70000, 1 << 20], size=q, p=[0.2, 0.2, 0.3, 0.2, 0.09, 0.01]).astype(np.uint64)
    offs = (rng.randint(0, N - (1 << 20) - 2, size=q)).astype(np.uint64)
    oo = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    d_ra = torch.zeros(int(sizes.sum()) + 64, dtype=torch.uint8, device=dev)
    engines[1].decompress_ra_batch(d_arc.data_ptr(), n1, d_ra.data_ptr(), offs, sizes, oo)
    for i in rng.randint(0, q, size=2000):
        o, s, w = int(offs[i]), int(sizes[i]), int(oo[i])
        assert torch.equal(d_ra[w: w + s], d_in[o: o + s]), i


def test_crafted_headers_cannot_write_out_of_bounds(zra, gpu_engine):
    """Device-pointer decode of archives whose header fields disagree: an inflated tableSize, a shrunk uncompressedSize. The
    reference's one multi-frame zstd call runs out of destination (dstSize_tooSmall); nothing may be written behind the caller's buffer
    (guard region), and the batched random access must refuse such a header instead of indexing past the table."""
    import torch
    dev = torch.device("cuda", 0)
    fs = 4096
    data = C.gen_C(10 * fs)
    st, arc = O.zra_compress(data, 3, fs, True)
    nent = len(data) // fs + 1
    guard = 1 << 20

    def run(a, cap):
        d_a = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).to(dev)
        d_o = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=dev)
        try:
            gpu_engine.decompress(d_a.data_ptr(), len(a), d_o.data_ptr(), cap)
            status = (0, 0)
        except zra.ZraError as e:
            status = (e.zra, e.zstd)
        assert bool((d_o[cap:] == 0xA5).all()), "bytes behind the output capacity were touched"
        return status, d_a

    # uncompressedSize shrunk to 2.5 frames: frames 3.. have no room
    a = bytearray(arc)
    a[18:26] = (2 * fs + fs // 2).to_bytes(8, "little")
    status, d_a = run(bytes(a), 2 * fs + fs // 2)
    assert status == (1, 70)
    with pytest.raises(zra.ZraError) as e:          # header fields disagree: frames != ceil(size / frameSize)
        gpu_engine.decompress_ra_batch(d_a.data_ptr(), len(a), d_a.data_ptr(), np.array([0], dtype=np.uint64), np.array([10], dtype=np.uint64), np.array([0], dtype=np.uint64))
    assert e.value.zra == 3
    # tableSize inflated (entries beyond the real table read frame bytes as offsets): must fail cleanly, whatever the code
    a = bytearray(arc)
    a[26:30] = (nent + 6).to_bytes(4, "little")
    a[4:8] = (int.from_bytes(arc[4:8], "little") + 30).to_bytes(4, "little")       # headerSize grows with the table
    status, _ = run(bytes(a), len(data))
    assert status[0] != 0
    # u64 wrap in offset + size
    d_a = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to(dev)
    d_o = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.decompress_ra_batch(d_a.data_ptr(), len(arc), d_o.data_ptr(), np.array([(1 << 64) - 5], dtype=np.uint64), np.array([10], dtype=np.uint64), np.array([0], dtype=np.uint64))
    assert e.value.zra == 5


def test_input_with_a_short_tail_stays_on_the_persistent_pipeline(zra, gpu_engine):
    """an input that is not a multiple of the frame size must take the same (benchmarked) persistent match-finder pipeline as
    an exact multiple — one match-finder launch — and still match the oracle byte for byte."""
    import torch
    dev = torch.device("cuda", 0)
    fs = 65536
    data = (C.gen_E(1 << 20) * 9)[: 8 * (1 << 20) + 1234]          # 128 full frames + a 1,234-byte tail (its own cparams: dfast, minMatch 4)
    st, ref = O.zra_compress(data, 3, fs, True)
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    d_arc = torch.empty(zra.GetOutputBufferSize(len(data), fs) + 64, dtype=torch.uint8, device=dev)
    n = gpu_engine.compress(d_in.data_ptr(), len(data), d_arc.data_ptr(), 3, fs, True)
    assert d_arc[:n].cpu().numpy().tobytes() == ref
    assert gpu_engine.kernel_stats()["mf_launches"] == 1


@pytest.mark.gpu
def test_multi_block_frames_in_two_half_batches(zra, gpu_engine):
    """Round 5: frames of several blocks whose batch would hold the whole call run as two half batches on the two scratch contexts (block
    b + 1's match finder waits for block b's entropy stage; two contexts fill each other's gaps) — from 32 frames per CU on. 8,192 frames
    of 132 KiB (two blocks each: 128 KiB + 4 KiB) at level 3, 1.03 GiB of log-like data: the archive is the oracle's, byte for byte
    (reference call site zra.cpp:216-225), the call took the match finder's 2 x 2 launches, and it decodes back."""
    import torch
    dev = torch.device("cuda", 0)
    fs, nfr = 135168, 8192
    base = np.frombuffer(C.gen_loglike(33 << 20, seed=9), dtype=np.uint8)
    data = np.resize(base, fs * nfr).tobytes()
    st, ref = O.zra_compress(data, 3, fs, True)
    assert st == (0, 0)
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    d_arc = torch.empty(zra.GetOutputBufferSize(len(data), fs) + 64, dtype=torch.uint8, device=dev)
    n = gpu_engine.compress(d_in.data_ptr(), len(data), d_arc.data_ptr(), 3, fs, True)
    assert n == len(ref)
    assert hashlib.sha256(d_arc[:n].cpu().numpy().tobytes()).digest() == hashlib.sha256(ref).digest()
    assert gpu_engine.kernel_stats()["mf_launches"] == 4
    d_back = torch.empty(len(data), dtype=torch.uint8, device=dev)
    gpu_engine.decompress(d_arc.data_ptr(), n, d_back.data_ptr(), len(data))
    assert torch.equal(d_back, d_in)


def test_the_same_calls_give_the_same_bytes_after_release_scratch(zra):
    """On a fresh engine one compress, one whole-archive decompress, one batched random-access read and one update reserve buffers of
    every group (decoder, planner, encoder contexts, update); after release_scratch() the same four calls have to allocate all of them
    again and give the same bytes. (What this cannot see is a buffer that release_scratch() forgets: the process-wide scratch counter
    behind the engine pool's cap is not exposed by the C ABI.)"""
    import torch
    dev = torch.device("cuda", 0)
    fs, n = 65536, 1 << 20
    data = C.gen_E(n)
    patch = bytes(range(256)) * 4                                           # 1 KiB across the boundary of frames 2 and 3
    poff = 3 * fs - 500
    want = bytearray(data); want[poff:poff + len(patch)] = patch
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    d_new = torch.from_numpy(np.frombuffer(patch, dtype=np.uint8).copy()).to(dev)
    offs = np.array([0, fs - 10, 5 * fs + 123, n - 4097], dtype=np.uint64)
    sizes = np.array([100, 20, 70000, 4096], dtype=np.uint64)
    oo = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    cap = zra.GetOutputBufferSize(n + len(patch), fs) + 64
    eng = zra.Engine(0)

    def four_calls():
        d_arc = torch.zeros(cap, dtype=torch.uint8, device=dev)
        asz = eng.compress(d_in.data_ptr(), n, d_arc.data_ptr(), 3, fs, True)
        d_out = torch.zeros(n, dtype=torch.uint8, device=dev)
        eng.decompress(d_arc.data_ptr(), asz, d_out.data_ptr(), n)
        d_ra = torch.zeros(int(sizes.sum()), dtype=torch.uint8, device=dev)
        eng.decompress_ra_batch(d_arc.data_ptr(), asz, d_ra.data_ptr(), offs, sizes, oo)
        d_upd = torch.zeros(cap, dtype=torch.uint8, device=dev)
        usz = eng.update(d_arc.data_ptr(), asz, d_upd.data_ptr(), cap, writes=([poff], [len(patch)], [0]), d_data=d_new.data_ptr())
        return [t.cpu().numpy().tobytes() for t in (d_arc[:asz], d_out, d_ra, d_upd[:usz])]

    try:
        first = four_calls()
        assert first[1] == data
        assert first[2] == b"".join(data[int(o):int(o) + int(s)] for o, s in zip(offs, sizes))
        assert zra.DecompressBuffer(first[3]) == bytes(want)
        eng.release_scratch()
        assert four_calls() == first
    finally:
        eng.close()


def test_archive_calls_interleaved_on_one_engine_share_the_staging_window(zra):
    """Search, verify, update and batched random access keep their staged plaintext in ONE window of the engine, sliced at the frame size
    of the archive at hand. On one engine the calls alternate between an archive of 4,096-byte frames and one of 1,000-byte frames (70
    frames each, the last one short, checksums on), so every call finds the window as another call, at another stride, left it; then the
    scratch is handed back and the sequence runs again in reverse. Yardsticks: the plaintext (search_model, slices), DecompressBuffer of
    an update's result, and for verify the one frame of a third copy whose payload the test damaged."""
    import search_model as SM
    import verify_model as VM
    from test_gpu_update import _compress, _dev, _patched, _touched, _update
    from test_gpu_verify import _flip_mid, _verify
    eng = zra.Engine(0)
    rng = np.random.RandomState(19)
    arcs = []
    for fs, U in ((4096, 69 * 4096 + 1234), (1000, 69 * 1000 + 321)):
        data = rng.randint(0, 4, size=U).astype(np.uint8).tobytes()            # 64 possible 3-byte strings: hundreds of occurrences
        arc = _compress(eng, zra, data, 3, fs, True)
        a = dict(fs=fs, U=U, data=data, arc=arc, d=_dev(arc), short=data[fs - 1:fs + 2], big=data[3 * fs - 100:3 * fs + 156])
        assert VM.fields(arc)[2] == 70 and any(p % fs > fs - 3 for p in SM.matches(data, a["short"]))   # 70 frames; a match across a seam
        arcs.append(a)
    bad_frame = 41
    bad = _flip_mid(arcs[1]["arc"], [bad_frame])
    d_bad = _dev(bad)

    def search(a, pat, staging, passes):
        want = SM.matches(a["data"], pat)
        assert eng.search(a["d"].data_ptr(), len(a["arc"]), pat, staging_bytes=staging) == (len(want), want) and want, (a["fs"], staging)
        s = eng.search_stats()
        assert s == dict(frames=70, decoded=70, content_bytes=a["U"], matches=len(want), listed=len(want), passes=passes), (a["fs"], staging, s)

    def verify(a, staging, passes):
        assert _verify(eng, a["arc"], a["d"], content=True, staging_bytes=staging) == ((0, 0), 0, []), (a["fs"], staging)
        s = eng.verify_stats()
        assert s == dict(frames=70, checked=70, structure_faults=0, content_faults=0, decoded=70, content_bytes=a["U"], passes=passes), (a["fs"], staging, s)
        if a["fs"] == 1000:
            st, n, faults = _verify(eng, bad, d_bad, content=True, staging_bytes=staging)
            assert (st, n) == ((0, 0), 1) and [(f, stage) for f, _, stage in faults] == [(bad_frame, VM.CONTENT)] and faults[0][1] != 0, (staging, st, faults)
            s = eng.verify_stats()
            assert (s["frames"], s["checked"], s["structure_faults"], s["content_faults"], s["decoded"], s["passes"]) == (70, 70, 0, 1, 70, passes), s

    def update(a):
        fs, U = a["fs"], a["U"]
        writes, append = [(5 * fs - 7, b"\x07" * 20)], bytes(range(200, 250)) * (fs // 50 + 1)     # across frames 4 | 5; a frame and a bit more
        st, out, size = _update(eng, zra, a["arc"], writes, append, d_arc=a["d"])
        assert st == (0, 0) and zra.DecompressBuffer(out[:size]) == _patched(a["data"], writes, append), (fs, st)
        s = eng.update_stats()
        touched = _touched(writes, append, U, fs)
        assert touched == {4, 5, 69, 70}
        # frames 4, 5 and the old last frame keep old bytes: decoded; frame 70 is all new
        assert (s["frames"], s["touched"], s["decoded"], s["compressed"], s["content_bytes"], s["passes"]) == (71, 4, 3, 4, 20 + len(append), 1), (fs, s)

    def read(a):
        import torch
        fs, U = a["fs"], a["U"]
        offs, sizes = [3 * fs - 10, U - 101], [30, 100]                         # across frames 2 | 3; up to the last byte but one
        d_out = torch.zeros(130, dtype=torch.uint8, device="cuda:0")
        eng.decompress_ra_batch(a["d"].data_ptr(), len(a["arc"]), d_out.data_ptr(), offs, sizes, [0, 30])
        assert d_out.cpu().numpy().tobytes() == a["data"][offs[0]:offs[0] + 30] + a["data"][U - 101:U - 1], fs
        assert eng.kernel_stats()["dec_launches"] >= 1

    steps = [lambda a: search(a, a["short"], 1, 70), lambda a: verify(a, 1, 70), update, read,
             lambda a: search(a, a["short"], 0, 1), lambda a: verify(a, 0, 1),
             lambda a: search(a, a["big"], 3 * a["fs"], 24)]                    # 256 bytes: the carry area in front of slot 0 is full
    try:
        for step in steps:
            for a in arcs:
                step(a)
        eng.release_scratch()
        for step in reversed(steps):
            for a in reversed(arcs):
                step(a)
    finally:
        eng.close()
