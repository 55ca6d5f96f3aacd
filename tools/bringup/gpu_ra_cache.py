"""bring-up: the archive handle's frame cache (zra_hip.h: ZraHipArchive*) against ZraHipDecompressRABatch, on a 4 GiB archive of the
bench corpus (level 3, 64 KiB frames). Writes profiles/ra_cache.json.
  hit latency   1,000 single 4 KiB reads from a resident frame: host wall time with a device synchronise (median, p99), against the batch
                call at batch size 1 and a handle without slots on the same queries
  skewed        reads of 65,536 x 4 KiB queries, frame ~ Zipf(1.2), uniform offset in the frame, 512 MiB cache: GiB/s returned and hit
                rate over 20 timed reads after 2 warm-up reads, against the batch call (default and whole frames)
  uniform       256 Ki uniform 4 KiB queries, 1 GiB cache: what caching costs when almost nothing is reused (misses decode whole frames)
Every answer is sampled against the source tensor. Usage: gpu_ra_cache.py [GiB, default 4]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import zra_amd as Z  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
N = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 4 << 30
fs, qb = 65536, 4096
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat(N // len(base) + 1)[:N].contiguous()
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
frames = (N + fs - 1) // fs
L = Z.load()
rng = np.random.RandomState(7)
out = dict(archive=dict(bytes=N, compressed=asz, frame_size=fs, frames=frames, level=3))


def check(d_out, offs, oo, k=64):
    """a sample of the answers (always the first and the last) against the source tensor"""
    idx = np.unique(np.concatenate([[0, len(offs) - 1], rng.randint(0, len(offs), size=k)]))
    for i in idx:
        o, w = int(offs[i]), int(oo[i])
        assert torch.equal(d_out[w:w + qb], d_in[o:o + qb]), (i, o)


def timed(fn, d_out, offs, sizes, oo):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn(d_out.data_ptr(), offs, sizes, oo)
    torch.cuda.synchronize()
    return time.perf_counter() - t


def batch_fn(whole):
    def f(*a):
        L.ZraHipSetOptions(8 if whole else 0)
        try:
            eng.decompress_ra_batch(d_arc.data_ptr(), asz, *a)
        finally:
            L.ZraHipSetOptions(0)
    return f


def pct(ts, p):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(p * len(ts)))]


# ---- hit latency: single 4 KiB reads from one resident frame
d_o = torch.empty(qb + 64, dtype=torch.uint8, device=dev)
hot = int(rng.randint(0, frames - 2))
offs1 = (hot * fs + rng.randint(0, fs - qb, size=1000)).astype(np.uint64)
one, zero = np.ones(1, dtype=np.uint64) * qb, np.zeros(1, dtype=np.uint64)
lat = {}
with Z.Archive(eng, d_arc.data_ptr(), asz, 64 * fs) as A, Z.Archive(eng, d_arc.data_ptr(), asz, 0) as A0:
    A.read(d_o.data_ptr(), offs1[:1], one, zero)                              # makes the frame resident
    for name, fn in (("handle_hit", A.read), ("batch", batch_fn(False)), ("handle_0_slots", A0.read)):
        ts = []
        for i in range(len(offs1)):
            ts.append(timed(fn, d_o, offs1[i:i + 1], one, zero))
            if i % 97 == 0:
                check(d_o, offs1[i:i + 1], zero, 0)
        lat[name] = dict(median_us=round(pct(ts, 0.5) * 1e6, 1), p99_us=round(pct(ts, 0.99) * 1e6, 1))
    s = A.stats()
    assert s["misses"] == 1 and s["hits"] == len(offs1), s
out["hit_latency"] = lat
print("hit latency", json.dumps(lat), flush=True)


def serving(name, nq, cache_bytes, draw, reads=20, warm=2):
    sizes = np.full(nq, qb, dtype=np.uint64)
    oo = np.arange(nq, dtype=np.uint64) * qb
    d_o = torch.empty(nq * qb + 64, dtype=torch.uint8, device=dev)
    queries = [draw(nq) for _ in range(warm + reads)]
    res = {}
    with Z.Archive(eng, d_arc.data_ptr(), asz, cache_bytes) as A:
        for label, fn in (("handle", A.read), ("batch", batch_fn(False)), ("batch_whole_frames", batch_fn(True))):
            ts, st0 = [], A.stats()
            for r, offs in enumerate(queries):
                t = timed(fn, d_o, offs, sizes, oo)
                check(d_o, offs, oo)
                if r == warm - 1:
                    st0 = A.stats()
                if r >= warm:
                    ts.append(t)
            sec = sum(ts)
            res[label] = dict(gib_s=round(reads * nq * qb / sec / (1 << 30), 3), ms_per_read=round(sec / reads * 1e3, 2))
            if label == "handle":
                s = A.stats()
                h, m = s["hits"] - st0["hits"], s["misses"] - st0["misses"]
                res[label].update(hit_rate=round(h / max(1, h + m), 4), frames_decoded_per_read=round(m / reads, 1), slots=s["slots"],
                                  resident=s["resident"], evictions=s["evictions"])
    res["speedup_vs_batch"] = round(res["handle"]["gib_s"] / res["batch"]["gib_s"], 2)
    res["speedup_vs_batch_whole_frames"] = round(res["handle"]["gib_s"] / res["batch_whole_frames"]["gib_s"], 2)
    out[name] = res
    print(name, json.dumps(res), flush=True)


def zipf_draw(nq):
    f = rng.zipf(1.2, size=nq) - 1
    f = np.where(f < frames - 1, f, rng.randint(0, frames - 1, size=nq))      # (tail beyond the archive: uniform; the last frame is short)
    perm_f = (f * 2654435761) % (frames - 1)                                    # hot frames spread over the archive
    return (perm_f * fs + rng.randint(0, fs - qb, size=nq)).astype(np.uint64)


def uniform_draw(nq):
    return rng.randint(0, N - qb - 1, size=nq).astype(np.uint64)


serving("skewed", 65536, 512 << 20, zipf_draw)
serving("uniform", 256 << 10, 1 << 30, uniform_draw, reads=5, warm=1)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ra_cache.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
