"""bring-up: ZraHipUpdateArchive against the full rewrite it replaces, on a 4 GiB archive of the bench corpus (level 3, 64 KiB frames).
Writes profiles/update.json.
  (a) one_write      one 4 KiB write
  (b) random_writes  65,536 x 4 KiB writes at distinct random 4 KiB blocks
  (c) append         64 MiB appended
  (d) every_frame    16 bytes written into every frame (cannot win: everything is decoded and encoded again, plus the gather)
Each is host wall time over the call with a device synchronise, median / min / max of RUNS runs after one warm-up. The baseline is the
full rewrite with calls that do not involve the update: ZraHipDecompressBuffer, a torch scatter of the new bytes, ZraHipCompressBuffer,
in the same process on the same buffers. The result of every update is decoded and compared with the baseline's patched content, and
with the baseline's archive byte for byte.
The gather kernel alone (ZraHipLastKernelMs after an update: HIP events on the engine's stream) is reported as (bytes read + bytes
written) / time beside a device-to-device copy of the same byte count timed with events on its stream.
Usage: gpu_update.py [GiB, default 4] [runs, default 5]"""
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
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
fs, qb, APP = 65536, 4096, 64 << 20
N -= N % fs
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat((N + APP) // len(base) + 2)[:N + APP].contiguous()
eng = Z.Engine(0)
cap = Z.GetOutputBufferSize(N + APP, fs) + 64
d_arc = torch.empty(cap, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
frames = N // fs
d_upd = torch.empty(cap, dtype=torch.uint8, device=dev)        # the update's output
d_plain = torch.empty(N + APP, dtype=torch.uint8, device=dev)  # the baseline's decoded content
d_ref = torch.empty(cap, dtype=torch.uint8, device=dev)        # the baseline's archive
d_chk = torch.empty(N + APP, dtype=torch.uint8, device=dev)
rng = np.random.RandomState(11)
g = torch.Generator(device=dev); g.manual_seed(11)
out = dict(archive=dict(bytes=N, compressed=asz, frame_size=fs, frames=frames, level=3), runs=RUNS)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2] * 1e3, 2), min_ms=round(ts[0] * 1e3, 2), max_ms=round(ts[-1] * 1e3, 2))


def workload(name, writes, d_new, scatter, app):
    """writes: (offsets, sizes, data offsets) or None; scatter(d_plain): the same change on decoded content; app: appended bytes"""
    d_app = d_in[N:N + app]
    total = N + app

    def update():
        return eng.update(d_arc.data_ptr(), asz, d_upd.data_ptr(), cap, writes=writes, d_data=d_new.data_ptr() if d_new is not None else 0,
                          d_append=d_app.data_ptr() if app else 0, append_size=app)

    def rewrite():
        eng.decompress(d_arc.data_ptr(), asz, d_plain.data_ptr(), N)
        if scatter is not None:
            scatter(d_plain)
        if app:
            d_plain[N:total] = d_app
        return eng.compress(d_plain.data_ptr(), total, d_ref.data_ptr(), 3, fs, True)

    tu, tb, gather = [], [], []
    for r in range(RUNS + 1):                                   # alternating, the first pair is the warm-up
        t, usz = wall(update)
        st, gms = eng.update_stats(), eng.last_kernel_ms()
        t2, rsz = wall(rewrite)
        if r:
            tu.append(t); tb.append(t2); gather.append(gms)
    assert usz == rsz and torch.equal(d_upd[:usz], d_ref[:rsz]), name     # byte-identical to the full rewrite
    eng.decompress(d_upd.data_ptr(), usz, d_chk.data_ptr(), total)
    assert torch.equal(d_chk[:total], d_plain[:total]), name
    body = st["carried_bytes"] + st["encoded_bytes"]
    gms = sorted(gather)[len(gather) // 2]
    # a device-to-device copy of the same byte count, timed the same way (events on its stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cms = []
    for _ in range(RUNS + 1):
        e0.record(); d_ref[:body].copy_(d_upd[:body]); e1.record(); torch.cuda.synchronize()
        cms.append(e0.elapsed_time(e1))
    cms = sorted(cms[1:])[len(cms[1:]) // 2]
    res = dict(update=spread(tu), full_rewrite=spread(tb), counters=st,
               speedup_median=round(sorted(tb)[len(tb) // 2] / sorted(tu)[len(tu) // 2], 2),
               update_range_below_rewrite=max(tu) < min(tb),
               gather=dict(ms=round(gms, 3), gib_s_read_plus_written=round(2 * body / (gms * 1e-3) / (1 << 30), 1) if gms else None,
                           d2d_copy_ms=round(cms, 3), d2d_copy_gib_s_read_plus_written=round(2 * body / (cms * 1e-3) / (1 << 30), 1)))
    out[name] = res
    print(name, json.dumps(res), flush=True)


# (a) one 4 KiB write
o = int(rng.randint(0, N - qb))
new_a = torch.randint(0, 256, (qb,), dtype=torch.uint8, device=dev, generator=g)
workload("one_write", ([o], [qb], [0]), new_a, lambda p: p[o:o + qb].copy_(new_a), 0)
# (b) 65,536 x 4 KiB at distinct blocks
blocks = np.sort(rng.choice(N // qb, size=65536, replace=False)).astype(np.int64)
new_b = torch.randint(0, 256, (65536 * qb,), dtype=torch.uint8, device=dev, generator=g)
idx = torch.from_numpy(blocks).to(dev)
workload("random_writes", ((blocks * qb).astype(np.uint64), np.full(65536, qb, dtype=np.uint64), np.arange(65536, dtype=np.uint64) * qb), new_b,
         lambda p: p[:N].view(-1, qb).index_copy_(0, idx, new_b.view(-1, qb)), 0)
# (c) append
workload("append", None, None, None, APP)
# (d) every frame
new_d = torch.randint(0, 256, (frames * 16,), dtype=torch.uint8, device=dev, generator=g)
workload("every_frame", (np.arange(frames, dtype=np.uint64) * fs + 1000, np.full(frames, 16, dtype=np.uint64), np.arange(frames, dtype=np.uint64) * 16), new_d,
         lambda p: p[:N].view(frames, fs)[:, 1000:1016].copy_(new_d.view(frames, 16)), 0)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "update.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
