"""bring-up: ZraHipArchiveUpdate (an update through an archive handle, which keeps the handle's cache) against the route it replaces:
ZraHipUpdateArchive, ZraHipArchiveClose, ZraHipArchiveOpen with the same cache, the reads. 4 GiB of the bench corpus, level 3, 64 KiB
frames, a 512 MiB cache. Writes profiles/archive_update.json.
  (a) one_write   one 4 KiB write into a resident frame: the handle's update beside ZraHipUpdateArchive alone
  (b) serve_loop  8 rounds of {one update of 256 x 4 KiB writes at Zipf(1.2) frames, one read of 65,536 x 4 KiB Zipf(1.2) queries}:
                  wall per round and hit rate per round, both routes on the same writes and queries
  (c) stage       the stage-from-cache kernel alone (HIP events on the engine's stream) in an update that writes 16 bytes into each of
                  8,192 resident frames: (bytes read + written) / time beside a device-to-device copy of the same byte count
Host wall time with a device synchronise, median / min / max of RUNS runs after one warm-up, the routes alternating in one process.
Every update's archive is compared with ZraHipUpdateArchive's, byte for byte, and sampled answers with the patched content.
Usage: gpu_archive_update.py [GiB, default 4] [runs, default 5]"""
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
fs, qb, CACHE = 65536, 4096, 512 << 20
N -= N % fs
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat(N // len(base) + 2)[:N].contiguous()
eng = Z.Engine(0)
cap = Z.GetOutputBufferSize(N, fs) + (64 << 20)
bufs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3)]      # [0], [1]: the handle's ping-pong; [2]: the other route's output
asz = eng.compress(d_in.data_ptr(), N, bufs[0].data_ptr(), 3, fs, True)
frames = N // fs
rng = np.random.RandomState(12)
g = torch.Generator(device=dev); g.manual_seed(12)
out = dict(archive=dict(bytes=N, compressed=asz, frame_size=fs, frames=frames, level=3, cache_bytes=CACHE), runs=RUNS)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2] * 1e3, 3), min_ms=round(ts[0] * 1e3, 3), max_ms=round(ts[-1] * 1e3, 3))


def zipf_frames(nq):
    f = rng.zipf(1.2, size=nq) - 1
    f = np.where(f < frames - 1, f, rng.randint(0, frames - 1, size=nq))
    return (f * 2654435761) % (frames - 1)                                      # hot frames spread over the archive (gpu_ra_cache.py)


def read(H, offs, d_ans):
    nq = len(offs)
    H.read(d_ans.data_ptr(), offs, np.full(nq, qb, dtype=np.uint64), np.arange(nq, dtype=np.uint64) * qb)


def hit_rate(after, before):
    h, m = after["hits"] - before["hits"], after["misses"] - before["misses"]
    return round(h / max(1, h + m), 4)


# ---- (c) the stage-from-cache kernel alone: 16 bytes written into each of 8,192 resident frames, so every touched frame is staged
# from the arena in one pass. HIP events around the kernel on the engine's stream (ZraHipDebugUpdateStageMs), beside a device-to-device
# copy of the same byte count timed with events on its stream.
hot = np.arange(8192, dtype=np.uint64) * 7 % frames
H = Z.Archive(eng, bufs[0].data_ptr(), asz, CACHE)
d_ans = torch.empty(8192 * 16, dtype=torch.uint8, device=dev)
H.read(d_ans.data_ptr(), hot * fs, np.full(8192, 16, dtype=np.uint64), np.arange(8192, dtype=np.uint64) * 16)
assert H.stats()["resident"] == 8192
d_new = torch.randint(0, 256, (8192 * 16,), dtype=torch.uint8, device=dev, generator=g)
w = (hot * fs + 1000, np.full(8192, 16, dtype=np.uint64), np.arange(8192, dtype=np.uint64) * 16)
sms = []
for r in range(RUNS + 1):
    H.update(bufs[(r + 1) % 2].data_ptr(), cap, writes=w, d_data=d_new.data_ptr())
    u, e = H.update_stats(), eng.update_stats()
    assert (u["staged"], e["decoded"], e["passes"]) == (8192, 0, 1), (u, e)
    sms.append(eng.L.ZraHipDebugUpdateStageMs(eng.h))
H.close()
moved = 8192 * fs
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
cms = []
for _ in range(RUNS + 1):
    e0.record(); bufs[2][:moved].copy_(d_in[:moved]); e1.record(); torch.cuda.synchronize()
    cms.append(e0.elapsed_time(e1))
sms, cms = sorted(sms[1:]), sorted(cms[1:])
sm, cm = sms[len(sms) // 2], cms[len(cms) // 2]
out["stage"] = dict(frames=8192, bytes_read_plus_written=2 * moved, stage_ms=round(sm, 4), stage_ms_min=round(sms[0], 4), stage_ms_max=round(sms[-1], 4),
                    stage_gib_s_read_plus_written=round(2 * moved / (sm * 1e-3) / (1 << 30), 1), d2d_copy_ms=round(cm, 4),
                    d2d_copy_gib_s_read_plus_written=round(2 * moved / (cm * 1e-3) / (1 << 30), 1))
print("stage", json.dumps(out["stage"]), flush=True)
asz = eng.compress(d_in.data_ptr(), N, bufs[0].data_ptr(), 3, fs, True)           # (a) and (b) start from the original archive again

# ---- (a) one 4 KiB write into a resident frame
fa = int(rng.randint(0, frames - 1))
oa = fa * fs + 1000
new_a = torch.randint(0, 256, (qb,), dtype=torch.uint8, device=dev, generator=g)
wa = ([oa], [qb], [0])
H = Z.Archive(eng, bufs[0].data_ptr(), asz, CACHE)
d_one = torch.empty(qb, dtype=torch.uint8, device=dev)
read(H, np.array([oa], dtype=np.uint64), d_one)
th, te, cur = [], [], 0
for r in range(RUNS + 1):                                       # alternating, the first pair is the warm-up
    t, hsz = wall(lambda: H.update(bufs[1 - cur].data_ptr(), cap, writes=wa, d_data=new_a.data_ptr()))
    hu, he = H.update_stats(), eng.update_stats()
    t2, esz = wall(lambda: eng.update(bufs[cur].data_ptr(), asz, bufs[2].data_ptr(), cap, writes=wa, d_data=new_a.data_ptr()))
    ee = eng.update_stats()
    assert hsz == esz and torch.equal(bufs[1 - cur][:hsz], bufs[2][:esz])
    cur, asz = 1 - cur, hsz
    if r:
        th.append(t); te.append(t2)
assert (hu["staged"], he["decoded"], ee["decoded"]) == (1, 0, 1), (hu, he, ee)
before = H.stats()
read(H, np.array([oa], dtype=np.uint64), d_one)
assert torch.equal(d_one, new_a) and hit_rate(H.stats(), before) == 1.0
out["one_write"] = dict(handle_update=spread(th), engine_update=spread(te), handle_decoded=he["decoded"], engine_decoded=ee["decoded"],
                        engine_over_handle_median=round(sorted(te)[len(te) // 2] / sorted(th)[len(th) // 2], 2))
print("one_write", json.dumps(out["one_write"]), flush=True)

# ---- (b) serve loop: the handle route (H, ping-pong over bufs[0] / bufs[1]) and the parent route (P: update into a new buffer, close, open,
# read) on the same writes and queries. The parent route keeps its own pair of buffers.
pb = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
pb[0][:asz].copy_(bufs[cur][:asz])
P, pcur, psz = Z.Archive(eng, pb[0].data_ptr(), asz, CACHE), 0, asz
NQ, NW = 65536, 256
d_ans = torch.empty(NQ * qb, dtype=torch.uint8, device=dev)
d_ans2 = torch.empty(NQ * qb, dtype=torch.uint8, device=dev)
rounds = []
for r in range(8):
    blocks = np.unique(zipf_frames(NW) * (fs // qb) + rng.randint(0, fs // qb, size=NW)).astype(np.uint64)
    nw = len(blocks)
    d_new = torch.randint(0, 256, (nw * qb,), dtype=torch.uint8, device=dev, generator=g)
    w = (blocks * qb, np.full(nw, qb, dtype=np.uint64), np.arange(nw, dtype=np.uint64) * qb)
    offs = (zipf_frames(NQ) * fs + rng.randint(0, fs - qb, size=NQ)).astype(np.uint64)

    def handle_route():
        global cur, asz
        asz = H.update(bufs[1 - cur].data_ptr(), cap, writes=w, d_data=d_new.data_ptr())
        cur = 1 - cur
        read(H, offs, d_ans)

    def parent_route():
        global P, pcur, psz
        psz = eng.update(pb[pcur].data_ptr(), psz, pb[1 - pcur].data_ptr(), cap, writes=w, d_data=d_new.data_ptr())
        pcur = 1 - pcur
        P.close()
        P = Z.Archive(eng, pb[pcur].data_ptr(), psz, CACHE)
        read(P, offs, d_ans2)

    hb = H.stats()
    t, _ = wall(handle_route)
    hu, he, ha = H.update_stats(), eng.update_stats(), H.stats()
    t2, _ = wall(parent_route)
    pe, pa = eng.update_stats(), P.stats()
    assert asz == psz and torch.equal(bufs[cur][:asz], pb[pcur][:psz]), r
    assert torch.equal(d_ans, d_ans2), r
    rounds.append(dict(writes=nw, handle_ms=round(t * 1e3, 2), parent_ms=round(t2 * 1e3, 2), handle_hit_rate=hit_rate(ha, hb),
                       parent_hit_rate=hit_rate(pa, dict(hits=0, misses=0)), handle_staged=hu["staged"], handle_decoded=he["decoded"],
                       parent_decoded=pe["decoded"], touched=he["touched"]))
    print("round", r, json.dumps(rounds[-1]), flush=True)
out["serve_loop"] = dict(rounds=rounds, handle_ms_median_after_first=sorted(x["handle_ms"] for x in rounds[1:])[3],
                         parent_ms_median_after_first=sorted(x["parent_ms"] for x in rounds[1:])[3])
H.close(); P.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "archive_update.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
