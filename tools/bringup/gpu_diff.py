"""bring-up: ZraHipDiffArchives against ZraHipCompareArchives on the same pair (its yardstick: the diff is the compare plus one write
of the dirty bytes) and against the route it replaces, two ZraHipDecompressBuffer calls into two content-sized buffers (and a gather of
the caller's own, which is not timed). The setup of gpu_compare.py: 1 GiB of the bench corpus, level 3, 64 KiB frames; the second
archive is the first after a ZraHipUpdateArchive that writes 64 bytes into 1 % of the frames. Writes profiles/diff.json.
  (a) compare        old against new
  (b) diff_grain_1   the same pair, grain 1
      diff_grain_64  the same pair, grain 64
  (c) reference      ZraHipDecompressBuffer of old, then of new
Host wall time around the synchronous calls, one warm run and then RUNS runs: median and every value. With each diff: its stats,
ZraHipDebugDiffMs (the diff's own launches) and ZraHipGetKernelStats (its decodes) of the last run. The writes of (b) are checked
against the update's, the packed bytes against the decoded content of the new archive, and the patch is applied: the update of the old
archive with it gives the new archive's bytes.
Usage: gpu_diff.py [GiB, default 1] [runs, default 5] [output, default profiles/diff.json]"""
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
U = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 1 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "diff.json")
FS = 65536
U -= U % FS
F = U // FS
eng = Z.Engine(0)
base = bench.synth_corpus(64 << 20, seed=1)
data = torch.from_numpy(base).to(dev).repeat(U // len(base) + 2)[:U].contiguous()
buf = torch.empty(Z.GetOutputBufferSize(U, FS) + (64 << 20), dtype=torch.uint8, device=dev)
asz = eng.compress(data.data_ptr(), U, buf.data_ptr(), 3, FS, True)
A = buf[:asz].clone()
touched = list(range(7, F, 100))                                               # 1 % of the frames
blob = torch.randint(128, 256, (64 * len(touched),), dtype=torch.uint8, device=dev)   # (the corpus is text and small values: every byte differs)
offs = [f * FS + 1000 for f in touched]
bsz = eng.update(A.data_ptr(), asz, buf.data_ptr(), buf.numel(), writes=(offs, [64] * len(touched), [64 * i for i in range(len(touched))]),
                 d_data=blob.data_ptr())
B = buf[:bsz].clone()
torch.cuda.synchronize()
out = dict(archive=dict(content_bytes=U, frame_size=FS, frames=F, level=3, compressed_a=asz, compressed_b=bsz, frames_written=len(touched)), runs=RUNS)
patch = torch.empty(128 * len(touched) + 4096, dtype=torch.uint8, device=dev)  # (grain 64: a write of 64 bytes at 1000 lies in two grains)


def timed(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 3), all_ms=[round(t, 3) for t in ts])


res = {}
out["compare"] = timed(lambda: res.update(compare=eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz, max_ranges=1 << 16)))
out["compare"].update(stats=eng.compare_stats(), compare_own_launches_ms=round(eng.compare_ms(), 3), kernel_stats=eng.kernel_stats(),
                      ranges=res["compare"][0], differing_bytes=res["compare"][1])
for grain in (1, 64):
    key = "diff_grain_%d" % grain
    out[key] = timed(lambda: res.update({key: eng.diff(A.data_ptr(), asz, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), grain=grain)}))
    w, ao, app, size = res[key]
    out[key].update(stats=eng.diff_stats(), diff_own_launches_ms=round(eng.diff_ms(), 3), kernel_stats=eng.kernel_stats(), writes=len(w[0]), data_bytes=size)
    assert app == 0 and ao == size == int(w[1].sum())
    if grain == 1:
        assert [(int(o), int(n)) for o, n in zip(w[0], w[1])] == res["compare"][2], "grain 1: the compare's ranges"
    else:
        assert [(int(o), int(n)) for o, n in zip(w[0], w[1])] == [(o - o % 64, 128) for o in offs], "grain 64: the two grains of every write"
    # the patch applied: the update of the old archive gives the new archive's bytes
    csz = eng.update(A.data_ptr(), asz, buf.data_ptr(), buf.numel(), writes=w, d_data=patch.data_ptr())
    assert csz == bsz and torch.equal(buf[:csz], B), key
    res[key + "_data"] = patch[:size].clone()
eng.release_scratch()
del buf
o1 = torch.empty(U, dtype=torch.uint8, device=dev)
o2 = torch.empty(U, dtype=torch.uint8, device=dev)


def ref():
    eng.decompress(A.data_ptr(), asz, o1.data_ptr(), U)
    eng.decompress(B.data_ptr(), bsz, o2.data_ptr(), U)


out["reference_two_decompress"] = timed(ref)
for grain in (1, 64):                                                          # the packed bytes are the new content's
    w = res["diff_grain_%d" % grain][0]
    idx = torch.cat([torch.arange(int(o), int(o + n), device=dev) for o, n in zip(w[0], w[1])])
    assert torch.equal(o2[idx], res["diff_grain_%d_data" % grain]), grain
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
