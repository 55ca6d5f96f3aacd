"""bring-up: ZraHipCompareArchives against the route it replaces, two ZraHipDecompressBuffer calls into two content-sized buffers (and
a comparison of the caller's own, which is not timed). 1 GiB of the bench corpus, level 3, 64 KiB frames; the second archive is the
first after a ZraHipUpdateArchive that writes 64 bytes into 1 % of the frames. Writes profiles/compare.json.
  (a) compare       old against new: frames equal by their compressed bytes are not decoded
  (b) decode_all    the same pair with ZRA_HIP_COMPARE_DECODE_ALL
  (ref)             ZraHipDecompressBuffer of old, then of new
  (stream)          one pass over both plaintexts by torch (ne + sum), for scale only
Host wall time around the synchronous calls, one warm run and then RUNS runs: median and every value. With each compare: its stats,
ZraHipDebugCompareMs (the compare's own launches) and ZraHipGetKernelStats (its decode) of the last run. The ranges of (a) and (b) are
checked against the writes, their byte count against a comparison of the two decoded contents.
Usage: gpu_compare.py [GiB, default 1] [runs, default 5] [output, default profiles/compare.json]"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "compare.json")
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
del buf
torch.cuda.synchronize()
out = dict(archive=dict(content_bytes=U, frame_size=FS, frames=F, level=3, compressed_a=asz, compressed_b=bsz, frames_written=len(touched)), runs=RUNS)


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
for key, decode_all in (("compare", False), ("decode_all", True)):
    def call():
        res[key] = eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz, decode_all=decode_all, max_ranges=1024)
    out[key] = timed(call)
    out[key].update(stats=eng.compare_stats(), compare_own_launches_ms=round(eng.compare_ms(), 3), kernel_stats=eng.kernel_stats(),
                    ranges=res[key][0], differing_bytes=res[key][1])
want = [(o, 64) for o in offs]
got = res["compare"][2]
assert res["compare"] == res["decode_all"] and res["compare"][0] >= len(touched), res["compare"][:2]
assert all(any(w[0] <= g[0] and g[0] + g[1] <= w[0] + w[1] for w in want) for g in got), got[:4]    # (a written byte may equal the old one)
eng.release_scratch()
o1 = torch.empty(U, dtype=torch.uint8, device=dev)
o2 = torch.empty(U, dtype=torch.uint8, device=dev)


def ref():
    eng.decompress(A.data_ptr(), asz, o1.data_ptr(), U)
    eng.decompress(B.data_ptr(), bsz, o2.data_ptr(), U)


out["reference_two_decompress"] = timed(ref)
out["stream_both_plaintexts_torch"] = timed(lambda: torch.ne(o1, o2).sum().item())
assert torch.equal(o1, data) and int(torch.ne(o1, o2).sum().item()) == res["compare"][1]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
