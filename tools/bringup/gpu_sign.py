"""bring-up: how the hash launches of ZraHipSignArchive (span hash, grain hash: ZraHipDebugSignMs) compare with the decode of the
same call (ZraHipGetKernelStats), and what ZraHipDiffSignature costs after an update of 1 % of the frames. The setup of gpu_diff.py:
1 GiB of the bench corpus, level 3, 64 KiB frames. Writes profiles/sign.json.
  sign_grain_G          the whole archive at grains 64, 4096 and 8192: wall ms, the call's own launches, its decode
  sigdiff_grain_G       the updated archive against that signature: wall ms, own launches, decode, stats; the writes are checked
                        against ZraHipDiffArchives of the two archives at the same grain
Host wall time around the synchronous calls, one warm run and then RUNS runs: median and every value.
Usage: gpu_sign.py [GiB, default 1] [runs, default 5] [output, default profiles/sign.json]"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "sign.json")
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
blob = torch.randint(128, 256, (64 * len(touched),), dtype=torch.uint8, device=dev)
offs = [f * FS + 1000 for f in touched]
bsz = eng.update(A.data_ptr(), asz, buf.data_ptr(), buf.numel(), writes=(offs, [64] * len(touched), [64 * i for i in range(len(touched))]),
                 d_data=blob.data_ptr())
B = buf[:bsz].clone()
del buf, data
torch.cuda.synchronize()
out = dict(archive=dict(content_bytes=U, frame_size=FS, frames=F, level=3, compressed_a=asz, compressed_b=bsz, frames_written=len(touched)), runs=RUNS)
patch = torch.empty(16384 * len(touched) + 4096, dtype=torch.uint8, device=dev)


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
for grain in (64, 4096, 8192):
    nw = Z.signature_words(U, FS, grain)
    d_sig = torch.zeros(nw, dtype=torch.int64, device=dev)
    key = "sign_grain_%d" % grain
    out[key] = timed(lambda: res.update(sig=eng.sign(A.data_ptr(), asz, d_sig.data_ptr(), nw, grain=grain)))
    ks = eng.kernel_stats()
    out[key].update(words=nw, stats=eng.sign_stats(), sign_own_launches_ms=round(eng.sign_ms(), 3), dec_ms=round(ks["dec_ms"], 3),
                    own_over_decode=round(eng.sign_ms() / ks["dec_ms"], 4) if ks["dec_ms"] else None)
    key = "sigdiff_grain_%d" % grain
    out[key] = timed(lambda: res.update(diff=eng.diff_signature(res["sig"], d_sig.data_ptr(), nw, B.data_ptr(), bsz, patch.data_ptr(), patch.numel())))
    w, ao, app, size = res["diff"]
    ks = eng.kernel_stats()
    out[key].update(stats=eng.diff_signature_stats(), sigdiff_own_launches_ms=round(eng.diff_signature_ms(), 3), dec_ms=round(ks["dec_ms"], 3), writes=len(w[0]),
                    data_bytes=size)
    got = patch[:size].clone()
    w2, ao2, app2, size2 = eng.diff(A.data_ptr(), asz, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), grain=grain)
    assert (ao, app, size) == (ao2, app2, size2) and all(np.array_equal(x, y) for x, y in zip(w, w2)) and torch.equal(got, patch[:size]), key
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
