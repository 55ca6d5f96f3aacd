"""bring-up: the calls that run through the frame-pass driver (zra_framepass.h: compare, diff, sign, signature diff, index) from the
package in TREE, to set two builds side by side on one card (profiles/frame_pass_driver.md: the parent commit's tree and this one, in
turn). The setup of gpu_compare.py / gpu_diff.py / gpu_sign.py: 1 GiB of the bench corpus, level 3, 64 KiB frames; archive B is A
after a ZraHipUpdateArchive that writes 64 bytes into 1 % of the frames. Each call at two staging sizes, one pass and 16 passes
(1,024 slots; frame pairs for compare and diff): one warm run, then 5 runs, host wall time around the synchronous call and the call's
own-launch time (ZraHipDebug*Ms), median and every value. Prints one line per staging size and writes OUT.
Usage: gpu_framepass_ab.py TREE OUT.json"""
import json, os, sys, time
import numpy as np
TREE, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, TREE)
import torch
import zra_amd as Z
import bench
assert os.path.abspath(Z.__file__).startswith(TREE), Z.__file__
dev = torch.device("cuda", 0)
U = 1 << 30
FS = 65536
F = U // FS
eng = Z.Engine(0)
base = bench.synth_corpus(64 << 20, seed=1)
data = torch.from_numpy(base).to(dev).repeat(U // len(base) + 2)[:U].contiguous()
buf = torch.empty(Z.GetOutputBufferSize(U, FS) + (64 << 20), dtype=torch.uint8, device=dev)
asz = eng.compress(data.data_ptr(), U, buf.data_ptr(), 3, FS, True)
A = buf[:asz].clone()
touched = list(range(7, F, 100))
blob = torch.randint(128, 256, (64 * len(touched),), dtype=torch.uint8, device=dev)
offs = [f * FS + 1000 for f in touched]
bsz = eng.update(A.data_ptr(), asz, buf.data_ptr(), buf.numel(), writes=(offs, [64] * len(touched), [64 * i for i in range(len(touched))]), d_data=blob.data_ptr())
B = buf[:bsz].clone()
del data
torch.cuda.synchronize()
patch = torch.empty(2 * 4096 * len(touched) + 4096, dtype=torch.uint8, device=dev)
GRAIN = 4096
words = Z.signature_words(U, FS, GRAIN)
sigbuf = torch.empty(words, dtype=torch.int64, device=dev)
idx = torch.empty(F, dtype=torch.int64, device=dev)
state = {}

def timed(fn, ms):
    fn()
    ts, own = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        own.append(ms())
    return dict(wall_median=round(float(np.median(ts)), 3), wall=[round(t, 3) for t in ts], own_median=round(float(np.median(own)), 3), own=[round(t, 3) for t in own])

out = {}
for label, single, pair in (("1_pass", 0, 0), ("16_passes", (F // 16) * FS, 2 * (F // 16) * FS)):
    r = {}
    r["compare"] = timed(lambda: eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz, staging_bytes=pair), eng.compare_ms)
    r["compare"]["passes"] = eng.compare_stats()["passes"]
    r["compare_all"] = timed(lambda: eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz, staging_bytes=pair, decode_all=True), eng.compare_ms)
    r["compare_all"]["passes"] = eng.compare_stats()["passes"]
    r["diff_64"] = timed(lambda: eng.diff(A.data_ptr(), asz, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), grain=64, staging_bytes=pair), eng.diff_ms)
    r["diff_64"]["passes"] = eng.diff_stats()["passes"]
    r["sign"] = timed(lambda: state.update(sig=eng.sign(A.data_ptr(), asz, sigbuf.data_ptr(), words, grain=GRAIN, staging_bytes=single)), eng.sign_ms)
    r["sign"]["passes"] = eng.sign_stats()["passes"]
    r["sigdiff"] = timed(lambda: eng.diff_signature(state["sig"], sigbuf.data_ptr(), words, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), staging_bytes=single),
                         lambda: Z.load().ZraHipDebugDiffSignatureMs(eng.h))
    r["sigdiff"]["passes"] = eng.diff_signature_stats()["passes"]
    r["sigdiff_all"] = timed(lambda: eng.diff_signature(state["sig"], sigbuf.data_ptr(), words, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), staging_bytes=single,
                                                        decode_all=True), lambda: Z.load().ZraHipDebugDiffSignatureMs(eng.h))
    r["index"] = timed(lambda: eng.index_records(A.data_ptr(), asz, idx.data_ptr(), F, staging_bytes=single), lambda: Z.load().ZraHipDebugIndexRecordsMs(eng.h))
    r["index"]["passes"] = eng.index_records_stats()["passes"]
    out[label] = r
    print(label, json.dumps(r), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print("done", OUT)
