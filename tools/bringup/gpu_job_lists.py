"""bring-up: the device-archive calls whose planning kernels are built from zra_joblist.h, from the package in TREE, to set two builds
side by side on one card (profiles/job_lists.md: the parent commit's tree and this one, in turn). The shape is the one where the
single-workgroup kernels weigh most: 65,536 frames of 1,024 bytes in one pass at the default staging size. Archive B is A with one
byte changed in every third frame; A has a delimiter in every second frame. Each call: one warm run, then REPS runs, the call's
own-launch time (ZraHipDebug*Ms; the handle's scan_stage_ms on a handle whose first 32,768 frames are resident), median and every
value. Verify and update have no such word: they run once at the end, for a kernel trace of the process (rocprofv3 --kernel-trace
--stats, the program behind `--`; a smaller REPS keeps the trace short). Prints one line and writes OUT.
Usage: gpu_job_lists.py TREE OUT.json [REPS]"""
import json, os, sys
import numpy as np
TREE, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 9
sys.path.insert(0, TREE)
import torch
import zra_amd as Z
assert os.path.abspath(Z.__file__).startswith(TREE + os.sep), Z.__file__
dev = torch.device("cuda", 0)
FS, F = 1024, 65536
U = F * FS
NL = 10
eng = Z.Engine(0)
L = Z.load()
g = torch.Generator(device=dev); g.manual_seed(1)
data = torch.randint(0, 24, (U,), dtype=torch.uint8, device=dev, generator=g)
data[data == NL] = 0x40
data.view(F, FS)[::2, 5] = NL
buf = torch.empty(Z.GetOutputBufferSize(U, FS) + (8 << 20), dtype=torch.uint8, device=dev)
asz = eng.compress(data.data_ptr(), U, buf.data_ptr(), 3, FS, True)
A = buf[:asz].clone()
data.view(F, FS)[::3, 2] ^= 0x80
bsz = eng.compress(data.data_ptr(), U, buf.data_ptr(), 3, FS, True)
B = buf[:bsz].clone()
del data
torch.cuda.synchronize()
changed = len(range(0, F, 3))
patch = torch.empty(64 * changed + 4096, dtype=torch.uint8, device=dev)
GRAIN = 64
words = Z.signature_words(U, FS, GRAIN)
sigbuf = torch.empty(words, dtype=torch.int64, device=dev)
idxbuf = torch.empty(F, dtype=torch.int64, device=dev)
index = eng.index_records(A.data_ptr(), asz, idxbuf.data_ptr(), F)
numbers = np.arange(index.records, dtype=np.uint64)
h = Z.Archive(eng, A.data_ptr(), asz, (F // 2 + 16) * FS)
warm = torch.empty(F // 2, dtype=torch.uint8, device=dev)
for f0 in range(0, F // 2, 4096):
    h.read(warm.data_ptr(), [f * FS for f in range(f0, f0 + 4096)], [1] * 4096, list(range(f0, f0 + 4096)))
assert h.stats()["resident"] == F // 2, h.stats()
state = {}
PAT = bytes([3, 1, 4, 1, 5, 9, 2, 6])

CALLS = (
    ("compare", lambda: eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz), eng.compare_ms, lambda: eng.compare_stats()["decoded"] == changed),
    ("compare_all", lambda: eng.compare(A.data_ptr(), asz, B.data_ptr(), bsz, decode_all=True), eng.compare_ms, lambda: eng.compare_stats()["decoded"] == F),
    ("diff_64", lambda: eng.diff(A.data_ptr(), asz, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), grain=GRAIN), eng.diff_ms,
     lambda: eng.diff_stats()["decoded"] == changed),
    ("diff_64_all", lambda: eng.diff(A.data_ptr(), asz, B.data_ptr(), bsz, patch.data_ptr(), patch.numel(), grain=GRAIN, decode_all=True), eng.diff_ms,
     lambda: eng.diff_stats()["decoded"] == F),
    ("sign", lambda: state.update(sig=eng.sign(A.data_ptr(), asz, sigbuf.data_ptr(), words, grain=GRAIN)), eng.sign_ms, lambda: eng.sign_stats()["passes"] == 1),
    ("sigdiff", lambda: eng.diff_signature(state["sig"], sigbuf.data_ptr(), words, B.data_ptr(), bsz, patch.data_ptr(), patch.numel()),
     lambda: L.ZraHipDebugDiffSignatureMs(eng.h), lambda: eng.diff_signature_stats()["decoded"] == changed),
    ("locate", lambda: eng.locate_records(A.data_ptr(), asz, index, idxbuf.data_ptr(), F, numbers), eng.locate_records_ms,
     lambda: eng.locate_records_stats()["decoded"] == F // 2),
    ("search", lambda: eng.search(A.data_ptr(), asz, PAT, max_matches=1 << 16), eng.search_scan_ms, lambda: eng.search_stats()["passes"] == 1),
    ("handle_search", lambda: h.search(PAT, max_matches=1 << 16), h.scan_stage_ms, lambda: h.scan_stats()["staged"] == F // 2 and h.scan_stats()["decoded"] == F // 2),
)


def timed(fn, ms, ok):
    fn()
    assert ok()
    own = []
    for _ in range(max(REPS, 1)):
        fn()
        torch.cuda.synchronize()
        own.append(ms())
    return dict(own_median=round(float(np.median(own)), 4), own=[round(t, 4) for t in own])


out = {name: timed(fn, ms, ok) for name, fn, ms, ok in CALLS}
# verify and update: no millisecond word; their planning kernels show in a kernel trace of this process
nf, _ = eng.verify(A.data_ptr(), asz, max_faults=16)
assert nf == 0 and eng.verify_stats()["decoded"] == F
touched = list(range(0, F, 3))
blob = torch.randint(128, 256, (len(touched),), dtype=torch.uint8, device=dev)
upd = torch.empty(asz + Z.GetOutputBufferSize(U, FS) + 64, dtype=torch.uint8, device=dev)
eng.update(A.data_ptr(), asz, upd.data_ptr(), upd.numel(), writes=([f * FS + 7 for f in touched], [1] * len(touched), list(range(len(touched)))), d_data=blob.data_ptr())
s = eng.update_stats()
assert (s["touched"], s["decoded"]) == (len(touched), len(touched)), s
torch.cuda.synchronize()
h.close()
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print("done", OUT)
