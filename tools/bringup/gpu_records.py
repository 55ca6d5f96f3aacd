"""bring-up: what the record index costs on the bench archive (the bench corpus tiled, level 3, 64 KiB frames, delimiter 0x0A).
Writes profiles/records.json.
  verify_content        ZraHipVerifyArchive in CONTENT mode over the whole archive: wall ms and the decode of the call
  index                 ZraHipIndexRecords over the whole archive: wall ms, its own launches (ZraHipDebugIndexRecordsMs), its decode
  locate_<set>          ZraHipLocateRecords of a set of record numbers: wall ms, own launches (ZraHipDebugLocateRecordsMs), decode, stats
  read_<set>            ZraHipReadRecords of the same set (a sizing call first, outside the time): wall ms, stats
The sets: 100 consecutive records, 10,000 and 1,000,000 uniformly drawn ones. The totals are checked against a count of the
delimiter in the plaintext, and a sample of the located records against the plaintext itself.
Host wall time around the synchronous calls, one warm run and then RUNS runs: median and every value.
Usage: gpu_records.py [GiB, default 16] [runs, default 3] [output, default profiles/records.json]"""
import ctypes
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
U = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 16 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "records.json")
FS = 65536
U -= U % FS
F = U // FS
NL = 0x0A
eng = Z.Engine(0)
L = Z.load()
base = bench.synth_corpus(64 << 20, seed=1)
data = torch.from_numpy(base).to(dev).repeat(U // len(base) + 2)[:U].contiguous()
buf = torch.empty(Z.GetOutputBufferSize(U, FS) + (64 << 20), dtype=torch.uint8, device=dev)
asz = eng.compress(data.data_ptr(), U, buf.data_ptr(), 3, FS, True)
A = buf[:asz].clone()
del buf
torch.cuda.synchronize()
D = sum(int((data[lo:lo + (1 << 30)] == NL).sum()) for lo in range(0, U, 1 << 30))
R = D + (int(data[U - 1]) != NL)
out = dict(archive=dict(content_bytes=U, frame_size=FS, frames=F, level=3, compressed=asz, delimiters=D, records=R), runs=RUNS)
P64 = ctypes.POINTER(ctypes.c_uint64)


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


out["verify_content"] = timed(lambda: eng.verify(A.data_ptr(), asz, content=True))
out["verify_content"].update(stats=eng.verify_stats(), dec_ms=round(eng.kernel_stats()["dec_ms"], 3))

d_index = torch.zeros(F, dtype=torch.int64, device=dev)
res = {}
out["index"] = timed(lambda: res.update(idx=eng.index_records(A.data_ptr(), asz, d_index.data_ptr(), F, delimiter=NL)))
idx = res["idx"]
assert (idx.delimiters, idx.records) == (D, R), (idx, D, R)
out["index"].update(stats=eng.index_records_stats(), index_own_launches_ms=round(eng.index_records_ms(), 3), dec_ms=round(eng.kernel_stats()["dec_ms"], 3),
                    index_bytes=8 * F)
info = Z.ZraHipRecordIndex(*idx)
rng = np.random.RandomState(7)
start = int(rng.randint(0, R - 100))
sets = {"100_consecutive": np.arange(start, start + 100, dtype=np.uint64), "10000_random": rng.randint(0, R, size=10000).astype(np.uint64),
        "1000000_random": rng.randint(0, R, size=1000000).astype(np.uint64)}
for name, nums in sets.items():
    n = len(nums)
    ranges = np.zeros(2 * n, dtype=np.uint64)

    def locate():
        eng._order()
        st = L.ZraHipLocateRecords(eng.h, A.data_ptr(), asz, ctypes.byref(info), d_index.data_ptr(), F, nums.ctypes.data_as(P64), n, 0, ranges.ctypes.data_as(P64))
        assert st.tup() == (0, 0), st.tup()
    key = "locate_" + name
    out[key] = timed(locate)
    out[key].update(stats=eng.locate_records_stats(), locate_own_launches_ms=round(eng.locate_records_ms(), 3), dec_ms=round(eng.kernel_stats()["dec_ms"], 3))
    # a sample against the plaintext: the byte in front is a delimiter, the byte behind is one, none lies inside
    for i in rng.randint(0, n, size=200):
        s, ln = int(ranges[2 * i]), int(ranges[2 * i + 1])
        assert s == 0 or int(data[s - 1]) == NL, (name, i, s)
        assert s + ln == U or int(data[s + ln]) == NL, (name, i, s, ln)
        assert not bool((data[s:s + ln] == NL).any()), (name, i, s, ln)
    for i in rng.randint(0, n, size=3):                                        # and its number is the delimiters in front of it
        s = int(ranges[2 * i])
        assert sum(int((data[lo:min(s, lo + (1 << 30))] == NL).sum()) for lo in range(0, s, 1 << 30)) == int(nums[i]), (name, i)
    size = ctypes.c_uint64(0)
    eng._order()
    st = L.ZraHipReadRecords(eng.h, A.data_ptr(), asz, ctypes.byref(info), d_index.data_ptr(), F, nums.ctypes.data_as(P64), n, 0, None, None, 0, ctypes.byref(size))
    assert st.tup() in ((6, 0), (0, 0)), st.tup()
    d_data = torch.empty(size.value + 64, dtype=torch.uint8, device=dev)

    def read():
        eng._order()
        st = L.ZraHipReadRecords(eng.h, A.data_ptr(), asz, ctypes.byref(info), d_index.data_ptr(), F, nums.ctypes.data_as(P64), n, 0, None, d_data.data_ptr(),
                                 size.value, ctypes.byref(size))
        assert st.tup() == (0, 0), st.tup()
    key = "read_" + name
    out[key] = timed(read)
    out[key].update(stats=eng.read_records_stats(), locate_sweep_own_launches_ms=round(eng.read_records_ms(), 3))
    at = 0
    for i in range(min(n, 50)):                                                # the first records of the packed text against the plaintext
        s, ln = int(ranges[2 * i]), int(ranges[2 * i + 1])
        assert torch.equal(d_data[at:at + ln], data[s:s + ln]) and int(d_data[at + ln]) == NL, (name, i)
        at += ln + 1
    del d_data
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
