"""bring-up: ZraHipSearchArchive on an archive of synthetic compressible data (level 3, 64 KiB frames): how long the scan of the staged
plaintext takes beside the decode of the same call.
A random 8-byte pattern is planted PLANTED times, every 64th copy across a frame boundary; the archive is written on the device and
searched whole with the default staging window. Per run:
  decode ms   ZraHipGetKernelStats (HIP events of the decode passes: existing code, the yardstick)
  scan ms     ZraHipDebugSearchScanMs (HIP events around the count / prefix scan / fill / carry launches, summed over the passes)
  wall ms     host time over the call, with a device synchronise on both sides
One warm-up call, then RUNS calls; median / min / max of each. The match count is printed beside the number planted, and the offsets
are compared with a scan of the same content on the CPU (bytes.find). A count-only search (capacity 0: no fill launch) and a search
for a frequent 1-byte pattern (counted with torch on the content) are timed the same way.
Usage: gpu_search.py [GiB, default 1] [runs, default 7]"""
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
N = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 1 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
fs, PLANTED = 65536, 4096
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat(N // len(base) + 2)[:N].contiguous()
rng = np.random.RandomState(17)
needle = bytes(rng.randint(0, 256, size=8).astype(np.uint8))
frames = (N + fs - 1) // fs
places = np.sort(rng.choice(N // 4096 - 2, size=PLANTED, replace=False).astype(np.int64) * 4096 + 100)
across = (places[::64] // fs + 1) * fs - 3                                    # three bytes in front of a frame boundary
places[::64] = across
places = np.unique(places)
d_needle = torch.tensor(list(needle), dtype=torch.uint8, device=dev)
idx = torch.from_numpy(places).to(dev)
for k in range(8):
    d_in[idx + k] = d_needle[k]
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
common = bytes([int(base[12345])])
n_common = int((d_in == common[0]).sum().item())
host = d_in.cpu().numpy().tobytes()
del d_in
truth, p = [], host.find(needle)
while p >= 0:
    truth.append(p)
    p = host.find(needle, p + 1)
del host


def spread(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def timed(name, pattern, cap):
    dec, scan, wall = [], [], []
    for r in range(RUNS + 1):                                                  # the first call is the warm-up (scratch is allocated in it)
        torch.cuda.synchronize()
        t = time.perf_counter()
        n, at = eng.search(d_arc.data_ptr(), asz, pattern, max_matches=cap)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            dec.append(eng.kernel_stats()["dec_ms"]); scan.append(eng.search_scan_ms()); wall.append(t * 1e3)
    res = dict(pattern_bytes=len(pattern), capacity=cap, matches=n, stats=eng.search_stats(), decode_ms=spread(dec), scan_ms=spread(scan), wall_ms=spread(wall),
               scan_over_decode=round(spread(scan)["median"] / spread(dec)["median"], 3),
               scan_gib_s=round(N / (1 << 30) / (spread(scan)["median"] * 1e-3), 1))
    print(name, json.dumps(res), flush=True)
    return n, at


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, frames=frames, level=3, planted=len(places), runs=RUNS)), flush=True)
n, at = timed("planted", needle, 1 << 16)
print("planted: %d matches, %d planted, %d found by the CPU scan; offsets equal to the CPU scan's: %s" % (n, len(places), len(truth), at == truth), flush=True)
assert n == len(truth) and at == truth
n, at = timed("planted_count_only", needle, 0)
assert n == len(truth) and at == []
n, at = timed("one_byte_frequent", common, 1 << 20)
print("one_byte_frequent: %d matches, %d counted on the content" % (n, n_common), flush=True)
assert n == n_common
