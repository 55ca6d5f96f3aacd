"""bring-up: ZraHipSearchArchiveMulti beside K calls of ZraHipSearchArchive on a log-like archive (level 3, 64 KiB frames): what one
decode pass that scans for K patterns costs, and what the K passes it replaces cost.
The content is lines of text: a timestamp, a level, a request id of 16 hex digits and a message of dictionary words. The patterns are
K in {1, 4, 16, 64} strings of 8 to 32 bytes cut from lines of the content (so every one occurs), the same strings for both routes.
Per K and route, one warm-up call and then RUNS calls, the median of each:
  wall ms     host time over the call(s), with a device synchronise on both sides
  decode ms   ZraHipGetKernelStats (HIP events of the decode passes; summed over the K single calls)
  scan ms     ZraHipDebugSearchMultiScanMs / ZraHipDebugSearchScanMs (summed over the K single calls)
  survivors   the share of the positions that passed the two-byte filter (multi only)
The matches of the two routes are compared: merged and sorted, the K single lists are the multi list.
Usage: gpu_msearch.py [GiB, default 1] [runs, default 3]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import zra_amd as Z  # noqa: E402

dev = torch.device("cuda", 0)
N = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 1 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
fs = 65536
rng = np.random.RandomState(23)
WORDS = ("request accepted rejected timeout retry upstream cache miss hit user session token expired renewed shard replica lagging "
         "caught up compaction started finished bytes written read latency ms queue depth worker idle busy connection reset by peer").split()
LEVELS = ["INFO", "INFO", "INFO", "DEBUG", "WARN", "ERROR"]


def log_block(n_bytes, t0):
    out, size, t = [], 0, t0
    while size < n_bytes:
        t += int(rng.randint(1, 900))
        line = "2026-03-%02d %02d:%02d:%02d.%03d %s req=%016x %s\n" % (
            1 + t // 86400000 % 28, t // 3600000 % 24, t // 60000 % 60, t // 1000 % 60, t % 1000, LEVELS[rng.randint(len(LEVELS))],
            int(rng.randint(0, 1 << 62)), " ".join(WORDS[i] for i in rng.randint(0, len(WORDS), size=int(rng.randint(3, 12)))))
        out.append(line); size += len(line)
    return "".join(out).encode()[:n_bytes]


base = log_block(8 << 20, 0)                                                   # 8 MiB of distinct lines, repeated to N bytes
d_base = torch.from_numpy(np.frombuffer(base, dtype=np.uint8).copy()).to(dev)
d_in = d_base.repeat(N // len(base) + 1)[:N].contiguous()
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
del d_in
lines = base[:1 << 20].split(b"\n")[1:-1]
patterns = []
while len(patterns) < 64:
    line = lines[int(rng.randint(len(lines)))]
    m = int(rng.randint(8, 33))
    at = int(rng.randint(20, max(21, len(line) - m)))                          # behind the date: a request id, a level, words
    if len(line[at:at + m]) == m and line[at:at + m] not in patterns:
        patterns.append(line[at:at + m])
CAP = 1 << 20


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS)), flush=True)
for K in (1, 4, 16, 64):
    pats = patterns[:K]
    wall, dec, scan = [], [], []
    for r in range(RUNS + 1):                                                  # the first call is the warm-up (scratch is allocated in it)
        torch.cuda.synchronize()
        t = time.perf_counter()
        n, listed, per = eng.search_multi(d_arc.data_ptr(), asz, pats, max_matches=CAP)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(eng.kernel_stats()["dec_ms"]); scan.append(eng.search_multi_scan_ms())
    ms = eng.search_multi_stats()
    multi = dict(K=K, route="multi", matches=n, wall_ms=med(wall), decode_ms=med(dec), scan_ms=med(scan), survivor_share=round(ms["survivors"] / N, 5))
    print(json.dumps(multi), flush=True)
    wall, dec, scan = [], [], []
    for r in range(RUNS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        d_ms = s_ms = 0.0
        singles = []
        for p in pats:
            singles.append(eng.search(d_arc.data_ptr(), asz, p, max_matches=CAP))
            d_ms += eng.kernel_stats()["dec_ms"]; s_ms += eng.search_scan_ms()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(d_ms); scan.append(s_ms)
    total = sum(k for k, _ in singles)
    print(json.dumps(dict(K=K, route="K singles", matches=total, wall_ms=med(wall), decode_ms=med(dec), scan_ms=med(scan),
                          multi_over_singles=round(multi["wall_ms"] / med(wall), 3))), flush=True)
    assert total == n and per == [k for k, _ in singles], (total, n)
    if n <= CAP:
        assert listed == sorted((o, i) for i, (_, at) in enumerate(singles) for o in at)
