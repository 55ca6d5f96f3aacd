"""bring-up: ZraHipGrepArchive beside ZraHipSearchArchiveMulti on the log-like archive of gpu_msearch.py (level 3, 64 KiB frames): what
the delimiter flag and the segmented reduction over the records cost on top of the multi search's filter.
The content and the patterns are gpu_msearch.py's (lines of text: a timestamp, a level, a request id of 16 hex digits, dictionary
words; strings of 8 to 32 bytes cut from lines of the content), K in {1, 8, 64}, the same archive and the same strings for both calls.
The grep runs with a delimiter that is common (the newline: a record every 100 bytes or so) and with one that never occurs (0x00: the
whole content is one record). Per K, one warm-up call and then RUNS calls of each, the median of each:
  wall ms     host time over the call, with a device synchronise on both sides
  decode ms   ZraHipGetKernelStats (HIP events of the decode passes)
  scan ms     ZraHipDebugGrepScanMs / ZraHipDebugSearchMultiScanMs
  over_multi  grep scan ms / multi search scan ms
The two calls are compared: `matches` of the grep is the multi search's count, and with the newline the selected records are the lines
that hold a listed match.
Usage: gpu_grep.py [GiB, default 1] [runs, default 5]"""
import bisect
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
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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


def timed(call, scan_ms):
    """(result of the last call, medians of wall / decode / scan ms); the first call is the warm-up (scratch is allocated in it)"""
    wall, dec, scan = [], [], []
    for r in range(RUNS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(eng.kernel_stats()["dec_ms"]); scan.append(scan_ms())
    return res, dict(wall_ms=med(wall), decode_ms=med(dec), scan_ms=med(scan))


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, device=torch.cuda.get_device_name(0))), flush=True)
for K in (1, 8, 64):
    pats = patterns[:K]
    (n, listed, per), multi = timed(lambda: eng.search_multi(d_arc.data_ptr(), asz, pats, max_matches=CAP), eng.search_multi_scan_ms)
    print(json.dumps(dict(K=K, call="multi search", matches=n, **multi)), flush=True)
    for name, delim in (("newline", 0x0A), ("absent", 0x00)):
        (k, recs), g = timed(lambda: eng.grep(d_arc.data_ptr(), asz, pats, delimiter=delim, max_records=CAP), eng.grep_scan_ms)
        s = eng.grep_stats()
        print(json.dumps(dict(K=K, call="grep", delimiter=name, records=s["records"], selected=k, matches=s["matches"], **g,
                              over_multi=round(g["scan_ms"] / multi["scan_ms"], 3), scan_over_decode=round(g["scan_ms"] / g["decode_ms"], 3))), flush=True)
        assert s["matches"] == n, (s, n)
        if delim == 0x00:
            assert (k, recs) == (1, [(0, N)]) if n else (k, recs) == (0, [])
        elif n <= CAP and k <= CAP:                                            # every selected record holds a listed match, and the other way round
            starts = [o for o, _ in recs]
            hit = set()
            for o, _ in listed:
                i = bisect.bisect_right(starts, o) - 1
                assert i >= 0 and o < recs[i][0] + recs[i][1], (o, i)
                hit.add(i)
            assert len(hit) == k == len(recs), (len(hit), k)
