"""bring-up: ZraHipGrepArchiveWhere beside ZraHipGrepArchive on the log-like archive of gpu_grep.py (1 GiB of text lines in 64 KiB
frames at level 3, newline delimiter, one pass): what carrying a 64-bit pattern set per record costs on top of the grep's one bit.
The content and the patterns are gpu_grep.py's, K in {1, 8, 64}. Per K and variant one warm-up call, then RUNS calls: the median of
ZraHipDebugGrepScanMs, max - min as the spread, and the median decode ms (ZraHipGetKernelStats). Variants:
  plain   ZraHipGrepArchive (any pattern)
  any     the new call with the one clause {0, all patterns, 0}: the same records as `plain`, checked
  pred    the new call with a realistic predicate: all = patterns 0 and 1, none = pattern 2, any = the rest (K >= 4); K = 1: all = {0}
A last row, K = "dense", takes 8 patterns of one and two common letters, so that nearly every lane of every trip hits: the trip
reduction's worst case. --tree DIR imports zra_amd from another checkout's root (a build of the parent commit, or one built with -DZRA_GREPW_SCAN_FROM=0 or =65): with a
tree that lacks the new call only `plain` runs. One JSON line per (K, variant).
Usage: gpu_grep_where.py [GiB, default 1] [runs, default 5] [--tree DIR]"""
import json
import os
import sys

import numpy as np

args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--tree" in args:
    i = args.index("--tree")
    ROOT = os.path.abspath(args[i + 1])
    del args[i:i + 2]
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import zra_amd as Z  # noqa: E402

dev = torch.device("cuda", 0)
N = int(float(args[0]) * (1 << 30)) if len(args) > 0 else 1 << 30
RUNS = int(args[1]) if len(args) > 1 else 5
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
HAS_WHERE = hasattr(Z, "check_record_clauses")


def timed(call):
    """(result of the last call, median and spread of the scan ms, median decode ms); the first call is the warm-up"""
    dec, scan = [], []
    for r in range(RUNS + 1):
        torch.cuda.synchronize()
        res = call()
        torch.cuda.synchronize()
        if r:
            dec.append(eng.kernel_stats()["dec_ms"]); scan.append(eng.grep_scan_ms())
    return res, dict(scan_ms=round(sorted(scan)[len(scan) // 2], 3), spread_ms=round(max(scan) - min(scan), 3), decode_ms=round(sorted(dec)[len(dec) // 2], 3))


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, where=HAS_WHERE, device=torch.cuda.get_device_name(0))), flush=True)
DENSE = [b"e", b"t", b"a", b" ", b"0", b"re", b"es", b"1"]
for K in (1, 8, 64, "dense"):
    pats = patterns[:K] if K != "dense" else DENSE
    full = (1 << len(pats)) - 1
    plain, t = timed(lambda: eng.grep(d_arc.data_ptr(), asz, pats, max_records=CAP))
    s = eng.grep_stats()
    print(json.dumps(dict(K=K, variant="plain", records=s["records"], selected=plain[0], matches=s["matches"], **t)), flush=True)
    if not HAS_WHERE:
        continue
    got, t = timed(lambda: eng.grep(d_arc.data_ptr(), asz, pats, max_records=CAP, where=[(0, full, 0)]))
    assert got == plain and eng.grep_stats() == s, (got[0], plain[0])
    print(json.dumps(dict(K=K, variant="any", selected=got[0], **t)), flush=True)
    pred = [(0b011, full & ~0b111, 0b100)] if len(pats) >= 4 else [(1, 0, 0)]
    got, t = timed(lambda: eng.grep(d_arc.data_ptr(), asz, pats, max_records=CAP, where=pred))
    print(json.dumps(dict(K=K, variant="pred", clauses=pred, selected=got[0], **t)), flush=True)
