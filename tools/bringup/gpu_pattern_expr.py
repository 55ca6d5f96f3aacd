"""bring-up: what the pattern expressions cost (ZraHipSearchArchiveMultiExpr, ZraHipGrepArchiveExpr) beside the literal calls, on the
log-like archive of gpu_msearch.py and gpu_grep.py (level 3, 64 KiB frames, one pass). The content and the literal patterns are
gpu_grep.py's (strings of 8 to 32 bytes cut from lines of the content), K in {1, 8, 64}. Per K and per call (the multi search, and the
grep with the newline as delimiter), one warm-up call and then RUNS calls, the median and the spread (max - min) of the scan
milliseconds (ZraHipDebugSearchMultiScanMs / ZraHipDebugGrepScanMs), the median decode milliseconds of the same passes beside them:
  a  the literal call (syntax 0: Table and the literal kernels)
  b  the same literals, every special byte escaped, through the class kernels (PATTERN_CLASSES): the price of the mechanism
  c  b with PATTERN_FOLD_CASE
  d  expressions: strings cut the same way that hold a digit, their first run of digits as [0-9]... and one other byte as `.`
b must find what a finds, c no less, and d is checked against a CPU scan of the first 8 MiB.
Usage: gpu_pattern_expr.py [GiB, default 1] [runs, default 5] [columns, default abcd]
With ZRA_AMD_ROOT set, zra_amd is imported from that tree: column a of another build of the library (`... 1 5 a`)."""
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.environ.get("ZRA_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import zra_amd as Z  # noqa: E402

dev = torch.device("cuda", 0)
N = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 1 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
COLUMNS = sys.argv[3] if len(sys.argv) > 3 else "abcd"
fs = 65536
rng = np.random.RandomState(23)
WORDS = ("request accepted rejected timeout retry upstream cache miss hit user session token expired renewed shard replica lagging "
         "caught up compaction started finished bytes written read latency ms queue depth worker idle busy connection reset by peer").split()
LEVELS = ["INFO", "INFO", "INFO", "DEBUG", "WARN", "ERROR"]
SPECIAL = b".[]\\*+?{}()|^$-"


def log_block(n_bytes, t0):
    out, size, t = [], 0, t0
    while size < n_bytes:
        t += int(rng.randint(1, 900))
        line = "2026-03-%02d %02d:%02d:%02d.%03d %s req=%016x %s\n" % (
            1 + t // 86400000 % 28, t // 3600000 % 24, t // 60000 % 60, t // 1000 % 60, t % 1000, LEVELS[rng.randint(len(LEVELS))],
            int(rng.randint(0, 1 << 62)), " ".join(WORDS[i] for i in rng.randint(0, len(WORDS), size=int(rng.randint(3, 12)))))
        out.append(line); size += len(line)
    return "".join(out).encode()[:n_bytes]


def esc(p):
    return b"".join(b"\\" + bytes([c]) if c in SPECIAL else bytes([c]) for c in p)


base = log_block(8 << 20, 0)                                                   # 8 MiB of distinct lines, repeated to N bytes
d_base = torch.from_numpy(np.frombuffer(base, dtype=np.uint8).copy()).to(dev)
d_in = d_base.repeat(N // len(base) + 1)[:N].contiguous()
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
del d_in
lines = base[:1 << 20].split(b"\n")[1:-1]
patterns, exprs, expr_res = [], [], []
while len(patterns) < 64 or len(exprs) < 64:
    line = lines[int(rng.randint(len(lines)))]
    m = int(rng.randint(8, 33))
    at = int(rng.randint(20, max(21, len(line) - m)))                          # behind the date: a request id, a level, words
    cut = line[at:at + m]
    if len(cut) != m:
        continue
    if len(patterns) < 64 and cut not in patterns:
        patterns.append(cut)
    run = re.search(rb"[0-9]+", cut)
    if len(exprs) < 64 and run:
        dot = next(q for q in (m // 2, m - 1, 0) if not run.start() <= q < run.end())
        parts = [b"[0-9]" if run.start() <= q < run.end() else b"." if q == dot else esc(cut[q:q + 1]) for q in range(m)]
        if b"".join(parts) not in exprs:
            exprs.append(b"".join(parts))
            expr_res.append(re.compile(b"(?=(" + b"".join(parts) + b"))"))     # (the newline is the grep's delimiter: no DOTALL)
CAP = 1 << 20


def stat(v):
    v = sorted(v)
    return round(v[len(v) // 2], 3), round(v[-1] - v[0], 3)


def timed(call, scan_ms):
    """(result of the last call, {scan ms median, its spread, decode ms median, wall ms median}); the first call is the warm-up"""
    wall, dec, scan = [], [], []
    for r in range(RUNS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(eng.kernel_stats()["dec_ms"]); scan.append(scan_ms())
    return res, dict(scan_ms=stat(scan)[0], scan_spread_ms=stat(scan)[1], decode_ms=stat(dec)[0], wall_ms=stat(wall)[0])


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, columns=COLUMNS, device=torch.cuda.get_device_name(0),
                      root=os.path.relpath(ROOT))), flush=True)
P = d_arc.data_ptr()
for K in (1, 8, 64):
    found = {}
    for col in COLUMNS:
        pats, kw = {"a": (patterns[:K], {}), "b": ([esc(p) for p in patterns[:K]], dict(syntax=Z.PATTERN_CLASSES)) if col != "a" else None,
                    "c": ([esc(p) for p in patterns[:K]], dict(syntax=Z.PATTERN_CLASSES | Z.PATTERN_FOLD_CASE)) if col != "a" else None,
                    "d": (exprs[:K], dict(syntax=Z.PATTERN_CLASSES)) if col != "a" else None}[col]
        (n, listed, per), multi = timed(lambda: eng.search_multi(P, asz, pats, max_matches=CAP, **kw), eng.search_multi_scan_ms)
        sm = eng.search_multi_stats()
        print(json.dumps(dict(K=K, column=col, call="multi search", matches=n, survivors_per_position=round(sm["survivors"] / N, 4), **multi)), flush=True)
        (k, recs), g = timed(lambda: eng.grep(P, asz, pats, max_records=CAP, **kw), eng.grep_scan_ms)
        print(json.dumps(dict(K=K, column=col, call="grep", selected=k, matches=eng.grep_stats()["matches"], **g)), flush=True)
        found[col] = (n, per, k)
        if col == "d":                                                         # the first 8 MiB against re, pattern by pattern
            n8, _, per8 = eng.search_multi(P, asz, pats, offset=0, length=len(base), max_matches=0, **kw)
            want = [sum(1 for _ in rx.finditer(base)) for rx in expr_res[:K]]
            assert per8 == want, (per8, want)
    if "a" in found and "b" in found:
        assert found["a"] == found["b"], (found["a"][0], found["b"][0])
    if "b" in found and "c" in found:
        assert found["c"][0] >= found["b"][0] and found["c"][2] >= found["b"][2]
