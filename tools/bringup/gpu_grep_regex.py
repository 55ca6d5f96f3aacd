"""bring-up: ZraHipGrepArchiveRegex beside ZraHipGrepArchive on the log-like archive of gpu_grep.py (text lines in 64 KiB frames at
level 3, newline delimiter, one pass): what carrying a DFA state per record costs beside the grep's one bit, and the accepted worst
case. Per row one warm-up call, then RUNS calls: the median of ZraHipDebugGrepScanMs, max - min as the spread, and the median decode
ms (ZraHipGetKernelStats). Rows:
  plain      ZraHipGrepArchive with the literal "timeout": the family's scan on the same bytes
  literal    the new call with the expression `timeout`: the same records as `plain`, checked
  status     `status=5[0-9]+ .*timeout`-like: ` (WARN|ERROR) req=[0-9a-f]+ .*timeout`
  anchored   `^2026-03-0[1-3] .*ms$`
  count      `took [0-9]{4,}ms$`-like: `[a-z]{9,} [a-z]{2}$`
  empty      `^$`
  nodelim    the worst case: the same call on content without a delimiter (delimiter byte 0x00, which the text never holds): every
             tile is one head, 8,192 dependent map steps on one wave; on NODELIM_MIB of the content only
The scan time does not depend on the expression, only on the bytes and on how the delimiters fall: the rows `literal` .. `empty` say so.
One JSON line per row. Usage: gpu_grep_regex.py [GiB, default 1] [runs, default 5]"""
import json
import os
import sys

import numpy as np

args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import zra_amd as Z  # noqa: E402

dev = torch.device("cuda", 0)
N = int(float(args[0]) * (1 << 30)) if len(args) > 0 else 1 << 30
RUNS = int(args[1]) if len(args) > 1 else 5
NODELIM_MIB = 64
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
CAP = 1 << 20


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


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, device=torch.cuda.get_device_name(0))), flush=True)
plain, t = timed(lambda: eng.grep(d_arc.data_ptr(), asz, [b"timeout"], max_records=CAP))
s = eng.grep_stats()
print(json.dumps(dict(row="plain", records=s["records"], selected=plain[0], **t)), flush=True)
for row, exprs in (("literal", [b"timeout"]), ("status", [b" (WARN|ERROR) req=[0-9a-f]+ .*timeout"]), ("anchored", [b"^2026-03-0[1-3] .*ms$"]), ("count", [b"[a-z]{9,} [a-z]{2}$"]),
                   ("empty", [b"^$"])):
    info = Z.check_regex(exprs)
    got, t = timed(lambda: eng.grep_regex(d_arc.data_ptr(), asz, exprs, max_records=CAP))
    if row == "literal":
        assert got == plain, (got[0], plain[0])
    print(json.dumps(dict(row=row, states=info["states"], classes=info["classes"], selected=got[0], **t)), flush=True)
M = min(N, NODELIM_MIB << 20)
got, t = timed(lambda: eng.grep_regex(d_arc.data_ptr(), asz, [b"timeout$"], delimiter=0, length=M, max_records=CAP))
print(json.dumps(dict(row="nodelim", content_bytes=M, selected=got[0], **t)), flush=True)
