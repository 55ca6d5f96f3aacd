"""bring-up: ZraHipGrepArchiveRegexContext beside ZraHipGrepArchiveRegex on the log-like archive of gpu_grep_regex.py (1 GiB of text
lines in 64 KiB frames at level 3, newline delimiter, one pass): what a summary that counts records, the walk backwards and the
pending ranges cost on top of the regex grep's carried state. The content is gpu_grep_regex.py's. Selections: `rare` = the lines whose
request id begins 000 (`req=000[0-9a-f]+ `, about 0.1 %), `tenth` = the lines that hold the word `lagging` (` lag+ing`, the nearest
this corpus has to a tenth), `all` = every line (`^2026-03-[0-9]{2} `). Per selection the regex grep, then the new call with
(after, before) = (0, 0), (2, 2) and (64, 64). Per variant one warm-up call, then RUNS calls: the median of ZraHipDebugGrepScanMs,
max - min as the spread, and the median decode ms. The (0, 0) list is checked against the regex grep's. --tree DIR imports zra_amd
from another checkout's root (a build of the parent commit): with a tree that lacks the new call only `regex` runs. One JSON line per
(selection, variant).
Usage: gpu_grep_regex_context.py [GiB, default 1] [runs, default 5] [--tree DIR]"""
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
CAP = 1 << 20
HAS_CONTEXT = hasattr(Z.Engine, "grep_regex_context")


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


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, context=HAS_CONTEXT, device=torch.cuda.get_device_name(0))), flush=True)
PAIRS = ((0, 0), (2, 2), (64, 64))
for name, exprs in (("rare", [b"req=000[0-9a-f]+ "]), ("tenth", [b" lag+ing"]), ("all", [b"^2026-03-[0-9]{2} "])):
    plain, t = timed(lambda: eng.grep_regex(d_arc.data_ptr(), asz, exprs, max_records=CAP))
    s = eng.grep_stats()
    print(json.dumps(dict(selection=name, variant="regex", records=s["records"], selected=plain[0], matches=s["matches"], **t)), flush=True)
    if not HAS_CONTEXT:
        continue
    for after, before in PAIRS:
        got, t = timed(lambda: eng.grep_regex_context(d_arc.data_ptr(), asz, exprs, before=before, after=after, max_records=CAP))
        c = eng.grep_stats()
        if (after, before) == (0, 0):
            assert (got[0], got[1], [(o, n) for o, n, _ in got[3]]) == (plain[0], plain[0], plain[1]) and c == s, (got[:3], plain[0])
        assert got[1] == plain[0] and c["records"] == s["records"] and c["matches"] == s["matches"], (got[:3], plain[0])
        print(json.dumps(dict(selection=name, variant="context", after=after, before=before, output=got[0], selected=got[1], groups=got[2], listed=c["listed"], **t)), flush=True)
