"""bring-up: ZraHipExtractRecordsWhere beside ZraHipExtractRecords and ZraHipGrepArchiveWhere on the log-like archive of gpu_grep.py
(text lines in 64 KiB frames at level 3, newline delimiter, one pass): what carrying a pattern set costs the extract, what keeping the
bytes costs the grep with a predicate, and what a caller pays today for the same bytes (one ZraHipGrepArchiveWhere, then one
ZraHipDecompressRABatch of the listed ranges under ZRA_HIP_OPT_RA_WHOLE_FRAMES, which decodes the touched frames again). The content
and the patterns are gpu_grep_where.py's. Per row one warm-up call and then RUNS calls of each, in one process; the median of each
figure and max - min as its spread:
  K = 1, 8, 64   the one clause {0, all patterns, 0}: extract_where_ms (ZraHipDebugExtractMs of the new call) beside extract_ms (the
                 same of ZraHipExtractRecords, same arguments); the packed bytes and both words compared
  K = "d"        64 patterns under gpu_grep_where.py's realistic predicate (all = patterns 0 and 1, none = pattern 2, any = the rest)
  K = "dense"    8 patterns of one and two common letters under the same shape of predicate: nearly every lane of every trip hits
                 for both: extract_where_ms beside grep_where_ms (ZraHipDebugGrepScanMs of ZraHipGrepArchiveWhere, same arguments)
  every row      wall_ms: host time over the new call, a device synchronise on both sides; two_call_ms: the same over the grep with
                 the predicate and the batch that fetches the listed ranges (the cumsum of the destination offsets is inside it).
                 The batch is one range per selected record, so rows that select more than TWO_CALL_FULL_RUNS_BELOW records time
                 the two calls ONCE behind the warm-up. Where the batch accepts the list the bytes are compared.
--tree DIR imports zra_amd from another checkout's root (a build of the parent commit): a tree that lacks the new call runs the
baselines only (extract_ms, grep_where_ms), with the same content, patterns and arguments. One JSON line per row.
Usage: gpu_extract_where.py [GiB, default 1] [runs, default 5] [--tree DIR]"""
import ctypes
import json
import os
import sys
import time

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
TWO_CALL_FULL_RUNS_BELOW = 2_000_000
WHOLE_FRAMES = 8                                                               # ZRA_HIP_OPT_RA_WHOLE_FRAMES
MAXU64 = (1 << 64) - 1
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
L = Z.load()
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
n_lines = N // len(base) * base.count(b"\n") + base[:N % len(base)].count(b"\n") + 1
CAP = n_lines + 16                                                             # every record can be listed
rec = np.zeros((CAP, 2), dtype=np.uint64)
p_rec = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
d_out = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the new call's packed bytes
d_two = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the plain extract's, then the batch's answers
HAS_NEW = hasattr(L, "ZraHipExtractRecordsWhere")
DENSE = [b"e", b"t", b"a", b" ", b"0", b"re", b"es", b"1"]


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, figures, runs):
    """(median, spread) of the wall ms, and per figure its median and spread; the first call is the warm-up (scratch is allocated in it)"""
    wall, fig = [], {k: [] for k in figures}
    for r in range(runs + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3)
            for k, f in figures.items():
                fig[k].append(f())
    out = {k: med(v) for k, v in fig.items()}
    out.update({k + "_spread": round(max(v) - min(v), 3) for k, v in fig.items()})
    return med(wall), round(max(wall) - min(wall), 3), out


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, lines=n_lines, new_call=HAS_NEW,
                      device=torch.cuda.get_device_name(0))), flush=True)
for K in (1, 8, 64, "d", "dense"):
    pats = DENSE if K == "dense" else patterns[:64 if K == "d" else K]
    full = (1 << len(pats)) - 1
    where = [(0b011, full & ~0b111, 0b100)] if K in ("d", "dense") else [(0, full, 0)]
    blob = b"".join(pats)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    cl = (ctypes.c_uint64 * 3)(*where[0])
    n, ds, n2, ds2 = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def extract_where():
        eng._order()
        st = L.ZraHipExtractRecordsWhere(eng.h, d_arc.data_ptr(), asz, blob, sizes, len(pats), 0, 0x0A, 0, cl, 1, 0, MAXU64, 0, None, 0, ctypes.byref(n), d_out.data_ptr(),
                                         d_out.numel(), ctypes.byref(ds)).tup()
        assert st == (0, 0), st

    def extract_plain():
        eng._order()
        st = L.ZraHipExtractRecords(eng.h, d_arc.data_ptr(), asz, blob, sizes, len(pats), 0x0A, 0, 0, MAXU64, 0, None, 0, ctypes.byref(n2), d_two.data_ptr(), d_two.numel(),
                                    ctypes.byref(ds2)).tup()
        assert st == (0, 0), st

    def grep_where():
        eng._order()
        st = L.ZraHipGrepArchiveWhere(eng.h, d_arc.data_ptr(), asz, blob, sizes, len(pats), 0, 0x0A, 0, cl, 1, 0, MAXU64, 0, p_rec, CAP, ctypes.byref(n2)).tup()
        assert st == (0, 0) and n2.value <= CAP, (st, n2.value)

    def two_calls():
        grep_where()
        k = n2.value
        if k == 0:
            return
        at = np.zeros(k, dtype=np.uint64)
        np.cumsum(rec[:k - 1, 1] + np.uint64(1), out=at[1:])                    # d_i, as the extract packs them
        eng.decompress_ra_batch(d_arc.data_ptr(), asz, d_two.data_ptr(), np.ascontiguousarray(rec[:k, 0]), np.ascontiguousarray(rec[:k, 1]), at)

    row = dict(K=K, clauses=where)
    if HAS_NEW:
        wall, spread, f = timed(extract_where, dict(extract_where_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
        sx = eng.extract_stats()
        row.update(records=sx["records"], selected=sx["selected"], packed_bytes=sx["packed_bytes"], matches=sx["matches"], wall_ms=wall, wall_spread_ms=spread, **f)
    if K not in ("d", "dense"):
        _, _, f = timed(extract_plain, dict(extract_ms=eng.extract_ms), RUNS)
        row.update(f)
        if HAS_NEW:
            assert (n.value, ds.value) == (n2.value, ds2.value) and torch.equal(d_out[:ds.value], d_two[:ds.value]), "the plain predicate is not the plain extract"
            row.update(same_as_plain=True, over_extract=round(row["extract_where_ms"] / f["extract_ms"], 3))
    _, _, f = timed(grep_where, dict(grep_where_ms=eng.grep_scan_ms), RUNS)
    row.update(f)
    if HAS_NEW:
        row["over_grep_where"] = round(row["extract_where_ms"] / f["grep_where_ms"], 3)
        before = L.ZraHipGetOptions()
        L.ZraHipSetOptions(before | WHOLE_FRAMES)
        try:
            d_two.zero_()
            row["two_call_runs"] = RUNS if row["selected"] < TWO_CALL_FULL_RUNS_BELOW else 1
            row["two_call_ms"], row["two_call_spread_ms"], _ = timed(two_calls, {}, row["two_call_runs"])
            row["wall_over_two_calls"] = round(row["wall_ms"] / row["two_call_ms"], 3)
            # the same bytes: the batch leaves the delimiter places alone, so put the delimiters there and compare everything
            k = n2.value
            assert k == row["selected"], (k, row)
            if k:
                ends = torch.from_numpy((np.cumsum(rec[:k, 1] + np.uint64(1)) - np.uint64(1)).astype(np.int64)).to(dev)
                d_two[ends] = 0x0A
            assert torch.equal(d_two[:row["packed_bytes"]], d_out[:row["packed_bytes"]]), "the packed bytes differ from the batch's"
            row["same_bytes"] = True
        except Z.ZraError as e:
            row["two_call_ms"] = None
            row["two_call_error"] = str(e)
        finally:
            L.ZraHipSetOptions(before)
    print(json.dumps(row), flush=True)
