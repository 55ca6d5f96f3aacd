"""bring-up: ZraHipExtractRecords beside ZraHipGrepArchive on the log-like archive of gpu_grep.py (level 3, 64 KiB frames, one pass):
what keeping the bytes of the selected records costs on top of listing them, and what a caller pays today for the same bytes (one
grep, then one ZraHipDecompressRABatch of the listed ranges under ZRA_HIP_OPT_RA_WHOLE_FRAMES, which decodes the touched frames again).
The content is gpu_grep.py's (lines of text: a timestamp, a level, a request id of 16 hex digits, dictionary words). Three selections:
  0.1%      the lines whose milliseconds are ".123 "
  10%       the lines whose seconds end in 7 ("7.")
  inverted  the lines that do NOT hold ".123 " (nearly all: the copy moves about the whole content)
each with K = 1 pattern and with K = 64 (the pattern above and the 16-digit request ids of 63 lines, which add one line in every
8 MiB each: the selection stays what it is, the filter has 64 patterns to test). Per row one warm-up call and then RUNS calls of each, the median of each:
  extract_ms       ZraHipDebugExtractMs (count, scan, copy, carry)
  grep_scan_ms     ZraHipDebugGrepScanMs of the grep with the same arguments
  decode_ms        ZraHipGetKernelStats of the extract (HIP events of its decode pass)
  extract_wall_ms  host time over the extract, with a device synchronise on both sides
  two_call_ms      host time over the grep and the batch that fetches the listed ranges
The packed bytes are compared with the batch's output (record i at d_i; the delimiter bytes are the extract's own).
Usage: gpu_extract.py [GiB, default 1] [runs, default 5]"""
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

dev = torch.device("cuda", 0)
N = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 1 << 30
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
fs = 65536
rng = np.random.RandomState(23)
WORDS = ("request accepted rejected timeout retry upstream cache miss hit user session token expired renewed shard replica lagging "
         "caught up compaction started finished bytes written read latency ms queue depth worker idle busy connection reset by peer").split()
LEVELS = ["INFO", "INFO", "INFO", "DEBUG", "WARN", "ERROR"]
MAXU64 = (1 << 64) - 1
WHOLE_FRAMES = 8                                                               # ZRA_HIP_OPT_RA_WHOLE_FRAMES


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
cuts = []
while len(cuts) < 63:
    rid = lines[int(rng.randint(len(lines)))].split(b"req=")[1][:16]            # a request id: one line in every 8 MiB
    if rid not in cuts:
        cuts.append(rid)
n_lines = N // len(base) * base.count(b"\n") + base[:N % len(base)].count(b"\n") + 1
CAP = n_lines + 16                                                             # every record can be listed
rec = np.zeros((CAP, 2), dtype=np.uint64)
p_rec = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
d_out = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the extract's packed bytes
d_two = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the batch's answers, at the same offsets


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, figures, runs):
    """medians of the wall ms and of every figure; the first call is the warm-up (scratch is allocated in it)"""
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
    return med(wall), {k: med(v) for k, v in fig.items()}


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, lines=n_lines, device=torch.cuda.get_device_name(0))), flush=True)
for name, first, inv in (("0.1%", b".123 ", False), ("10%", b"7.", False), ("inverted", b".123 ", True)):
    for K in (1, 64):
        pats = [first] + cuts[:K - 1]
        blob = b"".join(pats)
        sizes = (ctypes.c_uint32 * K)(*(len(p) for p in pats))
        mode = 1 if inv else 0
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def extract():
            eng._order()
            st = L.ZraHipExtractRecords(eng.h, d_arc.data_ptr(), asz, blob, sizes, K, 0x0A, mode, 0, MAXU64, 0, None, 0, ctypes.byref(n), d_out.data_ptr(),
                                        d_out.numel(), ctypes.byref(ds)).tup()
            assert st == (0, 0), st

        def grep():
            eng._order()
            st = L.ZraHipGrepArchive(eng.h, d_arc.data_ptr(), asz, blob, sizes, K, 0x0A, mode, 0, MAXU64, 0, p_rec, CAP, ctypes.byref(n)).tup()
            assert st == (0, 0) and n.value <= CAP, (st, n.value)

        def two_calls():
            grep()
            k = n.value
            if k == 0:
                return
            at = np.zeros(k, dtype=np.uint64)
            np.cumsum(rec[:k - 1, 1] + np.uint64(1), out=at[1:])                # d_i, as the extract packs them
            eng.decompress_ra_batch(d_arc.data_ptr(), asz, d_two.data_ptr(), np.ascontiguousarray(rec[:k, 0]), np.ascontiguousarray(rec[:k, 1]), at)

        wall_x, fx = timed(extract, dict(extract_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
        sx = eng.extract_stats()
        _, fg = timed(grep, dict(grep_scan_ms=eng.grep_scan_ms), RUNS)
        row = dict(selection=name, K=K, records=sx["records"], selected=sx["selected"], packed_bytes=sx["packed_bytes"], matches=sx["matches"], **fx, **fg,
                   extract_wall_ms=wall_x, over_grep_scan=round(fx["extract_ms"] / fg["grep_scan_ms"], 3),
                   extract_over_decode=round(fx["extract_ms"] / fx["decode_ms"], 3))
        before = L.ZraHipGetOptions()
        L.ZraHipSetOptions(before | WHOLE_FRAMES)
        try:
            d_two.zero_()
            row["two_call_ms"], _ = timed(two_calls, {}, RUNS if not inv else 1)
            row["wall_over_two_calls"] = round(wall_x / row["two_call_ms"], 3)
            # the same bytes: the batch leaves the delimiter places alone, so put the delimiters there and compare everything
            k = n.value
            assert k == sx["selected"], (k, sx)
            ends = torch.from_numpy((np.cumsum(rec[:k, 1] + np.uint64(1)) - np.uint64(1)).astype(np.int64)).to(dev)
            d_two[ends] = 0x0A
            assert torch.equal(d_two[:sx["packed_bytes"]], d_out[:sx["packed_bytes"]]), "the packed bytes differ from the batch's"
            row["same_bytes"] = True
        except Z.ZraError as e:
            row["two_call_ms"] = None
            row["two_call_error"] = str(e)
        finally:
            L.ZraHipSetOptions(before)
        print(json.dumps(row), flush=True)
