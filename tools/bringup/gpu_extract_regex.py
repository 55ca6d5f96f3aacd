"""bring-up: ZraHipExtractRecordsRegex beside ZraHipGrepArchiveRegex on the log-like archive of gpu_grep_regex.py (text lines in 64 KiB
frames at level 3, newline delimiter, one pass): what keeping the bytes of the selected records costs on top of listing them, and
what a caller pays today for the same bytes (one regex grep, then one ZraHipDecompressRABatch of the listed ranges under
ZRA_HIP_OPT_RA_WHOLE_FRAMES, which decodes the touched frames again). Rows: gpu_grep_regex.py's expression table, two rows of known
selection (0.1 %: the lines whose milliseconds are .123; 10 %: the lines whose seconds end in 7) and one inverted row. Per row one
warm-up call and then RUNS calls of each; the median of each figure, and max - min of the walls as their spread:
  extract_ms       ZraHipDebugExtractMs of the new call (count, scan, copy)
  grep_scan_ms     ZraHipDebugGrepScanMs of ZraHipGrepArchiveRegex with the same arguments
  decode_ms        ZraHipGetKernelStats of the new call (HIP events of its decode pass)
  wall_ms          host time over the new call, with a device synchronise on both sides
  two_call_ms      host time over the regex grep and the batch that fetches the listed ranges
                   (the host work a caller has to do between the two is inside it: the destination offsets d_i are a cumsum
                   of the listed sizes). The batch is one range per selected record, so the rows that select more than
                   TWO_CALL_FULL_RUNS_BELOW records time the two calls ONCE behind the warm-up (two_call_runs says how often)
The packed bytes are compared with the batch's output (record i at d_i; the delimiter bytes are the extract's own).
  nodelim          the worst case: content without a delimiter (delimiter byte 0x00), every tile one head; NODELIM_MIB of the content
One JSON line per row. Usage: gpu_extract_regex.py [GiB, default 1] [runs, default 5]"""
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
NODELIM_MIB = 64
TWO_CALL_FULL_RUNS_BELOW = 2_000_000
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
n_lines = N // len(base) * base.count(b"\n") + base[:N % len(base)].count(b"\n") + 1
CAP = n_lines + 16                                                             # every record can be listed
rec = np.zeros((CAP, 2), dtype=np.uint64)
p_rec = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
d_out = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the extract's packed bytes
d_two = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)              # the batch's answers, at the same offsets


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, figures, runs):
    """(median, spread) of the wall ms and the median of every figure; the first call is the warm-up (scratch is allocated in it)"""
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
    return med(wall), round(max(wall) - min(wall), 3), {k: med(v) for k, v in fig.items()}


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, lines=n_lines, device=torch.cuda.get_device_name(0))), flush=True)
ROWS = (("literal", b"timeout", False), ("status", b" (WARN|ERROR) req=[0-9a-f]+ .*timeout", False), ("anchored", b"^2026-03-0[1-3] .*ms$", False),
        ("count", b"[a-z]{9,} [a-z]{2}$", False), ("empty", b"^$", False), ("0.1%", b"\\.123 ", False), ("10%", b"7\\.[0-9]{3} ", False), ("inverted", b"\\.123 ", True))
for name, expr, inv in ROWS:
    sizes = (ctypes.c_uint32 * 1)(len(expr))
    mode = 1 if inv else 0
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def extract():
        eng._order()
        st = L.ZraHipExtractRecordsRegex(eng.h, d_arc.data_ptr(), asz, expr, sizes, 1, 0, 0x0A, mode, 0, MAXU64, 0, None, 0, ctypes.byref(n), d_out.data_ptr(),
                                         d_out.numel(), ctypes.byref(ds)).tup()
        assert st == (0, 0), st

    def grep():
        eng._order()
        st = L.ZraHipGrepArchiveRegex(eng.h, d_arc.data_ptr(), asz, expr, sizes, 1, 0, 0x0A, mode, 0, MAXU64, 0, p_rec, CAP, ctypes.byref(n)).tup()
        assert st == (0, 0) and n.value <= CAP, (st, n.value)

    def two_calls():
        grep()
        k = n.value
        if k == 0:
            return
        at = np.zeros(k, dtype=np.uint64)
        np.cumsum(rec[:k - 1, 1] + np.uint64(1), out=at[1:])                    # d_i, as the extract packs them
        eng.decompress_ra_batch(d_arc.data_ptr(), asz, d_two.data_ptr(), np.ascontiguousarray(rec[:k, 0]), np.ascontiguousarray(rec[:k, 1]), at)

    wall_x, spread_x, fx = timed(extract, dict(extract_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
    sx = eng.extract_stats()
    _, _, fg = timed(grep, dict(grep_scan_ms=eng.grep_scan_ms), RUNS)
    row = dict(row=name, records=sx["records"], selected=sx["selected"], packed_bytes=sx["packed_bytes"], matches=sx["matches"], **fx, **fg, wall_ms=wall_x,
               wall_spread_ms=spread_x, over_grep_scan=round(fx["extract_ms"] / fg["grep_scan_ms"], 3))
    before = L.ZraHipGetOptions()
    L.ZraHipSetOptions(before | WHOLE_FRAMES)
    try:
        d_two.zero_()
        row["two_call_runs"] = RUNS if sx["selected"] < TWO_CALL_FULL_RUNS_BELOW else 1
        row["two_call_ms"], row["two_call_spread_ms"], _ = timed(two_calls, {}, row["two_call_runs"])
        row["wall_over_two_calls"] = round(wall_x / row["two_call_ms"], 3)
        # the same bytes: the batch leaves the delimiter places alone, so put the delimiters there and compare everything
        k = n.value
        assert k == sx["selected"], (k, sx)
        if k:
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

# the accepted worst case: no delimiter in the content, every tile one head
M = min(N, NODELIM_MIB << 20)
expr = b"timeout$"
sizes = (ctypes.c_uint32 * 1)(len(expr))
n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)


def nodelim():
    eng._order()
    st = L.ZraHipExtractRecordsRegex(eng.h, d_arc.data_ptr(), asz, expr, sizes, 1, 0, 0, 1, 0, M, 0, None, 0, ctypes.byref(n), d_out.data_ptr(), d_out.numel(),
                                     ctypes.byref(ds)).tup()
    assert st == (0, 0), st


wall, spread, f = timed(nodelim, dict(extract_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
_, _, fg = timed(lambda: eng.grep_regex(d_arc.data_ptr(), asz, [expr], delimiter=0, invert=True, length=M, max_records=16), dict(grep_scan_ms=eng.grep_scan_ms), RUNS)
print(json.dumps(dict(row="nodelim", content_bytes=M, selected=n.value, packed_bytes=ds.value, wall_ms=wall, wall_spread_ms=spread, **f, **fg)), flush=True)
