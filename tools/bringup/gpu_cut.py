"""bring-up: ZraHipCutRecords beside ZraHipExtractRecords on the log-like archive of gpu_extract.py (level 3, 64 KiB frames, one pass):
what packing only the chosen fields costs against packing the whole records of the same selection. The content and the selections
are gpu_extract.py's (0.1 %: the lines whose milliseconds are ".123 "; 10 %: the lines whose seconds end in 7; inverted: the lines
that do NOT hold ".123 "), each with K = 1 and K = 64 patterns. The lines are cut at spaces (date, time, level, request id, words),
under two masks: one field (`3`, the level) and every second field (`1,3,5,...`). Per row one warm call and then RUNS calls, the
median of each:
  cut_ms           ZraHipDebugExtractMs of the cut (count, scan, keep, place, copy, carry)
  extract_ms       the same figure of ZraHipExtractRecords with the same patterns (a row of its own, mask null)
  decode_ms        ZraHipGetKernelStats of the same call (HIP events of its decode pass)
  wall_ms          host time over the call, with a device synchronise on both sides
and the packed sizes of both. The cut's bytes of the first 16 MiB of the content are compared with a host model (numpy: the field
number of every byte from the separators, the selection from the patterns' occurrences).
--tree DIR imports zra_amd from another checkout's root (a build of the parent commit): a tree that lacks the new call runs the
extract's rows only, which are the figures to hold the cut's against.
--rows SELECTION:K runs that one row group only (for a kernel trace of its own: `rocprofv3 --kernel-trace --stats -- python ...`).
Usage: gpu_cut.py [GiB, default 1] [runs, default 5] [--tree DIR] [--rows SELECTION:K]"""
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = sys.argv[1:]
if "--tree" in args:
    i = args.index("--tree")
    ROOT = os.path.abspath(args[i + 1])
    del args[i:i + 2]
ONLY = None
if "--rows" in args:
    i = args.index("--rows")
    ONLY = args[i + 1]
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
MAXU64 = (1 << 64) - 1
NL, SP = 0x0A, 0x20
PREFIX = 16 << 20


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
HAS_NEW = hasattr(L, "ZraHipCutRecords")
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
del d_in
lines = base[:1 << 20].split(b"\n")[1:-1]
cuts = []
while len(cuts) < 63:
    rid = lines[int(rng.randint(len(lines)))].split(b"req=")[1][:16]            # a request id: one line in every 8 MiB
    if rid not in cuts:
        cuts.append(rid)
d_out = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)
prefix = np.frombuffer((base * (PREFIX // len(base) + 1))[:min(PREFIX, N)], dtype=np.uint8)


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, figures, runs):
    """medians of the wall ms and of every figure; the first call is the warm one (scratch is allocated in it)"""
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


def model(pats, inv, mask):
    """the packed bytes of the cut of [0, len(prefix)): the records from the delimiters (the one the range's end cuts included), the
    selection from the patterns' occurrences, a byte's field from the separators in front of it in its record"""
    a = prefix
    text = a.tobytes()
    n = len(a)
    is_d, is_s = a == NL, a == SP
    rec = np.cumsum(is_d) - is_d                                               # the record of every byte, its delimiter included
    n_rec = int(rec[-1]) + 1
    hit = np.zeros(n_rec, dtype=bool)
    for p in pats:
        at = np.fromiter((m.start() for m in re.finditer(b"(?=" + re.escape(p) + b")", text) if m.start() + len(p) <= n), dtype=np.int64)
        hit[rec[at]] = True
    sel = hit != inv
    seps = np.cumsum(is_s) - is_s                                              # separators in front of the byte, in the content
    start = np.concatenate(([0], np.flatnonzero(is_d) + 1))[:n_rec]
    c = seps - seps[np.minimum(start, n - 1)][rec]                             # ... in its record
    field_bit = np.array([(mask >> min(k, 63)) & 1 for k in range(int(c.max()) + 1)], dtype=bool)
    some = np.array([(mask & ((1 << (min(k, 63) + 1)) - 1)) != 0 for k in range(int(c.max()) + 1)], dtype=bool)   # a field 1 .. k + 1 is chosen
    nxt = np.array([(mask >> min(k + 1, 63)) & 1 for k in range(int(c.max()) + 1)], dtype=bool)
    keep = np.where(is_d, True, np.where(is_s, nxt[c] & some[c], field_bit[c])) & sel[rec]
    out = a[keep].tobytes()
    if not is_d[-1] and sel[-1]:
        out += b"\n"
    return out


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, new_call=HAS_NEW, device=torch.cuda.get_device_name(0))),
      flush=True)
EVERY_SECOND = int("55" * 8, 16)
for name, first, inv in (("0.1%", b".123 ", False), ("10%", b"7.", False), ("inverted", b".123 ", True)):
    for K in (1, 64):
        if ONLY and ONLY != "%s:%d" % (name, K):
            continue
        pats = [first] + cuts[:K - 1]
        blob = b"".join(pats)
        sizes = (ctypes.c_uint32 * K)(*(len(p) for p in pats))
        mode = 1 if inv else 0
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def extract():
            eng._order()
            st = L.ZraHipExtractRecords(eng.h, d_arc.data_ptr(), asz, blob, sizes, K, NL, mode, 0, MAXU64, 0, None, 0, ctypes.byref(n), d_out.data_ptr(), d_out.numel(),
                                        ctypes.byref(ds)).tup()
            assert st == (0, 0), st

        wall, f = timed(extract, dict(extract_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
        sx = eng.extract_stats()
        print(json.dumps(dict(call="extract", selection=name, K=K, selected=sx["selected"], packed_bytes=sx["packed_bytes"], wall_ms=wall, **f)), flush=True)
        if not HAS_NEW:
            continue
        for mname, mask in (("3", 1 << 2), ("1,3,5,...", EVERY_SECOND)):
            def cut(length=MAXU64):
                eng._order()
                st = L.ZraHipCutRecords(eng.h, d_arc.data_ptr(), asz, blob, sizes, K, 0, NL, mode, SP, mask, 0, length, 0, None, 0, ctypes.byref(n), d_out.data_ptr(),
                                        d_out.numel(), ctypes.byref(ds)).tup()
                assert st == (0, 0), st

            wall, fc = timed(cut, dict(cut_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
            sc = eng.extract_stats()
            assert sc["selected"] == sx["selected"], (sc, sx)
            row = dict(call="cut", selection=name, K=K, fields=mname, selected=sc["selected"], packed_bytes=sc["packed_bytes"], wall_ms=wall, **fc,
                       over_extract=round(fc["cut_ms"] / f["extract_ms"], 3), cut_over_decode=round(fc["cut_ms"] / fc["decode_ms"], 3))
            cut(len(prefix))
            want = model(pats, inv, mask)
            row["same_bytes_16MiB"] = ds.value == len(want) and d_out[:ds.value].cpu().numpy().tobytes() == want
            print(json.dumps(row), flush=True)
