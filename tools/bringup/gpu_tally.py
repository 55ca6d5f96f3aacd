"""bring-up: ZraHipTallyFields on the log-like archive of gpu_cut.py (level 3, 64 KiB frames, one pass): what counting the distinct
values of a field costs where the cut's text lies, against the cut that produced the text and against what a caller does today. The
content is gpu_cut.py's (8 MiB of distinct lines repeated to the size; cut at spaces: date, time, level, request id, words). Rows:
  level         field 3 of the lines that do NOT hold ".123 " (DESIGN.md §33's case to watch): a handful of values, skewed
  level+words   fields 3,5,6 of every line: about 10^4 values
  request id    field 4 of every line: every value of the 8 MiB once per repetition
  lines         whole lines (a mask of all ones) of the lines whose seconds end in 7
  unique        the primitive alone on a synthetic text of as many 16-digit keys as the archive has lines, all different
Per row one warm call and then RUNS calls, the median of each:
  tally_ms      ZraHipDebugTallyMs (count, insert, mark, sum, scan, emit, copy)
  cut_ms        ZraHipDebugExtractMs of the same call's cut
  decode_ms     ZraHipGetKernelStats of the same call
  wall_ms       host time over the call, with a device synchronise on both sides
and the tally's stats. Then, once, what a caller does today: the cut alone, the copy of its text to the host, and
tools/bringup/host_tally.cpp (one core, std::unordered_map over std::string_view), whose entries are compared with the call's.
--rows NAME runs that one row only (for a kernel trace of its own: `rocprofv3 --kernel-trace --stats -- python ...`); --no-host leaves
the host side out.
Usage: gpu_tally.py [GiB, default 1] [runs, default 5] [--rows NAME] [--no-host]"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
args = sys.argv[1:]
ONLY = None
if "--rows" in args:
    i = args.index("--rows")
    ONLY = args[i + 1]
    del args[i:i + 2]
HOST = "--no-host" not in args
args = [a for a in args if a != "--no-host"]
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
MAX_ENTRIES = 1 << 24


def log_block(n_bytes, t0):
    out, size, t = [], 0, t0
    while size < n_bytes:
        t += int(rng.randint(1, 900))
        line = "2026-03-%02d %02d:%02d:%02d.%03d %s req=%016x %s\n" % (
            1 + t // 86400000 % 28, t // 3600000 % 24, t // 60000 % 60, t // 1000 % 60, t % 1000, LEVELS[rng.randint(len(LEVELS))],
            int(rng.randint(0, 1 << 62)), " ".join(WORDS[i] for i in rng.randint(0, len(WORDS), size=int(rng.randint(3, 12)))))
        out.append(line); size += len(line)
    return "".join(out).encode()[:n_bytes]


def host_lib():
    so = os.path.join(HERE, "host_tally.so")
    if not os.path.exists(so):
        subprocess.check_call(["c++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_tally.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.host_tally.restype = ctypes.c_uint64
    lib.host_tally.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


base = log_block(8 << 20, 0)
d_base = torch.from_numpy(np.frombuffer(base, dtype=np.uint8).copy()).to(dev)
d_in = d_base.repeat(N // len(base) + 1)[:N].contiguous()
eng = Z.Engine(0)
L = Z.load()
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
del d_in
d_work = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)
d_keys = torch.empty(N + (1 << 20), dtype=torch.uint8, device=dev)
entries = np.zeros(3 * MAX_ENTRIES, dtype=np.uint64)
host_entries = np.zeros(3 * MAX_ENTRIES, dtype=np.uint64)
H = host_lib() if HOST else None
E_PTR = entries.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, figures, runs):
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


def wall_of(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def on_host(d_text, size, distinct):
    """the copy of the text to the host and the map over it; are its entries the call's"""
    copy_ms, text = wall_of(lambda: d_text[:size].cpu().numpy())
    nr, ns = ctypes.c_uint64(0), ctypes.c_uint64(0)
    t = time.perf_counter()
    n = H.host_tally(text.ctypes.data, size, bytes([NL]), Z.TALLY_MAX_KEY, host_entries.ctypes.data, MAX_ENTRIES, ctypes.byref(nr), ctypes.byref(ns))
    map_ms = (time.perf_counter() - t) * 1e3
    same = n == distinct and bool((host_entries[:3 * n] == entries[:3 * n]).all())
    return round(copy_ms, 3), round(map_ms, 3), same


print(json.dumps(dict(tree=ROOT, content_bytes=N, archive_bytes=asz, frame_size=fs, level=3, runs=RUNS, device=torch.cuda.get_device_name(0))), flush=True)
ROWS = (("level", [b".123 "], True, 1 << 2), ("level+words", [], False, (1 << 2) | (1 << 4) | (1 << 5)), ("request id", [], False, 1 << 3), ("lines", [b"7."], False, MAXU64))
w = [ctypes.c_uint64(0) for _ in range(5)]
for name, pats, inv, mask in ROWS:
    if ONLY and ONLY != name:
        continue
    blob = b"".join(pats) if pats else None
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats)) if pats else None
    n_sel, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def fields():
        eng._order()
        st = L.ZraHipTallyFields(eng.h, d_arc.data_ptr(), asz, blob, sizes, len(pats), 0, NL, int(inv), SP, mask, 0, MAXU64, 0, d_work.data_ptr(), d_work.numel(),
                                 ctypes.byref(w[4]), 0, E_PTR, MAX_ENTRIES, d_keys.data_ptr(), d_keys.numel(), *(ctypes.byref(x) for x in w[:4])).tup()
        assert st == (0, 0), st

    def cut():
        eng._order()
        st = L.ZraHipCutRecords(eng.h, d_arc.data_ptr(), asz, blob, sizes, len(pats), 0, NL, int(inv), SP, mask, 0, MAXU64, 0, None, 0, ctypes.byref(n_sel), d_work.data_ptr(),
                                d_work.numel(), ctypes.byref(ds)).tup()
        assert st == (0, 0), st

    wall, f = timed(fields, dict(tally_ms=eng.tally_ms, cut_ms=eng.extract_ms, decode_ms=lambda: eng.kernel_stats()["dec_ms"]), RUNS)
    row = dict(row=name, work_bytes=w[4].value, wall_ms=wall, **f, tally_over_cut=round(f["tally_ms"] / f["cut_ms"], 3), **eng.tally_stats())
    if HOST:
        cut_wall, _ = wall_of(cut)
        copy_ms, map_ms, same = on_host(d_work, ds.value, w[1].value)
        row.update(today_cut_wall_ms=round(cut_wall, 3), today_copy_ms=copy_ms, today_map_ms=map_ms, today_ms=round(cut_wall + copy_ms + map_ms, 3), same_entries=same)
    print(json.dumps(row), flush=True)

if not ONLY or ONLY == "unique":
    M = base.count(b"\n") * (N // len(base))                                   # as many keys as the archive has lines
    ids = torch.arange(M, dtype=torch.int64, device=dev) * 0x9E3779B1 + 12345   # (odd multiplier: all different below 2^64)
    text = torch.empty((M, 17), dtype=torch.uint8, device=dev)
    for k in range(16):
        dgt = (ids >> (4 * (15 - k))) & 15
        text[:, k] = torch.where(dgt < 10, dgt + 48, dgt + 87).to(torch.uint8)
    text[:, 16] = NL
    text = text.reshape(-1)
    del ids

    def plain():
        eng._order()
        st = L.ZraHipTallyRecords(eng.h, text.data_ptr(), text.numel(), NL, 0, E_PTR, MAX_ENTRIES, d_keys.data_ptr(), d_keys.numel(),
                                  *(ctypes.byref(x) for x in w[:4])).tup()
        assert st == (0, 0), st

    wall, f = timed(plain, dict(tally_ms=eng.tally_ms), RUNS)
    row = dict(row="unique", work_bytes=text.numel(), wall_ms=wall, **f, **eng.tally_stats())
    if HOST:
        copy_ms, map_ms, same = on_host(text, text.numel(), w[1].value)
        row.update(today_copy_ms=copy_ms, today_map_ms=map_ms, same_entries=same)
    print(json.dumps(row), flush=True)
