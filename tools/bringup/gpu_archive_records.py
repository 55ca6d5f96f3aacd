"""bring-up: the record index through an archive handle (ZraHipArchiveIndexRecords, ZraHipArchiveLocateRecords,
ZraHipArchiveReadRecords) beside the plain engine calls, on an archive whose frames are resident in the handle's cache to 0 %, 50 %
(every other frame) and 100 %: what a whole-frame sweep fed from the arena costs beside one fed by the decoder, and what the read's
byte fetch costs as a read of the handle.
The content is the bench's (bench.synth_corpus: log-like lines, numeric rows, binary-ish records), level 3, 64 KiB frames, delimiter
0x0A, the cache as large as the content. Three request sets, tools/bringup/gpu_records.py's: 100 consecutive records, 10,000 and
1,000,000 uniformly drawn ones. Per case one warm-up call and then RUNS calls, medians (and the extremes of the wall time) of
  wall ms     host time over the call, with a device synchronise on both sides
  decode ms   ZraHipGetKernelStats (HIP events of the last decode of the call: the read's is its byte fetch)
  own ms      ZraHipDebugIndexRecordsMs / ZraHipDebugLocateRecordsMs / ZraHipDebugReadRecordsMs
  stage ms    ZraHipDebugArchiveRecordStageMs (the job-split and stage-from-cache launches), and the bytes staged per second from it
Cases: the plain calls; the handle at 0 %, 50 % and 100 %. The residency is set by dropping the cache and reading one byte of the
frames that are to be resident: once in front of an index or a locate case (they change nothing), and in front of EVERY call of a
read case, outside the time, because the read's byte fetch inserts the frames it decodes ("read ... again" is the same read repeated
without that reset: the second call of a server that comes back to its hot set). Every answer through the handle is compared with the
plain call's. --plain-only runs the plain calls alone: the form
that also runs against a library built from an earlier commit (the yardstick; run it twice, the difference is the noise floor).
Usage: gpu_archive_records.py [GiB, default 1] [runs, default 5] [--plain-only]"""
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
import bench  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
dev = torch.device("cuda", 0)
N = int(float(args[0]) * (1 << 30)) if args else 1 << 30
RUNS = int(args[1]) if len(args) > 1 else 5
fs, NL = 65536, 0x0A
N -= N % fs
frames = N // fs
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat(N // len(base) + 2)[:N].contiguous()
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
D = int((d_in == NL).sum())
R = D + (int(d_in[N - 1]) != NL)
del d_in
d_index = torch.zeros(frames, dtype=torch.int64, device=dev)


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, own_ms, h=None, before=None, each=False):
    """(result of the last call, medians); the first call is the warm-up (scratch is allocated in it). before: run once in front of the
    case, or, each, in front of every call, outside the time"""
    wall, dec, own, stage = [], [], [], []
    if before and not each:
        before()
    for r in range(RUNS + 1):
        if before and each:
            before()
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(eng.kernel_stats()["dec_ms"]); own.append(own_ms())
            if h is not None:
                stage.append(h.record_stage_ms())
    out = dict(wall_ms=med(wall), wall_min=round(min(wall), 3), wall_max=round(max(wall), 3), decode_ms=med(dec), own_ms=med(own))
    if h is not None:
        s = h.record_stats()
        out.update(stage_ms=med(stage), staged=s["staged"], decoded=s["decoded"], passes=s["passes"])
        if s["staged"] and out["stage_ms"]:
            out["staged_gb_s"] = round(s["staged"] * fs / (out["stage_ms"] * 1e-3) / 1e9, 1)
    return res, out


idx = eng.index_records(d_arc.data_ptr(), asz, d_index.data_ptr(), frames, delimiter=NL)
assert (idx.delimiters, idx.records) == (D, R), (idx, D, R)
rng = np.random.RandomState(7)
start = int(rng.randint(0, R - 100))
sets = {"100 consecutive": np.arange(start, start + 100, dtype=np.uint64), "10,000 random": rng.randint(0, R, size=10000).astype(np.uint64),
        "1,000,000 random": rng.randint(0, R, size=1000000).astype(np.uint64)}
data_cap = {}
for name, nums in sets.items():
    try:
        eng.read_records(d_arc.data_ptr(), asz, idx, d_index.data_ptr(), frames, nums, 0, 0, ranges=False)
    except Z.ZraError as e:
        data_cap[name] = e.needed_data
d_data = torch.empty(max(data_cap.values()) + 64, dtype=torch.uint8, device=dev)


P64 = ctypes.POINTER(ctypes.c_uint64)
L = Z.load()
info = Z.ZraHipRecordIndex(*idx)


def raw(h, name, nums, ranges, out):
    """the locate (out None) or the read of one set as a bare C call: the Python binding's list of a million tuples stays out of the time"""
    n, np_ = len(nums), nums.ctypes.data_as(P64)
    size = ctypes.c_uint64(0)
    eng._order()
    if out is None and h is None:
        st = L.ZraHipLocateRecords(eng.h, d_arc.data_ptr(), asz, ctypes.byref(info), d_index.data_ptr(), frames, np_, n, 0, ranges.ctypes.data_as(P64))
    elif out is None:
        st = L.ZraHipArchiveLocateRecords(h.h, ctypes.byref(info), d_index.data_ptr(), frames, np_, n, 0, ranges.ctypes.data_as(P64))
    elif h is None:
        st = L.ZraHipReadRecords(eng.h, d_arc.data_ptr(), asz, ctypes.byref(info), d_index.data_ptr(), frames, np_, n, 0, None, out.data_ptr(), data_cap[name],
                                 ctypes.byref(size))
    else:
        st = L.ZraHipArchiveReadRecords(h.h, ctypes.byref(info), d_index.data_ptr(), frames, np_, n, 0, None, out.data_ptr(), data_cap[name], ctypes.byref(size))
    assert st.tup() == (0, 0), (name, st.tup())
    return size.value


def three(case, h=None, before=None):
    """the index over the whole archive, then locate and read of every set; returns what the calls answered"""
    P, I = d_arc.data_ptr(), d_index.data_ptr()
    got = {}
    if h is None:
        got["index"], t = timed(lambda: eng.index_records(P, asz, I, frames, delimiter=NL), eng.index_records_ms)
    else:
        got["index"], t = timed(lambda: h.index_records(I, frames, delimiter=NL), eng.index_records_ms, h, before)
    print(json.dumps(dict(case=case, call="index", **t)), flush=True)
    for name, nums in sets.items():
        ranges = np.zeros(2 * len(nums), dtype=np.uint64)
        _, t = timed(lambda: raw(h, name, nums, ranges, None), eng.locate_records_ms, h, before)
        got["locate " + name] = ranges
        print(json.dumps(dict(case=case, call="locate " + name, **t)), flush=True)
        d_data.fill_(0xEE)
        got["read " + name], t = timed(lambda: raw(h, name, nums, None, d_data), eng.read_records_ms, h, before, each=True)
        got["data " + name] = d_data[:data_cap[name]].clone()
        t.update(eng.read_records_stats())
        print(json.dumps(dict(case=case, call="read " + name, **t)), flush=True)
        if h is not None:
            _, t = timed(lambda: raw(h, name, nums, None, d_data), eng.read_records_ms, h)
            t.update(eng.read_records_stats(), resident=h.stats()["resident"])
            print(json.dumps(dict(case=case, call="read " + name + " again", **t)), flush=True)
    return got


def same(a, b):
    eq = lambda x, y: np.array_equal(x, y) if isinstance(x, np.ndarray) else torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
    return a.keys() == b.keys() and all(eq(a[k], b[k]) for k in a)


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, frames=frames, level=3, delimiters=D, records=R, runs=RUNS,
                      device=torch.cuda.get_device_name(0), plain_only=PLAIN_ONLY)), flush=True)
want = three("plain")
if PLAIN_ONLY:
    sys.exit(0)


def resident(h, which):
    """the cache dropped, then one read of a byte of every frame of `which` (None: none): exactly those frames are resident"""
    def go():
        h.drop_cache()
        if which is None:
            return
        f = np.arange(frames, dtype=np.uint64)[which]
        out = torch.empty(len(f), dtype=torch.uint8, device=dev)
        h.read(out.data_ptr(), f * np.uint64(fs), np.ones(len(f), dtype=np.uint64), np.arange(len(f), dtype=np.uint64))
        assert h.stats()["resident"] == len(f)
    return go


with Z.Archive(eng, d_arc.data_ptr(), asz, frames * fs) as h:
    assert h.stats()["slots"] == frames
    for case, which in (("handle 0%", None), ("handle 50%", slice(0, None, 2)), ("handle 100%", slice(0, None))):
        got = three(case, h, resident(h, which))
        assert same(got, want), case
    assert eng.kernel_stats()["dec_launches"] == 0                             # the last read at 100 %: neither sweep launched the decoder
