"""bring-up: the range scans through an archive handle (ZraHipArchiveSearch, ZraHipArchiveGrep) beside the plain engine calls, on an
archive whose frames are resident in the handle's cache to 0 %, 50 % (every other frame) and 100 %: what a scan fed from the arena
costs beside one fed by the decoder.
The content is the bench's (bench.synth_corpus: log-like lines, numeric rows, binary-ish records), level 3, 64 KiB frames, the cache
as large as the content. Two calls: the single search for an 8-byte needle planted 4,096 times (tools/bringup/gpu_search.py's), and
the grep for K = 8 strings of 8 to 32 bytes cut from lines of the content, each of them rare (a few hundred selected lines per GiB: the
list that comes to the host stays small, so the wall time is the call's and not the list's). Per case one warm-up call and then RUNS calls, medians of
  wall ms     host time over the call, with a device synchronise on both sides
  decode ms   ZraHipGetKernelStats (HIP events of the decode passes)
  scan ms     ZraHipDebugSearchScanMs / ZraHipDebugGrepScanMs
  stage ms    ZraHipDebugArchiveScanStageMs (the job-split and stage-from-cache launches), and the bytes staged per second from it
Cases: the plain call; the handle at 0 %, 50 %, 100 %; and, for the per-pass cost of the split launch and its read-back, the plain
call and the handle at 0 % with a staging window of 64 MiB (16 passes per GiB). Every answer through the handle is compared with the
plain call's. --plain-only runs the plain calls alone: the form that also runs against a library built from an earlier commit (the
yardstick; run it twice, the difference is the noise floor).
Usage: gpu_archive_scan.py [GiB, default 1] [runs, default 5] [--plain-only]"""
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
fs, PLANTED, K, SMALL = 65536, 4096, 8, 64 << 20
base = bench.synth_corpus(64 << 20, seed=1)
d_in = torch.from_numpy(base).to(dev).repeat(N // len(base) + 2)[:N].contiguous()
rng = np.random.RandomState(17)
needle = bytes(rng.choice([b for b in range(256) if b != 10], size=8).astype(np.uint8))
frames = (N + fs - 1) // fs
places = np.sort(rng.choice(N // 4096 - 2, size=PLANTED, replace=False).astype(np.int64) * 4096 + 100)
places[::64] = (places[::64] // fs + 1) * fs - 3                              # every 64th copy across a frame boundary
places = np.unique(places)
idx = torch.from_numpy(places).to(dev)
for k in range(8):
    d_in[idx + k] = needle[k]
eng = Z.Engine(0)
d_arc = torch.empty(Z.GetOutputBufferSize(N, fs) + 64, dtype=torch.uint8, device=dev)
asz = eng.compress(d_in.data_ptr(), N, d_arc.data_ptr(), 3, fs, True)
del d_in
text = base.tobytes()
lines = [ln for ln in text[:4 << 20].split(b"\n") if 40 <= len(ln) <= 96]
patterns = []
while len(patterns) < K:                                                       # strings that select few lines: at most 4 places in the 64 MiB that repeat
    line = lines[int(rng.randint(len(lines)))]
    m = int(rng.randint(8, 33))
    at = int(rng.randint(0, len(line) - m))
    if line[at:at + m] not in patterns and text.count(line[at:at + m]) <= 4:
        patterns.append(line[at:at + m])
del text
CAP = 1 << 20


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def timed(call, scan_ms, h=None):
    """(result of the last call, medians); the first call is the warm-up (scratch is allocated in it)"""
    wall, dec, scan, stage = [], [], [], []
    for r in range(RUNS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        if r:
            wall.append(t * 1e3); dec.append(eng.kernel_stats()["dec_ms"]); scan.append(scan_ms())
            if h is not None:
                stage.append(h.scan_stage_ms())
    out = dict(wall_ms=med(wall), wall_min=round(min(wall), 3), wall_max=round(max(wall), 3), decode_ms=med(dec), scan_ms=med(scan))
    if h is not None:
        s = h.scan_stats()
        out.update(stage_ms=med(stage), staged=s["staged"], decoded=s["decoded"], passes=s["passes"])
        if s["staged"] and out["stage_ms"]:
            out["staged_gb_s"] = round(min(N, s["staged"] * fs) / (out["stage_ms"] * 1e-3) / 1e9, 1)
    return res, out


def both(case, staging, h=None):
    if h is None:
        a, ta = timed(lambda: eng.search(d_arc.data_ptr(), asz, needle, staging_bytes=staging, max_matches=1 << 16), eng.search_scan_ms)
        b, tb = timed(lambda: eng.grep(d_arc.data_ptr(), asz, patterns, staging_bytes=staging, max_records=CAP), eng.grep_scan_ms)
    else:
        a, ta = timed(lambda: h.search(needle, staging_bytes=staging, max_matches=1 << 16), eng.search_scan_ms, h)
        b, tb = timed(lambda: h.grep(patterns, staging_bytes=staging, max_records=CAP), eng.grep_scan_ms, h)
    print(json.dumps(dict(case=case, call="search planted", matches=a[0], **ta)), flush=True)
    print(json.dumps(dict(case=case, call="grep K=8", selected=b[0], **tb)), flush=True)
    return a, b, ta, tb


print(json.dumps(dict(content_bytes=N, archive_bytes=asz, frame_size=fs, frames=frames, level=3, planted=len(places), runs=RUNS,
                      device=torch.cuda.get_device_name(0), plain_only=PLAIN_ONLY)), flush=True)
want = both("plain", 0)
assert want[0][0] >= len(places), (want[0][0], len(places))
want_small = both("plain staging=64MiB", SMALL)
assert want_small[:2] == want[:2]
if PLAIN_ONLY:
    sys.exit(0)


def warm(h, which):
    """one read of a byte of every frame of `which`: the whole frame becomes resident"""
    f = np.arange(frames, dtype=np.uint64)[which]
    out = torch.empty(len(f), dtype=torch.uint8, device=dev)
    h.read(out.data_ptr(), f * np.uint64(fs), np.ones(len(f), dtype=np.uint64), np.arange(len(f), dtype=np.uint64))
    return h.stats()["resident"]


with Z.Archive(eng, d_arc.data_ptr(), asz, frames * fs) as h:
    assert h.stats()["slots"] == frames
    got = both("handle 0%", 0, h)
    assert got[:2] == want[:2]
    got_small = both("handle 0% staging=64MiB", SMALL, h)
    assert got_small[:2] == want[:2]
    for i, name in ((0, "search planted"), (1, "grep K=8")):
        passes = got_small[2 + i]["passes"]
        print(json.dumps(dict(call=name, passes=passes, per_pass_us_over_plain=round((got_small[2 + i]["wall_ms"] - want_small[2 + i]["wall_ms"]) / passes * 1e3, 1),
                              one_pass_us_over_plain=round((got[2 + i]["wall_ms"] - want[2 + i]["wall_ms"]) * 1e3, 1))), flush=True)
    assert warm(h, slice(0, None, 2)) == (frames + 1) // 2
    got = both("handle 50%", 0, h)
    assert got[:2] == want[:2]
    assert warm(h, slice(1, None, 2)) == frames
    cache = h.stats()
    got = both("handle 100%", 0, h)
    assert got[:2] == want[:2] and got[2]["decoded"] == 0 and eng.kernel_stats()["dec_launches"] == 0
    got = both("handle 100% staging=64MiB", SMALL, h)
    assert got[:2] == want[:2]
    assert h.stats() == cache                                                  # a scan is not a read
