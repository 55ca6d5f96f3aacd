"""GPU half of the decoder's conformance suite: valid zstd frames that no one-shot encoder of libzstd 1.4.9 writes (tests/frame_craft.py
writes them from a description), in ZRA archives stitched around them, through every decode route and every call that decodes.

The yardstick is the plaintext computed in Python from each frame's description (frame_craft.plaintext: literals plus an LZ copy loop);
the few frames that are invalid on purpose must give the status the CPU half recorded from libzstd (tests/golden/crafted_frames.json),
or the restated decoder's where no libzstd is at hand. The decoder's knobs are read once per process, so every route is a subprocess
that runs ALL archives (this file as a script, the archives handed over in a temporary file) and ends with a `bad N` line."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import frame_craft as F                                      # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "crafted_frames.json")
SIZES = (F.FRAME_SIZE, 300000, 400000)                       # frame sizes of the archives: two to four blocks per frame
ROUTES = [
    {},
    {"ZRA_DEC_SMALL_MAX": "0"},
    {"ZRA_DEC_SMALL_MAX": "0", "ZRA_DEC_FMB_MIN": "1"},
    {"ZRA_DEC_SMALL_MAX": "0", "ZRA_DEC_FMB_MIN": "1", "ZRA_DEC_CHAIN_LDS": "0"},
    {"ZRA_DEC_SMALL_MAX": "0", "ZRA_DEC_FMB_MIN": "1", "ZRA_DEC_CHAIN_LDS": "2", "ZRA_DEC_CHAIN_LDS_MIN": "1"},
]


def _boundaries(frames, fs):
    """content offsets of every crafted block boundary of an archive"""
    out = []
    for k, fr in enumerate(frames):
        if fr is None:
            continue
        pos = 0
        for s in F.block_sizes(fr)[:-1]:
            pos += s
            out.append(k * fs + pos)
    return out


def _archive(zra, name, parts, fs, error=None):
    """one archive: parts = [(description or None, frame bytes, plaintext)], every plaintext but the last `fs` long"""
    assert all(len(p[2]) == fs for p in parts[:-1]) and 0 < len(parts[-1][2]) <= fs, name
    plain = b"".join(p[2] for p in parts)
    arc = zra.stitch_header([len(p[1]) for p in parts], len(plain), fs) + b"".join(p[1] for p in parts)
    return dict(name=name, arc=arc, plain=plain, error=error, fs=fs, bounds=_boundaries([p[0] for p in parts], fs))


def build_archives(zra, O):
    """every archive of the suite: one per directed case, the randomised frames grouped by length, and one long mixed archive"""
    recorded = {e["name"]: e for e in json.load(open(GOLDEN))} if os.path.exists(GOLDEN) else {}
    out = []
    for c in F.directed_cases():
        fr = c["frame"]
        data = F.write_frame(fr)
        plain = F.plaintext(fr, check=False)
        err = None
        if c["error"]:
            rec = recorded.get(c["name"], {}).get("zl_status")
            err = rec if rec else O.decompress(data, 4096, "zl" if O.have_libzstd() else "zo")[1]
            assert err, c["name"]
            plain = bytes(sum(F.block_sizes(fr)))            # what the archive's header declares; nothing of it is defined
        out.append(_archive(zra, c["name"], [(fr, data, plain)], min(s for s in SIZES if s >= len(plain)), err))
    full, short = [], []
    for seed in F.RANDOM_SEEDS:
        for k, (fr, tags, data) in enumerate(F.random_frames(seed)[0]):
            plain = F.plaintext(fr)
            if len(plain) > F.FRAME_SIZE:
                out.append(_archive(zra, "random_%d_%d" % (seed, k), [(fr, data, plain)], SIZES[1]))
            else:
                (full if len(plain) == F.FRAME_SIZE else short).append(("random_%d_%d" % (seed, k), fr, data, plain))
    # the full-length frames dealt out in front of the shorter ones, every one of them in some archive
    assert short
    placed = len(out) - len(F.directed_cases())
    for i, (name, fr, data, plain) in enumerate(short):
        head = full[i::len(short)]
        out.append(_archive(zra, name, [(h[1], h[2], h[3]) for h in head] + [(fr, data, plain)], F.FRAME_SIZE))
        placed += len(head) + 1
    assert placed == sum(len(F.random_frames(seed)[0]) for seed in F.RANDOM_SEEDS) == 240
    # 70+ frames, crafted and ordinary ones alternating: a default call of this size takes the block-parallel pass, and the neighbours
    # of a frame that leaves it are checked too
    import corpus
    base = corpus.gen_loglike(1 << 20) + corpus.gen_E(1 << 20)
    parts = []
    for i in range(36):
        name, fr, data, plain = full[(i * 5) % len(full)]
        parts.append((fr, data, plain))
        o = base[(i * 40009) % (len(base) - F.FRAME_SIZE):][:F.FRAME_SIZE]
        parts.append((None, O.compress_frame(o, 3, bool(i & 1)), o))
    parts.append((short[0][1], short[0][2], short[0][3]))
    assert len(parts) == 73
    out.append(_archive(zra, "mixed_73_frames", parts, F.FRAME_SIZE))
    return out


# ------------------------------------------------------------------------------------------------ the script of one route
def _queries(a):
    """the random-access queries of an archive: the first byte, the last reachable one, every crafted block boundary -1 / +0 / across,
    and a query that spans two frames. The batches take all of them (one call); the single host-pointer calls take the first two, the
    last two and about six between, to keep the file quick."""
    n = len(a["plain"])
    q = {(0, 1), (max(0, n - 2), 1)}
    for b in a["bounds"]:
        q |= {(b - 1, 1), (b, 1), (b - 1, 2), (max(0, b - 5), 11)}
    if n > a["fs"] + 8:
        q.add((a["fs"] - 3, 7))
        q.add((a["fs"] - 1, min(a["fs"] + 2, n - a["fs"])))
    return sorted((o, s) for o, s in q if 0 <= o and s > 0 and o + s < n)      # (the reference's bound: offset + size < content size)


def run_route(path):
    import torch
    import zra_amd as Z
    import search_model
    archives = pickle.load(open(path, "rb"))
    L = Z.load()
    eng = Z.Engine(0)
    dev = torch.device("cuda", 0)
    bad = 0

    def fail(*what):
        nonlocal bad
        bad += 1
        print("FAIL", *what)

    def status(call):
        try:
            call()
            return (0, 0)
        except Z.ZraError as e:
            return (e.zra, e.zstd)
    for a in archives:
        arc, plain, n, name = a["arc"], a["plain"], len(a["plain"]), a["name"]
        d_arc = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to(dev)
        d_out = torch.full((n + 256,), 0xEE, dtype=torch.uint8, device=dev)
        qs = _queries(a)
        offs = np.array([q[0] for q in qs], dtype=np.uint64)
        sizes = np.array([q[1] for q in qs], dtype=np.uint64)
        oofs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        d_ra = torch.full((int(sizes.sum()) + 64,), 0xEE, dtype=torch.uint8, device=dev)
        if a["error"]:
            want = (1, a["error"])
            if status(lambda: Z.DecompressBuffer(arc)) != want:
                fail(name, "DecompressBuffer status", status(lambda: Z.DecompressBuffer(arc)), want)
            if status(lambda: eng.decompress(d_arc.data_ptr(), len(arc), d_out.data_ptr(), n)) != want:
                fail(name, "Engine.decompress status")
            if bytes(d_out[n:].cpu().numpy()) != b"\xEE" * 256:
                fail(name, "guard behind the output")
            if n > 2 and status(lambda: Z.DecompressRA(arc, n - 2, 1)) != want:
                fail(name, "DecompressRA status")
            for opt in (0, 8):
                L.ZraHipSetOptions(opt)
                try:
                    if n > 2 and status(lambda: eng.decompress_ra_batch(d_arc.data_ptr(), len(arc), d_ra.data_ptr(), [n - 2], [1], [0])) != want:
                        fail(name, "decompress_ra_batch status, options", opt)
                finally:
                    L.ZraHipSetOptions(0)
            nf, faults = eng.verify(d_arc.data_ptr(), len(arc), content=True)
            if nf != 1 or faults[0][0] != 0 or faults[0][1] != a["error"]:
                fail(name, "verify (content) names", nf, faults)
            nf, faults = eng.verify(d_arc.data_ptr(), len(arc), content=False)
            if nf > 1 or (nf == 1 and (faults[0][0] != 0 or faults[0][1] != a["error"])):
                fail(name, "verify (structure) names", nf, faults)
            continue
        try:
            if Z.DecompressBuffer(arc) != plain:
                fail(name, "DecompressBuffer")
            eng.decompress(d_arc.data_ptr(), len(arc), d_out.data_ptr(), n)
            host = bytes(d_out.cpu().numpy())
            if host[:n] != plain:
                fail(name, "Engine.decompress")
            if host[n:] != b"\xEE" * 256:
                fail(name, "guard behind the output")
            for o, s in qs if len(qs) <= 10 else qs[:2] + qs[2:-2][::(len(qs) - 4) // 6 + 1] + qs[-2:]:     # (the batches below take all of them)
                if Z.DecompressRA(arc, o, s) != plain[o:o + s]:
                    fail(name, "DecompressRA", o, s)
            for opt in (0, 8):
                L.ZraHipSetOptions(opt)
                try:
                    d_ra.fill_(0xEE)
                    eng.decompress_ra_batch(d_arc.data_ptr(), len(arc), d_ra.data_ptr(), offs, sizes, oofs)
                    host = bytes(d_ra.cpu().numpy())
                    for (o, s), oo in zip(qs, oofs):
                        if host[int(oo):int(oo) + s] != plain[o:o + s]:
                            fail(name, "decompress_ra_batch", o, s, "options", opt)
                    if host[int(sizes.sum()):] != b"\xEE" * 64:
                        fail(name, "guard behind the batch's output")
                finally:
                    L.ZraHipSetOptions(0)
            for content in (False, True):
                nf, faults = eng.verify(d_arc.data_ptr(), len(arc), content=content)
                if nf:
                    fail(name, "verify reports", faults[:3], "content" if content else "structure")
            if a["bounds"] and name in ("geom_only_second_to_last_short", "mixed_73_frames"):
                b = a["bounds"][-1]
                pat = plain[b - 4:b + 4]
                want = search_model.matches(plain, pat)
                nm, got = eng.search(d_arc.data_ptr(), len(arc), pat)
                if b - 4 not in want or nm != len(want) or got != want:
                    fail(name, "search across a block boundary", nm, len(want))
        except Z.ZraError as e:
            fail(name, "status", (e.zra, e.zstd))
    eng.close()
    print("archives", len(archives))
    print("bad", bad)


@pytest.fixture(scope="module")
def route_runs(zra, oracle, tmp_path_factory):
    """the five processes, started side by side over one file of archives: [(return code, stdout, stderr)] by route"""
    path = str(tmp_path_factory.mktemp("foreign") / "archives.pickle")
    arcs = build_archives(zra, oracle)
    assert len(arcs) > 200 and sum(a["name"] == "mixed_73_frames" for a in arcs) == 1
    with open(path, "wb") as f:
        pickle.dump(arcs, f)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for env in ROUTES]
    out = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
            se += "\n(killed at its time limit)"
        out.append((p.returncode, so, se))
    os.remove(path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", range(len(ROUTES)), ids=["default", "rounds", "block_parallel", "chain_hbm", "chain_lds"])
def test_foreign_frames_through_every_route(route_runs, route):
    """Every directed and randomised frame of the suite, and the long mixed archive, through the host-pointer calls, the engine's full
    decode (guard region behind the output), random access at the first byte, the last reachable one, every crafted block boundary
    and across two frames (single calls and batches, with and without whole-frame decoding), both depths of the verification and one
    search across a short block's boundary — in a process whose decoder takes the route's kernels."""
    rc, so, se = route_runs[route]
    assert rc == 0, (so[-1500:], se[-1500:])
    assert so.strip().endswith("bad 0"), so[-3000:]


if __name__ == "__main__":
    run_route(sys.argv[1])
