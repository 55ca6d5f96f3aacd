"""GPU tests of ZraHipGrepArchiveWhere and ZraHipArchiveGrepWhere (include/zra_hip.h): the records of a content range whose set of
occurring patterns satisfies a list of clauses {all, any, none}. The yardstick everywhere is tests/where_model.py on plaintext the
test generated itself (cross-checked in tests/test_grep_where_abi.py); the plain predicates are also held against Engine.grep. Archives
are written on the device. The shapes are the smallest at which each seam exists: the scan's trip is 64 positions, its wave 2,048, its
tile 8,192; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expr_model as EM
import grep_model as GM
import test_gpu_archive_scan as AS
import test_gpu_grep as G
import where_model as WM
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
FS = 1024
ZERO = G.ZERO


def _where(eng, zra, d, size, pats, where, **kw):
    """((zra, zstd), n_records, [(offset, size)]) of one grep with clauses"""
    try:
        n, recs = eng.grep(d.data_ptr(), size, pats, where=where, **kw)
        return (0, 0), n, recs
    except zra.ZraError as e:
        return (e.zra, e.zstd), 0, []


def _raw(eng, zra, d, size, pats, where, cap, mode=0, offset=0, length=MAXU64, staging=0, syntax=0):
    """(status, *nRecords, the bytes of a record array two entries longer than the capacity, 0xEE-filled before the call)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n = ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
    cl = (ctypes.c_uint64 * (3 * len(where)))(*(w for c in where for w in c))
    eng._order()
    st = zra.load().ZraHipGrepArchiveWhere(eng.h, d.data_ptr(), size, b"".join(pats), sizes, len(pats), syntax, NL, mode, cl, len(where), offset, length, staging,
                                           arr if cap else None, cap, ctypes.byref(n)).tup()
    return st, n.value, bytes(arr)


def _check(eng, zra, d, size, data, fs, pats, where, lo=0, hi=None, staging=0, modes=(False, True), syntax=0, matches=None):
    """one call per mode of [lo, hi) against the model: status, count, list and all eight stats. Returns {invert: selected}."""
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    out = {}
    for inv in modes:
        recs, sel, nm = WM.grep_where(data, pats, where, NL, inv, lo, hi, matches=matches)
        tag = (where, lo, hi, staging, inv)
        got = _where(eng, zra, d, size, pats, where, invert=inv, offset=lo, length=length, staging_bytes=staging, syntax=syntax)
        print("where", tag, "status", got[0], "selected", got[1], "model", len(sel))
        assert got[:2] == ((0, 0), len(sel)), (tag, got[:2], len(sel))
        assert got[2] == sel, (tag, sorted(set(got[2]) ^ set(sel))[:10], got[2][:6], sel[:6])
        s = eng.grep_stats()
        shortest = min(len(p) for p in pats) if matches is None else 1
        if end == lo or (end - lo < shortest and not WM.selected(where, 0, inv)):
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == G._stats(U, fs, lo, end, staging, len(recs), len(sel), len(sel), nm), (tag, s)
        out[inv] = sel
    return out


def _random_clauses(rng, k, n_max=8):
    """1 .. n_max clauses over k patterns: a few bits per term, `none` disjoint from the other two; bit k - 1 is used by the first"""
    out = []
    for c in range(int(rng.randint(1, n_max + 1))):
        bits = [int(b) for b in rng.permutation(k)[:int(rng.randint(0, 6))]]
        if c == 0:
            bits = [k - 1] + [b for b in bits if b != k - 1]
        a = y = n = 0
        for b in bits:
            t = int(rng.randint(0, 3))
            if t == 0:
                a |= 1 << b
            elif t == 1:
                y |= 1 << b
            else:
                n |= 1 << b
        out.append((a, y, n))
    return out


# ---- 1
@pytest.fixture(scope="module")
def tiny(zra, gpu_engine):
    """test_gpu_grep.py's content at frame size 4: about 260 frames, a 60-byte line, a pattern of 40 bytes"""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"acde"), size=60).astype(np.uint8))
    data = G._lines(rng, 500) + b"\n" + long_line + b"\n" + G._lines(rng, 480)
    pats = [b"b", b"cda", long_line[5:45], b"zz", b"ea"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    return dict(data=data, pats=pats, arc=arc, d=_dev(arc), fs=4)


@pytest.mark.parametrize("staging", [0, 1])
def test_known_answers_at_frame_size_4(zra, gpu_engine, tiny, staging):
    """With one slot a pass holds 4 bytes: shorter than most records, so nearly every record's set crosses passes in the carried state."""
    data, pats, arc, d = tiny["data"], tiny["pats"], tiny["arc"], tiny["d"]
    seen = []
    for where in ([(0b11, 0, 0)], [(0b1, 0, 0b10)], [(0b10001, 0, 0), (0b100, 0, 0b1)], [(0, 0, 0)]):
        sel = _check(gpu_engine, zra, d, len(arc), data, 4, pats, where, staging=staging)
        assert gpu_engine.grep_stats()["passes"] == (-(-len(data) // 4) if staging else 1)
        seen.append(sel)
    assert len(seen[0][False]) > 3 and len(seen[1][False]) > 10 and (501, 60) in seen[2][False]
    assert seen[3][False] == GM.records(data) and seen[3][True] == []


# ---- 2
A, B, C = b"\xF0NEEDLE\xF1", b"\xF2THREAD\xF3", b"\xF4C\xF5"


@pytest.fixture(scope="module")
def filler():
    """32 KiB without a delimiter and without a byte of the three patterns: the body of the long record"""
    return _data(np.random.RandomState(5), 32 << 10).replace(b"\n", b"\x0B")


@pytest.mark.parametrize("dist,what", [(64, "next trip"), (2048, "next wave"), (8192, "next tile"), (16384, "across a delimiter-free tile")])
def test_sets_are_ored_across_every_seam(zra, gpu_engine, filler, dist, what):
    """Short records, one of them with C, then a long record with A 50 bytes behind its start and B `dist` positions further on, then
    a short record with C and more short ones. A record's set is the OR of what its trips, waves, tiles and passes saw: all = {A, B}
    needs both halves to arrive, none = {C} must not see the neighbours' C."""
    rng = np.random.RandomState(dist)
    head = G._lines(rng, 300)[:-1] + b"\nxx" + C + b"yy\n"
    S = len(head)
    tail = b"\nq" + C + b"\n" + G._lines(rng, 200, b"abc") + b"\nlast"
    big = (S, 50 + dist + 100)
    pats = [A, B, C]
    for has_a, has_b in ((True, True), (False, True), (True, False)):
        body = bytearray(filler[:50 + dist + 100])
        if has_a:
            body[50:50 + len(A)] = A
        if has_b:
            body[50 + dist:50 + dist + len(B)] = B
        data = head + bytes(body) + tail
        assert (S + 50) // 64 != (S + 50 + dist) // 64
        if dist == 16384:
            assert (S + 50 + dist) // 8192 == (S + 50) // 8192 + 2
        arc = _compress(gpu_engine, zra, data, 3, FS, True)
        d = _dev(arc)
        for staging in (0, 2 * FS):
            both = _check(gpu_engine, zra, d, len(arc), data, FS, pats, [(0b011, 0, 0)], staging=staging)
            assert (big in both[False]) == (has_a and has_b) and (big in both[True]) != (has_a and has_b), (what, staging, has_a, has_b)
            a_not_b = _check(gpu_engine, zra, d, len(arc), data, FS, pats, [(0b001, 0, 0b010)], staging=staging, modes=(False,))
            assert (big in a_not_b[False]) == (has_a and not has_b), (what, staging, has_a, has_b)
            no_c = _check(gpu_engine, zra, d, len(arc), data, FS, pats, [(0, 0, 0b100)], staging=staging, modes=(False,))
            assert big in no_c[False] and (S - 5 - len(C), 4 + len(C)) not in no_c[False] and (S + big[1] + 1, 1 + len(C)) not in no_c[False]


# ---- 3
def test_several_records_and_patterns_inside_one_trip(zra, gpu_engine):
    """Records of 3 .. 10 bytes: a trip of 64 lanes holds six to sixteen delimiters with hits of different patterns between them. In the
    first half (letters a and b only) every position is a hit of a one-byte pattern: the longest trip loops."""
    rng = np.random.RandomState(3)
    out = bytearray()
    while len(out) < 20 << 10:
        alphabet = b"ab" if len(out) < 10 << 10 else b"abcd"
        out += bytes(rng.choice(list(alphabet), size=int(rng.randint(3, 11))).astype(np.uint8)) + b"\n"
    data = bytes(out)
    pats = [b"a", b"b", b"ab", b"ba", b"cc", b"cd", b"dc", b"dd"]
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    sizes = set()
    for k in range(12):
        where = _random_clauses(rng, len(pats), 4)
        sel = _check(gpu_engine, zra, d, len(arc), data, FS, pats, where, staging=(0, 3 * FS)[k & 1], modes=(bool(k & 2),))
        sizes.add(len(sel[bool(k & 2)]))
    assert len(sizes) > 4, sizes


# ---- 4
@pytest.fixture(scope="module")
def wide(zra, gpu_engine):
    """40 KiB of lines over a..h and 64 patterns of 2 .. 4 bytes"""
    rng = np.random.RandomState(64)
    data = G._lines(rng, 40 << 10, b"abcdefgh", 60)
    pats = []
    while len(pats) < 64:
        p = bytes(rng.choice(list(b"abcdefgh"), size=int(rng.randint(2, 5))).astype(np.uint8))
        if p not in pats:
            pats.append(p)
    arc = _compress(gpu_engine, zra, data, 3, 4096, True)
    return dict(data=data, pats=pats, arc=arc, d=_dev(arc), fs=4096)


def test_64_patterns_random_predicates(zra, gpu_engine, wide):
    data, pats, arc, d, fs = wide["data"], wide["pats"], wide["arc"], wide["d"], wide["fs"]
    rng = np.random.RandomState(4)
    nl = [p for p in range(len(data)) if data[p] == NL]
    cut = [p for p in nl if data[p + 1:p + 2] != b"\n" and data[p - 1:p] != b"\n"]
    ranges = [(0, None), (cut[3] + 5, cut[-3] - 4), (cut[40] - 3, cut[300] + 1), (9000, 9100)]
    sizes = set()
    for k in range(10):
        where = _random_clauses(rng, 64)
        assert (where[0][0] | where[0][1] | where[0][2]) >> 63
        lo, hi = ranges[k % len(ranges)]
        sel = _check(gpu_engine, zra, d, len(arc), data, fs, pats, where, lo, hi, staging=(0, 2 * fs)[k & 1], modes=(bool(k % 3 == 0),))
        sizes.add(len(sel[bool(k % 3 == 0)]))
    assert len(sizes) > 5, sizes


# ---- 5
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_the_plain_predicates_are_the_plain_grep(zra, gpu_engine, tiny, wide, which):
    t = tiny if which == "tiny" else wide
    data, pats, arc, d = t["data"], t["pats"], t["arc"], t["d"]
    full = WM.full(len(pats))
    for staging in (0, t["fs"]):
        for inv in (False, True):
            plain = gpu_engine.grep(d.data_ptr(), len(arc), pats, invert=inv, staging_bytes=staging)
            ps = gpu_engine.grep_stats()
            assert ps["selected"] == plain[0] > 0
            # any pattern, with the call's own invert; no pattern, with the opposite one
            for where, winv in (([(0, full, 0)], inv), ([(0, 0, full)], not inv)):
                got = gpu_engine.grep(d.data_ptr(), len(arc), pats, invert=winv, staging_bytes=staging, where=where)
                assert got == plain and gpu_engine.grep_stats() == ps, (which, staging, inv, where, got[0], plain[0])


# ---- 6
def test_expressions(zra, gpu_engine):
    rng = np.random.RandomState(6)
    words = [b"error", b"ERROR", b"Error", b"warn", b"info"]
    lines = []
    for _ in range(400):
        lines.append(b"%s status=%d id=%s %s" % (words[rng.randint(5)], rng.choice([200, 404, 500, 503, 5, 50]), bytes(rng.choice(list(b"abxyz0123"), size=rng.randint(2, 6)).astype(np.uint8)),
                                                 b"x" * int(rng.randint(0, 20))))
    data = b"\n".join(lines)[:16 << 10]
    pats = [b"error", b"status=5[0-9][0-9]", b"id=...."]
    syntax = zra.PATTERN_FOLD_CASE | zra.PATTERN_CLASSES
    matches = EM.set_matches(data, EM.compile(pats, syntax, NL))
    assert len({i for _, i in matches}) == 3
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    for where in ([(0b011, 0, 0)], [(0, 0b110, 0b001)]):
        for staging in (0, 2 * FS):
            sel = _check(gpu_engine, zra, d, len(arc), data, FS, pats, where, staging=staging, syntax=syntax, matches=matches)
            assert len(sel[False]) > 5 and len(sel[True]) > 5


# ---- 7
def test_capacity(zra, gpu_engine, wide):
    data, pats, arc, d, fs = wide["data"], wide["pats"], wide["arc"], wide["d"], wide["fs"]
    where = [(0b11, 0, 0), (0, 0b1100, 0b10000)]
    recs, sel, nm = WM.grep_where(data, pats, where)
    total = len(sel)
    assert total > 8
    for cap in (0, total - 3):
        for staging in (0, fs):
            st, n, mem = _raw(gpu_engine, zra, d, len(arc), pats, where, cap, staging=staging)
            assert (st, n) == ((0, 0), total), (cap, staging, st, n)
            got = np.frombuffer(mem[:16 * cap], dtype="<u8").reshape(-1, 2)
            assert [tuple(r) for r in got.tolist()] == sel[:cap], (cap, staging)
            assert mem[16 * cap:] == b"\xEE" * 32, (cap, staging)
            assert gpu_engine.grep_stats() == G._stats(len(data), fs, 0, len(data), staging, len(recs), total, cap, nm), (cap, staging)


# ---- 8
def test_shortcut_and_statuses(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    p = next(q for q in range(5 * fs + 100, 6 * fs) if NL not in data[q - 3:q + 9])
    pats = [data[p:p + 6], b"\xFF\xFE\xFD"]
    for lo, hi in ((p, p + 2), (12 * fs - 1, 12 * fs)):
        for staging in (0, fs):
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, pats, [(0b01, 0, 0)], lo, hi, staging)   # false on the empty set: not decoded
            assert sel[False] == [] and sel[True] == GM.records(data, NL, lo, hi) and gpu_engine.grep_stats()["decoded"] == 1
            assert _where(gpu_engine, zra, d, len(arc), pats, [(0b01, 0, 0)], offset=lo, length=hi - lo)[:2] == ((0, 0), 0)
            assert gpu_engine.grep_stats() == dict(ZERO, frames=12)
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, pats, [(0, 0, 0b01)], lo, hi, staging, modes=(False,))
            assert sel[False] == GM.records(data, NL, lo, hi) and gpu_engine.grep_stats()["decoded"] == 1   # scanned: every record
    assert _where(gpu_engine, zra, d, len(arc), pats, [(0, 0, 0)], offset=p, length=0) == ((0, 0), 0, [])
    assert gpu_engine.grep_stats() == dict(ZERO, frames=12)
    # a frame with a flipped byte
    bad = _flip_mid(arc, [7])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs):
            st, n, mem = _raw(gpu_engine, zra, db, len(bad), pats, [(0b01, 0, 0b10)], 6, mode=mode, staging=staging)
            assert (st, n, mem) == ((1, want[7]), 0, b"\xEE" * 128), (mode, staging, st, n)
            assert gpu_engine.grep_stats() == ZERO
    _check(gpu_engine, zra, db, len(bad), data, fs, pats, [(0b01, 0, 0b10)], 0, 7 * fs)       # the same damage outside the range
    # rule 1 with an engine: nothing decoded, nothing written
    for where in ([(0b100, 0, 0)], [(1, 0, 1)], [(0, 1, 1)], [(0, 0, 0)] * 9):
        st, n, mem = _raw(gpu_engine, zra, d, len(arc), pats, where, 2)
        assert (st, n, mem) == ((1, 42), 0, b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, where


# ---- 9
@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames of the range resident"""
    import torch
    fs = 1000
    data, pats = AS._content(77, fs)
    U = len(data)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, U, warm, slots)
    try:
        where = [(0b100000, 0, 0b1000000), (0, 0b11111, 0)]
        for lo, hi in ((0, U), (6 * fs + fs // 2, 10 * fs + fs // 2)):
            for staging in (0, 3 * fs):
                kw = dict(offset=lo, length=hi - lo, staging_bytes=staging)
                before = h.stats()
                s0 = h.scan_stats()
                plain = h.grep(pats, **kw)
                s1 = h.scan_stats()
                got = h.grep(pats, where=where, **kw)
                s2 = h.scan_stats()
                hs = gpu_engine.grep_stats()
                want = gpu_engine.grep(d.data_ptr(), len(arc), pats, where=where, **kw)
                es = gpu_engine.grep_stats()
                model = WM.grep_where(data, pats, where, NL, False, lo, hi)
                assert got == want == (len(model[1]), model[1]) and got[0] > 0, (slots, lo, staging)
                staged, decoded, dec_bytes = AS._split(warm, fs, U, lo, hi)
                assert hs == dict(es, decoded=decoded, content_bytes=dec_bytes), (hs, es)
                # the handle's counters move as for the plain grep on the same range
                assert {k: s2[k] - s1[k] for k in s1 if k.endswith("total") or k == "scans"} == {k: s1[k] - s0[k] for k in s1 if k.endswith("total") or k == "scans"}
                assert (s2["staged"], s2["decoded"], s2["passes"]) == (s1["staged"], s1["decoded"], s1["passes"]) and (s2["staged"], s2["decoded"]) == (staged, decoded)
                assert h.stats() == before                                     # a scan is not a read
        if slots:
            out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
            before = h.stats()
            h.read(out.data_ptr(), [warm[0] * fs + 3], [5], [0])
            torch.cuda.synchronize()
            after = h.stats()
            assert (after["hits"], after["misses"], after["resident"]) == (before["hits"] + 1, before["misses"], before["resident"])
            assert out[:5].cpu().numpy().tobytes() == data[warm[0] * fs + 3:warm[0] * fs + 8]
    finally:
        h.close()


# ---- 10
def test_cli_mode_glw(zra, gpu_engine, tmp_path):
    data = b"alpha one\nbeta two\n\ngamma one two\ndelta" + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "glw", str(p_arc)] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    def lines(sel):
        return ["%d\t%d" % r for r in sel] + ["%d records" % len(sel), ""]

    for args, pats, where, inv in ((("-w", "+0,-1", "one", "two"), [b"one", b"two"], [(1, 0, 2)], False),
                                   (("-v", "-w", "+0,-1", "one", "two"), [b"one", b"two"], [(1, 0, 2)], True),
                                   (("-w", "+0,+1", "-w", "?2", "-F", "one", "two", "hex:" + b"delta".hex()), [b"one", b"two", b"delta"], [(3, 0, 0), (0, 4, 0)], False),
                                   (("-i", "-w", "?0,?1,-2", "ALPHA", "b[a-e]ta", "z"), [b"alpha", b"beta", b"z"], [(0, 3, 4)], False)):
        sel = WM.grep_where(data, pats, where, NL, inv)[1]
        r = run(*args)
        assert r.returncode == 0 and r.stdout.split("\n") == lines(sel) and sel, (args, r.stdout, r.stderr)
    assert WM.grep_where(data, [b"one", b"two"], [(1, 0, 2)])[1] == [(0, 9), (40, 27)]
    r = run("-w", "+0,+1", "alpha", "beta")
    assert r.returncode == 1 and r.stdout == "0 records\n", (r.stdout, r.stderr)
    for args in (("-w", "+7", "one", "two"), ("-w", "+0,-0", "one"), ("-w", "0", "one"), ("-w", "+0,", "one"), ("-w", "+64", "one"), ("one",), ("-w", "+0"),
                 ["-w", "+0"] * 9 + ["one"]):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "", (args, r.stdout, r.stderr)
