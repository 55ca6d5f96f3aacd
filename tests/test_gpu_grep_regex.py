"""GPU tests of ZraHipGrepArchiveRegex and ZraHipArchiveGrepRegex (include/zra_hip.h): the records of a content range that a regular
expression matches. The yardstick everywhere is tests/regex_model.py on plaintext the test generated itself (held against Python's
`re` and against ZraHipCheckRegex in tests/test_regex_abi.py). Archives are written on the device. The shapes are the smallest at
which each seam exists: the scan's trip is 64 positions, its wave 2,048, its tile 8,192, a workgroup's group 8 tiles, the scan
kernel's lanes 1,024; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grep_model as GM
import regex_model as RM
import test_gpu_archive_scan as AS
import test_gpu_grep as G
from test_gpu_update import _compress, _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
ZERO = G.ZERO
TILE = 8192


class _Memo:
    """a matcher that walks the model's minimal DFA and remembers records: the contents here repeat a few short records"""

    def __init__(self, exprs, fold=False, delim=NL):
        self.m, self.memo = RM.TableMatcher(exprs, fold, delim), {}

    def matches(self, rec):
        if rec not in self.memo:
            self.memo[rec] = self.m.matches(rec)
        return self.memo[rec]


def _raw(eng, zra, d, size, exprs, cap, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, delim=NL):
    """(status, *nRecords, the bytes of a record array two entries longer than the capacity, 0xEE-filled before the call)"""
    arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n = ctypes.c_uint64(0x1234)
    sizes = (ctypes.c_uint32 * len(exprs))(*(len(p) for p in exprs))
    eng._order()
    st = zra.load().ZraHipGrepArchiveRegex(eng.h, d.data_ptr(), size, b"".join(exprs), sizes, len(exprs), syntax, delim, mode, offset, length, staging,
                                           arr if cap else None, cap, ctypes.byref(n)).tup()
    return st, n.value, bytes(arr)


def _check(eng, zra, d, size, data, fs, exprs, lo=0, hi=None, staging=0, fold=False, matcher=None, small=True):
    """one call per mode of [lo, hi) against the model: status, count, list and all eight stats; then the same call with a capacity
    below the count: the count stands, the first entries are the list's, and nothing is written behind the capacity. small: take the
    model's position sets, not its DFA (short contents). Returns {invert: selected}."""
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    matcher = matcher or (RM.Matcher(exprs, fold, NL) if small else _Memo(exprs, fold, NL))
    out = {}
    for inv in (False, True):
        recs, sel, nm = RM.grep_regex(data, exprs, NL, inv, fold, lo, hi, matcher=matcher)
        tag = (exprs, lo, hi, staging, inv)
        try:
            n, got = eng.grep_regex(d.data_ptr(), size, exprs, invert=inv, fold_case=fold, offset=lo, length=length, staging_bytes=staging)
            st = (0, 0)
        except zra.ZraError as e:
            st, n, got = (e.zra, e.zstd), 0, []
        print("regex", tag, "status", st, "selected", n, "model", len(sel))
        assert (st, n) == ((0, 0), len(sel)), (tag, st, n, len(sel))
        assert got == sel, (tag, sorted(set(got) ^ set(sel))[:10], got[:6], sel[:6])
        s = eng.grep_stats()
        if end == lo:
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == G._stats(U, fs, lo, end, staging, len(recs), len(sel), len(sel), nm), (tag, s)
        cap = min(len(sel) // 2, 3)
        st, n, mem = _raw(eng, zra, d, size, exprs, cap, int(inv), lo, MAXU64 if hi is None else hi - lo, staging, int(fold))
        want = b"".join(o.to_bytes(8, "little") + z.to_bytes(8, "little") for o, z in sel[:cap]) + b"\xEE" * 32
        assert (st, n, mem) == ((0, 0), len(sel), want), (tag, cap, st, n)
        if end != lo:
            assert eng.grep_stats() == G._stats(U, fs, lo, end, staging, len(recs), len(sel), cap, nm), (tag, cap)
        out[inv] = sel
    return out


def _text(rng, n, alphabet=b"abc", p_delim=0.0):
    a = rng.choice(list(alphabet), size=n).astype(np.uint8)
    if p_delim:
        a[rng.rand(n) < p_delim] = NL
    return bytearray(a.tobytes())


# ---- 1
def test_frame_size_4_one_slot_every_record_crosses_passes(zra, gpu_engine):
    """the state travels in the carried pair: one frame per pass, then the same content as one pass"""
    rng = np.random.RandomState(281)
    data = bytes(_text(rng, 230, b"aabc", 0.12)) + b"\n\nab\n\n\ncab"
    fs = 4
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for exprs in ([b"^a"], [b"c$"], [b"^$"], [b"(ab|ca)b"], [b"a+b"], [b"^(..)*$"], [b"^[ab]+c?$", b"cc"]):
        one = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=fs)
        assert gpu_engine.grep_stats()["passes"] == -(-len(data) // fs)
        whole = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=0)
        assert one == whole and one[False] and one[True], exprs
        _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=5, hi=len(data) - 6, staging=2 * fs)


# ---- 2
@pytest.mark.parametrize("ending", ["delimiter", "open"])
def test_delimiters_at_every_edge(zra, gpu_engine, ending):
    rng = np.random.RandomState(282)
    a = _text(rng, 3 * TILE + 700, b"abbc")
    for at in (0, 63, 64, 2047, 2048, 8191, 8192, 100, 101, 300, 301, 302, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 500):
        a[at] = NL
    a[-1] = NL if ending == "delimiter" else ord("a")
    data = bytes(a)
    fs = 4096
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for exprs in ([b"^$"], [b"^(..)*$"], [b"^a.*b$", b"^c"], [b"ab+c"]):
        for staging in (0, fs):
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=staging, small=False)
            if exprs == [b"^$"]:
                assert sel[False] == [(0, 0), (64, 0), (101, 0), (301, 0), (302, 0), (2048, 0), (8192, 0), (2 * TILE, 0), (2 * TILE + 1, 0)]
    # a record that ends exactly at a tile's last byte, and ranges that begin or end on a delimiter
    for lo, hi in ((0, 1), (63, 65), (64, 8192), (64, 8193), (8192, 8193), (2048, len(data)), (1, len(data) - 1)):
        _check(gpu_engine, zra, d, len(arc), data, fs, [b"^(..)*$"], lo=lo, hi=hi, small=False)


def test_content_without_a_delimiter(zra, gpu_engine):
    rng = np.random.RandomState(283)
    for n in (1, 63, 64, 65, TILE, TILE + 1, 2 * TILE + 77):
        data = bytes(_text(rng, n, b"ab"))
        fs = 4096
        arc = _compress(gpu_engine, zra, data, 3, fs, True)
        d = _dev(arc)
        for exprs in ([b"^(..)*$"], [b"^a.*b$"], [b"^$"]):
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, small=False)
            assert sel[False] + sel[True] == [(0, n)]
        _check(gpu_engine, zra, d, len(arc), data, fs, [b"^(..)*$"], staging=fs, small=False)


# ---- 3
@pytest.mark.parametrize("length", [30000, 30001])
def test_delimiter_free_tiles_compose_their_maps(zra, gpu_engine, length):
    """a long record among short ones: every tile inside it is one head. The record begins at an odd offset, so the parity automaton's
    map flips in its first and last tile; a whole tile keeps the parity, so `^(...)*$` is there too, whose map over 8,192 bytes is a
    rotation by two; `^a.*z$` hangs on the record's first byte and on its last, and its maps do not commute. A composition taken
    for the identity, or applied in the wrong order, fails here."""
    rng = np.random.RandomState(284)
    for first, last in (b"az", b"ay", b"bz"):
        long_ = _text(rng, length, b"abz")
        long_[0], long_[-1] = first, last
        data = bytes(_text(rng, 5000, b"abz", 0.05)) + b"\n" + bytes(long_) + b"\n" + bytes(_text(rng, 3000, b"abz", 0.05))
        fs = 4096
        arc = _compress(gpu_engine, zra, data, 3, fs, True)
        d = _dev(arc)
        for exprs in ([b"^(..)*$"], [b"^a.*z$"], [b"^(...)*$"]):
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, small=False)
            rec = (data.index(bytes(long_)), length)
            assert rec in sel[False] + sel[True]
            if exprs == [b"^(..)*$"]:
                assert (rec in sel[False]) == (length % 2 == 0)
            if exprs == [b"^a.*z$"]:
                assert (rec in sel[False]) == ((first, last) == tuple(b"az"))
        _check(gpu_engine, zra, d, len(arc), data, fs, [b"^(..)*$"], staging=2 * fs, small=False)
        _check(gpu_engine, zra, d, len(arc), data, fs, [b"^a.*z$"], lo=5003, hi=5001 + length + 300, small=False)


# ---- 4
def test_more_than_1024_tiles_in_one_pass(zra, gpu_engine):
    """a lane of the scan kernel owns two tiles (per = ceil(1030 / 1024)); delimiter-free stretches of three tiles and more cross the
    edges of the lanes' runs; two expressions, so that alternatives across the list are on the GPU too"""
    rng = np.random.RandomState(285)
    pool = [b"ab" * 20, b"", b"abab" * 9 + b"a", b"z" + b"ab" * 30, b"ab" * 25 + b"z", b"a" * 31, b"b" * 40, b"ba" * 33, b"z"]
    parts, size = [], 0
    longs = {3 * TILE: 3 * TILE + 5, 40 * TILE + 17: 3 * TILE, 511 * TILE - 9: 4 * TILE + 1, 900 * TILE: 3 * TILE + 64}
    target = 1030 * TILE - 4000
    while size < target:
        at = [k for k in longs if size >= k]
        if at:
            n = longs.pop(at[0])
            rec = bytes(_text(rng, n, b"ab"))
        else:
            rec = pool[int(rng.randint(0, len(pool)))]
        parts.append(rec)
        size += len(rec) + 1
    data = b"\n".join(parts)
    assert not longs and 1024 * TILE < len(data) <= 1030 * TILE
    fs = 1 << 16
    arc = _compress(gpu_engine, zra, data, 1, fs, True)
    d = _dev(arc)
    exprs = [b"^(..)*$", b"^z|z$"]
    m = _Memo(exprs)
    sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, matcher=m)
    assert gpu_engine.grep_stats()["passes"] == 1
    assert len(sel[False]) > 1000 and len(sel[True]) > 1000
    long_recs = [r for r in sel[False] + sel[True] if r[1] >= 3 * TILE]
    assert len(long_recs) == 4 and {r[1] % 2 for r in long_recs if r in sel[False]} == {0}


# ---- 5
def test_a_record_crosses_a_workgroups_group_of_tiles(zra, gpu_engine):
    rng = np.random.RandomState(286)
    edge = 8 * TILE
    a = _text(rng, 2 * edge + 2 * TILE, b"ab", 0.02)
    for lo, hi in ((edge - 700, edge + 300), (2 * edge - 3, 2 * edge + 2)):
        a[lo:hi] = bytes(_text(rng, hi - lo, b"ab"))
        a[lo - 1] = a[hi] = NL
    data = bytes(a)
    fs = 8192
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for exprs in ([b"^(..)*$"], [b"^a.*b$"]):
        sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, small=False)
        if exprs == [b"^(..)*$"]:
            assert (edge - 700, 1000) in sel[False] and (2 * edge - 3, 5) in sel[True]
        _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=700, hi=len(data) - 1, staging=3 * fs, small=False)   # (the tiles start at lo)


# ---- 6
def test_the_range_clips_records_and_anchors_hold_at_the_clip(zra, gpu_engine):
    data = b"xxGET /api\nyyPOST /x\n\nzz\nGET /a"
    fs = 8
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for exprs, lo, hi, want in (([b"^GET"], 2, 9, [(2, 7)]), ([b"^GET"], 0, 9, []), ([b"/ap$"], 2, 9, [(2, 7)]), ([b"/ap$"], 2, 10, []), ([b"^POST /x$"], 13, 30, [(13, 7)]),
                                ([b"^$"], 20, 22, [(20, 0), (21, 0)]), ([b"^$"], 21, 22, [(21, 0)]), ([b"^$"], 22, 22, []), ([b"^z$"], 22, 23, [(22, 1)]), ([b"^$"], 22, 23, []),
                                ([b"^ET", b"^y+P"], 1, len(data), [(11, 9)]), ([b"a*"], 10, 11, [(10, 0)]), ([b"^$"], len(data), len(data), [])):
        for staging in (0, fs):
            sel = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=lo, hi=hi, staging=staging)
            assert sel[False] == want, (exprs, lo, hi, sel[False])
    # fold case, and rule 1 with an engine: nothing decoded, nothing written
    assert _check(gpu_engine, zra, d, len(arc), data, fs, [b"^(get|post) "], lo=2, fold=True)[False] == [(2, 8), (25, 6)]
    for exprs, mode, syntax in (([b"a**"], 0, 0), ([b"\\n"], 0, 0), ([b"^.{63}$"], 0, 0), ([b"a"], 2, 0), ([b"a"], 0, 2), ([b"a"], 0, 4)):
        st, n, mem = _raw(gpu_engine, zra, d, len(arc), exprs, 2, mode=mode, syntax=syntax)
        assert (st, n, mem) == ((1, 42), 0, b"\xEE" * 64) and gpu_engine.grep_stats() == ZERO, exprs
    st, n, mem = _raw(gpu_engine, zra, d, len(arc), [b"a"], 2, offset=len(data) + 1)
    assert st[0] != 0 and n == 0 and mem == b"\xEE" * 64 and gpu_engine.grep_stats() == ZERO                     # the range rule: OutOfBounds


# ---- 7
@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames of the range resident"""
    fs = 1000
    data, pats = AS._content(77, fs)
    U = len(data)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, U, warm, slots)
    exprs = [b"^[a-c]+e|zz$", b"b{2,}a"]
    m = _Memo(exprs)
    try:
        for lo, hi in ((0, U), (6 * fs + fs // 2, 10 * fs + fs // 2)):
            for staging in (0, 3 * fs):
                kw = dict(offset=lo, length=hi - lo, staging_bytes=staging)
                before = h.stats()
                s0 = h.scan_stats()
                h.grep(pats, where=[(0, 1, 0)], **kw)
                s1 = h.scan_stats()
                got = h.grep_regex(exprs, **kw)
                s2 = h.scan_stats()
                hs = gpu_engine.grep_stats()
                want = gpu_engine.grep_regex(d.data_ptr(), len(arc), exprs, **kw)
                es = gpu_engine.grep_stats()
                model = RM.grep_regex(data, exprs, NL, False, False, lo, hi, matcher=m)
                assert got == want == (len(model[1]), model[1]) and got[0] > 0, (slots, lo, staging)
                staged, decoded, dec_bytes = AS._split(warm, fs, U, lo, hi)
                assert hs == dict(es, decoded=decoded, content_bytes=dec_bytes), (hs, es)
                # the handle's counters move as for the predicate grep on the same range
                assert {k: s2[k] - s1[k] for k in s1 if k.endswith("total") or k == "scans"} == {k: s1[k] - s0[k] for k in s1 if k.endswith("total") or k == "scans"}
                assert (s2["staged"], s2["decoded"], s2["passes"]) == (s1["staged"], s1["decoded"], s1["passes"]) and (s2["staged"], s2["decoded"]) == (staged, decoded)
                assert h.stats() == before                                     # a scan is not a read
    finally:
        h.close()


# ---- 8
def test_cli_mode_glr(zra, gpu_engine, tmp_path):
    data = b"GET /api/x took 12ms\nPOST /api/y took 1234ms\n\nget /other\nstatus=503 upstream timeout"
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "glr", str(p_arc)] + [str(x) for x in args], capture_output=True, text=True, timeout=120)

    for args, exprs, inv, fold, count in ((("^(GET|POST) /api/",), [b"^(GET|POST) /api/"], False, False, False), (("-v", "took [0-9]{4,}ms$", "^$"), [b"took [0-9]{4,}ms$", b"^$"], True, False, False),
                                          (("-i", "^get"), [b"^get"], False, True, False), (("-c", "status=5[0-9]+ .*timeout"), [b"status=5[0-9]+ .*timeout"], False, False, True)):
        sel = RM.grep_regex(data, exprs, NL, inv, fold)[1]
        r = run(*args)
        want = ([] if count else ["%d\t%d" % x for x in sel]) + ["%d records" % len(sel), ""]
        assert r.returncode == 0 and r.stdout.split("\n") == want and sel, (args, r.stdout, r.stderr)
    r = run("^nothing$")
    assert r.returncode == 1 and r.stdout == "0 records\n", (r.stdout, r.stderr)
    for args in (("a**",), ("ok", "(a"), ("\\n",), ("^.{63}$",), ()):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "" and r.stderr, (args, r.stdout, r.stderr)
