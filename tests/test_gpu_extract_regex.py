"""GPU tests of ZraHipExtractRecordsRegex and ZraHipArchiveExtractRecordsRegex (include/zra_hip.h): the records a regular expression
selects WITH their bytes, packed. The yardstick everywhere is tests/extract_regex_model.py on plaintext the test generated itself:
regex_model's selection (held against Python's `re` in tests/test_regex_abi.py) and extract_model's packing. Archives are written on
the device. dData is a 0xEE-filled buffer handed over 64 bytes in, with a capacity that leaves 64 guard bytes behind it: after every
call both guards are still 0xEE. Every case runs in both modes and, unless it is about emptiness, asserts that both select something.
The shapes are the smallest at which each seam exists: the scan's trip is 64 positions, its wave 2,048, its tile 8,192, a workgroup's
group 8 tiles, the scan kernel's lanes 1,024; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import extract_regex_model as XRM
import grep_model as GM
import test_gpu_archive_scan as AS
import test_gpu_extract as X
from test_gpu_grep_regex import _Memo, _text
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
GUARD = 64
TILE = 8192
ZERO, TOO_SMALL = X.ZERO, X.TOO_SMALL


def _raw(eng, zra, d, size, exprs, data_cap, rec_cap, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, delim=NL, handle=None):
    """(status, *nRecords, *dataSize, the bytes of a record array two entries longer than the capacity, the first data_cap bytes of
    dData) of one call, through `handle` when there is one; both 0xEE-filled before it. Asserts that the guards in front of dData and
    behind its capacity are intact."""
    import torch
    buf = torch.full((GUARD + data_cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (2 * (rec_cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
    sizes = (ctypes.c_uint32 * len(exprs))(*(len(p) for p in exprs))
    eng._order()
    tail = (b"".join(exprs), sizes, len(exprs), syntax, delim, mode, offset, length, staging, arr if rec_cap else None, rec_cap, ctypes.byref(n),
            buf.data_ptr() + GUARD, data_cap, ctypes.byref(ds))
    if handle is None:
        st = zra.load().ZraHipExtractRecordsRegex(eng.h, d.data_ptr(), size, *tail).tup()
    else:
        st = zra.load().ZraHipArchiveExtractRecordsRegex(handle.h, *tail).tup()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().tobytes()
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + data_cap:] == b"\xEE" * GUARD, ("guard", st, data_cap, rec_cap, mode, offset, length, staging)
    return st, n.value, ds.value, bytes(arr), host[GUARD:GUARD + data_cap]


def _check(eng, zra, d, size, data, fs, exprs, lo=0, hi=None, staging=0, fold=False, matcher=None, slack=5, nonempty=True):
    """one extract per mode of [lo, hi) against the model: status, both words, the packed bytes, the list, all eight stats, and the
    grep's and the searches' stats as they were. Returns {invert: (selected, packed)}."""
    U = len(data)
    end = U if hi is None else hi
    matcher = matcher or _Memo(exprs, fold, NL)
    others = (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats())
    out = {}
    for inv in (False, True):
        recs, sel, nm, packed = XRM.extract_regex(data, exprs, NL, inv, fold, lo, hi, matcher=matcher)
        tag = (exprs, lo, hi, staging, inv)
        st, n, ds, mem, got = _raw(eng, zra, d, size, exprs, len(packed) + slack, len(sel) + 1, int(inv), lo, MAXU64 if hi is None else hi - lo, staging, int(fold))
        print("extract_regex", tag, "status", st, "selected", n, "model", len(sel), "bytes", ds, "model", len(packed))
        assert (st, n, ds) == ((0, 0), len(sel), len(packed)), (tag, st, n, ds, len(sel), len(packed))
        if got[:ds] != packed:
            bad = next(i for i in range(ds) if got[i] != packed[i])
            raise AssertionError((tag, "first wrong byte", bad, got[max(0, bad - 8):bad + 8], packed[max(0, bad - 8):bad + 8]))
        assert X._pairs(mem, n) == sel and mem[16 * n:] == b"\xEE" * (16 * (len(sel) + 3 - n)), tag
        s = eng.extract_stats()
        if end == lo:
            assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)    # nothing decoded
        else:
            assert s == X._stats(U, fs, lo, end, staging, len(recs), len(sel), len(packed), nm), (tag, s)
        assert (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats()) == others, tag
        out[inv] = (sel, packed)
    if nonempty:
        assert out[False][0] and out[True][0], (exprs, lo, hi, "a test that selects nothing shows nothing")
    return out


# ---- 1
def test_frame_size_4_one_slot_every_record_crosses_passes(zra, gpu_engine):
    """the state and the packed offset travel in the carried words: one frame per pass, then the same content as one pass"""
    rng = np.random.RandomState(291)
    data = bytes(_text(rng, 230, b"aabc", 0.12)) + b"\n\nab\n\n\ncab"
    fs = 4
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    gpu_engine.grep_regex(d.data_ptr(), len(arc), [b"a"])                      # (the grep's stats are not all zero when they are compared)
    for exprs in ([b"^a"], [b"c$"], [b"^$"], [b"a+b"], [b"^(..)*$"], [b"^[ab]+c?$", b"cc"]):
        one = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=fs, slack=len(data))
        assert gpu_engine.extract_stats()["passes"] == -(-len(data) // fs)
        whole = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=0)
        assert one == whole, exprs
        _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=5, hi=len(data) - 6, staging=2 * fs, slack=len(data))


# ---- 2
@pytest.mark.parametrize("what", ["selected later", "overwritten", "behind dataSize"])
def test_provisional_tail(zra, gpu_engine, what):
    """Frames of 64 bytes, passes of two. A record of 700 bytes is open at the end of five passes in a row and is copied provisionally
    by each; `x$` decides it by its last byte. (a) It ends in x: the parts must line up at one packed offset. (b) It does not, and a
    selected record follows: that one overwrites what the passes left. (c) It does not and nothing follows: what they left lies
    behind *dataSize. A capacity of the whole content lets every provisional byte land inside the buffer."""
    rng = np.random.RandomState(292)
    fs = 64
    head = b"".join(bytes(_text(rng, int(rng.randint(0, 20)), b"abx")) + b"\n" for _ in range(14))
    body = bytes(_text(rng, 699, b"ab"))
    data = head + body + {"selected later": b"x\nab\nbx\nb", "overwritten": b"y\nab\nbx\nb", "behind dataSize": b"y"}[what]
    data += b"!" * (len(data) % fs == 0)                                       # (a short last frame)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    big = (len(head), 700)
    for staging in (2 * fs, 0):
        out = _check(gpu_engine, zra, d, len(arc), data, fs, [b"x$"], staging=staging, slack=len(data))
        assert (big in out[False][0], big in out[True][0]) == (what == "selected later", what != "selected later"), (what, staging)
        if staging:
            assert gpu_engine.extract_stats()["passes"] == -(-len(data) // (2 * fs)) >= 7
        if what == "overwritten":
            assert out[False][1].endswith(b"x\nbx\n") and out[True][1].endswith(body + b"y\nab\nb\n")
        if what == "behind dataSize":
            assert out[False][0][-1][0] < len(head) and out[True][0][-1] == big


# ---- 3
@pytest.mark.parametrize("ending", ["delimiter", "open"])
def test_delimiters_at_every_edge(zra, gpu_engine, ending):
    rng = np.random.RandomState(293)
    a = _text(rng, 3 * TILE + 700, b"abbc")
    for at in (0, 63, 64, 2047, 2048, 8191, 8192, 100, 101, 300, 301, 302, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 500):
        a[at] = NL
    a[-1] = NL if ending == "delimiter" else ord("a")
    data = bytes(a)
    fs = 4096
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    for exprs in ([b"^$"], [b"^(..)*$"], [b"^a.*b$", b"^c"]):
        for staging in (0, fs):
            out = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=staging, slack=len(data))
            if exprs == [b"^$"]:
                assert out[False][1] == b"\n" * 9 and out[False][0][:3] == [(0, 0), (64, 0), (101, 0)]
    # a record that ends exactly at a tile's last byte, and ranges that begin or end on a delimiter
    for lo, hi in ((64, 8192), (64, 8193), (2048, len(data)), (1, len(data) - 1)):
        for exprs in ([b"^(..)*$"], [b"^a.*b$", b"^c"]):                         # (a clipped range may leave one mode nothing: the whole content above does not)
            _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=lo, hi=hi, nonempty=False)


def test_delimiters_only_and_no_delimiter(zra, gpu_engine):
    """(about emptiness: one mode selects everything, the other nothing)"""
    fs = 4096
    only = b"\n" * 2500
    arc = _compress(gpu_engine, zra, only, 3, fs, True)
    for staging in (0, fs):
        out = _check(gpu_engine, zra, _dev(arc), len(arc), only, fs, [b"^$"], staging=staging, nonempty=False)
        assert out[False][1] == only and out[True] == ([], b"")
    rng = np.random.RandomState(294)
    for n in (1, 63, 64, 65, TILE, TILE + 1, 2 * TILE + 77):
        data = bytes(_text(rng, n, b"ab"))
        arc = _compress(gpu_engine, zra, data, 3, fs, True)
        d = _dev(arc)
        for exprs in ([b"^(..)*$"], [b"^a.*b$"]):
            for staging in (0, fs):
                out = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=staging, slack=n, nonempty=False)
                assert sorted([out[False], out[True]]) == [([], b""), ([(0, n)], data + b"\n")]     # one record plus one added delimiter


# ---- 4
@pytest.mark.parametrize("ends", [b"az", b"ay"])
def test_look_ahead_across_tiles(zra, gpu_engine, ends):
    """One record of 30,000 bytes and one of 30,001 among short ones: the tiles inside them hold no delimiter, and whether their bytes
    are copied is decided by a delimiter up to four tiles behind them. `^a.*z$` hangs on the first and the last byte (selected with
    `az`, not with `ay`), `^(..)*$` on the parity (30,000 selected, 30,001 not): a build that lists correctly but copies by a wrong
    bit fails here."""
    rng = np.random.RandomState(295)
    longs = []
    for n in (30000, 30001):
        r = _text(rng, n, b"abz")
        r[0], r[-1] = ends[0], ends[1]
        longs.append(bytes(r))
    data = bytes(_text(rng, 5000, b"abz", 0.05)) + b"\n" + longs[0] + b"\n" + bytes(_text(rng, 3000, b"abz", 0.05)) + b"\n" + longs[1] + b"\n" + \
        bytes(_text(rng, 3000, b"abz", 0.05))
    fs = 4096
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    recs = [(data.index(r), len(r)) for r in longs]
    for exprs in ([b"^a.*z$"], [b"^(..)*$"]):
        for staging in (0, 2 * fs):
            out = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, staging=staging, slack=len(data) if staging else 5)
            if exprs == [b"^a.*z$"]:
                assert [r in out[False][0] for r in recs] == [ends == b"az"] * 2 and [r in out[True][0] for r in recs] == [ends != b"az"] * 2
            else:
                assert [r in out[False][0] for r in recs] == [True, False] and [r in out[True][0] for r in recs] == [False, True]
    _check(gpu_engine, zra, d, len(arc), data, fs, [b"^a.*z$"], lo=5003, hi=5001 + 30000 + 300, nonempty=False)


# ---- 5
def test_more_than_1024_tiles_in_one_pass(zra, gpu_engine):
    """1,030 tiles: a lane of the scan kernel owns two (per = ceil(1030 / 1024)); delimiter-free stretches of three and four tiles cross
    the edges of the lanes' runs, and the one at 511 tiles crosses a workgroup's group of 8"""
    rng = np.random.RandomState(296)
    pool = [b"ab" * 20, b"", b"abab" * 9 + b"a", b"z" + b"ab" * 30, b"ab" * 25 + b"z", b"a" * 31, b"b" * 40, b"ba" * 33, b"z"]
    parts, size = [], 0
    longs = {3 * TILE: 3 * TILE + 5, 40 * TILE + 17: 3 * TILE, 511 * TILE - 9: 4 * TILE + 1, 900 * TILE: 3 * TILE + 64}
    target = 1030 * TILE - 4000
    while size < target:
        at = [k for k in longs if size >= k]
        if at:
            rec = bytes(_text(rng, longs.pop(at[0]), b"ab"))
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
    out = _check(gpu_engine, zra, d, len(arc), data, fs, exprs)
    assert gpu_engine.extract_stats()["passes"] == 1
    assert len(out[False][0]) > 1000 and len(out[True][0]) > 1000
    long_recs = [r for r in out[False][0] + out[True][0] if r[1] >= 3 * TILE]
    assert len(long_recs) == 4 and {r[1] % 2 for r in long_recs if r in out[False][0]} == {0}


# ---- 6
def test_the_range_clips_records_and_anchors_hold_at_the_clip(zra, gpu_engine):
    data = b"xxGET /api\nyyPOST /x\n\nzz\nGET /a"
    fs = 8
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    # (expressions, lo, hi, the plain selection); the ranges of more than one record select something in both modes
    for exprs, lo, hi, want in (([b"^GET"], 2, 25, [(2, 8)]), ([b"^GET"], 0, len(data), [(25, 6)]), ([b"/ap$"], 2, 9, [(2, 7)]), ([b"/ap$"], 2, 10, []),
                                ([b"^POST /x$"], 13, 30, [(13, 7)]), ([b"^$"], 20, 22, [(20, 0), (21, 0)]), ([b"^$"], 21, 22, [(21, 0)]), ([b"^$"], 22, 22, []),
                                ([b"^z$"], 22, 23, [(22, 1)]), ([b"^$"], 22, 23, []), ([b"^ET", b"^y+P"], 1, len(data), [(11, 9)]), ([b"a*"], 10, 11, [(10, 0)]),
                                ([b"^$"], len(data), len(data), []), ([b"^$"], 0, 0, []), ([b"x"], 0, 1, [(0, 1)]), ([b"^.$"], 9, 10, [(9, 1)])):
        for staging in (0, fs):
            several = len(GM.records(data, NL, lo, hi)) > 1 and want and exprs != [b"^$"]
            out = _check(gpu_engine, zra, d, len(arc), data, fs, exprs, lo=lo, hi=hi, staging=staging, nonempty=bool(several))
            assert out[False][0] == want, (exprs, lo, hi, out[False][0])
            if hi == lo:
                assert out[True] == ([], b"")
    assert _check(gpu_engine, zra, d, len(arc), data, fs, [b"^(get|post) "], lo=2, fold=True)[False] == ([(2, 8), (25, 6)], b"GET /api\nGET /a\n")
    # rule 1 with an engine: nothing decoded, nothing written; then the range rule
    for exprs, mode, syntax in (([b"a**"], 0, 0), ([b"\\n"], 0, 0), ([b"^.{63}$"], 0, 0), ([b"a"], 2, 0), ([b"a"], 0, 2), ([b"a"], 0, 4)):
        st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), exprs, 64, 2, mode=mode, syntax=syntax)
        assert (st, n, ds, mem, got) == ((1, 42), 0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO, exprs
    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), [b"a"], 64, 2, offset=len(data) + 1)
    assert st[0] != 0 and (n, ds, mem, got) == (0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO   # OutOfBounds


# ---- 7
def test_capacity(zra, gpu_engine):
    import torch
    fs = 1024
    data = X._lines(np.random.RandomState(297), 6 * fs + 300)
    U = len(data)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    exprs = [b"^[a-c]+e|dd$", b"b{2,}a"]
    for mode in (0, 1):
        recs, sel, nm, packed = XRM.extract_regex(data, exprs, NL, bool(mode))
        total, size = len(sel), len(packed)
        assert total > 5
        for dcap in (0, size - 1, size, size + 5):
            for rcap in (0, total - 1, total):
                for staging in (0, fs):
                    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), exprs, dcap, rcap, mode=mode, staging=staging)
                    tag = (mode, dcap, rcap, staging, st, n, ds)
                    fits = dcap >= size and (rcap == 0 or rcap >= total)
                    assert (st, n, ds) == ((0, 0) if fits else TOO_SMALL, total, size), tag   # the two words hold what the call needs
                    if fits:
                        assert got[:size] == packed, tag
                        assert X._pairs(mem, rcap) == sel[:rcap] and mem[16 * rcap:] == b"\xEE" * 32, tag
                        assert gpu_engine.extract_stats() == X._stats(U, fs, 0, U, staging, len(recs), total, size, nm), tag
                    else:
                        assert mem == b"\xEE" * (16 * (rcap + 2)), tag           # hRecords untouched
                        assert gpu_engine.extract_stats() == ZERO, tag
                        if dcap:
                            assert got[:min(dcap, size)] == packed[:dcap], tag   # what fits is in place
    # the Python layer: the sizing call carries what is needed, the call returns the triple
    want = XRM.extract_regex(data, exprs)
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.extract_regex(d.data_ptr(), len(arc), exprs, 0, 0)
    assert (e.value.zra, e.value.needed_records, e.value.needed_data) == (6, len(want[1]), len(want[3]))
    out = torch.empty(e.value.needed_data, dtype=torch.uint8, device="cuda:0")
    assert gpu_engine.extract_regex(d.data_ptr(), len(arc), exprs, out.data_ptr(), out.numel(), max_records=e.value.needed_records) == (len(want[1]), len(want[3]), want[1])
    assert out.cpu().numpy().tobytes() == want[3] and gpu_engine.extract_ms() > 0
    assert gpu_engine.extract_regex(d.data_ptr(), len(arc), exprs, out.data_ptr(), out.numel(), invert=True, length=0) == (0, 0, [])
    inv = XRM.extract_regex(data, [b"^[A-C]+E|DD$"], NL, True, True, fs, 3 * fs)
    big = torch.empty(2 * fs, dtype=torch.uint8, device="cuda:0")
    assert gpu_engine.extract_regex(d.data_ptr(), len(arc), [b"^[A-C]+E|DD$"], big.data_ptr(), big.numel(), invert=True, fold_case=True, offset=fs, length=2 * fs,
                                    staging_bytes=fs, max_records=len(inv[1])) == (len(inv[1]), len(inv[3]), inv[1])
    assert big[:len(inv[3])].cpu().numpy().tobytes() == inv[3] and inv[1]


# ---- 8
def test_a_damaged_frame_and_an_overlapping_buffer(zra, gpu_engine):
    import torch
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    exprs = [b"^[\\x00-\\x09].*[\\x0b-\\x17]$"]                             # (_data's alphabet is the bytes 0 .. 23)
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs):
            st, n, ds, mem, _ = _raw(gpu_engine, zra, db, len(bad), exprs, 13 * fs, 6, mode=mode, staging=staging)
            assert (st, n, ds, mem) == ((1, want[7]), 0, 0, b"\xEE" * 128), (mode, staging, st, n, ds)
            assert gpu_engine.extract_stats() == ZERO
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), data, fs, exprs, lo, hi)
    # rule 2: dData inside the archive, the archive inside dData, one byte of overlap at either end; touching is no overlap
    size = len(arc)
    whole = torch.full((512 + size + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
    whole[512:512 + size] = _dev(arc)
    P = whole.data_ptr() + 512
    L = zra.load()
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
    one = (ctypes.c_uint32 * 1)(len(exprs[0]))
    for dptr, dcap in ((P + 100, 50), (P - 256, size + 512), (P - 10, 11), (P + size - 1, 10)):
        n.value, ds.value = 0x1234, 0x5678
        assert L.ZraHipExtractRecordsRegex(gpu_engine.h, P, size, exprs[0], one, 1, 0, NL, 0, 0, MAXU64, 0, None, 0, ctypes.byref(n), dptr, dcap, ctypes.byref(ds)).tup() == (1, 42)
        assert (n.value, ds.value) == (0, 0) and gpu_engine.extract_stats() == ZERO
    model = XRM.extract_regex(data, exprs, hi=400)
    for dptr in (P - 512, P + size):
        st = L.ZraHipExtractRecordsRegex(gpu_engine.h, P, size, exprs[0], one, 1, 0, NL, 0, 0, 400, 0, None, 0, ctypes.byref(n), dptr, 512, ctypes.byref(ds)).tup()
        assert (st, n.value, ds.value) == ((0, 0), len(model[1]), len(model[3])) and model[1]
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert host[512:512 + size] == arc and host[512 + size:512 + size + len(model[3])] == model[3]   # the archive is only read


# ---- 9
@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames of the range resident: the plain call's answers, an unchanged cache, the handle's counters as for
    ZraHipArchiveExtractRecords"""
    fs = 1000
    data, pats = AS._content(77, fs)
    U = len(data)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, U, warm, slots)
    exprs = [b"^[a-c]+e|zz$", b"b{2,}a"]
    m = _Memo(exprs)
    moved = lambda a, b: {k: b[k] - a[k] for k in a if k.endswith("total") or k == "scans"}
    try:
        for lo, hi in ((0, U), (6 * fs + fs // 2, 10 * fs + fs // 2)):
            for staging in (0, 3 * fs):
                for inv in (False, True):
                    recs, sel, nm, packed = XRM.extract_regex(data, exprs, NL, inv, False, lo, hi, matcher=m)
                    assert sel
                    before = h.stats()
                    s0 = h.scan_stats()
                    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), exprs, len(packed) + 5, len(sel) + 1, int(inv), lo, hi - lo, staging, handle=h)
                    s1 = h.scan_stats()
                    hs = gpu_engine.extract_stats()
                    assert (st, n, ds, got[:ds]) == ((0, 0), len(sel), len(packed), packed) and X._pairs(mem, n) == sel, (slots, lo, staging, inv)
                    want = _raw(gpu_engine, zra, d, len(arc), exprs, len(packed) + 5, len(sel) + 1, int(inv), lo, hi - lo, staging)
                    es = gpu_engine.extract_stats()
                    assert want[:4] == (st, n, ds, mem) and want[4][:ds] == packed
                    staged, decoded, dec_bytes = AS._split(warm if slots else (), fs, U, lo, hi)
                    assert hs == dict(es, decoded=decoded, content_bytes=dec_bytes), (hs, es)
                    assert es == X._stats(U, fs, lo, hi, staging, len(recs), len(sel), len(packed), nm)
                    assert moved(s0, s1) == dict(scans=1, staged_total=staged, decoded_total=decoded), (s0, s1)
                    assert (s1["staged"], s1["decoded"]) == (staged, decoded)
                    assert h.stats() == before                                     # a scan is not a read
        # the same range through ZraHipArchiveExtractRecords moves the handle's counters by as much
        lo, hi = 6 * fs + fs // 2, 10 * fs + fs // 2
        s0 = h.scan_stats()
        with pytest.raises(zra.ZraError):
            h.extract(pats, 0, 0, offset=lo, length=hi - lo)                   # (the sizing call: OutputBufferTooSmall, not an accepted scan)
        assert h.scan_stats() == s0
        with pytest.raises(zra.ZraError):
            h.extract_regex(exprs, 0, 0, offset=lo, length=hi - lo)
        assert h.scan_stats() == s0
        with pytest.raises(zra.ZraError) as e:                                 # rule 2: dData inside the archive
            h.extract_regex(exprs, d.data_ptr() + 8, 16)
        assert (e.value.zra, e.value.zstd) == (1, 42) and h.scan_stats() == s0
        assert h.extract_regex(exprs, 0, 0, length=0) == (0, 0, [])
    finally:
        h.close()


# ---- 10
def test_cli_mode_gxr(zra, gpu_engine, tmp_path):
    data = b"GET /api/x took 12ms\nPOST /api/y took 1234ms\n\nget /other\nstatus=503 upstream timeout"
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc, p_out = tmp_path / "lines.zra", tmp_path / "out.txt"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "gxr", str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    for args, exprs, inv, fold, delim in ((("^(GET|POST) /api/",), [b"^(GET|POST) /api/"], False, False, NL), (("-v", "took [0-9]{4,}ms$", "^$"), [b"took [0-9]{4,}ms$", b"^$"], True, False, NL),
                                          (("-i", "^get"), [b"^get"], False, True, NL), (("status=5[0-9]+ .*timeout",), [b"status=5[0-9]+ .*timeout"], False, False, NL),
                                          (("-v", "-i", "-d", "20", "^TOOK$"), [b"^TOOK$"], True, True, 0x20)):
        packed = XRM.extract_regex(data, exprs, delim, inv, fold)[3]
        r = run(*args)
        assert r.returncode == 0 and r.stdout == packed and packed, (args, r.stdout, r.stderr)
        r = run("-o", p_out, *args)
        assert r.returncode == 0 and r.stdout == b"" and p_out.read_bytes() == packed, (args, r.stdout, r.stderr)
        p_out.unlink()
    r = run("^nothing$")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    for args in (("a**",), ("ok", "(a"), ("\\n",), ("^.{63}$",), (), ("-o",), ("-o", p_out), ("-d", "100", "a")):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr, (args, r.stdout, r.stderr)
