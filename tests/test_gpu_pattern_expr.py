"""GPU tests of the scans with a pattern syntax word (include/zra_hip.h: ZraHipSearchArchiveMultiExpr, ZraHipGrepArchiveExpr,
ZraHipExtractRecordsExpr and their handle twins): case folding and byte classes, every element of a pattern matching exactly one byte.
The yardstick everywhere is the plaintext the test generated itself, compiled, cut and scanned on the CPU (tests/expr_model.py,
cross-checked against Python's `re` in tests/test_pattern_expr.py); `matches` is also held equal across the three calls. Archives are
written on the device. The shapes are the smallest at which each seam exists: the scan's trip is 64 positions, its wave 2,048, its
tile 8,192; a pass is a whole number of frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expr_model as XM
import test_gpu_extract as X
import test_gpu_grep as G
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
FOLD, CLASSES = XM.FOLD_CASE, XM.CLASSES
MZERO = dict(frames=0, decoded=0, content_bytes=0, matches=0, listed=0, passes=0, patterns=0, survivors=0)


def _esc(p):
    """the expression that matches the bytes p literally: every special byte escaped"""
    return b"".join(b"\\" + bytes([c]) if c in XM.ESCAPABLE else bytes([c]) for c in p)


def _lens(pats, syntax, delim=None):
    return [len(p) for p in pats] if syntax == 0 else XM.lengths(XM.compile(pats, syntax, delim))


def _check(eng, zra, d, size, data, fs, pats, syntax, lo=0, hi=None, staging=0, delim=NL, modes=(False, True), records=True):
    """One multi search, and per mode one grep and one extract, of [lo, hi) against the model: status, counts, lists, packed bytes and
    all the stats. Returns (matches, {invert: selected}, {invert: packed})."""
    import torch
    U = len(data)
    end = U if hi is None else hi
    length = None if hi is None else hi - lo
    P = d.data_ptr()
    tag = (syntax, lo, hi, staging)
    want = XM.matches_multi(data, pats, syntax, lo, hi)
    n, at, per = eng.search_multi(P, size, pats, offset=lo, length=length, staging_bytes=staging, max_matches=len(want) + 8, syntax=syntax)
    assert n == len(want), (tag, n, len(want))
    assert at == want, (tag, sorted(set(at) ^ set(want))[:10], at[:6], want[:6])
    assert per == [sum(1 for _, i in want if i == j) for j in range(len(pats))], (tag, per)
    s = eng.search_multi_stats()
    assert (s["matches"], s["listed"], s["patterns"], s["survivors"]) == (len(want), len(want), len(pats), XM.survivors(data, pats, syntax, lo, hi)), (tag, s)
    sel, packed = {}, {}
    if not records:
        return want, sel, packed
    m_min = min(_lens(pats, syntax, delim))
    same = syntax == 0 or not any(delim in e for pat in XM.compile(pats, syntax, None) for e in pat)   # no element lost the delimiter
    for inv in modes:
        recs, sel[inv], matches, packed[inv] = XM.extract(data, pats, syntax, delim, inv, lo, hi)
        gn, glist = eng.grep(P, size, pats, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging, max_records=len(recs) + 1, syntax=syntax)
        assert (gn, glist) == (len(sel[inv]), sel[inv]), (tag, inv, gn, len(sel[inv]), sorted(set(glist) ^ set(sel[inv]))[:6])
        gs = eng.grep_stats()
        nothing = end == lo or (not inv and end - lo < m_min)
        if nothing:
            assert gs == dict(G.ZERO, frames=-(-U // fs)) and not sel[inv], (tag, gs)
        else:
            assert gs == G._stats(U, fs, lo, end, staging, len(recs), len(sel[inv]), len(sel[inv]), matches), (tag, inv, gs)
        assert not same or matches == len(want), (tag, matches, len(want))
        buf = torch.full((len(packed[inv]) + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        xn, ds, xlist = eng.extract(P, size, pats, buf.data_ptr(), len(packed[inv]) + 5, delimiter=delim, invert=inv, offset=lo, length=length, staging_bytes=staging,
                                    max_records=len(recs) + 1, syntax=syntax)
        torch.cuda.synchronize()
        host = buf.cpu().numpy().tobytes()
        assert (xn, ds, xlist) == (len(sel[inv]), len(packed[inv]), sel[inv]), (tag, inv, xn, ds)
        assert host[:ds] == packed[inv] and host[ds + 5:] == b"\xEE" * (59), (tag, inv)
        xs = eng.extract_stats()
        if nothing:
            assert xs == dict(X.ZERO, frames=-(-U // fs)), (tag, xs)
        else:
            assert xs == X._stats(U, fs, lo, end, staging, len(recs), len(sel[inv]), len(packed[inv]), matches), (tag, inv, xs)
    return want, sel, packed


# ---- 1
@pytest.mark.parametrize("staging", [0, 1])
def test_literal_expressions_through_the_class_kernels_at_frame_size_4(zra, gpu_engine, staging):
    """tests/test_gpu_grep.py's first shape over an alphabet with special bytes: about 260 frames of 4 bytes; with one slot a pass holds
    4 bytes, far below M - 1 = 39. The escaped expressions give, through the class kernels, what the literal kernels give."""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"a.[e"), size=60).astype(np.uint8))
    data = G._lines(rng, 500, b"a.c[e*") + b"\n" + long_line + b"\n" + G._lines(rng, 480, b"a.c[e*")
    pats = [b".", b"c[a", long_line[5:45], b"zz", b"e*", b"[e"]
    arc = _compress(gpu_engine, zra, data, 3, 4, True)
    d = _dev(arc)
    lit = _check(gpu_engine, zra, d, len(arc), data, 4, pats, 0, staging=staging)
    cls = _check(gpu_engine, zra, d, len(arc), data, 4, [_esc(p) for p in pats], CLASSES, staging=staging)
    assert cls == lit and len(lit[0]) > 200 and (501, 60) in lit[1][False] and len(lit[1][True]) > 5
    assert gpu_engine.grep_stats()["passes"] == (-(-len(data) // 4) if staging else 1)


FS = 1024


@pytest.fixture(scope="module")
def text(zra, gpu_engine):
    """tests/test_gpu_grep.py's `text`: 6 frames of 1,024 bytes and a last one of 300, delimiters forced at frame and pass boundaries"""
    U = 6 * FS + 300
    a = bytearray(_data(np.random.RandomState(33), U))
    a[FS - 1] = NL; a[2 * FS] = NL; a[4 * FS] = NL; a[4 * FS - 1] = 1; a[U - 1] = 2
    a[3 * FS - 100:3 * FS + 200] = b"\n" * 300
    data = bytes(a)
    pats = [data[700:703], data[5 * FS + 40:5 * FS + 42], data[5 * FS - 9:5 * FS + 9]]
    assert NL not in b"".join(pats)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    return dict(data=data, arc=arc, d=_dev(arc), pats=pats, U=U)


def test_literal_expressions_through_the_class_kernels_on_text(zra, gpu_engine, text):
    data, arc, d, pats = text["data"], text["arc"], text["d"], text["pats"]
    for staging in (0, 2 * FS, 1):
        for lo, hi in ((FS - 1, 2 * FS + 1), (3 * FS - 101, 3 * FS + 201), (0, None)):
            lit = _check(gpu_engine, zra, d, len(arc), data, FS, pats, 0, lo, hi, staging)
            assert _check(gpu_engine, zra, d, len(arc), data, FS, [_esc(p) for p in pats], CLASSES, lo, hi, staging) == lit
    assert len(lit[0]) > 10 and len(lit[1][False]) > 5 and any(i == 2 for _, i in lit[0])


# ---- 2
def test_fold(zra, gpu_engine):
    words = [b"error", b"ERROR", b"Error", b"eRRoR", b"errorerror", b"terror", b"err0r", b"@[`{", b"`{@[", b"@{`[", b"\xc1\xe1", b"\xe1\xc1", b"\xc1\xc1"]
    rng = np.random.RandomState(2)
    out = bytearray(bytes(range(256)) + b"\n")
    while len(out) < 5000:
        out += b" ".join(words[i] for i in rng.randint(0, len(words), size=int(rng.randint(0, 5)))) + b"\n"
    data = bytes(out) + bytes(range(255, -1, -1))
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    pats = [b"error", b"ERROR", b"eRrOr", b"@[`{", b"\xc1\xc1", b"\xe1"]
    for syntax, p in ((FOLD, pats), (FOLD | CLASSES, [_esc(x) for x in pats[:4]] + [b"\\xc1\\xC1", b"\\xe1"])):
        for staging in (0, FS):
            want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, FS, p, syntax, staging=staging)
            at = [[o for o, i in want if i == j] for j in range(6)]
            assert at[0] == at[1] == at[2] and len(at[0]) > 100
            exact = XM.matches_multi(data, pats, 0)
            assert [at[3], at[4], at[5]] == [[o for o, i in exact if i == j] for j in (3, 4, 5)] and len(at[3]) > 20 and len(at[4]) > 20
    assert 0 < len([o for o, i in XM.matches_multi(data, pats, 0) if i == 0]) < len(at[0]) - 100   # (without fold: only the lower-case ones)


# ---- 3
def _log(rng, n):
    out = bytearray()
    while len(out) < n:
        out += b"ts=20%02d-%02d-%02d status=%d id=%04x%s\n" % (rng.randint(0, 100), rng.randint(1, 13), rng.randint(1, 29), rng.choice([200, 404, 503, 500, 51]),
                                                             rng.randint(0, 65536), rng.choice([b"", b" x", b" ID=00FG", b"f"]))
    return bytes(out[:n - 3]) + b"end"


def test_sets(zra, gpu_engine):
    data = _log(np.random.RandomState(3), 20000)
    fs = 4096
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    pats = [b"status\\x3d5[0-9][0-9]", b"id=[0-9a-f][0-9a-f][0-9a-f][0-9a-f]", b"20..-..-.. ", b"s=\\d\\d\\d", b"=[^0-9]", b"[0-9a-f].ts", b"status=5\\d[^0-9]"]
    for staging in (0, fs):
        want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, pats, CLASSES, staging=staging)
        # with the multi search `.` matches the newline between two lines; with the grep it does not join them
        across = [o for o, i in want if i == 5]
        assert len(across) > 200 and all(data[o + 1] == NL for o in across)
        assert XM.grep(data, [pats[5]], CLASSES, NL)[1:] == ([], 0)
        n, recs = gpu_engine.grep(d.data_ptr(), len(arc), [pats[5]], staging_bytes=staging, syntax=CLASSES)
        assert (n, recs) == (0, []) and gpu_engine.grep_stats()["matches"] == 0
        assert any(data[o:o + 10] == b"status=51 " for o, i in want if i == 6) and len(sel[False]) > 100
    _check(gpu_engine, zra, d, len(arc), data, fs, pats, CLASSES | FOLD, 100, 15000, fs)


# ---- 4
NEEDLE = b"\xF0N[EF][EF]DLE\\d\\d\\d.[^a-z]\\x3d" + b"[0-9a-f]" * 8 + b"...." + b"\\w" * 13 + b"\\.\xF1"
OCC = b"\xF0NEFDLE042_Q=00ffab12\x00\xff\x0b~abcXYZ_0189zz.\xF1"


@pytest.fixture(scope="module")
def seams(zra, gpu_engine):
    """40 tiles of filler without a delimiter-free stretch problem: OCC, an occurrence of the 40-element NEEDLE, starts k positions in
    front of a tile boundary, of a wave boundary and of a trip boundary, for every k of 1 .. 39: the verify runs into the overhang."""
    assert XM.lengths(XM.compile([NEEDLE], CLASSES, NL)) == [40] and len(OCC) == 40 and XM.set_matches(OCC, XM.compile([NEEDLE], CLASSES, NL)) == [(0, 0)]
    U = 40 * 8192 + 500
    a = bytearray(_data(np.random.RandomState(4), U))
    at = []
    for k in range(1, 40):
        at += [8192 * k - k, 8192 * k + 2048 - k, 8192 * k + 4096 + 64 * k - k]
    for p in at:
        a[p:p + 40] = OCC
        a[p + 40] = NL
    data = bytes(a)
    fs = 4096
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    return dict(data=data, arc=arc, d=_dev(arc), at=sorted(at), fs=fs)


@pytest.mark.parametrize("staging", [0, 2 * 4096])
def test_seams(zra, gpu_engine, seams, staging):
    """With passes of two frames (8,192 bytes, from offset 0) a tile boundary of the single pass is a pass boundary: the occurrences
    that cross it are owned by the next pass, through the carry."""
    data, arc, d, at, fs = seams["data"], seams["arc"], seams["d"], seams["at"], seams["fs"]
    pats = [NEEDLE, b"\xF0N[EF]", b"[\\xF1]\\n"]
    want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, pats, CLASSES, staging=staging, records=False)
    assert [o for o, i in want if i == 0] == at and len(at) == 117
    want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, pats[:2], CLASSES, staging=staging)
    assert len(sel[False]) == 117
    assert gpu_engine.grep_stats()["passes"] == (41 if staging else 1)


def test_range_ends_and_the_shortcut(zra, gpu_engine, seams):
    data, arc, d, at, fs = seams["data"], seams["arc"], seams["d"], seams["at"], seams["fs"]
    p = at[5]
    for staging in (0, fs):
        for hi, found in ((p + 40, True), (p + 39, False), (p + 41, True)):     # the occurrence starts at hi - 40, at hi - 39, at hi - 41
            want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, [NEEDLE, b"\xFF\\xFE\xFD"], CLASSES, p - 300, hi, staging)
            assert ((p, 0) in want) == found and bool(sel[False]) == found, (hi, want)
    # six elements in 24 expression bytes: a range of 5 is shorter than the pattern and nothing is decoded; a range of 6 .. 23 is
    # shorter than the expression, not than the pattern, and is scanned
    six = [b"\\xF0\\x4e\\x45\\x46\\x44\\x4C"]
    assert data[p:p + 6] == b"\xF0NEFDL"
    for hi, n in ((p + 5, 0), (p + 6, 1), (p + 23, 1)):
        want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, six, CLASSES, p, hi)
        assert len(want) == n and gpu_engine.search_multi_stats()["decoded"] == (1 if n else 0) and gpu_engine.grep_stats()["decoded"] == 1   # (the inverted grep ran last)
        gpu_engine.grep(d.data_ptr(), len(arc), six, offset=p, length=hi - p, syntax=CLASSES)
        assert gpu_engine.grep_stats() == (dict(G.ZERO, frames=-(-len(data) // fs)) if n == 0 else G._stats(len(data), fs, p, hi, 0, 1, 1, 1, 1))


# ---- 5
def test_widths(zra, gpu_engine):
    rng = np.random.RandomState(5)
    a = bytearray(_data(rng, 16384))
    word = b"NEEDLE01"
    for p in (100, 2046, 16384 - 8):                                           # in a trip, across a wave boundary, at the content's end
        a[p:p + 8] = word
    body = bytes(rng.randint(32, 127, size=256).astype(np.uint8))
    a[8192 - 100:8192 + 156] = body
    data = bytes(a)
    arc = _compress(gpu_engine, zra, data, 3, FS, True)
    d = _dev(arc)
    # 64 patterns that all match at one position: pattern i has a dot where bit b of i is set (indices 31, 32 and 63 among them)
    pats = [b"".join(b"." if b < 6 and i >> b & 1 else word[b:b + 1] for b in range(8)) for i in range(64)]
    for staging in (0, FS):
        want, _, _ = _check(gpu_engine, zra, d, len(arc), data, FS, pats, CLASSES, staging=staging, records=False)
        assert [(o, i) for o, i in want if o == 2046] == [(2046, i) for i in range(64)] and len(want) >= 3 * 64
    _check(gpu_engine, zra, d, len(arc), data, FS, pats, CLASSES, modes=(False,))
    # one pattern of 256 elements across the tile boundary: every fourth element a set, a dot or a folded letter
    long_ = b"".join(_esc(body[q:q + 1]) if q % 4 else [b".", b"[ -~]", b"[^\\x00-\\x1f]", b"\\x%02x" % body[q]][q // 4 % 4] for q in range(256))
    assert XM.lengths(XM.compile([long_], CLASSES | FOLD, NL)) == [256]
    for staging in (0, FS):
        want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, FS, [long_, b"N."], CLASSES | FOLD, staging=staging)
        assert (8192 - 100, 0) in want
    # exactly 32 counted sets; 33 are refused with the stats zero
    sets = [b"[\\x%02x\\x%02x]" % (k, 32 + k) for k in range(33)]
    assert zra.check_pattern_expr([b"".join(sets[:32])], CLASSES, delimiter=None)[1] == 32
    _check(gpu_engine, zra, d, len(arc), data, FS, sets[:32], CLASSES, delim=0xFF)
    _check(gpu_engine, zra, d, len(arc), data, FS, [b"".join(sets[:32]), b"NE"], CLASSES, delim=0xFF, modes=(False,))
    for call in (lambda: gpu_engine.search_multi(d.data_ptr(), len(arc), sets, syntax=CLASSES), lambda: gpu_engine.grep(d.data_ptr(), len(arc), sets, syntax=CLASSES, delimiter=0xFF),
                 lambda: gpu_engine.extract(d.data_ptr(), len(arc), sets, 0, 0, syntax=CLASSES, delimiter=0xFF)):
        with pytest.raises(zra.ZraError) as e:
            call()
        assert (e.value.zra, e.value.zstd) == (1, 42)
    assert gpu_engine.search_multi_stats() == MZERO and gpu_engine.grep_stats() == G.ZERO and gpu_engine.extract_stats() == X.ZERO
    # a pattern that begins `..`: every position but the last is a candidate
    want, _, _ = _check(gpu_engine, zra, d, len(arc), data, FS, [b"..E", b"..[^\\x00-\\x7f]"], CLASSES)
    assert gpu_engine.search_multi_stats()["survivors"] == 16383 and len(want) >= 6


# ---- 6
def test_more_than_one_workgroup(zra, gpu_engine):
    """tests/test_gpu_grep.py's 8.6 MiB shape: 1,101 tiles in 138 workgroups, and with passes of 16 frames nine passes of 128 tiles."""
    fs = 65536
    U = 1100 * 8192 + 5000
    rng = np.random.RandomState(66)
    a = rng.randint(32, 127, size=U).astype(np.uint8)
    a[rng.randint(0, U, size=U // 200)] = NL
    a[3000000:3100000][a[3000000:3100000] == NL] = 32
    data = a.tobytes()
    pats = [b"[Ee]rr[0-9o]", b"\\d\\d\\d\\d\\d", _esc(data[3050000:3050012]), b"[^ -~]."]
    arc = _compress(gpu_engine, zra, data, 1, fs, True)
    d = _dev(arc)
    for staging in (0, 16 * fs):
        want, sel, _ = _check(gpu_engine, zra, d, len(arc), data, fs, pats, CLASSES, staging=staging, modes=(bool(staging),))
        assert len(want) > 1000 and {i for _, i in want} >= {1, 2, 3} and gpu_engine.grep_stats()["passes"] == (9 if staging else 1)


# ---- 7
def test_capacity(zra, gpu_engine, text):
    import torch
    L = zra.load()
    data, arc, d, U = text["data"], text["arc"], text["d"], text["U"]
    pats = [b"[\\x00-\\x05].", b"\\x07[^\\x07]"]
    sizes = (ctypes.c_uint32 * 2)(*(len(p) for p in pats))
    want = XM.matches_multi(data, pats, CLASSES)
    assert len(want) > 40
    for cap in (0, 1, len(want) - 1, len(want) + 5):
        arr = (zra.ZraHipPatternMatch * (cap + 2))()
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        n = ctypes.c_uint64(0x1234)
        gpu_engine._order()
        st = L.ZraHipSearchArchiveMultiExpr(gpu_engine.h, d.data_ptr(), len(arc), b"".join(pats), sizes, 2, CLASSES, 0, MAXU64, FS, arr if cap else None, cap, ctypes.byref(n),
                                            None).tup()
        k = min(cap, len(want))
        assert (st, n.value) == ((0, 0), len(want)) and [(arr[i].offset, arr[i].pattern) for i in range(k)] == want[:k], cap
        assert bytes(arr)[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)) and gpu_engine.search_multi_stats()["listed"] == k
    for mode in (0, 1):
        recs, sel, matches, packed = XM.extract(data, pats, CLASSES, NL, bool(mode))
        assert len(sel) > 5
        for cap in (0, 1, len(sel) - 1, len(sel) + 5):
            arr = (ctypes.c_uint64 * (2 * (cap + 2)))()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n = ctypes.c_uint64(0x1234)
            gpu_engine._order()
            st = L.ZraHipGrepArchiveExpr(gpu_engine.h, d.data_ptr(), len(arc), b"".join(pats), sizes, 2, CLASSES, NL, mode, 0, MAXU64, FS, arr if cap else None, cap,
                                         ctypes.byref(n)).tup()
            k = min(cap, len(sel))
            assert (st, n.value) == ((0, 0), len(sel)) and X._pairs(bytes(arr), k) == sel[:k] and bytes(arr)[16 * k:] == b"\xEE" * (16 * (cap + 2 - k)), (mode, cap)
            assert gpu_engine.grep_stats() == G._stats(U, FS, 0, U, FS, len(recs), len(sel), k, matches)
        # the extract: a list or a buffer that is too small keeps the two words
        for rec_cap, data_cap, st_want in ((len(sel) - 1, len(packed), X.TOO_SMALL), (len(sel), len(packed) - 1, X.TOO_SMALL), (0, 0, X.TOO_SMALL), (len(sel), len(packed), (0, 0))):
            buf = torch.full((len(packed) + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
            arr = (ctypes.c_uint64 * (2 * (rec_cap + 2)))()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
            gpu_engine._order()
            st = L.ZraHipExtractRecordsExpr(gpu_engine.h, d.data_ptr(), len(arc), b"".join(pats), sizes, 2, CLASSES, NL, mode, 0, MAXU64, FS, arr if rec_cap else None, rec_cap,
                                            ctypes.byref(n), buf.data_ptr() if data_cap else None, data_cap, ctypes.byref(ds)).tup()
            torch.cuda.synchronize()
            host = buf.cpu().numpy().tobytes()
            assert (st, n.value, ds.value) == (st_want, len(sel), len(packed)), (mode, rec_cap, data_cap, st)
            assert host[data_cap:] == b"\xEE" * (len(host) - data_cap)
            if st == (0, 0):
                assert host[:data_cap] == packed and X._pairs(bytes(arr), len(sel)) == sel
            else:
                assert bytes(arr) == b"\xEE" * len(bytes(arr)) and gpu_engine.extract_stats() == X.ZERO


# ---- 8
def test_through_the_handle(zra, gpu_engine):
    import torch
    fs, nf = 1000, 24
    data = _log(np.random.RandomState(8), (nf - 1) * fs + 300)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    h = zra.Archive(gpu_engine, d.data_ptr(), len(arc), 12 * fs)
    try:
        out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
        for f in (23, 20, 6, 2, 14, 5, 17, 8, 7, 21, 11, 0):                   # half of the frames, in an order that is not frame order
            h.read(out.data_ptr(), [f * fs], [1], [0])
        before = h.stats()
        assert (before["slots"], before["resident"]) == (12, 12)
        pats = [b"STATUS=5\\d\\d", b"id=[0-9A-F][0-9a-f]..f", b"20..-..-.. ", b"id=00fg"]
        syntax = CLASSES | FOLD
        for lo, hi, staging in ((0, None, 0), (0, None, 3 * fs), (2 * fs + 7, 21 * fs - 5, fs)):
            length = None if hi is None else hi - lo
            kw = dict(offset=lo, length=length, staging_bytes=staging, syntax=syntax)
            want, sel, packed = _check(gpu_engine, zra, d, len(arc), data, fs, pats, syntax, lo, hi, staging, modes=(False,))
            assert len(want) > 50 and len(sel[False]) > 20
            n, at, per = h.search_multi(pats, max_matches=len(want) + 1, **kw)
            assert (n, at) == (len(want), want)
            f0, f1 = lo // fs, ((len(data) if hi is None else hi) - 1) // fs
            resident = sum(1 for f in (23, 20, 6, 2, 14, 5, 17, 8, 7, 21, 11, 0) if f0 <= f <= f1)
            ss = h.scan_stats()
            assert (ss["staged"], ss["decoded"]) == (resident, f1 - f0 + 1 - resident), (ss, resident)
            assert gpu_engine.search_multi_stats()["decoded"] == f1 - f0 + 1 - resident
            assert h.grep(pats, max_records=len(sel[False]) + 1, **kw) == (len(sel[False]), sel[False])
            buf = torch.full((len(packed[False]) + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
            assert h.extract(pats, buf.data_ptr(), buf.numel(), max_records=len(sel[False]) + 1, **kw) == (len(sel[False]), len(packed[False]), sel[False])
            torch.cuda.synchronize()
            assert buf.cpu().numpy().tobytes() == packed[False] + b"\xEE" * 8
            assert h.stats() == before                                         # a scan is not a read
        with pytest.raises(zra.ZraError) as e:
            h.grep([b"a)"], syntax=CLASSES)
        assert (e.value.zra, e.value.zstd) == (1, 42) and h.stats() == before
    finally:
        h.close()


# ---- 9
def test_a_damaged_frame(zra, gpu_engine):
    import torch
    L = zra.load()
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    bad = _flip_mid(_compress(gpu_engine, zra, data, 3, fs, True), [7])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    pats = [b"[\\x01-\\x03].\\x05", b"\\x07\\x07"]
    sizes = (ctypes.c_uint32 * 2)(*(len(p) for p in pats))
    buf = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
    for staging in (0, 4 * fs, 1):
        arr = (ctypes.c_uint64 * 16)()
        ctypes.memset(arr, 0xEE, 128)
        marr = ctypes.cast(arr, ctypes.POINTER(zra.ZraHipPatternMatch))
        n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
        gpu_engine._order()
        args = (gpu_engine.h, db.data_ptr(), len(bad), b"".join(pats), sizes, 2, CLASSES)
        assert L.ZraHipSearchArchiveMultiExpr(*args, 0, MAXU64, staging, marr, 6, ctypes.byref(n), None).tup() == (1, want[7]) and n.value == 0
        assert gpu_engine.search_multi_stats() == MZERO
        n.value = 0x1234
        assert L.ZraHipGrepArchiveExpr(*args, NL, 0, 0, MAXU64, staging, arr, 6, ctypes.byref(n)).tup() == (1, want[7]) and n.value == 0
        assert gpu_engine.grep_stats() == G.ZERO
        n.value = 0x1234
        assert L.ZraHipExtractRecordsExpr(*args, NL, 1, 0, MAXU64, staging, arr, 6, ctypes.byref(n), buf.data_ptr(), 0, ctypes.byref(ds)).tup() == (1, want[7])
        assert (n.value, ds.value) == (0, 0) and gpu_engine.extract_stats() == X.ZERO and bytes(arr) == b"\xEE" * 128
    for lo, hi in ((0, 7 * fs), (8 * fs, 12 * fs)):                            # the same damage outside the range
        _check(gpu_engine, zra, db, len(bad), data, fs, pats, CLASSES, lo, hi, modes=(False,))


# ---- 10
def test_stats_isolation_and_a_literal_call_afterwards(zra, gpu_engine, text):
    data, arc, d, pats = text["data"], text["arc"], text["d"], text["pats"]
    P = d.data_ptr()
    gpu_engine.search(P, len(arc), pats[0], staging_bytes=2 * FS)
    lit_m = gpu_engine.search_multi(P, len(arc), pats, staging_bytes=3 * FS)
    s1, sm = gpu_engine.search_stats(), gpu_engine.search_multi_stats()
    lit_g = gpu_engine.grep(P, len(arc), pats, staging_bytes=FS)
    sg = gpu_engine.grep_stats()
    assert s1["passes"] == 4 and sm["passes"] == 3 and sg["passes"] == 7
    n, recs = gpu_engine.grep(P, len(arc), [b"[\\x00-\\x05].", b"\\x07"], staging_bytes=2 * FS, syntax=CLASSES | FOLD)
    se = gpu_engine.grep_stats()
    assert n > 0 and se["passes"] == 4 and se != sg and gpu_engine.grep_scan_ms() > 0
    assert gpu_engine.search_stats() == s1 and gpu_engine.search_multi_stats() == sm                  # the ...Expr grep wrote the grep's row only
    assert gpu_engine.grep(P, len(arc), pats, staging_bytes=FS) == lit_g and gpu_engine.grep_stats() == sg
    assert gpu_engine.search_multi(P, len(arc), pats, staging_bytes=3 * FS) == lit_m and gpu_engine.search_multi_stats() == sm
    assert gpu_engine.search_multi(P, len(arc), pats, staging_bytes=3 * FS, syntax=0) == lit_m
    gpu_engine.release_scratch()                                               # scratch handed back: the same answers
    assert gpu_engine.grep(P, len(arc), [b"[\\x00-\\x05].", b"\\x07"], staging_bytes=2 * FS, syntax=CLASSES | FOLD) == (n, recs) and gpu_engine.grep_stats() == se
    assert gpu_engine.grep(P, len(arc), pats, staging_bytes=FS) == lit_g


# ---- 11
def test_cli_modes_gme_gle_gxe(zra, gpu_engine, tmp_path):
    data = b"alpha One 17\nbeta two 230\n\ngamma ONE two 9\ndelta." + b"\n" + b"x;y;one;z" * 3
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(mode, *args):
        return subprocess.run([TOOL, mode, str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    def lines(sel):
        return b"".join(b"%d\t%d\n" % r for r in sel) + b"%d records\n" % len(sel)

    # (arguments, patterns as the calls see them, syntax, delimiter, invert)
    for args, pats, syntax, delim, inv in ((("o.e",), [b"o.e"], CLASSES, NL, False), (("-i", "one"), [b"one"], CLASSES | FOLD, NL, False),
                                           (("-v", "-i", "[a-c]\\w", "hex:" + b"two".hex()), [b"[a-c]\\w", b"\\x74\\x77\\x6f"], CLASSES | FOLD, NL, True),
                                           (("-F", "-i", "a."), [b"A."], FOLD, NL, False), (("-d", "3b", "-v", "\\d\\d"), [b"\\d\\d"], CLASSES, 0x3B, True)):
        recs, sel, matches, packed = XM.extract(data, pats, syntax, delim, inv)
        r = run("gle", *args)
        assert r.returncode == 0 and r.stdout == lines(sel) and sel, (args, r.stdout, r.stderr)
        if "-i" in args or "-d" in args:                                     # (the text of four of the five selections)
            r = run("gxe", *args)
            assert r.returncode == 0 and r.stdout == packed, (args, r.stdout, r.stderr)
    assert XM.grep(data, [b"A."], FOLD)[1] == [(43, 6)] and XM.grep(data, [b"one"], CLASSES | FOLD)[1] == [(0, 12), (27, 15), (50, 27)]
    want = XM.matches_multi(data, [b"[0-9][0-9]", b"ONE"], CLASSES | FOLD)
    r = run("gme", "-i", "[0-9][0-9]", "ONE")
    assert r.returncode == 0 and r.stdout == b"".join(b"%d\t%d\n" % m for m in want) + b"%d matches\n" % len(want) and len(want) == 8, (r.stdout, r.stderr)
    r = run("gme", "o.e\\.", "hex:fffe")
    assert r.returncode == 1 and r.stdout == b"0 matches\n", (r.stdout, r.stderr)
    r = run("gxe", "absent", "[q]x")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    # a refused expression: exit status 2, nothing on stdout, the pattern's index in the message (no engine is made for these)
    for mode, args, index in (("gme", ("a", "b)"), b"pattern 1"), ("gxe", ("a", "b", "\\q"), b"pattern 2"), ("gle", ("[z-a]",), b"pattern 0"), ("gme", ("-i",), b""),
                              ("gxe", ("a", "hex:0"), b""), ("gxe", ("[\\n]",), b"pattern 0"), ("gle", ("-d", "61", "alph[a]"), b"pattern 0")):
        r = run(mode, *args)
        assert r.returncode == 2 and r.stdout == b"" and index in r.stderr, (mode, args, r.stdout, r.stderr)
    r = run("gle", "-F", "b)")                                                 # literal after all
    assert r.returncode == 1 and r.stdout == b"0 records\n"
    r = run("gl", "-i", "one")                                                 # the existing modes do not change: -i is a pattern there
    assert r.returncode == 0 and r.stdout == lines(XM.grep(data, [b"-i", b"one"], 0)[1])
