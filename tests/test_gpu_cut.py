"""GPU tests of ZraHipCutRecords and ZraHipArchiveCutRecords (include/zra_hip.h): the chosen fields of the selected records, packed.
The yardstick everywhere is tests/cut_model.py (extract_model's selection, the field rule with true field numbers) on the inputs of
tests/cut_shapes.py, which tests/test_cut_abi.py holds to the seams they are built for. Archives are written on the device. dData is a
0xEE-filled buffer handed over 64 bytes in, with a capacity that leaves 64 guard bytes behind it: after every call both guards are
still 0xEE. Every check compares status, both words, the packed bytes, the list, all eight extract stats, and the grep's and the
searches' stats with what they were; it runs in both modes and, unless it is about emptiness, asserts that both select something.
Every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cut_model as CM
import cut_shapes as SH
import expr_model as EM
import grep_model as GM
import test_gpu_archive_scan as AS
import test_gpu_extract as X
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
GUARD = 64
FS = SH.FS
ZERO, TOO_SMALL = X.ZERO, X.TOO_SMALL
bits = SH.bits


def _raw(eng, zra, d, size, pats, sep, mask, data_cap, rec_cap, mode=0, offset=0, length=MAXU64, staging=0, syntax=0, handle=None, delim=NL):
    """(status, *nRecords, *dataSize, the bytes of a record array two entries longer than the capacity, the first data_cap bytes of
    dData) of one call, through `handle` when there is one; both 0xEE-filled before it. Asserts that the guards in front of dData and
    behind its capacity are intact. No pattern: NULL pattern arguments."""
    import torch
    buf = torch.full((GUARD + data_cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (2 * (rec_cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats)) if pats else None
    eng._order()
    tail = (b"".join(pats) if pats else None, sizes, len(pats), syntax, delim, mode, sep, mask, offset, length, staging, arr if rec_cap else None, rec_cap, ctypes.byref(n),
            buf.data_ptr() + GUARD, data_cap, ctypes.byref(ds))
    if handle is None:
        st = zra.load().ZraHipCutRecords(eng.h, d.data_ptr(), size, *tail).tup()
    else:
        st = zra.load().ZraHipArchiveCutRecords(handle.h, *tail).tup()
    torch.cuda.synchronize()
    host = buf.cpu().numpy().tobytes()
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + data_cap:] == b"\xEE" * GUARD, ("guard", st, data_cap, rec_cap, mode, offset, length, staging)
    return st, n.value, ds.value, bytes(arr), host[GUARD:GUARD + data_cap]


def _check(eng, zra, d, size, c, mask, lo=0, hi=None, staging=0, modes=(False, True), syntax=0, pats=None, slack=5, nonempty=True, handle=None):
    """one cut per mode of [lo, hi) of the case against the model. Returns {invert: (selected, packed)}."""
    data, fs = c["data"], c["fs"]
    pats = c["pats"] if pats is None else pats
    U = len(data)
    end = U if hi is None else hi
    out = {}
    for inv in modes:
        recs, sel, nm, packed = SH.model(c, mask, inv, lo, hi, pats=pats, syntax=syntax)
        tag = (c["name"], hex(mask), lo, hi, staging, inv)
        others = (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats())
        st, n, ds, mem, got = _raw(eng, zra, d, size, pats, c["sep"], mask, len(packed) + slack, len(sel) + 1, int(inv), lo, MAXU64 if hi is None else hi - lo, staging, syntax,
                                   handle)
        print("cut", tag, "status", st, "selected", n, "model", len(sel), "bytes", ds, "model", len(packed))
        assert (st, n, ds) == ((0, 0), len(sel), len(packed)), (tag, st, n, ds, len(sel), len(packed))
        if got[:ds] != packed:
            bad = next(i for i in range(ds) if got[i] != packed[i])
            raise AssertionError((tag, "first wrong byte", bad, got[max(0, bad - 8):bad + 8], packed[max(0, bad - 8):bad + 8]))
        assert X._pairs(mem, n) == sel and mem[16 * n:] == b"\xEE" * (16 * (len(sel) + 3 - n)), tag
        if handle is None:
            s = eng.extract_stats()
            shortest = min(len(p) for p in pats) if pats and not syntax else 1
            if end == lo or (end - lo < shortest and not inv):
                assert s == dict(ZERO, frames=-(-U // fs)) and not sel, (tag, s)  # nothing decoded
            else:
                assert s == X._stats(U, fs, lo, end, staging, len(recs), len(sel), len(packed), nm), (tag, s)
        assert (eng.grep_stats(), eng.search_stats(), eng.search_multi_stats()) == others, tag
        out[inv] = (sel, packed)
    if nonempty and len(modes) == 2:
        assert out[False][0] and out[True][0], (c["name"], hex(mask), lo, hi, "a test that selects nothing shows nothing")
    return out


def _arc(eng, zra, c, level=3):
    """the case's archive on the device, written once"""
    if "_arc" not in c:
        c["_arc"] = _compress(eng, zra, c["data"], level, c["fs"], True)
    return c["_arc"], _dev(c["_arc"])


# ---- 1
@pytest.mark.parametrize("k", range(len(SH.TINY_MASKS)))
def test_frame_size_4_one_slot_every_record_crosses_passes(zra, gpu_engine, k):
    """the field number, the kept bytes and the provisional tail travel in the carried words: one frame per pass, then the same as one
    pass"""
    c = SH.frame_size_4()
    arc, d = _arc(gpu_engine, zra, c)
    mask = SH.TINY_MASKS[k]
    one = _check(gpu_engine, zra, d, len(arc), c, mask, staging=1, slack=len(c["data"]))
    assert gpu_engine.extract_stats()["passes"] == -(-len(c["data"]) // 4)
    whole = _check(gpu_engine, zra, d, len(arc), c, mask, staging=0)
    assert one == whole
    # copied provisionally and selected passes later; copied provisionally, not selected, and the next selected record lies where it lay
    assert c["late"] in one[False][0] and c["dropped"] not in one[False][0] and c["after_dropped"] in one[False][0]
    assert c["dropped"] in one[True][0] and c["late"] not in one[True][0]
    plain = _check(gpu_engine, zra, d, len(arc), c, mask, staging=1, pats=[], modes=(False,), slack=len(c["data"]))
    assert plain[False][0] == GM.records(c["data"])


# ---- 2
@pytest.mark.parametrize("B", SH.SEAMS)
@pytest.mark.parametrize("what", ["separator", "field"])
def test_separators_and_fields_at_every_seam(zra, gpu_engine, B, what):
    """a separator, and a field's first byte, at the last byte of a trip, a wave, a tile and a workgroup and at the first byte of the
    next, under the masks that make it the only kept byte and the only dropped one; in one pass and in passes of two frames"""
    for side in (0, 1):
        c = (SH.seam_separator if what == "separator" else SH.seam_field)(B, side)
        arc, d = _arc(gpu_engine, zra, c)
        o, n = c["big"]
        for staging in (0, 2 * FS):
            for mask in (c["only_kept"], c["only_dropped"], SH.ALL):
                both = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, slack=64)
                assert c["big"] in both[False][0]
            kept = SH.model(c, c["only_kept"])[3]
            assert kept.split(b"\n")[0] == c["data"][c["P"]:c["P"] + 1]


@pytest.mark.parametrize("k", [1, 5, 63, 64])
def test_a_record_over_three_tiles(zra, gpu_engine, k):
    c = SH.three_tiles(k)
    arc, d = _arc(gpu_engine, zra, c)
    for staging in (0, 3 * FS):
        for mask in c["masks"]:
            both = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, slack=64)
            assert c["big"] in both[False][0]


# ---- 3
@pytest.mark.parametrize("mask", SH.SAT_MASKS)
def test_saturation(zra, gpu_engine, mask):
    c = SH.saturation()
    arc, d = _arc(gpu_engine, zra, c)
    for staging in (0, FS):
        _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging)
        _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, pats=[], modes=(False,))


@pytest.mark.parametrize("field", [64, 65])
@pytest.mark.parametrize("B", [SH.TILE, 3 * FS])
def test_fields_64_and_65_start_at_a_tile_and_at_a_pass_boundary(zra, gpu_engine, B, field):
    """B = 8,192: a tile boundary of the one-pass call; B = 3 * FS with a window of three frames: the first position of the second pass"""
    c = SH.saturation_at(B, field)
    arc, d = _arc(gpu_engine, zra, c)
    for staging in (0, 3 * FS):
        for mask in SH.SAT_MASKS + [bits(63, 64) | 1, SH.ALL & ~bits(64)]:
            both = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, slack=64)
            assert c["big"] in both[False][0]
            _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, pats=[], modes=(False,))


# ---- 4
@pytest.mark.parametrize("kind", ["separators", "no_separator", "empty_records", "delimiters", "single"])
def test_degenerate_text(zra, gpu_engine, kind):
    c = SH.degenerate(kind)
    arc, d = _arc(gpu_engine, zra, c)
    for mask in (bits(1), bits(2), bits(2, 3), SH.ALL):
        for staging in (0, FS):
            _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, nonempty=kind in ("no_separator", "empty_records"))
            out = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, pats=[], modes=(False,))
            assert out[False][0] == GM.records(c["data"])
            if kind == "delimiters":
                assert out[False][1] == c["data"]
            if kind == "no_separator":                                         # cut's answer with field 1, an empty line without it
                want = c["data"] + b"\n" if mask & 1 else b"\n" * len(out[False][0])
                assert out[False][1] == want


# ---- 5
def test_range_clipping(zra, gpu_engine):
    """lo and hi in the middle of a field and on a separator: the field count restarts at lo; the empty range, and a range shorter
    than the shortest pattern, where nothing is decoded"""
    c = SH.table()
    arc, d = _arc(gpu_engine, zra, c)
    data, U = c["data"], len(c["data"])
    commas = [p for p in range(5 * FS, 15 * FS) if data[p] == SH.COMMA and data[p + 1] not in (SH.COMMA, NL) and data[p - 1] not in (SH.COMMA, NL)]
    p, q = commas[10], commas[-10]
    for lo, hi in ((p, q), (p + 1, q + 1), (p - 1, q + 2), (p, U), (0, q)):
        for mask in (bits(1), bits(2, 3), bits(1, 4) | bits(64)):
            for staging in (0, 2 * FS):
                out = _check(gpu_engine, zra, d, len(arc), c, mask, lo, hi, staging=staging)
                _check(gpu_engine, zra, d, len(arc), c, mask, lo, hi, staging=staging, pats=[], modes=(False,))
    # the record that lo = p cuts begins with the separator: its field 1 is empty
    first = SH.model(c, bits(1), False, p, q, pats=[])
    assert first[1][0][0] == p and first[3].startswith(b"\n")
    _check(gpu_engine, zra, d, len(arc), c, bits(1), p, p, nonempty=False)
    assert gpu_engine.extract_stats() == dict(ZERO, frames=-(-U // FS))
    _check(gpu_engine, zra, d, len(arc), c, bits(1), p, p, pats=[], modes=(False,), nonempty=False)
    assert gpu_engine.extract_stats() == dict(ZERO, frames=-(-U // FS))
    out = _check(gpu_engine, zra, d, len(arc), c, bits(1), p, p + 1, nonempty=False)   # shorter than "qz": not decoded; inverted: scanned
    assert out[False] == ([], b"") and out[True][0] == [(p, 1)] and out[True][1] == b"\n"


# ---- 6
def test_zero_patterns(zra, gpu_engine):
    c = SH.table()
    arc, d = _arc(gpu_engine, zra, c)
    for mask in (bits(1, 3), bits(2), SH.ALL):
        for staging in (0, 3 * FS):
            plain = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, pats=[], modes=(False,))
            s = gpu_engine.extract_stats()
            never = _check(gpu_engine, zra, d, len(arc), c, mask, staging=staging, pats=[b"\xF7\xF8"], modes=(True,))
            assert plain[False] == never[True] and gpu_engine.extract_stats() == s and s["matches"] == 0
            lines = c["data"].split(b"\n")
            assert plain[False][1] == b"".join(CM.cut_record(ln, SH.COMMA, mask) + b"\n" for ln in lines[:-1] + ([lines[-1]] if lines[-1] else []))
    st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), [], SH.COMMA, 1, 64, 2, mode=1)
    assert (st, n, ds, mem, got) == ((1, 42), 0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO


# ---- 7
def test_capacity(zra, gpu_engine):
    c = SH.table()
    arc, d = _arc(gpu_engine, zra, c)
    pats, fs, U = c["pats"], c["fs"], len(c["data"])
    mask = bits(2, 4, 5)
    for mode in (0, 1):
        recs, sel, nm, packed = SH.model(c, mask, bool(mode))
        total, size = len(sel), len(packed)
        assert total > 8 and size > 100
        for staging in (0, fs):
            # the sizing call, a list one entry short, data one byte short: what the call needs, nothing listed
            for dcap, rcap in ((0, 0), (size + 9, total - 1), (size - 1, total), (size - 1, 0)):
                st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, c["sep"], mask, dcap, rcap, mode=mode, staging=staging)
                tag = (mode, staging, dcap, rcap)
                assert (st, n, ds) == (TOO_SMALL, total, size), (tag, st, n, ds)
                assert mem == b"\xEE" * (16 * (rcap + 2)), tag                   # hRecords untouched
                assert got[:min(dcap, size)] == packed[:min(dcap, size)] or dcap == 0, tag
                assert gpu_engine.extract_stats() == ZERO, tag
            # fitting: exactly, and without a list (recordCapacity 0, hRecords NULL)
            for dcap, rcap in ((size, total), (size, 0), (size + 100, total + 5)):
                st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), pats, c["sep"], mask, dcap, rcap, mode=mode, staging=staging)
                tag = (mode, staging, dcap, rcap)
                assert (st, n, ds) == ((0, 0), total, size) and got[:size] == packed, (tag, st, n, ds)
                assert X._pairs(mem, min(rcap, total) if rcap else 0) == (sel if rcap else []), tag
                assert mem[16 * (total if rcap else 0):] == b"\xEE" * (16 * (rcap + 2 - (total if rcap else 0))), tag
                assert gpu_engine.extract_stats() == X._stats(U, fs, 0, U, staging, len(recs), total, size, nm), tag


# ---- 8
def test_expression_syntax(zra, gpu_engine):
    c = SH.expressions()
    arc, d = _arc(gpu_engine, zra, c)
    for pats, syntax in ((c["fold"], zra.PATTERN_FOLD_CASE), (c["classes"], zra.PATTERN_CLASSES)):
        assert len(EM.set_matches(c["data"], EM.compile(pats, syntax, NL))) > 20
        for staging in (0, 2 * FS):
            out = _check(gpu_engine, zra, d, len(arc), c, bits(1, 3, 4), staging=staging, syntax=syntax, pats=pats)
            assert len(out[False][0]) > 5 and len(out[True][0]) > 5


# ---- 9
@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames of the range resident"""
    import torch
    fs = 1000
    data, pats = AS._content(77, fs)
    U = len(data)
    c = SH.case("handle", data, fs, pats, sep=ord("d"))
    arc, d = _arc(gpu_engine, zra, c)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, U, warm, slots)
    out = torch.empty(U + 64, dtype=torch.uint8, device="cuda:0")
    mask = bits(1, 3)
    try:
        for lo, hi in ((0, U), (6 * fs + fs // 2, 10 * fs + fs // 2)):
            for staging in (0, 3 * fs):
                kw = dict(offset=lo, length=hi - lo, staging_bytes=staging, max_records=AS.MAXREC)
                before = h.stats()
                s0 = h.scan_stats()
                plain = h.extract(pats, out.data_ptr(), U + 64, **kw)
                s1 = h.scan_stats()
                got = h.cut(pats, out.data_ptr(), U + 64, separator=c["sep"], fields="1,3", **kw)
                s2 = h.scan_stats()
                hs = gpu_engine.extract_stats()
                text = out[:got[1]].cpu().numpy().tobytes()
                recs, sel, nm, packed = SH.model(c, mask, False, lo, hi)
                assert got == (len(sel), len(packed), sel) and text == packed and got[0] > 0 and plain[0] == got[0] and got[1] < plain[1], (slots, lo, staging)
                _check(gpu_engine, zra, d, len(arc), c, mask, lo, hi, staging=staging, modes=(True,), handle=h)
                eng = gpu_engine.cut(d.data_ptr(), len(arc), pats, out.data_ptr(), U + 64, separator=c["sep"], fields=mask, **kw)
                es = gpu_engine.extract_stats()
                assert eng == got and out[:got[1]].cpu().numpy().tobytes() == packed
                staged, decoded, dec_bytes = AS._split(warm, fs, U, lo, hi)
                assert hs == dict(es, decoded=decoded, content_bytes=dec_bytes), (hs, es)
                # the handle's counters move as for the plain extract on the same range
                assert {k: s2[k] - s1[k] for k in s1 if k.endswith("total") or k == "scans"} == {k: s1[k] - s0[k] for k in s1 if k.endswith("total") or k == "scans"}
                assert (s2["staged"], s2["decoded"], s2["passes"]) == (s1["staged"], s1["decoded"], s1["passes"]) and (s2["staged"], s2["decoded"]) == (staged, decoded)
                assert h.stats() == before                                     # a scan is not a read
        with pytest.raises(zra.ZraError) as e:                                  # dData inside the archive
            h.cut(pats, d.data_ptr() + 8, 16, separator=c["sep"], fields=mask)
        assert (e.value.zra, e.value.zstd) == (1, 42)
        base, size = h.arena_range()
        assert (base != 0, size) == (slots != 0, slots * fs)
        if slots:
            L = zra.load()
            sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats))
            n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
            before, s0 = h.stats(), h.scan_stats()
            for dptr, dcap in ((base + size - 1, 64), (base - 63, 64), (base, size), (base + 8, 16), (base - 8, size + 16)):
                n.value, ds.value = 0x1234, 0x5678
                st = L.ZraHipArchiveCutRecords(h.h, b"".join(pats), sizes, len(pats), 0, NL, 0, c["sep"], mask, 0, MAXU64, 0, None, 0, ctypes.byref(n), dptr, dcap,
                                               ctypes.byref(ds)).tup()
                assert (st, n.value, ds.value) == ((1, 42), 0, 0) and gpu_engine.extract_stats() == ZERO, (dptr - base, dcap)
            assert (h.stats(), h.scan_stats()) == (before, s0)
            # the arena was not written: the resident frames still stage the content
            recs, sel, nm, packed = SH.model(c, mask, False, 0, U)
            assert h.cut(pats, out.data_ptr(), U + 64, separator=c["sep"], fields=mask, max_records=AS.MAXREC) == (len(sel), len(packed), sel)
            assert out[:len(packed)].cpu().numpy().tobytes() == packed
    finally:
        h.close()


# ---- 10
def test_a_damaged_frame_and_refusals_with_an_engine(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    p = next(q for q in range(5 * fs + 100, 6 * fs) if NL not in data[q - 3:q + 9])
    pats = [data[p:p + 6], b"\xFF\xFE\xFD"]
    sep = 3                                                                    # (a byte of _data's alphabet, not the delimiter)
    c = SH.case("statuses", data, fs, pats, sep=sep)
    arc, d = _arc(gpu_engine, zra, c)
    _check(gpu_engine, zra, d, len(arc), c, bits(1, 2))
    bad = _flip_mid(arc, [7])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    for mode in (0, 1):
        for staging in (0, 4 * fs):
            st, n, ds, mem, _ = _raw(gpu_engine, zra, db, len(bad), pats, sep, 3, 13 * fs, 6, mode=mode, staging=staging)
            assert (st, n, ds, mem) == ((1, want[7]), 0, 0, b"\xEE" * 128), (mode, staging, st, n, ds)
            assert gpu_engine.extract_stats() == ZERO
    _check(gpu_engine, zra, db, len(bad), c, bits(1, 2), 0, 7 * fs)            # the same damage outside the range
    # rule 1 with an engine: nothing decoded, nothing written
    for kw in (dict(sep=NL), dict(mask=0), dict(mode=2), dict(mode=3), dict(pats=[b"a\nb"]), dict(pats=[b""])):
        a = dict(pats=pats, sep=sep, mask=3, mode=0)
        a.update(kw)
        st, n, ds, mem, got = _raw(gpu_engine, zra, d, len(arc), a["pats"], a["sep"], a["mask"], 64, 2, mode=a["mode"])
        assert (st, n, ds, mem, got) == ((1, 42), 0, 0, b"\xEE" * 64, b"\xEE" * 64) and gpu_engine.extract_stats() == ZERO, kw
    # rule 2: dData inside the archive
    import torch
    whole = torch.full((512 + len(arc) + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
    whole[512:512 + len(arc)] = d
    P = whole.data_ptr() + 512
    L = zra.load()
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for dptr, dcap in ((P + 100, 50), (P - 256, len(arc) + 512), (P - 10, 11), (P + len(arc) - 1, 10)):
        n.value, ds.value = 0x1234, 0x5678
        st = L.ZraHipCutRecords(gpu_engine.h, P, len(arc), None, None, 0, 0, NL, 0, sep, 1, 0, MAXU64, 0, None, 0, ctypes.byref(n), dptr, dcap, ctypes.byref(ds)).tup()
        assert (st, n.value, ds.value) == ((1, 42), 0, 0) and gpu_engine.extract_stats() == ZERO, (dptr - P, dcap)
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert host[:512] == b"\xEE" * 512 and host[512 + len(arc):] == b"\xEE" * 512 and host[512:512 + len(arc)] == arc


# ---- 11
@pytest.mark.parametrize("seed", SH.SWEEP_SEEDS)
def test_random_sweep(zra, gpu_engine, seed):
    import torch
    c, calls = SH.sweep(seed)
    arc, d = _arc(gpu_engine, zra, c)
    out = torch.empty(len(c["data"]) + 64, dtype=torch.uint8, device="cuda:0")
    for mask, lo, hi, staging in calls:
        both = _check(gpu_engine, zra, d, len(arc), c, mask, lo, hi, staging=staging, nonempty=False)
        assert gpu_engine.extract_stats()["passes"] >= 3
        whole = gpu_engine.extract(d.data_ptr(), len(arc), c["pats"], out.data_ptr(), len(c["data"]) + 64, offset=lo, length=hi - lo, staging_bytes=staging,
                                   max_records=len(both[False][0]) + 1)
        assert whole[2] == both[False][0] and whole[1] >= len(both[False][1])


# ---- 12
def test_cli_mode_cut(zra, gpu_engine, tmp_path):
    import torch
    data = b"alpha;one;x\nbeta;two\n\ngamma;one;two;three\ndelta" + b"\n" + b"x;y;one;z" * 3
    c = SH.case("cli", data, 16, [b"one"], sep=0x3B)
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    d = _dev(arc)
    p_arc, p_out = tmp_path / "lines.zra", tmp_path / "out.txt"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "cut", str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    out = torch.empty(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    for args, pats, fields, inv in ((("3b", "1,3", "one"), [b"one"], "1,3", False), (("-v", "3b", "2-", "one"), [b"one"], "2-", True),
                                    (("3b", "2,4-"), [], "2,4-", False), (("3b", "-2", "one", "hex:" + b"delta".hex()), [b"one", b"delta"], "-2", False)):
        n, ds, _ = gpu_engine.cut(d.data_ptr(), len(arc), pats, out.data_ptr(), len(data) + 64, separator=0x3B, fields=fields, invert=inv)
        packed = out[:ds].cpu().numpy().tobytes()
        assert packed == SH.model(c, CM.field_mask(fields), inv, pats=pats)[3] and packed
        r = run(*args)
        assert r.returncode == 0 and r.stdout == packed, (args, r.stdout, r.stderr)
    assert SH.model(c, 0b101, False)[3] == b"alpha;x\ngamma;two\nx;one\n"
    r = run("-o", p_out, "3b", "1,3", "one")
    assert r.returncode == 0 and r.stdout == b"" and p_out.read_bytes() == b"alpha;x\ngamma;two\nx;one\n"
    r = run("3b", "1", "nowhere")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    for args in (("0a", "1"), ("3b", "0"), ("3b", "3-1"), ("3b",), ("3b", "65"), ("zz", "1"), ("-v", "3b", "1"), ("-d", "3b", "3b", "1")):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"", (args, r.stdout, r.stderr)
