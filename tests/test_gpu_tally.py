"""GPU tests of ZraHipTallyRecords, ZraHipTallyFields and ZraHipArchiveTallyFields (include/zra_hip.h): the distinct records of a
packed text and their counts. The yardstick everywhere is tests/tally_model.py on the inputs of tests/tally_shapes.py, which
tests/test_tally_abi.py holds to the seams they are built for. The text lies in a device buffer between 64 guard bytes; dKeys is a
0xEE-filled buffer handed over 64 bytes in, with a capacity that leaves 64 guard bytes behind it; the entry array is 0xEE-filled and
two entries longer than its capacity. After every call the guards, the text and the entries behind the result are what they were.
Every check compares the status, the four words, every entry, the bytes of dKeys, the tally's stats, and the extract's, the grep's
and the searches' stats with what they were. Every comparison is exact but two: the longest probe and the inserts into the table
depend on the order in which lanes arrive and are held to their bounds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cut_shapes as CS
import tally_model as TM
import tally_shapes as SH
import test_gpu_archive_scan as AS
from test_gpu_update import _compress, _data, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
NL = 10
GUARD = 64
TOO_SMALL = (6, 0)
ZERO = dict.fromkeys(("records", "distinct", "skipped", "key_bytes", "table_slots", "longest_probe", "table_inserts"), 0)
bits = CS.bits


def _others(eng):
    return eng.extract_stats(), eng.grep_stats(), eng.search_stats(), eng.search_multi_stats()


def _text_dev(text):
    """the text on the device between two guards: (tensor, pointer of its first byte)"""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xEE" * GUARD + bytes(text) + b"\xEE" * GUARD, dtype=np.uint8).copy()).to("cuda:0")
    return t, t.data_ptr() + GUARD


def _entries(mem, n):
    a = np.frombuffer(mem[:24 * n], dtype=np.uint64).reshape(n, 3)
    return [tuple(int(v) for v in row) for row in a]


def _raw(eng, zra, text, key_cap, entry_cap, max_distinct=0, delim=NL, dev=None):
    """(status, (records, distinct, skipped, key size), the bytes of an entry array two entries longer than the capacity, the first
    key_cap bytes of dKeys) of one ZraHipTallyRecords; asserts the guards of dKeys and the text with its guards intact"""
    import torch
    t, p = dev or _text_dev(text)
    keys = torch.full((GUARD + key_cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (3 * (entry_cap + 2)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    w = [ctypes.c_uint64(0x1234 + i) for i in range(4)]
    eng._order()
    st = zra.load().ZraHipTallyRecords(eng.h, p if len(text) else None, len(text), delim, max_distinct, arr if entry_cap else None, entry_cap,
                                       keys.data_ptr() + GUARD if key_cap else None, key_cap, *(ctypes.byref(x) for x in w)).tup()
    torch.cuda.synchronize()
    host = keys.cpu().numpy().tobytes()
    assert host[:GUARD] == b"\xEE" * GUARD and host[GUARD + key_cap:] == b"\xEE" * GUARD, ("guard", st, key_cap, entry_cap)
    assert t.cpu().numpy().tobytes() == b"\xEE" * GUARD + bytes(text) + b"\xEE" * GUARD, "the text is only read"
    return st, tuple(x.value for x in w), bytes(arr), host[GUARD:GUARD + key_cap]


def _check_stats(eng, tag, n, skipped, entries, keys, max_distinct=0):
    s = eng.tally_stats()
    want = dict(records=n, distinct=len(entries), skipped=skipped, key_bytes=len(keys), table_slots=TM.slots(n, max_distinct))
    assert {k: s[k] for k in want} == want, (tag, s, want)
    assert (1 if entries else 0) <= s["longest_probe"] <= s["table_slots"] and len(entries) <= s["table_inserts"] <= n - skipped, (tag, s)
    return s


def _check(eng, zra, c, max_distinct=0, slack=5, dev=None, delim=NL):
    """one tally of the shape against the model; returns (the words, the entries, the key text, the stats)"""
    text = c["text"]
    n, skipped, entries, keys = TM.tally(text, delim)
    tag = (c["name"], max_distinct)
    others = _others(eng)
    st, w, mem, got = _raw(eng, zra, text, len(keys) + slack, len(entries) + 1, max_distinct, delim, dev)
    print("tally", tag, "status", st, "words", w, "model", (n, len(entries), skipped, len(keys)))
    assert (st, w) == ((0, 0), (n, len(entries), skipped, len(keys))), (tag, st, w)
    have = _entries(mem, w[1])
    if have != entries:
        bad = next(i for i in range(len(entries)) if have[i] != entries[i])
        raise AssertionError((tag, "first wrong entry", bad, have[bad], entries[bad]))
    assert mem[24 * w[1]:] == b"\xEE" * (24 * (len(entries) + 3 - w[1])), tag
    assert got[:w[3]] == keys, (tag, "keys")
    assert sum(e[2] for e in have) == n - skipped
    s = _check_stats(eng, tag, n, skipped, entries, keys, max_distinct) if text else None
    if not text:
        assert eng.tally_stats() == ZERO
    assert _others(eng) == others, tag
    return w, have, got[:w[3]], s


# ---- 1
@pytest.mark.parametrize("kind", SH.DEGENERATE)
def test_degenerate_text(zra, gpu_engine, kind):
    c = SH.degenerate(kind)
    w, have, keys, _ = _check(gpu_engine, zra, c)
    if kind == "delimiters":
        assert have == [(0, 0, 7)] and keys == b"\n"
    if kind in ("one_with", "one_without"):
        assert have == [(0, 10, 1)] and keys == b"status=200\n"
    if kind == "tile_plus_1":
        assert have[-1] == (SH.T, 1, 1) and keys.endswith(b"\nz\n")


def test_empty_text(zra, gpu_engine):
    c = SH.shape("empty", b"")
    assert _check(gpu_engine, zra, c)[0] == (0, 0, 0, 0)
    st, w, mem, got = _raw(gpu_engine, zra, b"", 0, 0)
    assert (st, w) == ((0, 0), (0, 0, 0, 0))


# ---- 2
@pytest.mark.parametrize("kind", SH.SEAMS)
def test_tile_seams(zra, gpu_engine, kind):
    c = SH.seam(kind)
    w, have, keys, _ = _check(gpu_engine, zra, c)
    o, n = c["big"]
    by_offset = {e[0]: e for e in have}
    if kind == "bare_tile":
        assert w[2] == 1 and o not in by_offset                                # longer than the cap: skipped, in no entry
    elif kind == "mirror":
        assert by_offset[o] == (o, n, 4) and not any(r in by_offset for r in c["repeats"])
    elif kind == "straddle":
        assert by_offset[o] == (o, n, 2)
    else:
        assert by_offset[o] == (o, n, 1)


# ---- 3
@pytest.mark.parametrize("kind", SH.KEY_LENGTHS)
def test_key_lengths(zra, gpu_engine, kind):
    c = SH.key_length(kind)
    w, have, keys, _ = _check(gpu_engine, zra, c)
    K = SH.MAX_KEY
    if kind == "sizes":
        assert w == (7, 3, 2, K - 1 + K + 5 + 3) and [e[1:] for e in have] == [(K - 1, 2), (K, 2), (5, 1)]
    if kind == "last_byte":
        assert [e[1:] for e in have] == [(K, 2), (K, 1)]
    if kind == "first_byte":
        assert [e[1:] for e in have] == [(K, 1), (K, 2)]
    if kind == "prefix":
        assert keys == b"abcd\nabc\n\nab\nabcde\n" and [e[2] for e in have] == [2, 2, 2, 1, 1]


# ---- 4
@pytest.mark.parametrize("kind", SH.SKEWS)
def test_skew(zra, gpu_engine, kind):
    c = SH.skew(kind)
    w, have, keys, s = _check(gpu_engine, zra, c)
    assert w[0] == SH.SKEW_RECORDS and w[1] == {"one": 1, "three": 3, "distinct": SH.SKEW_RECORDS}[kind]
    tiles = -(-len(c["text"]) // SH.T)
    if kind != "distinct":                                                     # (combining) one insert per key a workgroup saw, not one per record
        assert s["table_inserts"] <= w[1] * tiles, s


# ---- 5, 6
def test_collisions_and_determinism(zra, gpu_engine):
    """the 300-key text at the full hash three times, then with 0, 1 and 2 bits of it: the same bytes every time"""
    c = SH.collisions()
    dev = _text_dev(c["text"])
    full = [_check(gpu_engine, zra, c, dev=dev)[:3] for _ in range(3)]
    assert full[0] == full[1] == full[2]
    try:
        for hash_bits in (0, 1, 2):
            gpu_engine.debug_tally_hash_bits(hash_bits)
            w, have, keys, s = _check(gpu_engine, zra, c, dev=dev)
            assert (w, have, keys) == full[0], hash_bits
            print("hash bits", hash_bits, s)
            # by pigeonhole: 300 keys start at no more than 2 ** hash_bits slots, so one start has 300 / 2 ** hash_bits keys, and the
            # last of those to claim looked at the slots of all the others and at its own: 300, 150 and 75
            assert s["longest_probe"] >= -(-c["keys"] // (1 << hash_bits)), (hash_bits, s)
    finally:
        gpu_engine.debug_tally_hash_bits(None)
    assert _check(gpu_engine, zra, c, dev=dev)[:3] == full[0]


# ---- 7
def test_max_distinct(zra, gpu_engine):
    c = SH.promised()
    D, text = c["D"], c["text"]
    n, skipped, entries, keys = TM.tally(text)
    assert len(entries) == D
    dev = _text_dev(text)
    _check(gpu_engine, zra, c, max_distinct=D, dev=dev)
    _check(gpu_engine, zra, c, max_distinct=D + 1000000, dev=dev)              # (the table is sized by the records then)
    try:
        for hash_bits in (None, 0):
            gpu_engine.debug_tally_hash_bits(hash_bits)
            others = _others(gpu_engine)
            st, w, mem, got = _raw(gpu_engine, zra, text, len(keys) + 8, D + 4, max_distinct=D - 1, dev=dev)
            assert (st, w) == (TOO_SMALL, (n, n - skipped, skipped, 0)), (hash_bits, st, w)
            assert mem == b"\xEE" * len(mem) and got == b"\xEE" * len(got), hash_bits
            assert gpu_engine.tally_stats() == ZERO and _others(gpu_engine) == others
            _check(gpu_engine, zra, c, max_distinct=D, dev=dev)
    finally:
        gpu_engine.debug_tally_hash_bits(None)


# ---- 8
def test_capacities(zra, gpu_engine):
    c = SH.collisions()
    text = c["text"]
    n, skipped, entries, keys = TM.tally(text)
    D, K = len(entries), len(keys)
    dev = _text_dev(text)
    words = (n, D, skipped, K)
    st, w, mem, got = _raw(gpu_engine, zra, text, 0, 0, dev=dev)               # the sizing call
    assert (st, w) == ((0, 0), words)
    _check_stats(gpu_engine, "sizing", n, skipped, entries, keys)
    for kcap, ecap in ((K + 9, D - 1), (K - 1, D), (K - 1, 0), (0, D - 1)):
        st, w, mem, got = _raw(gpu_engine, zra, text, kcap, ecap, dev=dev)
        assert (st, w) == (TOO_SMALL, words), (kcap, ecap, st, w)
        assert mem == b"\xEE" * len(mem) and got == b"\xEE" * len(got), (kcap, ecap)
        assert gpu_engine.tally_stats() == ZERO
    for kcap, ecap in ((K, D), (K, 0), (0, D), (K + 100, D + 5)):
        st, w, mem, got = _raw(gpu_engine, zra, text, kcap, ecap, dev=dev)
        assert (st, w) == ((0, 0), words), (kcap, ecap, st, w)
        assert got[:K] == (keys if kcap else b"") and got[K:] == b"\xEE" * max(0, kcap - K), (kcap, ecap)
        assert _entries(mem, D if ecap else 0) == (entries if ecap else []) and mem[24 * (D if ecap else 0):] == b"\xEE" * (24 * (ecap + 2 - (D if ecap else 0)))
        _check_stats(gpu_engine, (kcap, ecap), n, skipped, entries, keys)


def test_refusals_with_an_engine(zra, gpu_engine):
    import torch
    L = zra.load()
    c = SH.degenerate("tile")
    t, p = _text_dev(c["text"])
    size = len(c["text"])
    w = [ctypes.c_uint64(7) for _ in range(4)]
    refs = [ctypes.byref(x) for x in w]
    arr = (ctypes.c_uint64 * 6)()
    _check(gpu_engine, zra, c)
    calls = [(None, size, None, 0, None, 0, refs), (p, size, None, 2, None, 0, refs), (p, size, None, 0, None, 8, refs),
             (p, size, None, 0, p + 10, 8, refs), (p, size, None, 0, p - 4, 5, refs), (p, size, None, 0, p + size - 1, 64, refs), (p, 1 << 40, None, 0, None, 0, refs)]
    calls += [(p, size, arr, 2, None, 0, refs[:i] + [None] + refs[i + 1:]) for i in range(4)]
    for text, n, ent, ecap, keys, kcap, words in calls:
        for x in w:
            x.value = 7
        st = L.ZraHipTallyRecords(gpu_engine.h, text, n, NL, 0, ent, ecap, keys, kcap, *words).tup()
        assert st == (1, 42) and all(x.value == 0 for x, r in zip(w, words) if r is not None), (n, ecap, kcap, st)
        assert gpu_engine.tally_stats() == ZERO
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == b"\xEE" * GUARD + c["text"] + b"\xEE" * GUARD


# ---- 9: the composite
def _fields(eng, zra, d, size, c, mask, pats, inv=False, staging=0, handle=None, work_cap=None, lo=0, hi=None):
    """one composite call against the model: the workspace between guards, then the tally's outputs as _check compares them"""
    import torch
    packed, (n, skipped, entries, keys) = TM.tally_fields(c["data"], pats, c["sep"], mask, NL, inv, lo, hi)
    cap = len(packed) + 7 if work_cap is None else work_cap
    work = torch.full((GUARD + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    kbuf = torch.full((GUARD + len(keys) + 5 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * (3 * (len(entries) + 3)))()
    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
    w = [ctypes.c_uint64(0x1234 + i) for i in range(5)]
    sizes = (ctypes.c_uint32 * len(pats))(*(len(p) for p in pats)) if pats else None
    tail = (b"".join(pats) if pats else None, sizes, len(pats), 0, NL, int(inv), c["sep"], mask, lo, MAXU64 if hi is None else hi - lo, staging, work.data_ptr() + GUARD, cap,
            ctypes.byref(w[4]), 0, arr, len(entries) + 1, kbuf.data_ptr() + GUARD, len(keys) + 5, *(ctypes.byref(x) for x in w[:4]))
    eng._order()
    L = zra.load()
    st = (L.ZraHipTallyFields(eng.h, d.data_ptr(), size, *tail) if handle is None else L.ZraHipArchiveTallyFields(handle.h, *tail)).tup()
    torch.cuda.synchronize()
    hw, hk = work.cpu().numpy().tobytes(), kbuf.cpu().numpy().tobytes()
    assert hw[:GUARD] == b"\xEE" * GUARD and hw[GUARD + cap:] == b"\xEE" * GUARD and hk[:GUARD] == b"\xEE" * GUARD and hk[GUARD + len(keys) + 5:] == b"\xEE" * GUARD
    tag = (c["name"], hex(mask), len(pats), inv, staging, handle is not None)
    words = tuple(x.value for x in w)
    print("tally fields", tag, "status", st, "words", words, "model", (n, len(entries), skipped, len(keys), len(packed)))
    if cap < len(packed):
        assert (st, words) == (TOO_SMALL, (0, 0, 0, 0, len(packed))) and bytes(arr) == b"\xEE" * ctypes.sizeof(arr) and hk == b"\xEE" * len(hk), (tag, st, words)
        assert eng.tally_stats() == ZERO
        return None
    assert (st, words) == ((0, 0), (n, len(entries), skipped, len(keys), len(packed))), (tag, st, words)
    assert hw[GUARD:GUARD + len(packed)] == packed and _entries(bytes(arr), len(entries)) == entries, tag
    assert bytes(arr)[24 * len(entries):] == b"\xEE" * 72 and hk[GUARD:GUARD + len(keys)] == keys, tag
    if packed:
        _check_stats(eng, tag, n, skipped, entries, keys)
        assert eng.extract_stats()["packed_bytes"] == len(packed)
    return n, entries, keys


def _arc(eng, zra, c):
    if "_arc" not in c:
        c["_arc"] = _compress(eng, zra, c["data"], 3, c["fs"], True)
    return c["_arc"], _dev(c["_arc"])


@pytest.mark.parametrize("kind", ["csv", "log"])
def test_fields_of_csv_and_log_lines(zra, gpu_engine, kind):
    """one pass and at least three; with and without a pattern; inverted; whole records against an extract followed by the primitive"""
    import torch
    fs = 4096
    if kind == "csv":
        c = CS.case("tally_csv", CS.csv_lines(31, 40 * fs + 123, 3, 5), fs, [CS.NEEDLE])
        masks = (bits(1), bits(2, 3))
    else:
        c = CS.case("tally_log", CS.log_lines(33, 40 * fs + 77), fs, [b"ERROR", b"failed"], sep=0x20)
        masks = (bits(3), bits(3, 4))                                          # the level: 4 values; level and component: 36
    arc, d = _arc(gpu_engine, zra, c)
    for staging in (0, 8 * fs):
        for mask in masks:
            for pats, inv in ((c["pats"], False), ([], False), (c["pats"], True)):
                got = _fields(gpu_engine, zra, d, len(arc), c, mask, pats, inv, staging)
                assert got[0] > 20 and len(got[1]) > 1
                assert (gpu_engine.extract_stats()["passes"] == 1) if staging == 0 else (gpu_engine.extract_stats()["passes"] >= 3)
    if kind == "log":
        levels = _fields(gpu_engine, zra, d, len(arc), c, bits(3), [], False, 0)[2].split(b"\n")[:-1]
        assert sorted(levels[:4]) == [b"DEBUG", b"ERROR", b"INFO", b"WARN"]      # (a fifth key is what the text's cut end left of a level)
    # a mask of all ones: the extract's text, tallied by the primitive
    whole = _fields(gpu_engine, zra, d, len(arc), c, CS.ALL, c["pats"], False, 8 * fs)
    out = torch.empty(len(c["data"]) + 64, dtype=torch.uint8, device="cuda:0")
    n, ds, _ = gpu_engine.extract(d.data_ptr(), len(arc), c["pats"], out.data_ptr(), len(c["data"]) + 64)
    two = gpu_engine.tally_text(out.data_ptr(), ds, max_entries=len(whole[1]) + 1)
    assert (two[0], two[2]) == (whole[0], whole[1]) and n == whole[0]
    # dWork one byte short: the cut's rule 7 with what dWork needs; the sizing call of the workspace
    packed = TM.tally_fields(c["data"], c["pats"], c["sep"], masks[0])[0]
    for cap in (len(packed) - 1, 0):
        assert _fields(gpu_engine, zra, d, len(arc), c, masks[0], c["pats"], work_cap=cap) is None
    with pytest.raises(zra.ZraError) as e:
        gpu_engine.tally(d.data_ptr(), len(arc), c["pats"], 0, 0, separator=c["sep"], fields=masks[0])
    assert (e.value.zra, e.value.needed_work) == (6, len(packed))
    work = torch.empty(len(packed), dtype=torch.uint8, device="cuda:0")
    n, skipped, entries = gpu_engine.tally(d.data_ptr(), len(arc), c["pats"], work.data_ptr(), len(packed), separator=c["sep"], fields=masks[0])
    assert (n, skipped, entries) == TM.tally(packed)[:3] and gpu_engine.last_tally["work_size"] == len(packed)


@pytest.mark.parametrize("warm,slots", [((), 0), (AS.WARM, 12), (tuple(range(AS.NF)), AS.NF)])
def test_fields_through_the_handle(zra, gpu_engine, warm, slots):
    """none, some and all frames resident: the engine call's answer, the handle's scan counters moved as by its cut, the cache left alone"""
    import torch
    fs = 1000
    data, pats = AS._content(77, fs)
    c = CS.case("tally_handle", data, fs, pats, sep=ord("d"))
    arc, d = _arc(gpu_engine, zra, c)
    h = AS._open_warm(zra, gpu_engine, d, len(arc), fs, len(data), warm, slots)
    try:
        for staging in (0, 3 * fs):
            for use, inv in ((pats, False), ([], False), (pats, True)):
                before, s0 = h.stats(), h.scan_stats()
                got = _fields(gpu_engine, zra, d, len(arc), c, bits(1, 3), use, inv, staging, handle=h)
                s1 = h.scan_stats()
                assert got == _fields(gpu_engine, zra, d, len(arc), c, bits(1, 3), use, inv, staging) and got[0] > 0
                assert h.stats() == before and s1["scans"] == s0["scans"] + 1
        packed = TM.tally_fields(data, pats, c["sep"], bits(1, 3))[0]
        work = torch.empty(len(packed), dtype=torch.uint8, device="cuda:0")
        assert h.tally(pats, work.data_ptr(), len(packed), separator=c["sep"], fields="1,3") == TM.tally(packed)[:3]
        base, size = h.arena_range()
        for keys in ([d.data_ptr() + 8] + ([base + 8] if slots else [])):       # dKeys inside the archive, inside the arena
            with pytest.raises(zra.ZraError) as e:
                h.tally(pats, work.data_ptr(), len(packed), separator=c["sep"], fields="1,3", d_keys=keys, key_cap=16)
            assert (e.value.zra, e.value.zstd) == (1, 42)
    finally:
        h.close()


def test_a_damaged_frame_gives_the_cuts_status_and_zeroed_words(zra, gpu_engine):
    import torch
    fs = 4096
    data = _data(np.random.RandomState(7), 12 * fs)
    sep = 3
    c = CS.case("tally_statuses", data, fs, [], sep=sep)
    arc, d = _arc(gpu_engine, zra, c)
    _fields(gpu_engine, zra, d, len(arc), c, bits(1, 2), [])
    bad = _flip_mid(arc, [7])
    db = _dev(bad)
    want = _frame_status(gpu_engine, zra, bad, d_arc=db)
    assert set(want) == {7} and want[7] != 0, want
    L = zra.load()
    work = torch.full((13 * fs,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arr = (ctypes.c_uint64 * 30)()
    for staging in (0, 4 * fs):
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        w = [ctypes.c_uint64(0x1234) for _ in range(5)]
        gpu_engine._order()
        st = L.ZraHipTallyFields(gpu_engine.h, db.data_ptr(), len(bad), None, None, 0, 0, NL, 0, sep, 3, 0, MAXU64, staging, work.data_ptr(), 13 * fs, ctypes.byref(w[4]), 0,
                                 arr, 10, None, 0, *(ctypes.byref(x) for x in w[:4])).tup()
        assert st == (1, want[7]) and [x.value for x in w] == [0] * 5 and bytes(arr) == b"\xEE" * 240, (staging, st)
        assert gpu_engine.tally_stats() == ZERO and gpu_engine.extract_stats()["records"] == 0
    # the cut's rule 1 through the composite
    for kw in (dict(sep=NL), dict(mask=0)):
        a = dict(sep=sep, mask=3)
        a.update(kw)
        w = [ctypes.c_uint64(0x1234) for _ in range(5)]
        st = L.ZraHipTallyFields(gpu_engine.h, d.data_ptr(), len(arc), None, None, 0, 0, NL, 0, a["sep"], a["mask"], 0, MAXU64, 0, work.data_ptr(), 13 * fs,
                                 ctypes.byref(w[4]), 0, None, 0, None, 0, *(ctypes.byref(x) for x in w[:4])).tup()
        assert st == (1, 42) and [x.value for x in w] == [0] * 5 and gpu_engine.tally_stats() == ZERO, kw


# ---- 10
def test_cli_mode_tally(zra, gpu_engine, tmp_path):
    data = b"GET;200;/a\nGET;404;/b\nPUT;200;/a\n\nGET;200;/c\nbad\nPUT;500;/a;one" + b"\n" + b"GET;200;/one" * 1
    c = CS.case("cli", data, 16, [b"one"], sep=0x3B)
    arc = _compress(gpu_engine, zra, data, 3, 16, True)
    p_arc = tmp_path / "lines.zra"
    p_arc.write_bytes(arc)

    def run(*args):
        return subprocess.run([TOOL, "tally", str(p_arc)] + [str(x) for x in args], capture_output=True, timeout=120)

    for args, pats, fields, inv in ((("3b", "2"), [], "2", False), (("3b", "1,3"), [], "1,3", False), (("3b", "2", "one"), [b"one"], "2", False),
                                    (("-v", "3b", "1", "one"), [b"one"], "1", True)):
        import cut_model as CM
        packed, (n, skipped, entries, keys) = TM.tally_fields(data, pats, 0x3B, CM.field_mask(fields), NL, inv)
        r = run(*args)
        assert r.returncode == 0 and r.stdout == TM.lines(packed, entries) and r.stdout, (args, r.stdout, r.stderr)
    assert run("3b", "2").stdout == b"4 200\n1 404\n2 \n1 500\n"
    r = run("3b", "1", "nowhere")
    assert r.returncode == 1 and r.stdout == b"", (r.stdout, r.stderr)
    for args in (("0a", "1"), ("3b", "0"), ("3b",), ("zz", "1"), ("-v", "3b", "1")):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"", (args, r.stdout, r.stderr)
