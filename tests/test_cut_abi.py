"""CPU tests of the cut (include/zra_hip.h: ZraHipFieldMask, ZraHipCutRecords, ZraHipArchiveCutRecords): declared, exported and bound;
the LIST parser against pinned answers; every rule-1 refusal before anything touches a device; no CPU result without a GPU; the model
the GPU tests use as their yardstick (tests/cut_model.py) against answers pinned by hand and against coreutils; the device's
per-byte rule (a separator count that saturates at 63, a field mask and a separator mask) and the separator carry of its combine()
restated in Python and held against the model's true field numbers; the inputs of the GPU tests (tests/cut_shapes.py) held to the
seams they are built for; and the zra_cut_* kernels compiled inside their bounds."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cut_model as CM
import cut_shapes as SH
import extract_model as XM
import grep_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipFieldMask", "ZraHipCutRecords", "ZraHipArchiveCutRecords"]
MAXU64 = (1 << 64) - 1
NL = 10
COMMA = SH.COMMA
bits = SH.bits


def test_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_CUT_MAX_FIELD\s+64\b", txt)
    assert "zra_cut.hip" in open(os.path.join(ROOT, "zra_amd", "build.py")).read()
    for f in (zra.Engine.cut, zra.Archive.cut):
        p = inspect.signature(f).parameters
        assert all(k in p for k in ("separator", "fields", "delimiter", "invert", "offset", "length", "staging_bytes", "max_records", "syntax")), p
    assert callable(zra.field_mask)


# ---- ZraHipFieldMask
PINNED_LISTS = {"1,3": 0b101, "5-7,9-": (MAXU64 & ~0xFF) | 0x70, "-3": 0b111, "64-": 1 << 63, "60-70": 0x1F << 59, "63-": 0b11 << 62, "1": 1, "64": 1 << 63, "1-": MAXU64,
                "3,1,2": 0b111, "2-2": 0b10, "100-": 1 << 63, "70-80": 1 << 63, "1-64": MAXU64, "62-1000": 0b111 << 61, "-64": MAXU64, "-65": MAXU64, "7,7": 1 << 6,
                "1,64-": 1 | 1 << 63}
REFUSED_LISTS = ["", "0", "0-", "-0", "1-0", "3-1", "7-6", "65", "100", "1,65", "a", "1,a", "1 ,2", " 1", "1,", ",1", "1,,2", "-", "1--2", "1-2-3", "+1", "1;2", "1.5",
                 "99999999999999999999999", "64-63"]


def test_field_mask_pinned_answers(zra):
    L = zra.load()
    for text, want in PINNED_LISTS.items():
        m = ctypes.c_uint64(0x1234)
        assert L.ZraHipFieldMask(text.encode(), ctypes.byref(m)).tup() == (0, 0) and m.value == want, (text, hex(m.value), hex(want))
        assert zra.field_mask(text) == want == CM.field_mask(text), text
    for text in REFUSED_LISTS:
        m = ctypes.c_uint64(0x1234)
        assert L.ZraHipFieldMask(text.encode(), ctypes.byref(m)).tup() == (1, 42) and m.value == 0, (text, hex(m.value))
        assert CM.field_mask(text) is None or text == "99999999999999999999999", text
        with pytest.raises(zra.ZraError):
            zra.field_mask(text)
    m = ctypes.c_uint64(0x1234)
    assert L.ZraHipFieldMask(None, ctypes.byref(m)).tup() == (1, 42) and m.value == 0
    assert L.ZraHipFieldMask(b"1", None).tup() == (1, 42)


# ---- rule 1
def test_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords and *dataSize are zeroed, the record array is left alone and dData is never touched (it is not even
    memory here): the three refusals of the cut (separator == delimiter, fieldMask == 0, INVERT with no pattern), the extract's, and,
    for want of an engine or an archive, the accepted calls; every mode word, and the null combinations."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 400)
    sizes = (ctypes.c_uint32 * 64)(*([3] * 64))
    arr = (ctypes.c_uint64 * 8)()
    for sep, mask, k in ((COMMA, 1, 1), (NL, 1, 1), (COMMA, 0, 1), (COMMA, 1, 0), (COMMA, MAXU64, 64), (COMMA, 1, 65), (NL, 0, 0)):
        for mode in (0, 1, 2, 3, 1 << 31):
            for pp, ss in ((pats, sizes), (None, None)):
                for arc in ((None, 0), (P(64), 100)):
                    for dd in ((None, 0), (P(4096), 64), (None, 64)):
                        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                        n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
                        tag = (sep, mask, k, mode, pp is None, arc, dd)
                        st = L.ZraHipCutRecords(None, *arc, pp, ss, k, 0, NL, mode, sep, mask, 0, MAXU64, 0, arr, 4, ctypes.byref(n), *dd, ctypes.byref(ds)).tup()
                        assert st == (1, 42) and (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64, tag
                        assert L.ZraHipCutRecords(None, *arc, pp, ss, k, 0, NL, mode, sep, mask, 0, MAXU64, 0, None, 0, None, *dd, None).tup() == (1, 42), tag
                ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
                st = L.ZraHipArchiveCutRecords(None, pp, ss, k, 0, NL, mode, sep, mask, 0, MAXU64, 0, arr, 4, ctypes.byref(n), P(4096), 64, ctypes.byref(ds)).tup()
                assert st == (1, 42) and (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64, (sep, mask, k, mode)
                assert L.ZraHipArchiveCutRecords(None, pp, ss, k, 0, NL, mode, sep, mask, 0, MAXU64, 0, None, 4, None, None, 64, None).tup() == (1, 42)


def test_fails_loudly_without_gpu(zra):
    """no engine, no result: the entry points refuse a null engine and a null handle with zeroed words (on any machine), and without
    a GPU Engine.cut has no engine to run on: never a CPU answer"""
    L = zra.load()
    sizes = (ctypes.c_uint32 * 2)(3, 1)
    n, ds = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.ZraHipCutRecords(None, None, 0, b"abcd", sizes, 2, 0, NL, 0, COMMA, 5, 0, MAXU64, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(ds)).tup() == (1, 42)
    assert (n.value, ds.value) == (0, 0)
    n.value = ds.value = 7
    assert L.ZraHipArchiveCutRecords(None, None, None, 0, 0, NL, 0, COMMA, 5, 0, MAXU64, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(ds)).tup() == (1, 42)
    assert (n.value, ds.value) == (0, 0)
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_cut.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).cut(64, 100, [b"abc"], 0, 0, separator=COMMA, fields="1,3")


# ---- the model
PROBE = b"a,b,c,d\na,b\nnosep\n\n,x,,y\n"


def _lines(packed):
    return packed.split(b"\n")[:-1]


def test_answers_pinned_by_hand():
    """the probes of GNU cut 8.32 (`cut -d, -f1,3` and `-f2,4-`), and where the call differs from cut: a record without a separator
    keeps what field 1 keeps"""
    assert _lines(CM.cut(PROBE, [], COMMA, bits(1, 3))[3]) == [b"a,c", b"a", b"nosep", b"", b","]
    got = _lines(CM.cut(PROBE, [], COMMA, CM.field_mask("2,4-"))[3])
    assert [got[0], got[1], got[4]] == [b"b,d", b"b", b"x,y"] and got[2] == got[3] == b""   # (cut prints `nosep` whole)
    assert CM.cut(b"x\nlast,no,newline", [], COMMA, bits(2))[3] == b"\nno\n"
    assert CM.cut(b"last,no,newline", [], COMMA, bits(2)) == ([(0, 15)], [(0, 15)], 0, b"no\n")
    # selection is the extract's: the list and the matches are its, whatever the mask
    d = b"k=1,ERR,x\nk=2,ok,y\n\nk=3,ERR,ERR"
    for inv in (False, True):
        recs, sel, nm, packed = CM.cut(d, [b"ERR"], COMMA, bits(1, 3), NL, inv)
        assert (recs, sel, nm) == XM.extract(d, [b"ERR"], NL, inv)[:3] and nm == 3
        assert packed == (b"k=2,y\n\n" if inv else b"k=1,x\nk=3,ERR\n")
    # lo cuts a record: field 1 starts at lo; hi ends one: it gets its delimiter
    assert CM.cut(d, [], COMMA, bits(1), NL, False, 4, 14) == ([(4, 5), (10, 4)], [(4, 5), (10, 4)], 0, b"ERR\nk=2\n")
    assert CM.cut(d, [], COMMA, bits(1), NL, False, 3, 14) == ([(3, 6), (10, 4)], [(3, 6), (10, 4)], 0, b"\nk=2\n")
    assert CM.cut(d, [], COMMA, bits(2), NL, False, 3, 14)[3] == b"ERR\n\n"
    # fields 64 and above answer to bit 63; the separator in front of field 64 needs a chosen field below it
    r = b",".join(b"%d" % j for j in range(1, 71))
    assert CM.cut_record(r, COMMA, 1 << 63) == b",".join(b"%d" % j for j in range(64, 71))
    assert CM.cut_record(r, COMMA, 1 << 62) == b"63" and CM.cut_record(r, COMMA, 0b11 << 62) == b",".join(b"%d" % j for j in range(63, 71))
    assert CM.cut_record(r, COMMA, 1 | 1 << 63) == b"1," + b",".join(b"%d" % j for j in range(64, 71))
    assert CM.cut_record(b",,,", COMMA, bits(2, 4)) == b"," and CM.cut_record(b",,,", COMMA, bits(1)) == b"" and CM.cut_record(b"", COMMA, 1) == b""


def _list_of(mask):
    return ",".join(("%d-" % 64) if j == 64 else str(j) for j in range(1, 65) if mask >> (j - 1) & 1)


def test_model_against_coreutils():
    """`grep -F PATTERN | cut -d, -f LIST` under LC_ALL=C: any mask that holds field 1 on any text; masks without field 1 on text whose
    every record holds a separator"""
    grep, cut = shutil.which("grep"), shutil.which("cut")
    if not grep or not cut:
        pytest.skip("grep and cut of coreutils are not installed")
    env = dict(os.environ, LC_ALL="C")
    rng = np.random.RandomState(17)

    def text(always_sep):
        lines = []
        for _ in range(int(rng.randint(1, 40))):
            f = [bytes(rng.choice(list(b"abER"), size=int(rng.randint(0, 5))).astype(np.uint8)) for _ in range(int(rng.randint(2 if always_sep else 1, 9)))]
            lines.append(b",".join(f))
        if always_sep and rng.randint(2):
            lines.append(b"," * 70 + b"ER")
        return b"\n".join(lines) + (b"\n" if rng.randint(2) else b"")

    n = 0
    for case in range(120):
        always = bool(case & 1)
        data = text(always)
        if not data.strip(b"\n") and not data:
            continue
        mask = 0
        for j in rng.randint(1, 10, size=int(rng.randint(1, 4))):
            mask |= 1 << (int(j) - 1)
        if rng.randint(3) == 0:
            mask |= 1 << 63
        if not always:
            mask |= 1
        for pats, inv in (([], False), ([b"ER"], False), ([b"ER"], True)):
            if data.endswith(b"\n\n") or data == b"\n" or (data and not data.endswith(b"\n") and data.split(b"\n")[-1] == b""):
                continue
            src = data
            if pats:
                src = subprocess.run([grep, "-F"] + (["-v"] if inv else []) + ["-e", pats[0].decode()], input=data, capture_output=True, env=env).stdout
            want = subprocess.run([cut, "-d,", "-f", _list_of(mask)], input=src, capture_output=True, env=env, check=True).stdout
            assert CM.cut(data, pats, COMMA, mask, NL, inv)[3] == want, (data, hex(mask), pats, inv)
            n += 1
    assert n > 200


# ---- the device's rule (zra_cut.hip: (fields), separator_mask(), combine(), advance()), restated
SAT = 63


def _separator_mask(mask):
    m = 0
    for c in range(64):
        bit = min(c + 1, 63)
        front = MAXU64 if c >= 63 else (1 << (c + 1)) - 1
        if (mask >> bit) & 1 and mask & front:
            m |= 1 << c
    return m


def _device_cut(record, mask, c0=0):
    """the kept bytes of a record by the device's rule: c = the separators in front of the byte, saturated at 63; a content byte asks
    bit c of the field mask, a separator bit c of the separator mask"""
    sm, out, c = _separator_mask(mask), bytearray(), c0
    for b in record:
        if ((sm if b == COMMA else mask) >> min(c, SAT)) & 1:
            out.append(b)
        c += b == COMMA
    return bytes(out)


def test_saturation():
    """records with 62, 63, 64, 65 and 130 separators under {bit 62}, {bit 63}, {bits 62, 63} and {bits 0, 63}: the rule with a count
    that saturates is the rule with true field numbers; then random records and masks"""
    c = SH.saturation()
    recs = [c["data"][o:o + n] for o, n in GM.records(c["data"])]
    assert sorted({r.count(b",") for r in recs}) == list(SH.SAT_COUNTS)
    for mask in SH.SAT_MASKS + [MAXU64, 1, bits(63, 64) | 1, MAXU64 & ~bits(64), MAXU64 & ~bits(63)]:
        for r in recs:
            assert _device_cut(r, mask) == CM.cut_record(r, COMMA, mask), (r[:20], hex(mask))
        assert len({CM.cut_record(r, COMMA, mask) for r in recs}) >= 3
    rng = np.random.RandomState(5)
    for _ in range(300):
        r = bytes(rng.choice(list(b",,ab"), size=int(rng.randint(0, 200))).astype(np.uint8))
        mask = int(rng.randint(0, 1 << 30)) << int(rng.randint(0, 35)) | int(rng.randint(2)) << 63 | int(rng.randint(2)) << 62
        if mask:
            assert _device_cut(r, mask) == CM.cut_record(r, COMMA, mask), (r, hex(mask))


def _leaf(b):
    """the separator carry of one position: (has a delimiter, separators in front of the first, separators behind the last)"""
    return (1, 0, 0) if b == NL else (0, 1, 1) if b == COMMA else (0, 0, 0)


def _combine(a, b):
    ha, fa, ba = a
    hb, fb, bb = b
    if not hb:
        back = min(ba + fb, SAT)
        return (1, fa, back) if ha else (0, back, back)
    if not ha:
        return (1, min(fa + fb, SAT), bb)
    return (1, fa, bb)


def _fold_random(rng, leaves):
    if len(leaves) == 1:
        return leaves[0]
    k = int(rng.randint(1, len(leaves)))
    return _combine(_fold_random(rng, leaves[:k]), _fold_random(rng, leaves[k:]))


def test_separator_carry_is_associative_and_the_models_field_number():
    rng = np.random.RandomState(9)
    for case in range(200):
        n = int(rng.randint(1, 400))
        heavy = case % 3 == 0                                                  # enough separators to saturate
        text = bytes(rng.choice(list(b",,,,,,a\n") if heavy else list(b",ab\n\n"), size=n).astype(np.uint8))
        if heavy:
            text = text.replace(b"\n", b",", n // 2)
        leaves = [_leaf(b) for b in text]
        left = leaves[0]
        for x in leaves[1:]:
            left = _combine(left, x)
        for _ in range(4):
            assert _fold_random(rng, leaves) == left, (case, text)
        # the model: separators in front of the first delimiter and behind the last, true counts
        first, last = text.find(b"\n"), text.rfind(b"\n")
        if first < 0:
            assert left == (0, min(text.count(b","), SAT), min(text.count(b","), SAT))
        else:
            assert left == (1, min(text[:first].count(b","), SAT), min(text[last + 1:].count(b","), SAT))
        # advance() over random runs: the count that reaches every run is the saturated true one, and the device's rule from there is
        # the model's for the rest of the record
        cuts = sorted(set(int(x) for x in rng.randint(1, n, size=int(rng.randint(0, 6))))) if n > 1 else []
        seps = 0
        for a, b in zip([0] + cuts, cuts + [n]):
            start = text.rfind(b"\n", 0, a) + 1
            assert seps == min(text[start:a].count(b","), SAT), (case, a)
            end = text.find(b"\n", a)
            end = n if end < 0 else end
            mask = int(rng.randint(1, 1 << 16)) | int(rng.randint(2)) << 63 | int(rng.randint(2)) << 62
            assert CM.cut_record(text[start:end], COMMA, mask).endswith(_device_cut(text[a:end], mask, seps)), (case, a, hex(mask))
            run = _fold_random(rng, leaves[a:b])
            seps = run[2] if run[0] else min(seps + run[1], SAT)


# ---- the inputs of the GPU tests reach their seams (conditions on the model, not measurements)
def test_shapes_reach_their_seams():
    assert SH.SEAMS == (64, 2048, 8192, 65536) and SH.FS == 1024
    for B in SH.SEAMS:
        for side in (0, 1):
            c = SH.seam_separator(B, side)
            P = c["P"]
            assert P == B - 1 + side and c["data"][P] == COMMA and c["big"] == (0, c["data"].index(b"\n")) and len(c["data"]) < 80 << 10
            assert _lines(SH.model(c, c["only_kept"])[3])[0] == b"," and _lines(SH.model(c, c["only_dropped"])[3])[0] == c["data"][:P] + c["data"][P + 1:c["big"][1]]
            c = SH.seam_field(B, side)
            P = c["P"]
            assert P == B - 1 + side and c["data"][P - 1] == COMMA and c["data"][P] == ord("F")
            assert _lines(SH.model(c, c["only_kept"])[3])[0] == b"F" and _lines(SH.model(c, c["only_dropped"])[3])[0] == c["data"][:P - 1] + c["data"][P + 1:c["big"][1]]
            for cc in (c, SH.seam_separator(B, side)):
                both = SH.model(cc, SH.ALL), SH.model(cc, SH.ALL, True)
                assert both[0][1] and both[1][1] and cc["big"] in both[0][1]
    for k in (1, 5, 63, 64):
        c = SH.three_tiles(k)
        o, n = c["big"]
        rec = c["data"][o:o + n]
        T = SH.TILE
        assert o < T and rec[:T - o].count(b",") == k and o + n > 2 * T
        mid = c["data"][T:2 * T]
        assert COMMA not in mid and NL not in mid and c["data"][2 * T:o + n].count(b",") == 3
        assert len({SH.model(c, m)[3] for m in c["masks"]}) == len(set(c["masks"])) >= 3
    for B in (SH.TILE, 3 * SH.FS):
        for field in (64, 65):
            c = SH.saturation_at(B, field)
            assert c["data"][B - 1] == COMMA and c["data"][:B].count(b",") == field - 1 and c["data"][B] == ord("G")
            assert _lines(SH.model(c, 1 << 63)[3])[0] == (b"G,H,I" if field == 64 else b"4,G,H,I") + SH.NEEDLE   # (field 64 of the second is the digit in front)
    c = SH.frame_size_4()
    sel = SH.model(c, bits(1))[1]
    assert c["fs"] == 4 and c["late"] in sel and c["dropped"] not in sel and c["after_dropped"] in sel and c["late"][1] > 20 and c["dropped"][1] > 20
    assert c["data"][c["late"][0]:sum(c["late"])].endswith(SH.NEEDLE) and not c["data"].endswith(b"\n")
    for kind, what in (("separators", {COMMA, NL}), ("delimiters", {NL})):
        assert set(SH.degenerate(kind)["data"]) == what
    assert COMMA not in SH.degenerate("no_separator")["data"] and NL not in SH.degenerate("single")["data"]
    assert b"\n\n\n" in SH.degenerate("empty_records")["data"]
    for f in (SH.table, SH.expressions, SH.saturation):
        assert len(f()["data"]) < 300 << 10


def test_random_sweep_meets_its_caps():
    """every input at most 1 MiB, at least 3 passes per call; in at least 90 % of the calls both modes pack something, and in at least
    half the packed size is strictly below the extract's for the same selection"""
    total = both = smaller = 0
    kinds = set()
    for seed in SH.SWEEP_SEEDS:
        c, calls = SH.sweep(seed)
        kinds.add(c["sep"])
        assert len(c["data"]) <= 1 << 20
        for mask, lo, hi, staging in calls:
            frames = (hi - 1) // c["fs"] - lo // c["fs"] + 1
            assert staging % c["fs"] == 0 and -(-frames // (staging // c["fs"])) >= 3
            a, b = SH.model(c, mask, False, lo, hi), SH.model(c, mask, True, lo, hi)
            total += 1
            both += bool(a[3].strip(b"\n")) and bool(b[3].strip(b"\n"))
            smaller += len(a[3]) < sum(n + 1 for _, n in a[1]) and len(b[3]) < sum(n + 1 for _, n in b[1])
    assert kinds == {COMMA, 0x20} and total >= 18
    assert both * 10 >= total * 9 and smaller * 2 >= total, (total, both, smaller)


# ---- the kernels
# per kernel: the LDS bound (a workgroup of the count, the keep or the copy may not take more than 65,536 bytes; so may neither of the
# two one-workgroup launches), and the VGPRs of the build rounded up to the allocation granule of 8 (DESIGN.md §33's table)
KERNELS = {"zra_cut_count_kernel": 64, "zra_cut_count_class_kernel": 64, "zra_cut_scan_kernel": 40, "zra_cut_keep_kernel": 72, "zra_cut_keep_class_kernel": 80,
           "zra_cut_place_kernel": 24, "zra_cut_copy_kernel": 40}


def test_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_cut_")) == sorted(KERNELS)
    for k, vgprs in KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_cut.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= 65536 and r["vgprs"] <= vgprs, (k, r)
