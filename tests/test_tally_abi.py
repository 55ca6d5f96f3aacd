"""CPU tests of the tally (include/zra_hip.h: ZraHipTallyRecords, ZraHipTallyFields, ZraHipArchiveTallyFields, ZraHipGetTallyStats,
ZraHipDebugTallyMs, ZraHipDebugTallyHashBits): declared, exported and bound; every rule-1 refusal before anything touches a device;
no CPU result without a GPU; the model the GPU tests use as their yardstick (tests/tally_model.py) against answers pinned by hand,
against coreutils and against the cut's model composed with it; the inputs of the GPU tests (tests/tally_shapes.py) held to the seams
they are built for; and the zra_tally_* kernels compiled inside their bounds."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest

import cut_model as CM
import cut_shapes as CS
import tally_model as TM
import tally_shapes as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipTallyRecords", "ZraHipTallyFields", "ZraHipArchiveTallyFields", "ZraHipGetTallyStats", "ZraHipDebugTallyMs", "ZraHipDebugTallyHashBits"]
MAXU64 = (1 << 64) - 1
NL = 10
T, K = SH.T, SH.MAX_KEY


def test_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_TALLY_MAX_KEY\s+4096\b", txt) and zra.TALLY_MAX_KEY == TM.MAX_KEY == 4096
    assert re.search(r"#define\s+ZRA_HIP_TALLY_HASH_NONE\s+0xFFFFFFFFu", txt) and zra.TALLY_HASH_NONE == 0xFFFFFFFF
    assert "zra_tally.hip" in open(os.path.join(ROOT, "zra_amd", "build.py")).read()
    p = inspect.signature(zra.Engine.tally_text).parameters
    assert all(k in p for k in ("delimiter", "max_distinct", "d_keys", "key_cap", "max_entries")), p
    for f in (zra.Engine.tally, zra.Archive.tally):
        p = inspect.signature(f).parameters
        assert all(k in p for k in ("separator", "fields", "delimiter", "invert", "offset", "length", "staging_bytes", "syntax", "max_distinct", "d_keys", "key_cap",
                                    "max_entries")), p
    assert callable(zra.Engine.tally_stats) and len(zra.TALLY_STATS) == 7
    # no earlier call's row moves: the tally's is the last one
    eng = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_engine.h")).read()
    assert re.search(r"kCallRead, kCallVerify, kCallTally, kCalls \}", eng)


# ---- rule 1
def test_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42} and zeroed words; the entry array is left alone and neither dText nor dKeys is touched (they are not even
    memory here): for want of an engine every call, the accepted ones included; every null combination of the words"""
    L = zra.load()
    P = ctypes.c_void_p
    arr = (ctypes.c_uint64 * 9)()
    sizes = (ctypes.c_uint32 * 2)(3, 1)
    for text in ((None, 0), (P(4096), 100), (None, 100)):
        for ent in ((None, 0), (arr, 2), (None, 2)):
            for keys in ((None, 0), (P(8192), 64), (None, 64), (P(4100), 64)):
                for missing in (None, 0, 1, 2, 3):
                    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                    w = [ctypes.c_uint64(0x1234 + i) for i in range(5)]
                    refs = [None if i == missing else ctypes.byref(w[i]) for i in range(4)]
                    tag = (text, ent[1], keys, missing)
                    assert L.ZraHipTallyRecords(None, *text, NL, 0, *ent, *keys, *refs).tup() == (1, 42), tag
                    assert all(w[i].value == 0 for i in range(4) if i != missing) and bytes(arr) == b"\xEE" * 72, tag
                    for x in w:
                        x.value = 0x1234
                    st = L.ZraHipTallyFields(None, P(64), 100, b"abcd", sizes, 2, 0, NL, 0, 0x2C, 5, 0, MAXU64, 0, text[0], text[1], ctypes.byref(w[4]), 0, *ent, *keys,
                                             *refs).tup()
                    assert st == (1, 42) and all(w[i].value == 0 for i in range(5) if i != missing) and bytes(arr) == b"\xEE" * 72, tag
                    for x in w:
                        x.value = 0x1234
                    st = L.ZraHipArchiveTallyFields(None, None, None, 0, 0, NL, 0, 0x2C, 5, 0, MAXU64, 0, text[0], text[1], ctypes.byref(w[4]), 0, *ent, *keys, *refs).tup()
                    assert st == (1, 42) and all(w[i].value == 0 for i in range(5) if i != missing) and bytes(arr) == b"\xEE" * 72, tag
    assert L.ZraHipTallyFields(None, None, 0, None, None, 0, 0, NL, 0, 0x2C, 1, 0, MAXU64, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, None).tup() == (1, 42)
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetTallyStats(None, out)
    assert list(out) == [0] * 8 and L.ZraHipDebugTallyMs(None) == 0.0
    L.ZraHipGetTallyStats(None, None)
    L.ZraHipDebugTallyHashBits(None, 2)


def test_fails_loudly_without_gpu(zra):
    """no engine, no result: never a CPU answer"""
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_tally.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).tally_text(4096, 100)
    with pytest.raises(zra.ZraError):
        zra.Engine(0).tally(64, 100, [b"abc"], 0, 0, separator=0x2C, fields="1,3")


# ---- the model
PROBE = b"200\n404\n200\n\n500\n200\n\n404"


def test_answers_pinned_by_hand():
    assert TM.records(PROBE) == [(0, 3), (4, 3), (8, 3), (12, 0), (13, 3), (17, 3), (21, 0), (22, 3)]
    assert TM.tally(PROBE) == (8, 0, [(0, 3, 3), (4, 3, 2), (12, 0, 2), (13, 3, 1)], b"200\n404\n\n500\n")
    assert TM.tally(PROBE + b"\n") == (8, 0, [(0, 3, 3), (4, 3, 2), (12, 0, 2), (13, 3, 1)], b"200\n404\n\n500\n")
    assert TM.tally(PROBE + b"\n\n")[:3] == (9, 0, [(0, 3, 3), (4, 3, 2), (12, 0, 3), (13, 3, 1)])
    assert TM.tally(b"") == (0, 0, [], b"") and TM.tally(b"\n") == (1, 0, [(0, 0, 1)], b"\n") and TM.tally(b"x") == (1, 0, [(0, 1, 1)], b"x\n")
    assert TM.tally(b"a;b;a", 0x3B) == (3, 0, [(0, 1, 2), (2, 1, 1)], b"a;b;")
    long, cap = b"L" * (K + 1), b"C" * K
    assert TM.tally(long + b"\n" + cap + b"\n" + long + b"\nx\n" + cap) == (5, 2, [(K + 2, K, 2), (3 * K + 5, 1, 1)], cap + b"\nx\n")
    assert TM.tally(b"ab\nabc\nab", max_key=2) == (3, 1, [(0, 2, 2)], b"ab\n")
    assert TM.lines(PROBE, TM.tally(PROBE)[2]) == b"3 200\n2 404\n2 \n1 500\n"
    assert [TM.slots(n) for n in (0, 1, 43, 44, 128, 129, 50000)] == [64, 128, 128, 256, 256, 512, 131072] and TM.slots(50000, 199) == 512 and TM.slots(100, 5000) == 256


def test_model_against_coreutils():
    """`sort | uniq -c` as a multiset of (count, key); `awk '!seen[$0]++'` for the order of the keys"""
    if not (shutil.which("sort") and shutil.which("uniq")):
        pytest.skip("no coreutils")
    env = dict(os.environ, LC_ALL="C")
    for text in (PROBE + b"\n", CS.log_lines(3, 20000).rsplit(b"\n", 1)[0] + b"\n", SH.collisions()["text"] + b"\n", SH.skew("three")["text"]):
        n, skipped, entries, keys = TM.tally(text)
        out = subprocess.run("sort | uniq -c", shell=True, input=text, capture_output=True, env=env, timeout=60).stdout
        want = sorted((int(ln.split(None, 1)[0]), ln.lstrip().split(b" ", 1)[1] if b" " in ln.lstrip() else b"") for ln in out.split(b"\n")[:-1])
        assert sorted((c, text[o:o + m]) for o, m, c in entries) == want and skipped == 0
        if shutil.which("awk"):
            assert subprocess.run(["awk", "!seen[$0]++"], input=text, capture_output=True, env=env, timeout=60).stdout == keys


def test_composite_is_the_cut_model_then_the_tally():
    data = CS.log_lines(33, 30000)
    for pats, inv, mask in (([b"ERROR"], False, CS.bits(3)), ([], False, CS.bits(3, 4)), ([b"failed"], True, CS.bits(4)), ([b"ms"], False, CS.ALL)):
        packed, got = TM.tally_fields(data, pats, 0x20, mask, NL, inv)
        recs, sel, nm, again = CM.cut(data, pats, 0x20, mask, NL, inv)
        assert packed == again and got == TM.tally(again) and got[0] == len(sel) and sum(e[2] for e in got[2]) == len(sel) - got[1]
        if mask == CS.ALL:                                                     # whole selected records
            assert packed == b"".join(data[o:o + n] + b"\n" for o, n in sel)
    levels = TM.tally_fields(data, [], 0x20, CS.bits(3))[1]
    assert sorted(levels[3].split(b"\n")[:-1]) == [b"DEBUG", b"ERROR", b"INFO", b"WARN"]


# ---- the shapes
def test_shapes_reach_their_seams():
    d = {k: SH.degenerate(k)["text"] for k in SH.DEGENERATE}
    assert d["one_with"][-1] == NL and NL not in d["one_without"] and set(d["delimiters"]) == {NL} and len(d["one_byte"]) == 1 and d["one_delimiter"] == b"\n"
    assert len(d["tile"]) == T and d["tile"][-1] == NL and len(d["tile_plus_1"]) == T + 1 and d["tile_plus_1"][T - 1] == NL
    for kind in SH.SEAMS:
        c = SH.seam(kind)
        text, (o, n) = c["text"], c["big"]
        recs = TM.records(text)
        assert (o, n) in recs, kind
        if kind == "straddle":
            assert o < T - 1 and o + n > T + 1 and recs.count((o, n)) == 1 and text.count(text[o:o + n]) == 2
        if kind == "bare_tile":
            assert o < T and o + n > 2 * T and n > K and not any(T <= r[0] < 2 * T for r in recs) and any(r[0] >= 2 * T for r in recs)
        if kind == "delimiter_last":
            assert text[T - 1] == NL and o == T
        if kind == "delimiter_first":
            assert text[T] == NL and o + n == T and (T + 1, 4) in recs
        if kind == "mirror":
            assert o < T and [r // T for r in c["repeats"]] == [1, 2, 3] and all((r, n) in recs and text[r:r + n] == text[o:o + n] for r in c["repeats"])
            assert c["repeats"][1] + n + 1 == 3 * T                            # the repeat's delimiter is the last byte of tile 2
            assert dict((e[0], e[2]) for e in TM.tally(text)[2])[o] == 4
    k = {kind: SH.key_length(kind) for kind in SH.KEY_LENGTHS}
    assert sorted(set(len(r) for r in k["sizes"]["recs"])) == [5, K - 1, K, K + 1] and TM.tally(k["sizes"]["text"])[:2] == (7, 2)
    a, b, _ = k["last_byte"]["recs"]
    assert len(a) == len(b) == K and a[:-1] == b[:-1] and a[-1] != b[-1]
    a, b, _ = k["first_byte"]["recs"]
    assert len(a) == len(b) == K and a[1:] == b[1:] and a[0] != b[0]
    assert b"abcd".startswith(b"abc") and {b"", b"ab", b"abc", b"abcd", b"abcde"} == set(k["prefix"]["recs"])
    one, three, distinct = (TM.tally(SH.skew(kind)["text"]) for kind in SH.SKEWS)
    assert one[0] == three[0] == distinct[0] == 50000 and len(one[2]) == 1 and len(distinct[2]) == 50000
    shares = [e[2] / 50000 for e in three[2]]
    assert len(shares) == 3 and abs(shares[0] - 0.98) < 0.005 and abs(shares[1] - 0.019) < 0.004 and 0 < shares[2] < 0.003
    assert len(SH.skew("one")["text"]) > 16 * T                               # more than one workgroup, many times
    c = SH.collisions()
    n, skipped, entries, keys = TM.tally(c["text"])
    assert len(entries) == 300 and skipped == 0 and set(e[2] for e in entries) == {1, 2, 3, 4, 5} and c["text"][-1] != NL
    assert min(e[1] for e in entries) == 1 and max(e[1] for e in entries) >= 500 and len(c["text"]) > 16 * T
    assert SH.collisions()["text"] == c["text"]                                # a seeded generator
    p = SH.promised()
    assert len(TM.tally(p["text"])[2]) == p["D"] == 200 and len(p["text"]) > T


# ---- the kernels
# per kernel: the VGPRs of the build rounded up to the allocation granule of 8 (DESIGN.md §34's table); no workgroup may take more than
# 65,536 bytes of LDS
KERNELS = {"zra_tally_count_kernel": 40, "zra_tally_insert_kernel": 56, "zra_tally_mark_kernel": 16, "zra_tally_sum_kernel": 16, "zra_tally_scan_kernel": 32,
           "zra_tally_emit_kernel": 24, "zra_tally_copy_kernel": 32}


def test_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_tally_")) == sorted(KERNELS)
    for k, vgprs in KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_tally.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= 65536 and r["vgprs"] <= vgprs, (k, r)
