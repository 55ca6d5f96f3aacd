"""CPU tests of the boundary of the regex grep with context records (include/zra_hip.h: ZraHipGrepArchiveRegexContext,
ZraHipArchiveGrepRegexContext): declared, exported and bound, every rule-1 refusal before anything touches a device with the outputs
zeroed, no CPU result without a GPU, the three zra_grepxc_* kernels compiled without scratch, the summary algebra of
zra_amd/csrc/zra_regex_context.h under the host sanitizers (tools/model/regex_context_check.cpp), the model the GPU tests use as
their yardstick (tests/regex_context_model.py) against the system's `grep -E -b -A -B` (and `-v`) and against answers pinned by hand,
and the inputs of the GPU tests (tests/regex_context_shapes.py): each reaches the seam it is built for."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import grep_model as GM
import regex_context_model as RCM
import regex_context_shapes as SH
import regex_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipGrepArchiveRegexContext", "ZraHipArchiveGrepRegexContext"]
CHECKER = os.path.join(ROOT, "tools", "model", "regex_context_check.cpp")
MAXU64 = (1 << 64) - 1
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (64, 64)]                            # (after, before)
TILE = 8192


def test_regex_context_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert callable(zra.Engine.grep_regex_context) and callable(zra.Archive.grep_regex_context)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_regex_context_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42} from both entry points; the three counts are zeroed, with either extra pointer NULL, and the record array is
    left alone."""
    L = zra.load()
    P = ctypes.c_void_p
    ok = ctypes.create_string_buffer(b"ne+dle|^pin")
    deep = b"^.{70}$"                                                         # more than 64 states
    # (expressions, sizes, count, syntax, delimiter, mode, before, after)
    cases = [(ok, _sizes(11), 1, 0, 10, 0, 65, 0), (ok, _sizes(11), 1, 0, 10, 0, 0, 65), (ok, _sizes(11), 1, 0, 10, 1, 1 << 31, 2),             # the context
             (ok, _sizes(11), 1, 0, 10, 2, 1, 1), (ok, _sizes(11), 1, 0, 10, 3, 1, 1), (ok, _sizes(11), 1, 0, 10, 0x80000000, 0, 0),            # a foreign mode bit
             (ok, _sizes(11), 1, 2, 10, 0, 1, 1), (ok, _sizes(11), 1, 1 | 4, 10, 0, 1, 1),                                                      # a syntax bit other than FOLD_CASE
             (ok, _sizes(11), 0, 0, 10, 0, 1, 1), (ok, _sizes(6, 0), 2, 0, 10, 0, 1, 1),                                                        # reason 1
             (ctypes.create_string_buffer(b"a**"), _sizes(3), 1, 0, 10, 0, 1, 1), (ctypes.create_string_buffer(b"(ab"), _sizes(3), 1, 1, 10, 0, 1, 1),   # reason 2
             (ctypes.create_string_buffer(b"a\\nb"), _sizes(4), 1, 0, 10, 0, 1, 1), (ctypes.create_string_buffer(b"a[q]"), _sizes(4), 1, 0, ord("q"), 0, 1, 1),   # reason 3
             (ctypes.create_string_buffer(deep), _sizes(len(deep)), 1, 0, 10, 0, 1, 1),                                                          # reason 4
             (None, _sizes(11), 1, 0, 10, 0, 1, 1), (ok, None, 1, 0, 10, 0, 1, 1),                                                               # NULL pointers
             (ok, _sizes(11), 1, 0, 10, 0, 2, 3), (ok, _sizes(11), 1, 1, 10, 1, 64, 64)]                                                         # accepted arguments: no engine
    for why, exprs in ((1, []), (2, [b"a**"]), (2, [b"(ab"]), (3, [b"a\\nb"]), (4, [deep])):
        assert RM.check(exprs)["why"] == why, exprs                             # (the reasons are the model's too)
    assert RM.check([b"a[q]"], delim=ord("q"))["why"] == 3 and RM.check([b"ne+dle|^pin"])["ok"]
    for hp, hs, k, syntax, delim, mode, before, after in cases:
        for arc in ((None, 0), (P(64), 100)):
            for extra in ((True, True), (False, True), (True, False), (False, False)):
                arr = (ctypes.c_uint64 * 8)()
                ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                n, ns, ng = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
                tail = (arr, 4, ctypes.byref(n), ctypes.byref(ns) if extra[0] else None, ctypes.byref(ng) if extra[1] else None)
                tag = (k, syntax, delim, mode, before, after, arc, extra)
                assert L.ZraHipGrepArchiveRegexContext(None, *arc, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, *tail).tup() == (1, 42), tag
                assert (n.value, ns.value, ng.value) == (0, 0 if extra[0] else 0x1234, 0 if extra[1] else 0x1234) and bytes(arr) == b"\xEE" * 64, tag
                n.value = ns.value = ng.value = 0x1234
                assert L.ZraHipArchiveGrepRegexContext(None, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, *tail).tup() == (1, 42), tag
                assert (n.value, ns.value, ng.value) == (0, 0 if extra[0] else 0x1234, 0 if extra[1] else 0x1234) and bytes(arr) == b"\xEE" * 64, tag
            assert L.ZraHipGrepArchiveRegexContext(None, *arc, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, None, 0, None, None, None).tup() == (1, 42)


def test_regex_context_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_grep_regex_context.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep_regex_context(64, 100, [b"ne+dle", b"^pin"], before=1, after=1)   # no engine without a GPU: never a CPU result


def test_regex_context_kernel_rows():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_grep_regex_context.hip")).read()
    kernels = [k for k in res if k.startswith("zra_grepxc_")]
    assert sorted(kernels) == ["zra_grepxc_count_kernel", "zra_grepxc_fill_kernel", "zra_grepxc_scan_kernel"], kernels
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_grepxc_\w+)\s*\(", src)))
    for k in kernels:
        assert res[k]["source"] == "zra_grep_regex_context.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes"] <= (163840 if k == "zra_grepxc_scan_kernel" else 65536), (k, res[k])


# ---- the summary algebra under the host sanitizers
def test_summary_algebra_check_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "regex_context_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "zra_amd", "csrc"),
                    CHECKER, "-o", exe], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    m = re.fullmatch(r"regex_context_check: (\d+) cases ok", r.stdout.strip().split("\n")[-1])
    assert m and int(m.group(1)) >= 100000, r.stdout[-500:]
    # stand-alone: the new header and what it includes, and the kernels include the same header
    assert re.findall(r'#include\s+"([^"]+)"', open(CHECKER).read()) == ["zra_regex_context.h"]
    hdr = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_regex_context.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', hdr) == ["zra_context.h"]
    ctx = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_context.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', ctx) == [] and "hip" not in " ".join(re.findall(r"#include\s+<([^>]+)>", hdr + ctx))
    kernels = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_grep_regex_context.hip")).read()
    assert '#include "zra_regex_context.h"' in kernels
    for fn in ("zra_rxc::combine(", "zra_rxc::advance(", "zra_rxc::resolved_look("):
        assert fn in kernels, fn


# ---- the model
def _system_grep(tmp_path, data, exprs, invert, after, before):
    """([(offset, selected)], groups) as GNU grep prints them: `offset:` in front of a selected line, `offset-` in front of a context
    line, `--` between groups"""
    f = tmp_path / "lines.txt"
    f.write_bytes(data)
    args = ["grep", "-E", "-b", "-a", "-A", str(after), "-B", str(before)] + (["-v"] if invert else [])
    for p in exprs:
        args += ["-e", p.decode()]
    r = subprocess.run(args + [str(f)], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    out, groups = [], 0
    for line in r.stdout.split(b"\n")[:-1] if r.stdout else []:
        if line == b"--":
            groups += 1
            continue
        m = re.match(rb"(\d+)([:-])", line)
        assert m, line
        out.append((int(m.group(1)), m.group(2) == b":"))
    return out, groups + (1 if out else 0)


@pytest.mark.skipif(shutil.which("grep") is None, reason="no system grep")
def test_model_agrees_with_the_system_grep(tmp_path):
    """generated lines, some empty; expressions whose syntax the two share (no \\d \\w \\s \\xHH)"""
    rng = np.random.RandomState(52)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"eps", b"zeta", b"x", b"abc", b"acb"]
    exprs = [[b"ne+dle|^pin"], [b"a(b|c){2,3}$"], [b"^$"], [b"^.{0,3}$"], [b"ne+dle", b"^pin"], [b"^(x|eps)( (x|eps))*$|pin$"]]
    seen_groups = 0
    for case in range(12):
        density = [2, 8, 40, 200][case % 4]
        lines = []
        for _ in range(int(rng.randint(1, 400))):
            k = int(rng.randint(0, 5))                                         # (0: an empty line)
            w = [words[int(rng.randint(0, len(words)))] for _ in range(k)]
            if rng.randint(0, density) == 0:
                w.insert(int(rng.randint(0, k + 1)), (b"needle", b"neeedle", b"pin")[int(rng.randint(0, 3))])
            lines.append(b" ".join(w))
        data = b"\n".join(lines) + (b"\n" if case % 2 else b"")
        if data.endswith(b"\n\n") or data == b"\n":
            data += b"x"                                                       # (grep and the records agree on every text but one that ends in an empty line)
        ex = exprs[case % len(exprs)]
        for after, before in PAIRS:
            for invert in (False, True):
                listed, nsel, groups, recs, _ = RCM.context(data, ex, 10, invert, False, before, after)
                want, wgroups = _system_grep(tmp_path, data, ex, invert, after, before)
                assert [(o, s) for o, _, s in listed] == want, (case, ex, after, before, invert)
                assert groups == wgroups and nsel == sum(1 for _, s in want if s), (case, ex, after, before, invert, groups, wgroups)
                seen_groups += groups > 1
    assert seen_groups > 10


def test_regex_context_answers_pinned_by_hand():
    d = b"a\nb\nXv\nc\nd\ne\nuX\nf\ng"
    R = GM.records(d)
    assert [o for o, _ in R] == [0, 2, 4, 7, 9, 11, 13, 16, 18]
    T = lambda ks, sel: [(R[k][0], R[k][1], k in sel) for k in ks]
    ex = [b"^X|X$"]
    assert RCM.context(d, ex, before=0, after=0)[:3] == (T([2, 6], {2, 6}), 2, 2)
    assert RCM.context(d, ex, before=1, after=0)[:3] == (T([1, 2, 5, 6], {2, 6}), 2, 2)
    assert RCM.context(d, ex, before=1, after=2)[:3] == (T([1, 2, 3, 4, 5, 6, 7, 8], {2, 6}), 2, 1)      # a gap of 3 == after + before: one group
    assert RCM.context(d, ex, before=1, after=1)[:3] == (T([1, 2, 3, 5, 6, 7], {2, 6}), 2, 2)            # 3 > 2: two
    assert RCM.context(d, ex, before=64, after=64)[:3] == (T(range(9), {2, 6}), 2, 1)
    assert RCM.context(d, ex, invert=True, before=0, after=0)[:3] == (T([0, 1, 3, 4, 5, 7, 8], {0, 1, 3, 4, 5, 7, 8}), 7, 3)
    assert RCM.context(d, ex, before=3, after=3)[4] == 2 and RCM.context(d, [b"q"], before=3, after=3)[:3] == ([], 0, 0)
    # an anchor at a clipped range end: [5, 14) cuts `Xv` to `v` (no longer selected) and `uX` to `u`; [4, 15) keeps X$ out, [4, 16) has it
    assert RCM.context(d, ex, before=1, after=1, lo=5, hi=14)[:3] == ([], 0, 0)
    assert RCM.context(d, ex, before=1, after=1, lo=4, hi=14)[:3] == ([(4, 2, True), (7, 1, False)], 1, 1)
    assert RCM.context(d, [b"u$"], before=1, after=1, lo=9, hi=14)[:3] == ([(11, 1, False), (13, 1, True)], 1, 1)   # `uX` clipped to `u`: selected only by the clip
    assert RCM.context(d, [b"^v"], before=0, after=1, lo=5, hi=10)[:3] == ([(5, 1, True), (7, 1, False)], 1, 1)
    # ^$ on empty records, with context
    e = b"a\n\nb\nc\nd\n\n\ne"
    assert RCM.context(e, [b"^$"], before=0, after=1)[:3] == ([(2, 0, True), (3, 1, False), (9, 0, True), (10, 0, True), (11, 1, False)], 3, 2)
    assert RCM.context(e, [b"^$"], before=1, after=0)[:3] == ([(0, 1, False), (2, 0, True), (7, 1, False), (9, 0, True), (10, 0, True)], 3, 2)
    assert RCM.context(e, [b"^$"], before=2, after=1)[:3] == ([(o, n, n == 0) for o, n in GM.records(e)], 3, 1)
    assert RCM.context(e, [b"^$"], before=0, after=0, lo=1, hi=2)[:3] == ([(1, 0, True)], 1, 1)           # [1, 2) is the delimiter alone: one empty record


# ---- the inputs of the GPU tests reach their seams
def _tile(p):
    return p // TILE


def test_shape_frame_size_4():
    c, long_line = SH.frame_size_4()
    want, nsel, groups, recs, _ = SH.model(c, 2, 3, False)
    at = c["data"].find(long_line)
    assert len(long_line) == 60 and (at, 60, True) in want and c["fs"] == 4 and 900 < len(c["data"]) < 1200
    assert nsel > 5 and groups > 3 and len(want) > nsel + 10 and any(not b for _, _, b in want)
    before3 = [r for r in want if r[0] < at][-3:]
    assert len(before3) == 3 and not any(b for _, _, b in before3)               # its before-context waits through the passes that end no record
    assert all(any(ch in p for ch in b"^$+") for p in c["pats"])


def test_shape_one_record_per_pass():
    c = SH.one_record_per_pass()
    want, nsel, groups, recs, _ = SH.model(c, 0, 3, False)
    assert nsel == 6 and sum(1 for o, n, b in want if not b) == 3 + 3 + 3 + 2 + 3 + 3 and groups == 4
    sel = [c["data"][o:o + n] for o, n, b in want if b]
    assert any(s.startswith(b"X") for s in sel) and any(s.endswith(b"Xv") and s[0] != ord("X") for s in sel)     # both alternatives select
    assert all(n + 1 in (16, 8, 4, 48) for _, n in recs)


def test_shape_first_record_of_a_tile():
    c = SH.first_record_of_a_tile()
    data = c["data"]
    want, nsel, groups, recs, _ = SH.model(c, 2, 3, False)
    sel = {o + n: (o, n) for o, n, b in want if b}
    assert set(sel) == {t for t, _ in SH.SEAM_TARGETS} and nsel == len(SH.SEAM_TARGETS) == groups
    for t, kind in SH.SEAM_TARGETS:
        o, n = sel[t]
        seam = t - t % 64
        assert o < seam <= t and data.find(b"\n", seam, t) < 0                   # the record that the seam's first delimiter ends
        assert (data[o] == ord("Q") and t - seam <= 5) if kind == "start" else (data[seam - 1] == ord("Q") and t == seam), (t, kind)
        k = want.index((o, n, True))
        ctx_before, ctx_after = want[k - 3:k], want[k + 1:k + 3]
        assert all(not b and a + m < seam for a, m, b in ctx_before) and all(not b and a > seam for a, m, b in ctx_after), (t, kind)
    seams = {t - t % 64 for t, _ in SH.SEAM_TARGETS}
    assert sum(1 for s in seams if s % TILE == 0) >= 7 and any(s % TILE == 2048 for s in seams) and any(s % TILE == 64 for s in seams)
    assert sum(1 for s in seams if s % 2048 == 0) >= 9                          # with two frames of 1,024 to a pass: a pass's last byte


def test_shape_delimiter_free_tiles():
    c, (long1, long2, long3) = SH.delimiter_free_tiles()
    data = c["data"]
    want, nsel, groups, recs, _ = SH.model(c, 2, 2, False)
    a1, a2, a3 = data.find(long1), data.find(long2), data.find(long3)
    assert len(long1) == len(long2) == 20480 and (a1, 20480, False) in want and (a2, 20480, True) in want and (a3, 9000, False) in want and nsel == 4
    for a, n in ((a1, 20480), (a2, 20480)):
        assert _tile(a + n) - _tile(a) >= 2                                     # whole tiles without a delimiter: their maps compose
    assert (a3 + 9000) // 2048 - a3 // 2048 >= 4                                # whole passes of two frames without a delimiter
    k = want.index((a1, 20480, False))
    assert want[k - 2][2] and want[k + 2][2] and not want[k - 1][2] and not want[k + 1][2]   # context reaches across it in both directions
    k = want.index((a3, 9000, False))
    assert want[k + 1][2] and not want[k - 1][2]                                # pending, with the record in front of it, until the record behind is selected
    assert SH.model(c, 0, 1, False)[0].count((a1, 20480, False)) == 0 and (a3, 9000, False) in SH.model(c, 0, 1, False)[0]


@pytest.mark.parametrize("after,before", SH.GAP_PAIRS)
def test_shape_gaps(after, before):
    c = SH.gaps(after, before)
    want, nsel, groups, recs, _ = SH.model(c, after, before, False)
    g = after + before
    assert nsel == 8 and groups == 6 and len(want) == 8 + 8 * g
    sel = [o for o, n, b in want if b]
    assert _tile(sel[4]) == 0 and _tile(sel[5]) == 1 and _tile(sel[6]) == 1 and _tile(sel[7]) == 2    # the gaps of the second pair of blocks cross a tile's boundary
    idx = [k for k, r in enumerate(recs) if (r[0], r[1], True) in want]
    assert [idx[1] - idx[0] - 1, idx[3] - idx[2] - 1, idx[5] - idx[4] - 1, idx[7] - idx[6] - 1] == [g, g + 1, g, g + 1]


def test_shape_more_tiles_than_scan_lanes():
    c = SH.more_tiles_than_scan_lanes()
    data = c["data"]
    tiles = -(-len(data) // TILE)
    assert tiles == 1030 and c["fs"] == 65536
    want, nsel, groups, recs, _ = SH.model(c, 64, 64, False)
    assert nsel == 16 and 12 <= groups <= 16 and len(want) > 12 * 129 and any(n > 100000 and b for _, n, b in want)
    lanes = {_tile(o + n) // 2 for o, n, b in want if b}                        # a lane's run is two tiles
    assert len(lanes) <= 16 and tiles > 1024                                    # most lanes' runs hold no selected record
    assert len(SH.model(c, 1, 1, True)[0]) == len(recs)


def test_shape_random_small_shapes():
    cases = SH.random_small_shapes()
    assert len(cases) == 40 and all(200 <= len(c["data"]) <= 20000 for c in cases) and len(SH.RANDOM_EXPRESSIONS) == 8
    some = many = 0
    for c in cases:
        (after, before), inv = c["pairs"][0], c["modes"][0]
        want, nsel, groups, recs, _ = SH.model(c, after, before, inv)
        some += nsel > 0
        many += groups > 1
    assert some >= 30 and many >= 20, (some, many)
    assert len({c["pats"][0] for c in cases}) >= 6 and {c["fs"] for c in cases} == {64, 256, 1024} and any(c["hi"] is not None for c in cases)


def test_shape_text_and_clipped_ranges():
    t = SH.text()
    want, nsel, groups, recs, _ = SH.model(t, 1, 4, False)
    U = len(t["data"])
    assert U == 6 * 1024 + 300 and t["data"][-1] != 10 and want[-1][2] and want[-1][0] + want[-1][1] == U     # the record open at hi is the last listed one
    assert len(want) > 12 and groups > 2
    assert any(not want[k][2] and not want[k - 1][2] and not want[k + 1][2] and want[k + 2][2] for k in range(2, len(want) - 2))   # a capacity can cut inside a group
    c, ranges = SH.clipped_ranges()
    whole = {(o, n) for o, n, b in SH.model(c, 0, 0, False, 0, None)[0]}
    (a, b6) = ranges[0]
    got = SH.model(c, 2, 3, False, a, b6)[0]
    first, last = got[0], got[-1]
    assert first[0] == a and first[2] and not any(o <= a < o + n for o, n in whole)      # selected only because lo cuts it at `needle`
    assert last[0] + last[1] == b6 and last[2] and not any(o < b6 <= o + n for o, n in whole)
    assert not SH.model(c, 2, 3, False, ranges[2][0], ranges[2][1])[0][0][2] or SH.model(c, 2, 3, False, ranges[2][0], ranges[2][1])[0][0][0] != ranges[2][0]
    assert SH.model(c, 2, 3, False, 5, 5)[0] == []


def test_shape_degenerate():
    d = SH.degenerate()
    recs = GM.records(d["everything"]["data"])
    assert SH.model(d["everything"], 2, 3, False)[:3] == ([(o, n, True) for o, n in recs], len(recs), 1) and SH.model(d["everything"], 2, 3, True)[:3] == ([], 0, 0)
    assert SH.model(d["nothing"], 64, 64, False)[:3] == ([], 0, 0) and SH.model(d["nothing"], 64, 64, True)[1] == len(recs)
    want, nsel, groups, _, _ = SH.model(d["empties"], 1, 1, False)
    assert nsel > 70 and all(n == 0 for _, n, b in want if b) and any(not b for _, _, b in want) and groups > 3
    assert SH.model(d["delimiter_0"], 2, 3, False)[1] > 3 and 10 not in d["delimiter_0"]["data"]
    folded, plain = SH.model(d["fold_case"], 1, 2, False), RCM.context(d["fold_case"]["data"], d["fold_case"]["pats"], before=2, after=1)
    assert folded[1] > plain[1] >= 0 and folded[1] > 5
