"""CPU tests of the regex grep (include/zra_hip.h: ZraHipCheckRegex, ZraHipGrepArchiveRegex, ZraHipArchiveGrepRegex): declared,
exported and bound; the model the GPU tests use as their yardstick (tests/regex_model.py) against Python's `re`; ZraHipCheckRegex
against the model on the checker program's table, on random expression lists and on lists of arbitrary bytes; the state limit at and
one beyond 64; rule 1 of the two calls before anything touches a device; the kernels' summary and its combine restated in Python,
associative and equal to the model; the host header's checker program under the host sanitizers; and the zra_grepx_* kernels
compiled inside their bounds."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import grep_model as GM
import regex_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipCheckRegex", "ZraHipGrepArchiveRegex", "ZraHipArchiveGrepRegex"]
CHECKER = os.path.join(ROOT, "tools", "model", "regex_check.cpp")
MAXU64 = (1 << 64) - 1
NL = 10


def test_regex_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_REGEX_MAX_STATES\s+64u\b", txt) and re.search(r"#define\s+ZRA_HIP_REGEX_MAX_POSITIONS\s+4096u\b", txt)
    assert re.search(r"typedef struct ZraHipRegexInfo \{ uint32_t states, classes, positions, why, pattern; \} ZraHipRegexInfo;", txt)
    assert zra.REGEX_MAX_STATES == 64 and zra.REGEX_MAX_POSITIONS == 4096 and callable(zra.check_regex)
    assert callable(zra.Engine.grep_regex) and callable(zra.Archive.grep_regex)


# ---- the model against Python's re
def _random_lists(seed, n):
    rng = np.random.RandomState(seed)
    return [[RM.random_expr(rng).encode() for _ in range(int(rng.randint(1, 4)))] for _ in range(n)]


def _records(rng, alphabet, n=24):
    out = [b""]
    for _ in range(n):
        out.append(bytes(rng.choice(list(alphabet), size=int(rng.randint(1, 9))).astype(np.uint8)))
    return out


def test_model_agrees_with_python_re_on_random_expressions():
    """Every list is held against `re` with BOL and EOL as two characters around the record: the header's definition word for word.
    The lists whose anchors are plain (never an anchor directly behind an anchor other than ^$: regex_model.anchors_are_plain) are
    also held against \\A and \\Z; there must be at least 400 of them."""
    rng = np.random.RandomState(2801)
    plain = anchored = matched = unmatched = 0
    for exprs in _random_lists(28, 700):
        fold = bool(rng.randint(0, 4) == 0)
        try:
            m = RM.Matcher(exprs, fold, NL)
        except RM.Refused as r:
            assert r.why == RM.WHY_STATES or r.why == RM.WHY_ARGUMENTS, (exprs, r.why)   # the generator writes no syntax error
            continue
        sym, is_plain = RM.re_symbols(m.asts), RM.anchors_are_plain(m.A)
        anc = RM.re_anchored(m.asts) if is_plain else None
        plain += is_plain
        anchored += any(b"^" in e or b"$" in e for e in exprs) and is_plain
        for rec in _records(rng, b"abcAB1 ."):
            got = m.A.matches(rec)
            want = sym.search(RM.SENTINEL_BOL + rec.decode("latin-1") + RM.SENTINEL_EOL) is not None
            assert got == want, (exprs, fold, rec, got, want)
            if anc is not None:
                assert got == (anc.search(rec) is not None), (exprs, fold, rec, got)
            matched += got
            unmatched += not got
    assert plain >= 400 and anchored >= 100 and matched > 1000 and unmatched > 1000, (plain, anchored, matched, unmatched)


def test_model_agrees_with_python_re_on_all_byte_values():
    rng = np.random.RandomState(2802)
    exprs_all = [[b"^[^a]+$"], [b"\\x00"], [b"\\xff+$"], [b"^.\\x80"], [b"[\\x7f-\\x81]{2}"], [b"^\\w+\\s\\d$"], [b"[^\\x00-\\x7f]"], [b"^(.[\\x00-\\x1f])*$"],
                 [b"\\.|\\\\|\\-"], [b"^[\\]\\[-]+$"], [b".{3}\\xfe"]]
    for delim in (NL, 0x20, 0xC3):
        data = bytearray(bytes(rng.permutation(256).astype(np.uint8)) + bytes(rng.randint(0, 256, size=600).astype(np.uint8)))
        for at in (40, 41, 100, 130, 300, 500, 503, 700):
            data[at] = delim
        data = bytes(data)
        recs = [data[o:o + n] for o, n in GM.records(data, delim)]
        assert len(recs) >= 8 and set(b"".join(recs)) == set(range(256)) - {delim}
        for exprs in exprs_all:
            m = RM.Matcher(exprs, False, delim)
            anc, sym = RM.re_anchored(m.asts), RM.re_symbols(m.asts)
            for rec in recs + [rec[:k] for rec in recs for k in (1, 2, 3)]:
                got = m.A.matches(rec)
                assert got == (anc.search(rec) is not None) == (sym.search(RM.SENTINEL_BOL + rec.decode("latin-1") + RM.SENTINEL_EOL) is not None), (exprs, delim, rec)


def test_model_answers_pinned_by_hand():
    d = b"GET /api/x\n\nPOST /x took 1234ms\nstatus=503 timeout\n\n\nGET /api"
    recs = GM.records(d)

    def sel(exprs, **kw):
        return [recs.index(r) for r in RM.grep_regex(d, exprs, **kw)[1]]

    assert sel([b"^(GET|POST) /api/"]) == [0]
    assert sel([b"took [0-9]{4,}ms$"]) == [2]
    assert sel([b"status=5[0-9]+ .*timeout"]) == [3]
    assert sel([b"^$"]) == [1, 4, 5]
    assert sel([b"^$"], invert=True) == [0, 2, 3, 6]
    assert sel([b"a*"]) == list(range(7))
    assert sel([b"a^b"]) == [] and sel([b"^^G"]) == []
    assert sel([b"get"], fold=True) == [0, 6] and sel([b"get"]) == []
    assert sel([b"ms$", b"^status"]) == [2, 3]
    # the range clips records, and the anchors hold at the clip
    assert RM.grep_regex(d, [b"^ET"], lo=1, hi=8)[1] == [(1, 7)] and RM.grep_regex(d, [b"/a$"], lo=1, hi=6)[1] == [(1, 5)]
    assert RM.grep_regex(d, [b"^$"], lo=11, hi=12)[1] == [(11, 0)] and RM.grep_regex(d, [b"^$"], lo=12, hi=12)[0] == []


# ---- ZraHipCheckRegex against the model
def _check(zra, exprs, fold=False, delim=NL):
    exprs = [bytes(e) for e in exprs]
    sizes = (ctypes.c_uint32 * max(len(exprs), 1))(*(len(e) for e in exprs))
    info = (ctypes.c_uint32 * 5)(*([0xEEEEEEEE] * 5))
    blob = b"".join(exprs)
    st = zra.load().ZraHipCheckRegex((ctypes.c_char * max(len(blob), 1)).from_buffer_copy(blob or b"\0"), sizes, len(exprs), 1 if fold else 0, delim, info).tup()
    states, classes, positions, why, pattern = (int(v) for v in info)
    assert st == ((0, 0) if why == 0 else (1, 42)), (exprs, st, why)
    return dict(ok=why == 0, why=why, pattern=pattern, states=states, classes=classes, positions=positions)


def test_check_regex_agrees_with_the_model_on_random_expressions(zra):
    accepted = 0
    rng = np.random.RandomState(2803)
    for exprs in _random_lists(29, 500):
        fold, delim = bool(rng.randint(0, 3) == 0), (NL, ord("a"), ord("b"), 0)[int(rng.randint(0, 4))]
        got, want = _check(zra, exprs, fold, delim), RM.check(exprs, fold, delim)
        assert got == want, (exprs, fold, delim, got, want)
        accepted += got["ok"]
    assert accepted >= 300, accepted


def test_check_regex_agrees_with_the_model_on_arbitrary_bytes(zra):
    """1,600 lists: uniformly random bytes, and bytes drawn from the characters of the grammar, where a list has a fair chance of
    being accepted"""
    rng = np.random.RandomState(2804)
    grammar = list(b"ab.[]^$*+?{}()|\\-,0123dwsnx:\n")
    why = [0] * 5
    for case in range(1600):
        src = grammar if case % 4 else list(range(256))
        exprs = [bytes(rng.choice(src, size=int(rng.randint(0 if case % 20 == 0 else 1, 9))).astype(np.uint8)) for _ in range(int(rng.randint(1, 4)))]
        fold, delim = bool(case & 1), (NL, ord("a"), 0x5D)[case % 3]
        got, want = _check(zra, exprs, fold, delim), RM.check(exprs, fold, delim)
        assert got == want, (exprs, fold, delim, got, want)
        why[got["why"]] += 1
    assert why[0] > 150 and why[1] > 5 and why[2] > 300 and why[3] > 20, why


def test_check_regex_state_limit_from_the_model(zra):
    """the largest n for which the model accepts ^.{n}$ has 64 states; one more is refused with reason 4"""
    n = max(k for k in range(50, 70) if RM.check([b"^.{%d}$" % k])["ok"])
    want = RM.check([b"^.{%d}$" % n])
    assert want["states"] == 64 and want["classes"] == 1 and want["positions"] == n + 2, want
    assert _check(zra, [b"^.{%d}$" % n]) == want
    assert _check(zra, [b"^.{%d}$" % (n + 1)]) == RM.check([b"^.{%d}$" % (n + 1)]) == dict(ok=False, why=4, pattern=0, states=0, classes=0, positions=0)
    assert zra.check_regex([b"^.{%d}$" % n]) == {k: want[k] for k in zra.REGEX_INFO}
    with pytest.raises(zra.ZraError) as e:
        zra.check_regex([b"^.{%d}$" % (n + 1)])
    assert (e.value.zra, e.value.zstd) == (1, 42) and e.value.info["why"] == 4
    with pytest.raises(zra.ZraError) as e:
        zra.check_regex([b"ok", b"a**"])
    assert e.value.info == dict(states=0, classes=0, positions=0, why=2, pattern=1)
    assert zra.check_regex([b"a"], fold_case=True, delimiter=0)["classes"] == 2
    # info may be NULL; the arguments
    L = zra.load()
    one = (ctypes.c_uint32 * 1)(1)
    assert L.ZraHipCheckRegex(b"a", one, 1, 0, NL, None).tup() == (0, 0) and L.ZraHipCheckRegex(b"*", one, 1, 0, NL, None).tup() == (1, 42)
    for args in ((None, one, 1, 0, NL), (b"a", None, 1, 0, NL), (b"a", one, 0, 0, NL), (b"a", one, 1, 2, NL), (b"a", one, 1, 4, NL), (b"a", one, 1, 3, NL),
                 (b"a", one, 1, 0, -1), (b"a", one, 1, 0, 256)):
        info = (ctypes.c_uint32 * 5)(*([0xEEEEEEEE] * 5))
        assert L.ZraHipCheckRegex(*args, info).tup() == (1, 42) and list(info) == [0, 0, 0, 1, 0], args


def test_regex_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords is zeroed and the record array is left alone: NULL pointers, mode bits, syntax bits 2 and 4, a
    refused expression, and, for want of an engine or an archive, the accepted ones."""
    L = zra.load()
    P = ctypes.c_void_p
    good = (ctypes.create_string_buffer(b"^a+$", 4), (ctypes.c_uint32 * 1)(4), 1)
    bad = (ctypes.create_string_buffer(b"a**b", 4), (ctypes.c_uint32 * 1)(4), 1)
    for pats, sizes, k in (good, bad, (None, good[1], 1), (good[0], None, 1), (good[0], good[1], 0), (good[0], good[1], 65)):
        for syntax in (0, 1, 2, 4):
            for mode in (0, 1, 2):
                for arc in ((None, 0), (P(64), 100), (None, 100)):
                    arr = (ctypes.c_uint64 * 8)()
                    ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                    n = ctypes.c_uint64(0x1234)
                    tag = (k, syntax, mode, arc)
                    assert L.ZraHipGrepArchiveRegex(None, *arc, pats, sizes, k, syntax, NL, mode, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), tag
                    assert n.value == 0 and bytes(arr) == b"\xEE" * 64, tag
                    assert L.ZraHipGrepArchiveRegex(None, *arc, pats, sizes, k, syntax, NL, mode, 0, MAXU64, 0, None, 4, None).tup() == (1, 42), tag
                n = ctypes.c_uint64(0x1234)
                assert L.ZraHipArchiveGrepRegex(None, pats, sizes, k, syntax, NL, mode, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42), tag
                assert n.value == 0 and bytes(arr) == b"\xEE" * 64, tag
                assert L.ZraHipArchiveGrepRegex(None, pats, sizes, k, syntax, NL, mode, 0, MAXU64, 0, None, 4, None).tup() == (1, 42), tag


def test_regex_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_grep_regex.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep_regex(64, 100, [b"^a+$"])                           # no engine without a GPU: never a CPU result


# ---- the kernels' summary (zra_grep_regex.hip: (summary) and its combine), restated over the model's DFA
def _leaf(pos, byte, delim, table):
    """the summary of one position: (has a delimiter, F, tail, last, sel)"""
    start, _, delta = table
    ident = tuple(range(len(delta)))
    return (1, ident, start, pos + 1, 0) if byte == delim else (0, tuple(delta[s][byte] for s in ident), 0, 0, 0)


def _combine(a, b, table, inv):
    _, accepting, _ = table
    ha, fa, ta, la, sa = a
    hb, fb, tb, lb, sb = b
    if not hb:
        return (1, fa, fb[ta], la, sa) if ha else (0, tuple(fb[s] for s in fa), 0, 0, 0)
    if not ha:
        return (1, tuple(fb[s] for s in fa), tb, lb, sb)
    return (1, fa, tb, lb, sa + sb + int((fb[ta] in accepting) != inv))


def _fold_random(rng, leaves, table, inv):
    if len(leaves) == 1:
        return leaves[0]
    k = int(rng.randint(1, len(leaves)))
    return _combine(_fold_random(rng, leaves[:k], table, inv), _fold_random(rng, leaves[k:], table, inv), table, inv)


def _finish(total, lo, hi, table, inv):
    """the selected count of the range from its summary, as the scan kernel's last lane does from {start = lo, the start state}"""
    start, accepting, _ = table
    has, F, tail, last, sel = total
    if not has:
        return int(lo < hi and (F[start] in accepting) != inv)
    return sel + int((F[start] in accepting) != inv) + int(last < hi and (tail in accepting) != inv)


def test_summary_algebra_is_associative_and_equals_the_model():
    rng = np.random.RandomState(2805)
    lists = [[b"^(..)*$"], [b"ab+c", b"^c"], [b"^$"], [b"a$"], [b"^[ab]*c"], [b"(a|b)c{2,3}$"]]
    tables = []
    for exprs in lists:
        asts, _ = RM.compile_list(exprs)
        tables.append((RM.dfa(RM.Automaton(asts), NL)[2], RM.Matcher(exprs)))
    for case in range(240):
        table, matcher = tables[case % len(tables)]
        n, lo, inv = int(rng.randint(1, 60)), int(rng.randint(0, 1000)), bool(case & 1)
        text = bytes(rng.choice(list(b"abc\n"), p=[(0.3, 0.3, 0.3, 0.1), (0.25, 0.25, 0.2, 0.3)][case % 2], size=n).astype(np.uint8))
        leaves = [_leaf(lo + j, text[j], NL, table) for j in range(n)]
        left = leaves[0]
        for leaf in leaves[1:]:
            left = _combine(left, leaf, table, inv)
        for _ in range(4):
            assert _fold_random(rng, leaves, table, inv) == left, (case, text)
        want = len(RM.grep_regex(text, None, NL, inv, matcher=matcher)[1])
        assert _finish(left, lo, lo + n, table, inv) == want, (case, text, left, want)


# ---- the host header under the sanitizers
def test_regex_check_program_under_the_host_sanitizers_and_its_table_against_the_model(zra, tmp_path):
    exe = str(tmp_path / "regex_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "zra_amd", "csrc"),
                    CHECKER, "-o", exe], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe, "--dump"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert re.fullmatch(r"regex_check: \d{3,} cases ok", lines[-1]), r.stdout[-500:]
    src = open(CHECKER).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["zra_regex.h"]
    hdr = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_regex.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', hdr) == ["zra_pattern_expr.h"] and "hip" not in " ".join(re.findall(r"#include\s+<([^>]+)>", hdr))
    # the checker's table: what the header answered there, what the library answers, what the model answers
    cases = [l.split(" ") for l in lines if l.startswith("case ")]
    assert len(cases) > 500
    seen = set()
    for _, fold, delim, hexes, ok, why, pattern, states, classes, positions in cases:
        exprs = [bytes.fromhex(h) for h in hexes.split(",")] if hexes else []
        got = dict(ok=ok == "1", why=int(why), pattern=int(pattern), states=int(states), classes=int(classes), positions=int(positions))
        if len(exprs) and sum(len(e) for e in exprs) < 20000:
            assert _check(zra, exprs, fold == "1", int(delim)) == got, exprs[:3]
        assert RM.check(exprs, fold == "1", int(delim)) == got, (exprs[:3], got)
        seen.add(got["why"])
    assert seen == {0, 1, 2, 3, 4}


# ---- the kernels
REGEX_KERNELS = {"zra_grepx_count_kernel": 65536, "zra_grepx_scan_kernel": 163840, "zra_grepx_fill_kernel": 65536}


def test_regex_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_grepx_")) == sorted(REGEX_KERNELS)
    for k, lds in REGEX_KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_grep_regex.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= lds, (k, r)
