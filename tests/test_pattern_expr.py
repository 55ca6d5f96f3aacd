"""CPU tests of the pattern expressions (include/zra_hip.h: ZraHipCheckPatternExpr and the six ...Expr scans): the host compiler
(zra_amd/csrc/zra_pattern_expr.h) walked by its stand-alone checker under the address and undefined-behaviour sanitizers; the model
the GPU tests use as their yardstick (tests/expr_model.py) against Python's `re` and against a naive per-position loop; the exported
checker against the checker program's table and against the model; every rule-1 refusal of the six calls before anything touches a
device; the constants; and the kernels' resources, the literal ones held at what they were before the class kernels came."""
import ctypes
import json
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import expr_model as XM
import grep_model as GM
import msearch_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tools", "model", "pattern_expr_check.cpp")
MAXU64 = (1 << 64) - 1
EXPR_CALLS = ["ZraHipSearchArchiveMultiExpr", "ZraHipGrepArchiveExpr", "ZraHipExtractRecordsExpr", "ZraHipArchiveSearchMultiExpr", "ZraHipArchiveGrepExpr",
              "ZraHipArchiveExtractRecordsExpr"]
CHECKER_CASES = 684


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the checker program, built as a stand-alone program with the host sanitizers"""
    exe = str(tmp_path_factory.mktemp("expr") / "pattern_expr_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "zra_amd", "csrc"),
                    CHECKER, "-o", exe], check=True, capture_output=True, timeout=600)
    return exe


def _table(checker):
    """the checker's single-expression cases: (syntax, delimiter or None, expression, [frozenset per element] or None)"""
    out = []
    for line in subprocess.run([checker, "--list"], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines():
        syntax, delim, hexed, want = line.split(" ", 3)
        sets = None
        if want != "refused":
            sets = []
            for el in want.split("|"):
                s = set()
                for item in el.split():
                    lo, _, hi = item.partition("-")
                    s |= set(range(int(lo, 16), int(hi or lo, 16) + 1))
                sets.append(frozenset(s))
        out.append((int(syntax), int(delim), bytes.fromhex(hexed), sets))
    return out


def test_checker_program_under_the_host_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().split("\n")[-1] == "pattern_expr_check: %d cases ok" % CHECKER_CASES, r.stdout[-500:]


def _check(zra, pats, syntax, delim):
    """ZraHipCheckPatternExpr through ctypes: (status, lengths, sets); the outputs are 0xEE-filled before the call"""
    L = zra.load()
    k = max(len(pats), 1)
    sizes = (ctypes.c_uint32 * k)(*(len(p) for p in pats))
    lens = (ctypes.c_uint32 * k)(*([0xEEEEEEEE] * k))
    ns = ctypes.c_uint32(0xEEEEEEEE)
    buf = ctypes.create_string_buffer(b"".join(pats), max(1, sum(len(p) for p in pats)))
    st = L.ZraHipCheckPatternExpr(buf, sizes, len(pats), syntax, delim, lens, ctypes.byref(ns)).tup()
    return st, list(lens)[:len(pats)], ns.value


def _model(pats, syntax, delim):
    """(lengths, sets, compiled) of the model, or None when it refuses"""
    try:
        c = XM.compile(pats, syntax, None if delim == -1 else delim)
    except XM.Refused:
        return None
    return XM.lengths(c), XM.n_sets(c), c


def test_exported_checker_and_model_on_the_checker_programs_table(zra, checker):
    table = _table(checker)
    assert len(table) > 180 and sum(1 for t in table if t[3] is None) > 70
    for syntax, delim, expr, want in table:
        st, lens, ns = _check(zra, [expr], syntax, delim)
        tag = (syntax, delim, expr)
        if not 0 <= syntax <= 3 or not -1 <= delim <= 255:
            assert want is None and st == (1, 42), tag                         # (outside the model's domain: the word, the delimiter's range)
            continue
        m = _model([expr], syntax, delim)
        if want is None:
            assert st == (1, 42) and lens == [0xEEEEEEEE] and ns == 0xEEEEEEEE and m is None, (tag, st, m)
        else:
            assert m is not None and m[2] == [want], (tag, m)
            assert (st, lens, ns) == ((0, 0), m[0], m[1]), (tag, st, lens, ns, m[:2])
    assert zra.check_pattern_expr([b"[0-9]x.", b"ab"]) == ([3, 2], 2)
    assert zra.check_pattern_expr([b"[0-9]x.", b"ab"], zra.PATTERN_CLASSES | zra.PATTERN_FOLD_CASE, delimiter=10) == ([3, 2], 2)
    assert zra.check_pattern_expr([b"a.b"], 0) == ([3], 0)
    for bad in ([b"a", b"b)"], [b"[\n]"]):
        with pytest.raises(zra.ZraError) as e:
            zra.check_pattern_expr(bad, delimiter=10)
        assert (e.value.zra, e.value.zstd) == (1, 42)
    L = zra.load()
    assert L.ZraHipCheckPatternExpr(b"a", (ctypes.c_uint32 * 1)(1), 1, 2, -1, None, None).tup() == (0, 0)     # both outputs are optional
    assert L.ZraHipCheckPatternExpr(None, (ctypes.c_uint32 * 1)(1), 1, 2, -1, None, None).tup() == (1, 42)
    assert L.ZraHipCheckPatternExpr(b"a", None, 1, 2, -1, None, None).tup() == (1, 42)


def _set_expr(k):
    return b"[\\x%02x\\x%02x]" % (0x80 + k, 0xC0 + k)


def test_limits_agree_between_the_exported_checker_and_the_model(zra):
    s32 = [_set_expr(k) for k in range(32)]
    cases = [([b"".join(s32)], 2), ([b"".join(s32) + _set_expr(32)], 2), (s32, 2), (s32 + [_set_expr(32)], 2), ([b"".join(s32) + b"[aA][b]x[Zz]\\x41"], 2),
             ([b"".join(s32) + b"abc"], 3), ([b"".join(s32) + b"[ab]"], 2), ([b"".join(s32) + b"[a-b]"], 3), ([b"[0-9]\\d", b"\\d.", b".[\\x00-\\xff]"], 2),
             ([b"a"] * 64, 2), ([b"a"] * 65, 2), ([b"a", b""], 2), ([], 2), ([b"." * 256], 2), ([b"." * 257], 2), ([b"a" * 256], 1), ([b"a" * 257], 1),
             ([b"." * 256] * 16, 2), ([b"." * 256] * 16 + [b"a"], 2), ([b"." * 256] * 16, 0), ([b"." * 256] * 16 + [b"a"], 0),
             ([b"\\x41" * 256] * 15 + [b"\\x41" * 253 + b"[\\x41a][abc]"], 2), ([b"\\x41" * 256] * 15 + [b"\\x41" * 253 + b"[\\x41a][\\x41]"], 2),
             ([b"a" * 16385], 2), ([b"a" * 4097], 0)]
    accepted = 0
    for pats, syntax in cases:
        for delim in (-1, 10):
            st, lens, ns = _check(zra, pats, syntax, delim)
            m = _model(pats, syntax, delim)
            tag = (syntax, delim, len(pats), pats[:1])
            if m is None:
                assert st == (1, 42), (tag, st)
            else:
                assert (st, lens, ns) == ((0, 0), m[0], m[1]), (tag, st, ns, m[1])
                accepted += 1
    assert accepted == 2 * 11 - 1, accepted                                    # (eleven acceptable lists; [\x00-\xff] holds the delimiter 10)
    assert sum(len(p) for p in cases[-4][0]) == 16384 and sum(len(p) for p in cases[-3][0]) == 16385
    assert _model(cases[0][0], 2, -1)[1] == 32 and _model(cases[4][0], 2, -1)[:2] == ([37], 32) and _model(cases[8][0], 2, -1)[1] == 2


# ---- random expressions: valid by construction (against `re`), and arbitrary bytes (the exported checker against the model)
ALPHABET = b"abAB01\n-]^ _"


def _lit(rng, in_set):
    c = int(rng.choice(list(ALPHABET)))
    if rng.randint(8) == 0:
        return b"\\x%02x" % c
    if c in b"]^-" or (not in_set and c in XM.RESERVED):
        return b"\\" + bytes([c])
    return bytes([c])


def _random_set(rng):
    out = b"[" + (b"^" if rng.randint(3) == 0 else b"")
    k = rng.randint(12)
    if k < 2:
        out += b"]"                                                            # ] directly behind [ or [^
    elif k < 4:
        out += b"-"                                                            # - first
    for _ in range(int(rng.randint(1, 4))):
        k = rng.randint(6)
        if k == 0:
            out += [b"\\d", b"\\w", b"\\s"][rng.randint(3)]
            if rng.randint(2):
                out += b"_"                                                    # (so that no - follows a class)
        elif k == 1:
            lo, hi = sorted(int(rng.choice(list(b"abAB01 _"))) for _ in range(2))
            out += bytes([lo]) + b"-" + bytes([hi])
        else:
            out += _lit(rng, True)
    if rng.randint(6) == 0 and not out.endswith((b"\\d", b"\\w", b"\\s")):
        out += b"-"                                                            # - last
    return out + b"]"


def _random_expr(rng):
    out = b""
    for _ in range(int(rng.randint(1, 5))):
        k = rng.randint(8)
        out += b"." if k == 0 else _random_set(rng) if k <= 2 else [b"\\d", b"\\w", b"\\s"][rng.randint(3)] if k == 3 else _lit(rng, False)
    return out


def test_model_agrees_with_re_and_with_a_naive_loop():
    rng = np.random.RandomState(24)
    every = bytes(range(256))
    nonempty = folded = dotted = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                        # (re's FutureWarning about [[ and -- in a set)
        for case in range(400):
            syntax = XM.CLASSES | (XM.FOLD_CASE if case & 1 else 0)
            pats = [_random_expr(rng) for _ in range(int(rng.randint(1, 4)))]
            data = bytes(rng.choice(list(ALPHABET), size=120).astype(np.uint8)) + every + bytes(rng.choice(list(ALPHABET), size=40).astype(np.uint8))
            lo = int(rng.randint(0, 60)) if case % 3 else 0
            hi = int(rng.randint(len(data) - 60, len(data) + 1)) if case % 3 else None
            end = len(data) if hi is None else hi
            comp = XM.compile(pats, syntax, None)
            got = XM.matches_multi(data, pats, syntax, lo, hi)
            want = []
            for i, e in enumerate(pats):
                rx = re.compile(b"(?=(" + e + b"))", re.DOTALL | (re.IGNORECASE if syntax & XM.FOLD_CASE else 0))
                for m in rx.finditer(data, lo, end):
                    assert len(m.group(1)) == len(comp[i])                     # every element matches exactly one byte
                    want.append((m.start(), i))
            assert got == sorted(want), (pats, syntax, lo, hi, got[:5], sorted(want)[:5])
            naive = sorted((p, i) for i, pat in enumerate(comp) for p in range(lo, end) if p + len(pat) <= end and all(data[p + q] in pat[q] for q in range(len(pat))))
            assert got == naive
            # the grep over sets: the delimiter leaves `.` and [^...]; a pattern that would hold it is refused
            try:
                recs, sel, matches = XM.grep(data, pats, syntax, 10, bool(case & 2), lo, hi)
            except XM.Refused:
                assert any(10 in s for pat in comp for s in pat)
            else:
                compd = XM.compile(pats, syntax, 10)
                assert all(a - {10} == b for pa, pb in zip(comp, compd) for a, b in zip(pa, pb))
                starts = {p for p, i in naive if all(data[p + q] != 10 for q in range(len(comp[i])))}
                assert matches == sum(1 for p, i in naive if all(data[p + q] != 10 for q in range(len(comp[i]))))
                assert recs == GM.records(data, 10, lo, hi)
                assert sel == [(o, n) for o, n in recs if any(o <= p < o + n for p in starts) != bool(case & 2)]
                assert XM.extract(data, pats, syntax, 10, bool(case & 2), lo, hi) == (recs, sel, matches, b"".join(data[o:o + n] + b"\n" for o, n in sel))
                dotted += any(10 in s for pat in comp for s in pat)
            nonempty += bool(got)
            folded += bool(syntax & 1) and got != XM.matches_multi(data, pats, XM.CLASSES, lo, hi)
    assert nonempty > 300 and folded > 60 and dotted > 60, (nonempty, folded, dotted)


def test_syntax_0_is_the_literal_models():
    rng = np.random.RandomState(25)
    data = bytes(rng.choice(list(b"ab.\n["), size=300).astype(np.uint8))
    pats = [b"a.", b"[", b"ab"]
    assert XM.matches_multi(data, pats, 0, 3, 290) == MM.matches_multi(data, pats, 3, 290) and XM.survivors(data, pats, 0) == MM.survivors(data, pats)
    assert XM.grep(data, pats, 0, 10, True, 3, 290) == GM.grep(data, pats, 10, True, 3, 290)
    # literal expressions (every special byte escaped) and FOLD_CASE alone agree with the literal models too
    esc = [b"a\\.", b"\\[", b"ab"]
    assert XM.matches_multi(data, esc, XM.CLASSES, 3, 290) == MM.matches_multi(data, pats, 3, 290)
    assert XM.survivors(data, esc, XM.CLASSES, 3, 290) == MM.survivors(data, pats, 3, 290)
    assert XM.grep(data, esc, XM.CLASSES, 10, False)[1:] == GM.grep(data, pats, 10, False)[1:]
    assert XM.matches_multi(data.upper(), pats, XM.FOLD_CASE) == MM.matches_multi(data, pats)


def test_arbitrary_bytes_get_the_models_verdict_from_the_exported_checker(zra):
    rng = np.random.RandomState(26)
    soup = list(b"[]^-\\.adxw0f:z\n*A")
    accepted = refused = 0
    for case in range(1500):
        pats = [bytes(rng.choice(soup, size=int(rng.randint(1, 9))).astype(np.uint8)) for _ in range(int(rng.randint(1, 3)))]
        syntax, delim = int(rng.randint(0, 4)), int(rng.choice([-1, 10, ord("a"), ord("A")]))
        st, lens, ns = _check(zra, pats, syntax, delim)
        m = _model(pats, syntax, delim)
        if m is None:
            assert st == (1, 42), (pats, syntax, delim)
            refused += 1
        else:
            assert (st, lens, ns) == ((0, 0), m[0], m[1]), (pats, syntax, delim, st, lens, ns, m[:2])
            accepted += 1
    assert accepted > 300 and refused > 300, (accepted, refused)


# ---- the six calls
def test_expr_calls_are_declared_exported_and_bound_and_the_constants_agree(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in EXPR_CALLS + ["ZraHipCheckPatternExpr"]:
        assert s in declared and s in zra.HIP_ABI_SYMBOLS and hasattr(L, s), s
    for name, value, py in (("FOLD_CASE", "1u", zra.PATTERN_FOLD_CASE), ("CLASSES", "2u", zra.PATTERN_CLASSES), ("MAX_SETS", "32u", zra.PATTERN_MAX_SETS),
                            ("MAX_EXPR_BYTES", "16384u", zra.PATTERN_MAX_EXPR_BYTES)):
        assert re.search(r"#define\s+ZRA_HIP_PATTERN_%s\s+%s" % (name, value), txt) and py == int(value[:-1]), name
    assert (XM.FOLD_CASE, XM.CLASSES, XM.MAX_SETS, XM.MAX_EXPR_BYTES) == (zra.PATTERN_FOLD_CASE, zra.PATTERN_CLASSES, zra.PATTERN_MAX_SETS, zra.PATTERN_MAX_EXPR_BYTES)
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_pattern_expr.h")).read()
    for name, value in (("kFoldCase = 1, kClasses = 2", ""), ("kMaxSets", "32"), ("kMaxExprBytes", "16384"), ("kMaxElements", "256"), ("kMaxElementsAll", "4096"),
                        ("kMaxPatterns", "64")):
        assert re.search(r"\b%s\b%s" % (re.escape(name), (r"\s*=\s*" + value + r"\b") if value else ""), src), name
    # the literal twins keep their signatures: one word more, behind nPatterns
    for twin in ("ZraHipSearchArchiveMulti", "ZraHipGrepArchive", "ZraHipExtractRecords", "ZraHipArchiveSearchMulti", "ZraHipArchiveGrep", "ZraHipArchiveExtractRecords"):
        a = re.search(r"ZRA_EXPORT ZraStatus %s\((.*?)\);" % twin, txt, re.S).group(1)
        b = re.search(r"ZRA_EXPORT ZraStatus %sExpr\((.*?)\);" % twin, txt, re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s.replace("struct ", "")).strip()
        assert norm(b) == norm(a).replace("size_t nPatterns,", "size_t nPatterns, uint32_t syntax,"), twin
    for cls in (zra.Engine, zra.Archive):
        for meth in ("search_multi", "grep", "extract"):
            assert "syntax" in getattr(cls, meth).__kwdefaults__ and getattr(cls, meth).__kwdefaults__["syntax"] == 0, (cls, meth)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_expr_calls_refuse_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; the count words are zeroed and the arrays are left alone, whatever the patterns and the syntax word are."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 20000)
    nl = ctypes.create_string_buffer(b"ab\ncd")
    ex = ctypes.create_string_buffer(b"[0-9]a)[z-a]\\")
    # (patterns, sizes, count, syntax, delimiter, mode)
    cases = [(pats, _sizes(3), 1, 0, 10, 0), (pats, _sizes(3), 1, 2, 10, 0), (pats, _sizes(3), 1, 3, 10, 1),                       # acceptable, but for the engine
             (pats, _sizes(3), 1, 4, 10, 0), (pats, _sizes(3), 1, 0x80000000, 10, 0), (pats, _sizes(3), 1, 7, 10, 0),               # syntax bits
             (pats, _sizes(3), 1, 2, 10, 2), (pats, _sizes(3), 1, 3, 10, 3), (pats, _sizes(3), 1, 1, 10, 0x80000000),               # mode bits
             (nl, _sizes(5), 1, 2, 10, 0), (nl, _sizes(2, 3), 2, 1, 10, 1), (pats, _sizes(3), 1, 3, 7, 0),                          # an element matches the delimiter
             (ex, _sizes(7), 1, 2, 10, 0), (ex, _sizes(5, 2, 5), 3, 2, 10, 0), (ex, _sizes(5, 8), 2, 3, 10, 0), (ex, _sizes(1), 1, 2, 10, 0),   # refused expressions
             (pats, _sizes(3, 0), 2, 2, 10, 0), (pats, _sizes(257), 1, 2, 10, 0), (pats, _sizes(257), 1, 1, 10, 0), (pats, _sizes(*([1] * 65)), 65, 3, 10, 0),
             (pats, _sizes(*([256] * 17)), 17, 2, 10, 0), (pats, _sizes(16385), 1, 2, 10, 0), (pats, _sizes(3), 0, 2, 10, 0), (None, _sizes(3), 1, 2, 10, 0),
             (pats, None, 1, 2, 10, 0)]
    for hp, hs, k, syntax, delim, mode in cases:
        tag = (k, syntax, delim, mode)
        for arc in ((None, 0), (P(64), 100), (None, 100)):
            arr = (ctypes.c_uint64 * 8)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            marr = ctypes.cast(arr, ctypes.POINTER(zra.ZraHipPatternMatch))
            per = (ctypes.c_uint64 * 65)(*([0xEE] * 65))
            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
            rn, rd = ctypes.byref(n), ctypes.byref(ds)
            assert L.ZraHipGrepArchiveExpr(None, *arc, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, arr, 4, rn).tup() == (1, 42), tag
            assert n.value == 0 and bytes(arr) == b"\xEE" * 64
            assert L.ZraHipGrepArchiveExpr(None, *arc, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, None, 0, None).tup() == (1, 42), tag
            n.value = 0x1234
            assert L.ZraHipExtractRecordsExpr(None, *arc, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, arr, 4, rn, P(4096), 64, rd).tup() == (1, 42), tag
            assert (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64
            assert L.ZraHipExtractRecordsExpr(None, *arc, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, None, 0, None, None, 0, None).tup() == (1, 42), tag
            n.value = 0x1234
            assert L.ZraHipSearchArchiveMultiExpr(None, *arc, hp, hs, k, syntax, 0, MAXU64, 0, marr, 4, rn, per).tup() == (1, 42), tag
            assert n.value == 0 and bytes(arr) == b"\xEE" * 64 and list(per) == [0xEE] * 65
            assert L.ZraHipSearchArchiveMultiExpr(None, *arc, hp, hs, k, syntax, 0, MAXU64, 0, None, 0, None, None).tup() == (1, 42), tag
        # through no handle
        arr = (ctypes.c_uint64 * 8)()
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        marr = ctypes.cast(arr, ctypes.POINTER(zra.ZraHipPatternMatch))
        n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
        assert L.ZraHipArchiveSearchMultiExpr(None, hp, hs, k, syntax, 0, MAXU64, 0, marr, 4, ctypes.byref(n), None).tup() == (1, 42) and n.value == 0, tag
        n.value = 0x1234
        assert L.ZraHipArchiveGrepExpr(None, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup() == (1, 42) and n.value == 0, tag
        n.value = 0x1234
        assert L.ZraHipArchiveExtractRecordsExpr(None, hp, hs, k, syntax, delim, mode, 0, MAXU64, 0, arr, 4, ctypes.byref(n), P(4096), 64, ctypes.byref(ds)).tup() == (1, 42), tag
        assert (n.value, ds.value) == (0, 0) and bytes(arr) == b"\xEE" * 64


def test_expr_scans_fail_loudly_without_gpu(zra):
    if zra.load().ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_pattern_expr.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep(64, 100, [b"[0-9]"], syntax=zra.PATTERN_CLASSES)    # no engine without a GPU: never a CPU result


# ---- the kernels
CLASS_KERNELS = {"zra_msearch_count_class_kernel": 32768, "zra_msearch_fill_class_kernel": 32768, "zra_grep_count_class_kernel": 32768,
                 "zra_grep_fill_class_kernel": 32768, "zra_extract_count_class_kernel": 65536, "zra_extract_copy_class_kernel": 65536}
# (VGPRs, SGPRs, LDS bytes) of the literal pattern kernels and the three scan kernels as the commit in front of the class kernels built them
LITERAL_KERNELS = {"zra_msearch_count_kernel": (53, 65, 22160), "zra_msearch_fill_kernel": (47, 83, 21888), "zra_grep_count_kernel": (51, 71, 21952),
                   "zra_grep_fill_kernel": (56, 83, 24000), "zra_extract_count_kernel": (68, 68, 22048), "zra_extract_copy_kernel": (87, 94, 24096),
                   "zra_search_scan_kernel": (14, 18, 8192), "zra_grep_scan_kernel": (20, 32, 20480), "zra_extract_scan_kernel": (34, 46, 40968)}


def test_class_kernels_fit_and_the_literal_kernels_did_not_move():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    for k, cap in CLASS_KERNELS.items():
        assert k in res, k
        r = res[k]
        assert r["source"] == k.split("_")[0] + "_" + k.split("_")[1] + ".hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds_bytes"] <= cap, (k, r)
    for k, (vgprs, sgprs, lds) in LITERAL_KERNELS.items():
        r = res[k]
        assert r["vgprs"] <= vgprs and r["sgprs"] <= sgprs and r["lds_bytes"] <= lds, (k, r, (vgprs, sgprs, lds))
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
