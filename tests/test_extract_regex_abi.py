"""CPU tests of the regex extract (include/zra_hip.h: ZraHipExtractRecordsRegex, ZraHipArchiveExtractRecordsRegex): declared,
exported and bound with the extract's argument order; the zeroing of the outputs in front of the engine; the kernels' summary with
its two added fields (zra_extract_regex.hip: (summary)) restated in Python over the model's DFA, associative and equal to the model; the model itself against pinned answers; and the zra_extractx_* kernels
compiled inside their bounds."""
import ctypes
import inspect
import json
import os
import re

import numpy as np

import extract_regex_model as XRM
import regex_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipExtractRecordsRegex", "ZraHipArchiveExtractRecordsRegex"]
MAXU64 = (1 << 64) - 1
NL = 10


def test_regex_extract_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    # the C arguments are ZraHipExtractRecordsExpr's, one for one
    assert L.ZraHipExtractRecordsRegex.argtypes == L.ZraHipExtractRecordsExpr.argtypes and len(L.ZraHipExtractRecordsRegex.argtypes) == 18
    assert L.ZraHipArchiveExtractRecordsRegex.argtypes == L.ZraHipArchiveExtractRecordsExpr.argtypes and len(L.ZraHipArchiveExtractRecordsRegex.argtypes) == 16
    decl = re.search(r"ZRA_EXPORT ZraStatus ZraHipExtractRecordsRegex\(([^;]*)\);", txt).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", decl) == ["engine", "dArchive", "archiveSize", "hPatterns", "hPatternSizes", "nPatterns", "syntax", "delimiter", "mode", "offset",
                                                    "size", "stagingBytes", "hRecords", "recordCapacity", "nRecords", "dData", "dataCapacity", "dataSize"]
    # the Python bindings
    keywords = ["delimiter", "invert", "fold_case", "offset", "length", "staging_bytes", "max_records"]
    for fn, positional in ((zra.Engine.extract_regex, ["self", "d_archive", "size", "patterns", "d_data", "data_cap"]),
                           (zra.Archive.extract_regex, ["self", "patterns", "d_data", "data_cap"])):
        p = inspect.signature(fn).parameters
        assert list(p) == positional + keywords, list(p)
        assert all(p[k].kind == inspect.Parameter.KEYWORD_ONLY for k in keywords)
        assert (p["delimiter"].default, p["invert"].default, p["fold_case"].default, p["offset"].default, p["length"].default, p["staging_bytes"].default,
                p["max_records"].default) == (0x0A, False, False, 0, None, 0, 0)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_regex_extract_without_an_engine_refuses_and_zeroes_its_outputs(zra):
    """What the entry points do in front of the engine: {ZStdError, 42}, *nRecords and *dataSize zeroed when they are there, the
    record array and dData left alone, for every shape of arguments a caller can send wrong, each ZraHipCheckRegex reason among them.
    With no engine EVERY call is refused, the valid one included, so this test cannot tell which rule refused: that rules 1 and 2
    themselves refuse, and only what they should, is held with an engine in tests/test_gpu_extract_regex.py (cases 6 and 8)."""
    L = zra.load()
    P = ctypes.c_void_p
    good = (ctypes.create_string_buffer(b"^a+$", 4), _sizes(4), 1)
    refusals = {1: [b"a"] * 65, 2: [b"ok", b"a**"], 3: [b"\\n"], 4: [b"^.{63}$"]}     # each reason of ZraHipCheckRegex once
    cases = []                                                                 # (patterns, sizes, count, syntax, mode)
    for why, exprs in refusals.items():
        assert RM.check(exprs)["why"] == why, (why, exprs)
        blob = b"".join(exprs)
        cases.append((ctypes.create_string_buffer(blob, len(blob)), _sizes(*(len(e) for e in exprs)), len(exprs), 0, 0))
    cases += [good + (2, 0), good + (4, 0), good + (3, 1), good + (0, 2), good + (1, 3), (None, good[1], 1, 0, 0), (good[0], None, 1, 0, 0), (good[0], good[1], 0, 0, 0)]
    ok = good + (0, 0)
    for hp, hs, k, syntax, mode in cases + [ok, good + (1, 1)]:
        for arc in ((None, 0), (P(64), 100), (None, 100)):
            arr = (ctypes.c_uint64 * 8)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
            nn, dd = ctypes.byref(n), ctypes.byref(ds)
            # (hRecords, recordCapacity, nRecords, dData, dataCapacity, dataSize): whole, no nRecords, NULL dataSize, NULL hRecords with a
            # capacity, NULL dData with a capacity, nothing at all, and rule 2: dData inside the archive
            outs = [(arr, 4, nn, P(4096), 64, dd), (None, 0, None, P(4096), 64, dd), (arr, 4, nn, P(4096), 64, None), (None, 4, nn, P(4096), 64, dd),
                    (arr, 4, nn, None, 64, dd), (None, 0, None, None, 0, None), (arr, 4, nn, P(100), 64, dd)]
            for out in outs:
                n.value, ds.value = 0x1234, 0x5678
                tag = (k, syntax, mode, arc, out[1], out[4])
                assert L.ZraHipExtractRecordsRegex(None, *arc, hp, hs, k, syntax, NL, mode, 0, MAXU64, 0, *out).tup() == (1, 42), tag
                assert n.value == (0 if out[2] is not None else 0x1234) and ds.value == (0 if out[5] is not None else 0x5678), tag
                assert bytes(arr) == b"\xEE" * 64, tag
                n.value, ds.value = 0x1234, 0x5678
                assert L.ZraHipArchiveExtractRecordsRegex(None, hp, hs, k, syntax, NL, mode, 0, MAXU64, 0, *out).tup() == (1, 42), tag
                assert n.value == (0 if out[2] is not None else 0x1234) and ds.value == (0 if out[5] is not None else 0x5678), tag
                assert bytes(arr) == b"\xEE" * 64, tag


def test_model_answers_pinned_by_hand():
    d = b"GET /api/x\n\nPOST /x took 1234ms\nstatus=503 timeout\n\n\nGET /api"
    assert XRM.extract_regex(d, [b"^(GET|POST) /api/"])[3] == b"GET /api/x\n"
    assert XRM.extract_regex(d, [b"^$"])[3] == b"\n\n\n" and XRM.extract_regex(d, [b"^$"])[2] == 3
    assert XRM.extract_regex(d, [b"^$"], invert=True)[3] == b"GET /api/x\nPOST /x took 1234ms\nstatus=503 timeout\nGET /api\n"
    assert XRM.extract_regex(d, [b"get"], fold=True)[3] == b"GET /api/x\nGET /api\n" and XRM.extract_regex(d, [b"get"])[3] == b""
    assert XRM.extract_regex(d, [b"^ET"], lo=1, hi=8)[1:] == ([(1, 7)], 1, b"ET /api\n")
    assert XRM.extract_regex(d, [b"ms$", b"^status"])[1] == [(12, 19), (32, 18)] and XRM.starts([(12, 19), (32, 18)]) == [0, 20]
    assert XRM.extract_regex(b"", [b"a*"])[3] == b"" and XRM.extract_regex(b"\n", [b"a*"])[3] == b"\n"


# ---- the kernels' summary (zra_extract_regex.hip: (summary), combine and the front's advance), restated over the model's DFA.
# A summary is (has a delimiter, F, tail, last, sel, first, bytes).
def _piece(pos, chunk, delim, table, inv):
    """the summary of the positions [pos, pos + len(chunk)) from its definition, without combine"""
    start, accepting, delta = table
    ident = tuple(range(len(delta)))

    def run(state, bs):
        for b in bs:
            state = delta[state][b]
        return state

    at = [j for j, b in enumerate(chunk) if b == delim]
    if not at:
        return (0, tuple(run(s, chunk) for s in ident), 0, 0, 0, 0, 0)
    sel = nbytes = 0
    for a, b in zip(at, at[1:]):                                               # the records between two delimiters of the piece
        if (run(start, chunk[a + 1:b]) in accepting) != inv:
            sel += 1
            nbytes += b - a
    return (1, tuple(run(s, chunk[:at[0]]) for s in ident), run(start, chunk[at[-1] + 1:]), pos + at[-1] + 1, sel, pos + at[0], nbytes)


def _combine(a, b, table, inv):
    _, accepting, _ = table
    ha, fa, ta, la, sa, ia, ba = a
    hb, fb, tb, lb, sb, ib, bb = b
    if not hb:
        return (1, fa, fb[ta], la, sa, ia, ba) if ha else (0, tuple(fb[s] for s in fa), 0, 0, 0, 0, 0)
    if not ha:
        return (1, tuple(fb[s] for s in fa), tb, lb, sb, ib, bb)
    s = int((fb[ta] in accepting) != inv)
    return (1, fa, tb, lb, sa + sb + s, ia, ba + bb + s * (ib - la + 1))


def _fold_random(rng, pieces, table, inv):
    if len(pieces) == 1:
        return pieces[0]
    k = int(rng.randint(1, len(pieces)))
    return _combine(_fold_random(rng, pieces[:k], table, inv), _fold_random(rng, pieces[k:], table, inv), table, inv)


def _finish(total, lo, hi, table, inv):
    """(selected records, packed bytes) of the range from its summary, as the scan kernel's last lane does: the front
    {start = lo, the start state, 0, 0} moved over the summary, then the record that hi ends"""
    start, accepting, _ = table
    has, F, tail, last, sel, first, nbytes = total
    if not has:
        s = int(lo < hi and (F[start] in accepting) != inv)
        return s, s * (hi - lo + 1)
    s = int((F[start] in accepting) != inv)
    t = int(last < hi and (tail in accepting) != inv)
    return sel + s + t, nbytes + s * (first - lo + 1) + t * (hi - last + 1)


P_DELIM = 0.08            # a piece of 1 .. 8 bytes is delimiter-free with probability 0.7 or so, and so are two in a row in most streams


def test_summary_algebra_with_first_and_bytes_is_associative_and_equals_the_model():
    rng = np.random.RandomState(2901)
    lists = [[b"^(..)*$"], [b"ab+c", b"^c"], [b"^$"], [b"a$"], [b"^[ab]*c"], [b"(a|b)c{2,3}$"], [b"^a"]]
    tables = []
    for exprs in lists:
        asts, _ = RM.compile_list(exprs)
        tables.append((RM.dfa(RM.Automaton(asts), NL)[2], RM.Matcher(exprs)))
    streams = composed = first_selected = some_bytes = 0
    for case in range(280):
        table, matcher = tables[case % len(tables)]
        n, lo, inv = int(rng.randint(1, 90)), int(rng.randint(0, 1000)), bool(case & 1)
        text = bytes(rng.choice(list(b"abc\n"), p=[(1 - P_DELIM) / 3] * 3 + [P_DELIM], size=n).astype(np.uint8))
        pieces, j = [], 0
        while j < n:
            k = int(rng.randint(1, 9))
            pieces.append(_piece(lo + j, text[j:j + k], NL, table, inv))
            j += k
        left = pieces[0]
        for p in pieces[1:]:
            left = _combine(left, p, table, inv)
        assert left == _piece(lo, text, NL, table, inv), (case, text)          # the fold is the definition
        for _ in range(4):
            assert _fold_random(rng, pieces, table, inv) == left, (case, text)
        recs, sel, _, packed = XRM.extract_regex(text, None, NL, inv, matcher=matcher)
        assert _finish(left, lo, lo + n, table, inv) == (len(sel), len(packed)), (case, text, left, sel)
        streams += 1
        composed += any(not a[0] and not b[0] for a, b in zip(pieces, pieces[1:]))
        first_selected += bool(sel) and sel[0] == recs[0]
        some_bytes += left[6] > 0
    assert streams >= 200 and 4 * composed >= streams and 4 * first_selected >= streams and 4 * some_bytes >= streams, (streams, composed, first_selected, some_bytes)


# ---- the kernels
KERNELS = {"zra_extractx_count_kernel": 65536, "zra_extractx_scan_kernel": 163840, "zra_extractx_copy_kernel": 163840}


def test_regex_extract_kernels_stay_inside_their_bounds():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    assert sorted(k for k in res if k.startswith("zra_extractx_")) == sorted(KERNELS)
    for k, lds in KERNELS.items():
        r = res[k]
        assert r["source"] == "zra_extract_regex.hip", (k, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds_bytes"] <= lds, (k, r)
