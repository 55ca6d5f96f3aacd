"""The yardstick of the pattern-expression tests (include/zra_hip.h: ZraHipCheckPatternExpr and the ...Expr scans): what a list of
patterns means under a syntax word, as one byte set per element, and the matches, the grep and the extract over such sets, computed on
the CPU from the plaintext a test generated itself. Written from the header's grammar, independently of zra_pattern_expr.h; with
syntax 0 the three scans ARE msearch_model, grep_model and extract_model. Cross-checked in tests/test_pattern_expr.py."""
import numpy as np

import extract_model
import grep_model
import msearch_model

FOLD_CASE, CLASSES = 1, 2
MAX_PATTERNS, MAX_ELEMENTS, MAX_ELEMENTS_ALL, MAX_SETS, MAX_EXPR_BYTES = 64, 256, 4096, 32, 16384
RESERVED = b"]*+?{}()|^$"
ESCAPABLE = b".[]\\*+?{}()|^$-"
ALL = frozenset(range(256))
CLASS = {ord("d"): frozenset(range(48, 58)), ord("w"): frozenset(list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123)) + [95]),
         ord("s"): frozenset([32, 9, 10, 11, 12, 13])}
HEX = b"0123456789abcdefABCDEF"


class Refused(ValueError):
    """a pattern list the calls answer with {ZStdError, 42}; .index: the pattern, or None for the list as a whole"""

    def __init__(self, why, index=None):
        ValueError.__init__(self, "%s (pattern %s)" % (why, index))
        self.index = index


def _escape(e, p):
    """the escape behind the backslash at e[p - 1]: (p behind it, a byte or a frozenset)"""
    if p >= len(e):
        raise Refused("\\ at the end")
    c = e[p]
    if c == ord("x"):
        if p + 3 > len(e) or e[p + 1] not in HEX or e[p + 2] not in HEX:
            raise Refused("\\x without two hex digits")
        return p + 3, int(e[p + 1:p + 3], 16)
    if c in b"ntr":
        return p + 1, {ord("n"): 10, ord("t"): 9, ord("r"): 13}[c]
    if c in CLASS:
        return p + 1, CLASS[c]
    if c in ESCAPABLE:
        return p + 1, c
    raise Refused("unknown escape")


def _bracket(e, p):
    """the set behind the [ at e[p - 1]: (p behind its ], the items' bytes, negated)"""
    if p < len(e) and e[p] == ord(":"):
        raise Refused("[: is reserved")
    neg = p < len(e) and e[p] == ord("^")
    p += neg
    s, first = set(), True
    while True:
        if p >= len(e):
            raise Refused("unterminated set")
        c = e[p]
        p += 1
        if c == ord("]") and not first:
            return p, s, neg
        first = False
        if c == ord("[") and p < len(e) and e[p] == ord(":"):
            raise Refused("[: is reserved")
        if c == ord("\\"):
            p, c = _escape(e, p)
        is_range = p + 1 < len(e) and e[p] == ord("-") and e[p + 1] != ord("]")
        if isinstance(c, frozenset):
            if is_range:
                raise Refused("a class as a range end")
            s |= c
            continue
        if not is_range:
            s.add(c)
            continue
        hi = e[p + 1]
        p += 2
        if hi == ord("[") and p < len(e) and e[p] == ord(":"):
            raise Refused("[: is reserved")
        if hi == ord("\\"):
            p, hi = _escape(e, p)
            if isinstance(hi, frozenset):
                raise Refused("a class as a range end")
        if c > hi:
            raise Refused("range out of order")
        s |= set(range(c, hi + 1))


def _finish(s, neg, soft, syntax, delimiter):
    s = set(s)
    if syntax & FOLD_CASE:
        s |= {b ^ 0x20 for b in s if 65 <= (b & ~0x20) <= 90}
    if neg:
        s = set(ALL) - s
    if delimiter is not None and delimiter in s:
        if not soft:
            raise Refused("an element matches the delimiter")
        s.discard(delimiter)
    if not s:
        raise Refused("empty set")
    return frozenset(s)


def _elements(e, syntax, delimiter):
    out, p = [], 0
    while p < len(e):
        c = e[p]
        p += 1
        s, neg, soft = {c}, False, False
        if syntax & CLASSES:
            if c == ord("."):
                s, soft = ALL, True
            elif c == ord("["):
                p, s, neg = _bracket(e, p)
                soft = neg
            elif c == ord("\\"):
                p, v = _escape(e, p)
                s = v if isinstance(v, frozenset) else {v}
            elif c in RESERVED:
                raise Refused("reserved byte")
        out.append(_finish(s, neg, soft, syntax, delimiter))
        if len(out) > MAX_ELEMENTS:
            raise Refused("more than %d elements" % MAX_ELEMENTS)
    if not out:
        raise Refused("empty pattern")
    return out


def counted(sets):
    """is this final set one of the call's counted sets: neither a single byte nor one ASCII letter in its two cases"""
    if len(sets) == 1:
        return False
    lo = min(sets)
    return not (len(sets) == 2 and 65 <= lo <= 90 and lo | 0x20 in sets)


def compile(patterns, syntax=CLASSES, delimiter=None):
    """[[frozenset of bytes per element] per pattern], or Refused: rule 1's pattern checks of the ...Expr calls"""
    patterns = [bytes(p) for p in patterns]
    if syntax & ~(FOLD_CASE | CLASSES) or not 1 <= len(patterns) <= MAX_PATTERNS:
        raise Refused("syntax word or pattern count")
    limit = MAX_EXPR_BYTES if syntax & CLASSES else MAX_ELEMENTS_ALL
    if any(len(p) == 0 for p in patterns) or sum(len(p) for p in patterns) > limit:
        raise Refused("sizes")
    out = []
    for i, e in enumerate(patterns):
        try:
            out.append(_elements(e, syntax, delimiter))
        except Refused as r:
            raise Refused(r.args[0], i)
        if sum(len(x) for x in out) > MAX_ELEMENTS_ALL:
            raise Refused("more than %d elements in all" % MAX_ELEMENTS_ALL, i)
    if n_sets(out) > MAX_SETS:
        raise Refused("more than %d sets" % MAX_SETS)
    return out


def n_sets(compiled):
    return len({s for pat in compiled for s in pat if counted(s)})


def lengths(compiled):
    return [len(p) for p in compiled]


def set_matches(data, compiled, lo=0, hi=None):
    """msearch_model.matches_multi over sets: sorted (p, i) with lo <= p, p + m_i <= hi and data[p + q] in element q for all q"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    hi = len(a) if hi is None else min(hi, len(a))
    out = []
    for i, pat in enumerate(compiled):
        n = hi - lo - len(pat) + 1
        if n <= 0:
            continue
        ok = np.ones(n, dtype=bool)
        for q, s in enumerate(pat):
            table = np.zeros(256, dtype=bool)
            table[list(s)] = True
            ok &= table[a[lo + q:lo + q + n]]
        out += [(int(p) + lo, i) for p in np.flatnonzero(ok)]
    return sorted(out)


def matches_multi(data, patterns, syntax=0, lo=0, hi=None):
    if syntax == 0:
        return msearch_model.matches_multi(data, patterns, lo, hi)
    return set_matches(data, compile(patterns, syntax, None), lo, hi)


def survivors(data, patterns, syntax=0, lo=0, hi=None):
    """msearch_model.survivors over sets: the positions whose first two elements admit their bytes for some pattern"""
    if syntax == 0:
        return msearch_model.survivors(data, patterns, lo, hi)
    a, c = np.frombuffer(bytes(data), dtype=np.uint8), compile(patterns, syntax, None)
    hi = len(a) if hi is None else min(hi, len(a))
    if hi - lo < min(len(p) for p in c):
        return 0
    b0, b1 = a[lo:hi], np.append(a[lo + 1:hi], np.uint8(0))
    has_next = np.arange(lo, hi) + 1 < hi
    ok = np.zeros(hi - lo, dtype=bool)
    for pat in c:
        t0, t1 = np.zeros(256, dtype=bool), np.ones(256, dtype=bool)
        t0[list(pat[0])] = True
        if len(pat) > 1:
            t1[:] = False
            t1[list(pat[1])] = True
            ok |= t0[b0] & t1[b1] & has_next
        else:
            ok |= t0[b0]
    return int(ok.sum())


def grep(data, patterns, syntax=0, delimiter=0x0A, invert=False, lo=0, hi=None):
    """grep_model.grep over sets: (records of the range, the selected ones, matches)"""
    if syntax == 0:
        return grep_model.grep(data, patterns, delimiter, invert, lo, hi)
    found = set_matches(data, compile(patterns, syntax, delimiter), lo, hi)
    recs = grep_model.records(data, delimiter, lo, hi)
    starts = sorted({p for p, _ in found})
    sel, k = [], 0
    for off, size in recs:
        while k < len(starts) and starts[k] < off:
            k += 1
        if (k < len(starts) and starts[k] < off + size) != bool(invert):
            sel.append((off, size))
    return recs, sel, len(found)


def extract(data, patterns, syntax=0, delimiter=0x0A, invert=False, lo=0, hi=None):
    """extract_model.extract over sets: (records of the range, the selected ones, matches, the packed bytes)"""
    if syntax == 0:
        return extract_model.extract(data, patterns, delimiter, invert, lo, hi)
    data = bytes(data)
    recs, sel, matches = grep(data, patterns, syntax, delimiter, invert, lo, hi)
    return recs, sel, matches, b"".join(data[o:o + n] + bytes([delimiter]) for o, n in sel)
