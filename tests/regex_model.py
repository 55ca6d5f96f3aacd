"""The yardstick of the regex grep (include/zra_hip.h: ZraHipCheckRegex, ZraHipGrepArchiveRegex): a second implementation written from
the grammar in that header, not from zra_amd/csrc/zra_regex.h. A recursive-descent parser makes an AST, counted repetitions are
expanded into Glushkov positions (first / last / follow as Python integers used as bit sets), a record is matched by stepping position
sets over BOL, its bytes and EOL, and a subset construction with Moore's refinement of its own gives `states` and `classes`.
For the comparison with Python's `re` the AST is emitted as a pattern in which every atom is an explicit [\\xHH...] set."""
import re

import grep_model as GM

MAX_STATES, MAX_POSITIONS, MAX_SUBSETS, MAX_EXPR_BYTES, MAX_PATTERNS, MAX_REPEAT = 64, 4096, 4096, 16384, 64, 255
ACCEPTED, WHY_ARGUMENTS, WHY_SYNTAX, WHY_EMPTY_ATOM, WHY_STATES = 0, 1, 2, 3, 4
ESCAPABLE = b".[]\\*+?{}()|^$-"


class Refused(Exception):
    def __init__(self, why, pattern=0):
        Exception.__init__(self, "why=%d pattern=%d" % (why, pattern))
        self.why, self.pattern = why, pattern


class _Syntax(Exception):
    pass


class _EmptyAtom(Exception):
    pass


# ---- the parser: ('set', frozenset) ('bol',) ('eol',) ('cat', [..]) ('alt', [..]) ('rep', node, min, max or None)
class _Parser:
    def __init__(self, expr, fold, delim):
        self.s, self.i, self.fold, self.delim = bytes(expr), 0, fold, delim

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else None

    def take(self):
        if self.i >= len(self.s):
            raise _Syntax()
        c = self.s[self.i]
        self.i += 1
        return c

    def escape(self):
        """behind a backslash: ('byte', b) or ('class', set)"""
        c = self.take()
        if c == ord("x"):
            h = self.s[self.i:self.i + 2]
            if len(h) < 2 or not all(chr(x) in "0123456789abcdefABCDEF" for x in h):
                raise _Syntax()
            self.i += 2
            return "byte", int(h, 16)
        if c in b"ntr":
            return "byte", {ord("n"): 10, ord("t"): 9, ord("r"): 13}[c]
        if c == ord("d"):
            return "class", set(range(48, 58))
        if c == ord("w"):
            return "class", set(range(48, 58)) | set(range(65, 91)) | set(range(97, 123)) | {95}
        if c == ord("s"):
            return "class", {32} | set(range(9, 14))
        if c in ESCAPABLE:
            return "byte", c
        raise _Syntax()

    def bracket(self):
        """behind '[': (set, negated)"""
        if self.peek() == ord(":"):
            raise _Syntax()
        neg = self.peek() == ord("^")
        if neg:
            self.i += 1
        out, first = set(), True
        while True:
            lo = self.take()
            if lo == ord("]") and not first:
                return out, neg
            first = False
            if lo == ord("[") and self.peek() == ord(":"):
                raise _Syntax()
            is_class = False
            if lo == ord("\\"):
                kind, v = self.escape()
                if kind == "class":
                    out |= v
                    is_class = True
                else:
                    lo = v
            is_range = len(self.s) - self.i >= 2 and self.s[self.i] == ord("-") and self.s[self.i + 1] != ord("]")
            if is_class:
                if is_range:
                    raise _Syntax()
                continue
            if not is_range:
                out.add(lo)
                continue
            self.i += 1
            hi = self.take()
            if hi == ord("[") and self.peek() == ord(":"):
                raise _Syntax()
            if hi == ord("\\"):
                kind, hi = self.escape()
                if kind != "byte":
                    raise _Syntax()
            if lo > hi:
                raise _Syntax()
            out |= set(range(lo, hi + 1))

    def finish(self, s, neg):
        if self.fold:
            s = s | {c ^ 0x20 for c in s if 65 <= (c & ~0x20) <= 90}
        if neg:
            s = set(range(256)) - s
        s = s - {self.delim}
        if not s:
            raise _EmptyAtom()
        return ("set", frozenset(s))

    def number(self):
        if self.peek() is None or not 48 <= self.peek() <= 57:
            raise _Syntax()
        v = 0
        while self.peek() is not None and 48 <= self.peek() <= 57:
            v = v * 10 + self.take() - 48
            if v > MAX_REPEAT:
                raise _Syntax()
        return v

    def bound(self):
        mn = self.number()
        c = self.take()
        if c == ord("}"):
            return mn, mn
        if c != ord(","):
            raise _Syntax()
        if self.peek() == ord("}"):
            self.i += 1
            return mn, None
        mx = self.number()
        if self.take() != ord("}") or mn > mx:
            raise _Syntax()
        return mn, mx

    def alternation(self, depth):
        branches = [self.concatenation(depth)]
        while self.peek() == ord("|"):
            self.i += 1
            branches.append(self.concatenation(depth))
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def concatenation(self, depth):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.piece(depth))
        if not items:
            raise _Syntax()                                                    # an empty branch, an empty group, an empty expression
        return items[0] if len(items) == 1 else ("cat", items)

    def piece(self, depth):
        c = self.take()
        if c in b"*+?{]}":
            raise _Syntax()                                                    # nothing to repeat; a stray ] or }
        if c == ord("^"):
            return ("bol",)                                                    # (a quantifier behind it is refused by the next piece)
        if c == ord("$"):
            return ("eol",)
        if c == ord("("):
            node = self.alternation(depth + 1)
            if self.peek() != ord(")"):
                raise _Syntax()
            self.i += 1
        elif c == ord("."):
            node = self.finish(set(range(256)), False)
        elif c == ord("["):
            node = self.finish(*self.bracket())
        elif c == ord("\\"):
            kind, v = self.escape()
            node = self.finish(v if kind == "class" else {v}, False)
        else:
            node = self.finish({c}, False)
        q = self.peek()
        if q is not None and q in b"*+?{":
            self.i += 1
            mn, mx = {ord("*"): (0, None), ord("+"): (1, None), ord("?"): (0, 1)}.get(q) or self.bound()
            node = ("rep", node, mn, mx)                                       # (a second quantifier is the next piece's refusal)
        return node

    def parse(self):
        node = self.alternation(0)
        if self.i != len(self.s):
            raise _Syntax()                                                    # an unbalanced )
        return node


def parse(expr, fold=False, delim=10):
    """the AST of one expression; _Syntax or _EmptyAtom"""
    return _Parser(expr, fold, delim).parse()


def count_positions(node):
    t = node[0]
    if t in ("set", "bol", "eol"):
        return 1
    if t in ("cat", "alt"):
        return sum(count_positions(k) for k in node[1])
    _, x, mn, mx = node
    return count_positions(x) * (max(mn, 1) if mx is None else mx)


# ---- Glushkov positions
BOL, EOL, END = "bol", "eol", "end"


class Automaton:
    """first / follow over the positions of (e_1|...|e_K) END; sym[p] is a frozenset of bytes, BOL, EOL or END"""

    def __init__(self, asts):
        self.sym, self.follow = [], []
        top = asts[0] if len(asts) == 1 else ("alt", list(asts))
        nullable, first, last = self._build(top)
        end = self._leaf(END)[1]
        self._link(last, end)
        self.init = first | (end if nullable else 0)
        self.end_bit = end

    def _leaf(self, sym):
        self.sym.append(sym)
        self.follow.append(0)
        bit = 1 << (len(self.sym) - 1)
        return False, bit, bit

    def _link(self, last, first):
        p = 0
        while last:
            if last & 1:
                self.follow[p] |= first
            last >>= 1
            p += 1

    def _build(self, node):
        t = node[0]
        if t == "set":
            return self._leaf(node[1])
        if t in ("bol", "eol"):
            return self._leaf(t)
        if t == "alt":
            parts = [self._build(k) for k in node[1]]
            return any(p[0] for p in parts), _or(p[1] for p in parts), _or(p[2] for p in parts)
        if t == "cat":
            return self._cat([self._build(k) for k in node[1]])
        _, x, mn, mx = node
        if mx == 0 or count_positions(x) == 0:
            return True, 0, 0
        copies = [self._build(x) for _ in range(max(mn, 1) if mx is None else mx)]
        if mx is None:
            n0, f, l = copies[-1]
            self._link(l, f)                                                   # the last copy loops
            if mn == 0:
                copies[-1] = (True, f, l)
        else:
            # copies mn .. mx - 1 are optional and nested: x (x (x)?)?, so leaving is possible behind every one of them
            parts = copies[:mn]
            tail = None
            for c in reversed(copies[mn:]):
                tail = c if tail is None else self._cat([c, (True, tail[1], tail[2])])
            if tail is not None:
                parts.append((True, tail[1], tail[2]))
            return self._cat(parts) if parts else (True, 0, 0)
        return self._cat(copies)

    def _cat(self, parts):
        nullable, first, last = True, 0, 0
        for n, f, l in parts:
            self._link(last, f)
            first = first | f if nullable else first
            last = last | l if n else l
            nullable = nullable and n
        return nullable, first, last

    # ---- matching
    def step(self, cur, symbol):
        """the positions expected behind `symbol` (a byte, BOL or EOL), the initial ones included: the leading S*"""
        nxt, p = self.init, 0
        while cur:
            if cur & 1:
                s = self.sym[p]
                if s == symbol or (isinstance(s, frozenset) and symbol in s):
                    nxt |= self.follow[p]
            cur >>= 1
            p += 1
        return nxt

    def matches(self, record):
        cur = self.init
        for symbol in [BOL] + list(bytes(record)) + [EOL]:
            if cur & self.end_bit:
                return True
            cur = self.step(cur, symbol)
        return bool(cur & self.end_bit)


def _or(it):
    v = 0
    for x in it:
        v |= x
    return v


# ---- the checks of ZraHipCheckRegex, in its order
def compile_list(patterns, fold=False, delim=10):
    """(asts, positions); Refused"""
    patterns = [bytes(p) for p in patterns]
    if not 1 <= len(patterns) <= MAX_PATTERNS or any(len(p) == 0 for p in patterns) or sum(len(p) for p in patterns) > MAX_EXPR_BYTES:
        raise Refused(WHY_ARGUMENTS)
    asts = []
    for i, p in enumerate(patterns):
        try:
            asts.append(parse(p, fold, delim))
        except _Syntax:
            raise Refused(WHY_SYNTAX, i)
        except _EmptyAtom:
            raise Refused(WHY_EMPTY_ATOM, i)
    positions = sum(count_positions(a) for a in asts)
    if positions > MAX_POSITIONS:
        raise Refused(WHY_ARGUMENTS)
    return asts, positions


def dfa(A, delim):
    """the minimal complete DFA over the non-delimiter bytes, reachable states only: (states, classes, table) where table =
    (start, accepting set, {state: {byte: state}}); Refused(4) on the construction bound or above MAX_STATES."""
    alphabet = [b for b in range(256) if b != delim]
    # bytes that every position treats alike step alike
    sets = sorted({s for s in A.sym if isinstance(s, frozenset)}, key=sorted)
    groups = {}
    for b in alphabet:
        groups.setdefault(tuple(b in s for s in sets), []).append(b)
    reps = [g[0] for g in groups.values()]
    SINK = -1
    start = A.init
    if not start & A.end_bit:
        start = A.step(start, BOL)
    if start & A.end_bit:
        start = SINK
    index, delta, order = {start: 0}, [], [start]
    k, plain = 0, int(start != SINK)                                           # plain: the sets other than the sink
    while k < len(order):
        cur = order[k]
        k += 1
        row = []
        for r in reps:
            nxt = SINK if cur == SINK else A.step(cur, r)
            if nxt != SINK and nxt & A.end_bit:
                nxt = SINK
            if nxt not in index:
                if nxt != SINK:
                    if plain >= MAX_SUBSETS:
                        raise Refused(WHY_STATES)
                    plain += 1
                index[nxt] = len(order)
                order.append(nxt)
            row.append(index[nxt])
        delta.append(row)
    accepting = [s == SINK or bool(A.step(s, EOL) & A.end_bit) for s in order]
    block = [int(a) for a in accepting]
    count = 0
    while True:
        sigs = {}
        nb = [sigs.setdefault((block[d],) + tuple(block[t] for t in delta[d]), len(sigs)) for d in range(len(order))]
        block = nb
        if len(sigs) > MAX_STATES:
            raise Refused(WHY_STATES)
        if len(sigs) == count:
            break
        count = len(sigs)
    rep_state = {}
    for d in range(len(order)):
        rep_state.setdefault(block[d], d)
    columns = {tuple(block[delta[rep_state[s]][c]] for s in range(count)) for c in range(len(reps))}
    table = (block[0], {block[d] for d in range(len(order)) if accepting[d]},
             {s: {b: block[delta[rep_state[s]][c]] for c, g in enumerate(groups.values()) for b in g} for s in range(count)})
    return count, len(columns), table


def check(patterns, fold=False, delim=10):
    """what ZraHipCheckRegex answers: dict(ok, why, pattern, states, classes, positions)"""
    try:
        asts, positions = compile_list(patterns, fold, delim)
        states, classes, _ = dfa(Automaton(asts), delim)
    except Refused as r:
        return dict(ok=False, why=r.why, pattern=r.pattern, states=0, classes=0, positions=0)
    return dict(ok=True, why=ACCEPTED, pattern=0, states=states, classes=classes, positions=positions)


class Matcher:
    """the records an accepted expression list matches"""

    def __init__(self, patterns, fold=False, delim=10):
        self.asts, self.positions = compile_list(patterns, fold, delim)
        self.A = Automaton(self.asts)
        self.delim = delim
        self._memo = {}

    def matches(self, record):
        record = bytes(record)
        if record not in self._memo:
            self._memo[record] = self.A.matches(record)
        return self._memo[record]


def grep_regex(data, patterns, delimiter=0x0A, invert=False, fold=False, lo=0, hi=None, matcher=None):
    """(records of the range, the selected ones, matched records): ZraHipGrepArchiveRegex on the plaintext `data`"""
    m = matcher or Matcher(patterns, fold, delimiter)
    recs = GM.records(data, delimiter, lo, hi)
    hit = [m.matches(data[o:o + n]) for o, n in recs]
    return recs, [r for r, h in zip(recs, hit) if h != bool(invert)], sum(hit)


class TableMatcher:
    """Matcher's answers from the minimal DFA: linear in the record, for the long records of the GPU tests"""

    def __init__(self, patterns, fold=False, delim=10):
        asts, _ = compile_list(patterns, fold, delim)
        _, _, (self.start, self.accepting, self.delta) = dfa(Automaton(asts), delim)
        import numpy as np
        n = len(self.delta)
        self.np = np
        self.tab = np.zeros((256, n), dtype=np.int64)
        for s, row in self.delta.items():
            for b, t in row.items():
                self.tab[b, s] = t

    def matches(self, record):
        s = self.start
        tab = self.tab
        for b in bytes(record):
            s = tab[b, s]
        return int(s) in self.accepting


# ---- Python's re
def _re_set(s):
    return "[" + "".join("\\x%02x" % b for b in sorted(s)) + "]"


def to_re(node, bol="\\A", eol="\\Z"):
    """the AST as a pattern of Python's re (a str): atoms as explicit sets, groups as (?:...)"""
    t = node[0]
    if t == "set":
        return _re_set(node[1])
    if t == "bol":
        return bol
    if t == "eol":
        return eol
    if t == "cat":
        return "".join(to_re(k, bol, eol) for k in node[1])
    if t == "alt":
        return "(?:" + "|".join(to_re(k, bol, eol) for k in node[1]) + ")"
    _, x, mn, mx = node
    return "(?:%s){%d,%s}" % (to_re(x, bol, eol), mn, "" if mx is None else mx)


def re_anchored(asts):
    """compiled for bytes: ^ as \\A and $ as \\Z"""
    return re.compile(("(?:" + "|".join(to_re(a) for a in asts) + ")").encode("ascii"), re.DOTALL)


SENTINEL_BOL, SENTINEL_EOL = "Ā", "ā"


def re_symbols(asts):
    """compiled for str: ^ and $ as two characters outside the bytes, to be searched in SENTINEL_BOL + record (latin-1) + SENTINEL_EOL.
    This is the header's definition word for word: BOL r EOL in S* (e) S*."""
    return re.compile("(?:" + "|".join(to_re(a, SENTINEL_BOL, SENTINEL_EOL) for a in asts) + ")", re.DOTALL)


def anchors_are_plain(A):
    """True when no word of the expressions has an anchor directly behind an anchor, other than $ behind ^. Then reading BOL / EOL as
    symbols and testing \\A / \\Z as zero-width assertions are the same thing; `^^a`, `(^|a)^b` and `$$` are where the two differ (an
    assertion may be repeated, a symbol cannot be read twice)."""
    for p, s in enumerate(A.sym):
        if s not in (BOL, EOL):
            continue
        f, q = A.follow[p], 0
        while f:
            if f & 1 and A.sym[q] in (BOL, EOL) and not (s == BOL and A.sym[q] == EOL):
                return False
            f >>= 1
            q += 1
    return True


# ---- a generator of expressions: every operator, nesting to depth 3, anchors in odd places
def random_expr(rng, depth=0, alphabet="abc"):
    def atom():
        r = rng.randint(0, 12)
        if r < 6:
            return alphabet[rng.randint(0, len(alphabet))]
        if r == 6:
            return "."
        if r == 7:
            return "[%s%s]" % ("^" if rng.randint(0, 2) else "", "".join(alphabet[rng.randint(0, len(alphabet))] for _ in range(rng.randint(1, 3))))
        if r == 8:
            return "[a-b]"
        if r == 9:
            return ("\\d", "\\w", "\\s", "\\x61", "\\.")[rng.randint(0, 5)]
        return "^" if r == 10 else "$" if r == 11 else alphabet[0]

    def piece():
        if depth < 3 and rng.randint(0, 4) == 0:
            x, can = "(" + random_expr(rng, depth + 1, alphabet) + ")", True
        else:
            x = atom()
            can = x not in "^$"
        if can and rng.randint(0, 3) == 0:
            x += ("*", "+", "?", "{2}", "{0}", "{1,}", "{0,2}", "{2,3}", "{0,0}", "{3,}")[rng.randint(0, 10)]
        return x

    branches = ["".join(piece() for _ in range(rng.randint(1, 4))) for _ in range(1 if rng.randint(0, 3) else rng.randint(2, 4))]
    return "|".join(branches)
