"""The inputs of tests/test_gpu_grep_regex_context.py, generated here so that a CPU test (tests/test_regex_context_abi.py) can run
them through the model and assert that every input reaches the seam it is built for. A case is a dict: data, fs (frame size), pats,
pairs [(after, before)], stagings, lo / hi, delim, modes (the inversions), fold; model() answers a call of a case from
tests/regex_context_model.py, once per (case, widths, inversion, range): the GPU tests and the shape test share the answers.
The scan's trip is 64 positions, its wave 2,048, its tile 8,192; a pass is a whole number of frames, one frame with staging 1."""
import numpy as np

import regex_context_model as RCM
import regex_model as RM

NL = 10
TILE, WAVE, TRIP = 8192, 2048, 64
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (64, 64)]                            # (after, before)
FS = 1024


class MemoTable:
    """regex_model.TableMatcher (linear in the record: the long records) with a memo by content (the many equal lines)"""

    def __init__(self, pats, fold=False, delim=NL):
        self.t, self.memo = RM.TableMatcher(pats, fold, delim), {}

    def matches(self, record):
        record = bytes(record)
        if record not in self.memo:
            self.memo[record] = self.t.matches(record)
        return self.memo[record]


def case(name, data, fs, pats, pairs=PAIRS, stagings=(0,), lo=0, hi=None, delim=NL, modes=(False, True), fold=False):
    return dict(name=name, data=bytes(data), fs=fs, pats=[bytes(p) for p in pats], pairs=list(pairs), stagings=tuple(stagings), lo=lo, hi=hi, delim=delim,
                modes=tuple(modes), fold=fold, _matcher=None, _memo={})


def model(c, after, before, inv, lo=None, hi="case"):
    """(listed, |S|, groups, records of the range, matches) of one call of the case; lo / hi override the case's range"""
    lo = c["lo"] if lo is None else lo
    hi = c["hi"] if hi == "case" else hi
    key = (after, before, bool(inv), lo, hi)
    if key not in c["_memo"]:
        if c["_matcher"] is None:
            c["_matcher"] = MemoTable(c["pats"], c["fold"], c["delim"])
        c["_memo"][key] = RCM.context(c["data"], c["pats"], c["delim"], inv, c["fold"], before, after, lo, hi, matcher=c["_matcher"])
    return c["_memo"][key]


def lines(rng, n, alphabet=b"abcde", longest=30):
    """about n bytes of short lines over `alphabet`, some empty, the last one without its newline"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(list(alphabet), size=int(rng.randint(0, longest + 1))).astype(np.uint8)) + b"\n"
    return bytes(out[:n - 1]) + alphabet[-1:]


_CACHE = {}


def _once(fn):
    def get(*args):
        key = (fn.__name__,) + args
        if key not in _CACHE:
            _CACHE[key] = fn(*args)
        return _CACHE[key]
    get.__name__ = fn.__name__
    return get


# ---- 1
@_once
def frame_size_4():
    """About 260 frames of 4 bytes; with one slot a pass holds 4 bytes, and the 60-byte line gives 15 passes in a row that end no
    record while ranges are pending in front of them (it is selected: its before-context waits)."""
    rng = np.random.RandomState(41)
    long_line = b"cd" + bytes(rng.choice(list(b"acde"), size=56).astype(np.uint8)) + b"de"
    data = lines(rng, 500) + b"\nb\nc\nbb\n" + long_line + b"\n" + lines(rng, 480)
    return case("frame_size_4", data, 4, [b"^a+b", b"[de]e+$", b"^cd[acd]+e[acde]+de$"], stagings=(1, 0)), long_line


# ---- 2
@_once
def one_record_per_pass():
    """Frames of 16 bytes, one per pass. Segments of whole frames: A one line of 15 bytes, B two of 7, C four of 3, D one of 47 (two
    passes that end no record). A selected line is X v.. (by ^X) or u v.. X v (by Xv+$). before = 3: the pending set grows over passes
    without a selected record and is trimmed to the last 3 (5 A in front of the first X), is kept whole (an X alone in its pass), kept
    in part (B: one unselected record of the pass in front of its X), dropped whole (C: three in front), stays smaller than 3 (two A
    between two X), waits through D's passes, and is dropped by the last pass (6 A behind the last X)."""
    def seg(kind, *sel):
        n, m = dict(A=(1, 15), B=(2, 7), C=(4, 3), D=(1, 47))[kind]
        def line(k):
            if k not in sel:
                return b"u" + b"v" * (m - 1)
            return b"X" + b"v" * (m - 1) if (k + m) % 2 else b"u" + b"v" * (m - 3) + b"Xv"
        return b"".join(line(k) + b"\n" for k in range(n))

    parts = [seg("A")] * 5 + [seg("A", 0)] + [seg("A")] * 4 + [seg("B", 1)] + [seg("A")] * 4 + [seg("C", 3)] + [seg("A")] * 2 + [seg("A", 0)] + \
            [seg("A")] * 2 + [seg("D")] + [seg("A", 0)] + [seg("A"), seg("D"), seg("B"), seg("C", 0)] + [seg("A")] * 6
    data = b"".join(parts)
    assert len(data) % 16 == 0
    return case("one_record_per_pass", data, 16, [b"^X|Xv+$"], pairs=[(0, 3), (1, 3), (2, 3), (5, 3), (0, 1), (64, 64)], stagings=(1, 0, 48))


# ---- 3
SEAM_TARGETS = [(1 * TILE + 0, "start"), (2 * TILE + 1, "start"), (3 * TILE + 2, "start"), (4 * TILE + 3, "start"), (5 * TILE + 4, "start"), (6 * TILE + 5, "start"),
                (7 * TILE, "end"), (8 * TILE + WAVE, "end"), (9 * TILE + WAVE + 1, "start"), (10 * TILE + TRIP, "end"), (11 * TILE + TRIP + 2, "start"),
                (12 * TILE + 3 * WAVE, "end"), (13 * TILE + 2 * WAVE + 3, "start")]


@_once
def first_record_of_a_tile():
    """Short lines over `abc`, and for every target (delimiter position, kind) a record selected only by what lies in front of the
    seam: kind start, `Q` + a.. by ^Q, the Q four bytes in front of the seam and the delimiter 0 .. 5 behind it; kind end, a.. + `Q`
    by Q$, the Q the last byte in front of the seam, the delimiter the first behind. Seams: a tile's first position, a wave's
    (2,047 / 2,048), a trip's (63 / 64), and with two frames of 1,024 to a pass a pass's last byte (every multiple of 2,048)."""
    rng = np.random.RandomState(3)
    out = bytearray()

    def fill(to):
        while len(out) + 14 < to:
            out.extend(bytes(rng.choice(list(b"abc"), size=int(rng.randint(0, 13))).astype(np.uint8)) + b"\n")
        if to - len(out) >= 1:
            out.extend(b"c" * (to - len(out) - 1) + b"\n")

    for t, kind in SEAM_TARGETS:
        seam = t - t % TRIP
        if kind == "start":
            fill(seam - 4)
            out.extend(b"Q" + b"a" * (t - len(out) - 1) + b"\n")
        else:
            fill(seam - 6)
            out.extend(b"aaaaaQ\n")
        assert out[t] == NL and len(out) == t + 1, (t, kind, len(out))
    fill(len(out) + 3000)
    out.extend(b"b")
    return case("first_record_of_a_tile", out, FS, [b"^Q", b"Q$"], pairs=[(2, 3), (1, 0), (0, 1), (64, 64), (0, 0)], stagings=(0, 2 * FS))


# ---- 4
@_once
def delimiter_free_tiles():
    """Records of 20,480 bytes (2.5 tiles: the maps of whole tiles compose) between short ones. The first is unselected and lies in the
    after-context of a selected record two in front of it and in the before-context of one two behind it; the second is selected
    itself, by ^Q.*Z$, which needs the state carried from its first byte to its last; the third, 9,000 bytes, is the pending
    before-context of the record behind it while with two frames to a pass four passes go by without a delimiter."""
    rng = np.random.RandomState(9)
    body = lambda n: bytes(rng.choice(list(b"abcdefgh \x0B"), size=n).astype(np.uint8))
    short = lambda n: lines(rng, n, b"abc")[:-1] + b"\n"
    long1, long2, long3 = body(20480), b"Q" + body(20478) + b"Z", body(9000)
    data = short(300) + b"QoneZ\n" + b"ab\n" + long1 + b"\n" + b"ba\n" + b"QtwoZ\n" + short(200) + long2 + b"\n" + short(200) + b"cc\n" + long3 + b"\n" + b"QthreeZ\n" + \
        short(150) + b"end"
    c = case("delimiter_free_tiles", data, FS, [b"^Q.*Z$"], pairs=[(2, 2), (1, 0), (0, 1), (64, 64)], stagings=(0, 2 * FS))
    return c, (long1, long2, long3)


# ---- 5
GAP_PAIRS = [(2, 3), (64, 64), (0, 5), (5, 0)]


@_once
def gaps(after, before):
    """Two selected records after + before unselected ones apart (one group, all of the gap output), and two one more apart (two
    groups, one record left out); then both again with the gap across a tile's boundary (8,192 and 16,384)."""
    g = after + before
    blk = lambda tag, k: b"".join(b"X\n" if i in (0, k + 1) else b"%s%d\n" % (tag, i) for i in range(k + 2))
    pad = lambda tag, k: b"".join(b"%s%d\n" % (tag, i) for i in range(k))
    a, b = blk(b"g", g), blk(b"h", g + 1)
    out = bytearray(pad(b"u", 70) + a + pad(b"w", 140) + b + pad(b"v", 140))

    def pad_to(n):
        i = 0
        while len(out) + 8 < n:
            out.extend(b"p%d\n" % i)
            i += 1
        out.extend(b"q" * (n - len(out) - 1) + b"\n")

    pad_to(TILE - len(a) // 2)
    out.extend(a + pad(b"w", 140))
    pad_to(2 * TILE - len(b) // 2)
    out.extend(b + pad(b"t", 70))
    return case("gaps_%d_%d" % (after, before), out, 256, [b"^X$"], pairs=[(after, before)], stagings=(0, 1), modes=(False,))


# ---- 6
@_once
def more_tiles_than_scan_lanes():
    """8.4 MiB in frames of 64 KiB: 1,030 tiles, so a lane of the one-workgroup scan walks two tiles forwards and backwards; with
    passes of 16 frames nine passes of 128 tiles. Log lines drawn from forty that do not match, fifteen placed ones that do, and one
    line of 100,000 bytes (whole tiles without a delimiter) with a match in it."""
    fs = 65536
    U = 1029 * TILE + 5000
    rng = np.random.RandomState(67)
    words = [b"GET", b"POST", b"/index.html", b"/api/v1/items", b"status=200", b"status=404", b"took 12ms", b"user=anna", b"user=ben", b"cache hit", b"cache miss",
             b"bytes=5120", b"retry 1", b"from 10.0.0.7", b"tls1.3", b"worker-3"]
    plain = [b" ".join(words[int(k)] for k in rng.randint(0, len(words), size=int(rng.randint(6, 14)))) for _ in range(40)]
    hits = [b"GET /api/v1/items status=503 took 7ms", b"upstream timeout after 1500ms worker-3"]
    picks = rng.randint(0, 40, size=U // 60)
    out, k, placed = bytearray(), 0, []
    marks = sorted(int(x) for x in rng.randint(0, U - 200000, size=15))
    while len(out) < U - 300:
        if len(out) >= 3000000 and not placed.count("long"):
            out.extend(b"x" * 50000 + hits[1] + b"y" * 50000 + b"\n")
            placed.append("long")
        elif marks and len(out) >= marks[0]:
            marks.pop(0)
            out.extend(hits[len(placed) % 2] + b"\n")
            placed.append("hit")
        else:
            out.extend(plain[picks[k]] + b"\n")
            k += 1
    assert len(out) <= U
    out.extend(b"z" * (U - len(out)))
    return case("more_tiles_than_scan_lanes", out, fs, [b"status=5[0-9]{2}|timeout after [0-9]+ms"], pairs=[(2, 3), (64, 64)], stagings=(0, 16 * fs), modes=(False,))


# ---- 7
RANDOM_EXPRESSIONS = [b"da+b|^cab", b"a(b|c){2,3}$", b"^$", b"^.{0,3}$", b"^a.*b$", b"ab+c", b"[cd]{4}", b"^(a|b)+$"]
RANDOM_SEED = 79                                                              # (40 of the 40 have a selected record, 23 more than one group)


@_once
def random_small_shapes():
    """Forty small archives, 200 to 20,000 bytes: lines of 0 to 12 bytes over four letters, an expression of RANDOM_EXPRESSIONS, frames
    of 64, 256 or 1,024 bytes, one, three or all frames to a pass, a range that begins and ends anywhere, widths up to 64."""
    rng = np.random.RandomState(RANDOM_SEED)
    out = []
    for k in range(40):
        n = int(rng.randint(200, 3000)) if k % 4 else int(rng.randint(3000, 20001))
        data = lines(rng, n, b"abcd", 12)
        fs = (64, 256, 1024)[int(rng.randint(0, 3))]
        lo = int(rng.randint(0, n // 3)) if k % 3 else 0
        hi = int(rng.randint(2 * n // 3, n + 1)) if k % 3 == 2 else None
        pair = (int(rng.randint(0, 65)), int(rng.randint(0, 65))) if k % 4 == 1 else (int(rng.randint(0, 5)), int(rng.randint(0, 5)))
        out.append(case("random_%d" % k, data, fs, [RANDOM_EXPRESSIONS[int(rng.randint(0, len(RANDOM_EXPRESSIONS)))]], pairs=[pair], stagings=((1, 3 * fs, 0)[k % 3],),
                        lo=lo, hi=hi, modes=(bool(k & 1),)))
    return out


# ---- 8, 9, 11, 12, 13
@_once
def text():
    """6 frames of 1,024 bytes and a last one of 300: word lines, no newline at the end, and the last line, which hi ends, selected"""
    rng = np.random.RandomState(33)
    words = [b"alpha", b"beta", b"gamma", b"needle", b"delta", b"pin", b"eps", b"", b"zeta", b"neeedle", b"eta", b"x"]
    U = 6 * FS + 300
    out = bytearray()
    while len(out) < U - 40:
        out += b" ".join(words[int(k)] for k in rng.randint(0, len(words), size=int(rng.randint(0, 5)))) + b"\n"
    out += b"pin " + b"t" * (U - len(out) - 4)
    assert len(out) == U
    return case("text", out, FS, [b"ne+dle$", b"^pin"], stagings=(0, FS, 1))


@_once
def clipped_ranges():
    """ranges of text() that begin and end inside records: a `needle` in the middle of a line is matched by neither ^needle nor
    needle$, a range that begins at its first byte or ends behind its last one selects the clipped record"""
    t = text()
    c = case("clipped", t["data"], FS, [b"^needle", b"needle$"], pairs=[(2, 3), (64, 64), (0, 0)], stagings=(0, FS, 1))
    data = c["data"]
    mids = []
    p = data.find(b" needle ")
    while p >= 0 and len(mids) < 40:
        mids.append(p + 1)
        p = data.find(b" needle ", p + 1)
    nl = [i for i in range(len(data)) if data[i] == NL]
    whole = [(o, n) for o, n, sel in model(c, 0, 0, False, 0, None)[0]]        # (a line may begin or end with a `needle` of its own)
    mids = [m for m in mids if not any(o <= m < o + n for o, n in whole)]
    a, b = mids[1], mids[-2]
    ranges = [(a, b + 6), (a, a + 6), (a + 1, b + 6), (a, b + 5), (nl[3] + 2, nl[-4] - 1), (nl[10], nl[40] + 1), (nl[10] + 1, nl[40]), (5, 5), (len(data) - 1, len(data))]
    return c, ranges


# ---- 10
@_once
def degenerate():
    rng = np.random.RandomState(12)
    data = lines(rng, 3000) + b"\n\n\n" + lines(rng, 2500, b"ab") + b"\n" * 70 + lines(rng, 600)
    zdata = data.replace(b"\n", b"\x00")
    up = bytes(data).replace(b"ab", b"AB")
    return dict(everything=case("everything", data, 512, [b"a*"], pairs=[(2, 3), (64, 64)], stagings=(0, 1)),
                nothing=case("nothing", data, 512, [b"a^b"], pairs=[(2, 3), (64, 64)], stagings=(0, 1)),
                empties=case("empties", data, 512, [b"^$"], pairs=[(1, 1), (0, 64), (2, 3)], stagings=(0, 1)),
                delimiter_0=case("delimiter_0", zdata, 512, [b"bb+$", b"^cd"], pairs=[(2, 3)], stagings=(512 * 3,), delim=0),
                fold_case=case("fold_case", up, 512, [b"^aB+", b"d+A$"], pairs=[(1, 2)], stagings=(0, 512), fold=True))
