"""The inputs of tests/test_gpu_extract_where.py, generated here by fixed seeds so that a CPU test (tests/test_extract_where_abi.py)
can run them through the model and assert that every input reaches the seam it is built for. A case is a dict: data, fs (frame
size), pats, and what its test needs beside them; model() answers a call of a case from tests/extract_where_model.py, once per
(case, clauses, inversion, range): the GPU tests and the shape test share the answers.
The scan's trip is 64 positions, its wave 2,048, its tile 8,192, a workgroup's group 8 tiles, the scan kernel's lanes 1,024; a pass is
a whole number of frames, one frame with staging 1."""
import numpy as np

import extract_where_model as XWM

NL = 10
TILE, WAVE, TRIP, GROUP, LANES = 8192, 2048, 64, 8, 1024
FS = 1024
A, B, C = b"\xF0NEEDLE\xF1", b"\xF2THREAD\xF3", b"\xF4C\xF5"
ABC = [A, B, C]
# over [A, B, C]: selected while the set is {}, not once C has arrived, again once A has
NONMONO = [(0, 0, 0b100), (0b101, 0, 0)]


def case(name, data, fs, pats, **more):
    return dict(name=name, data=bytes(data), fs=fs, pats=[bytes(p) for p in pats], _memo={}, **more)


def model(c, where, inv, lo=0, hi=None, matches=None, pats=None):
    """(records of the range, the selected ones, the (p, i) pairs, the packed bytes) of one call of the case"""
    key = (tuple(where), bool(inv), lo, hi, None if pats is None else tuple(pats))
    if key not in c["_memo"]:
        c["_memo"][key] = XWM.extract_where(c["data"], pats or c["pats"], where, NL, inv, lo, hi, matches=matches)
    return c["_memo"][key]


def lines(rng, n, alphabet=b"abcde", longest=30):
    """about n bytes of short lines over `alphabet`, some empty, the last one without its newline"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(list(alphabet), size=int(rng.randint(0, longest + 1))).astype(np.uint8)) + b"\n"
    return bytes(out[:n - 1]) + alphabet[-1:]


def random_clauses(rng, k, n_max=8):
    """1 .. n_max clauses over k patterns: a few bits per term, `none` disjoint from the other two; bit k - 1 is used by the first"""
    out = []
    for c in range(int(rng.randint(1, n_max + 1))):
        bits = [int(b) for b in rng.permutation(k)[:int(rng.randint(0, 6))]]
        if c == 0:
            bits = [k - 1] + [b for b in bits if b != k - 1]
        terms = [0, 0, 0]
        for b in bits:
            terms[int(rng.randint(0, 3))] |= 1 << b
        out.append(tuple(terms))
    return out


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
# tests/test_gpu_grep_where.py's first group over [b, cda, the long line's middle, zz, ea], then the non-monotone list over cda and ea
TINY_WHERE = ([(0b11, 0, 0)], [(0b1, 0, 0b10)], [(0b10001, 0, 0), (0b100, 0, 0b1)], [(0, 0, 0)], [(0, 0, 0b10), (0b10010, 0, 0)])


@_once
def frame_size_4():
    """About 270 frames of 4 bytes; with one slot a pass holds 4 bytes. `late` has b at its head and cda 31 bytes on: under all = {b,
    cda} it is copied provisionally by eight passes and selected by the ninth, under {b, 0, cda} it is selected until the ninth
    unselects it. `turn` gains cda and then ea: the non-monotone list selects, unselects and selects it again."""
    rng = np.random.RandomState(41)
    long_line = bytes(rng.choice(list(b"acde"), size=60).astype(np.uint8))
    late = b"b" + b"a" * 30 + b"cda" + b"ac"
    turn = b"aaaa" + b"dd" * 5 + b"cda" + b"a" * 20 + b"ea" + b"dd"
    head = lines(rng, 500) + b"\n" + long_line + b"\n"
    data = head + late + b"\n" + b"ad\n" + turn + b"\n" + lines(rng, 480)
    pats = [b"b", b"cda", long_line[5:45], b"zz", b"ea"]
    return case("frame_size_4", data, 4, pats, late=(len(head), len(late)), turn=(len(head) + len(late) + 4, len(turn)), long_line=(501, 60))


# ---- 2
@_once
def filler():
    """40 KiB without a delimiter and without a byte of the three patterns: the body of a long record"""
    return bytes(np.random.RandomState(5).randint(32, 127, size=40 << 10).astype(np.uint8))


@_once
def seam(dist, has_a, has_b):
    """Short records, one of them with C, then a long record with A 50 bytes behind its start and B `dist` positions further on, then a
    short record with C and more short ones (tests/test_gpu_grep_where.py's second group). S: the long record's start."""
    rng = np.random.RandomState(dist)
    head = lines(rng, 300)[:-1] + b"\nxx" + C + b"yy\n"
    S = len(head)
    tail = b"\nq" + C + b"\n" + lines(rng, 200, b"abc") + b"\n" + A + b"-" + B + b"\nlast"   # (a short record with both: no mode selects nothing)
    body = bytearray(filler()[:50 + dist + 100])
    if has_a:
        body[50:50 + len(A)] = A
    if has_b:
        body[50 + dist:50 + dist + len(B)] = B
    return case("seam", head + bytes(body) + tail, FS, ABC, S=S, big=(S, len(body)), dist=dist, c_left=(S - 5 - len(C), 4 + len(C)), c_right=(S + len(body) + 1, 1 + len(C)))


@_once
def seam_turns(has_c, has_a):
    """the same long record with C 8,192 and A 16,384 bytes behind position 50: under NONMONO its selection is decided two tiles (at
    staging 2 * FS: sixteen passes) behind its first bytes, and differs from what it was when they were copied"""
    rng = np.random.RandomState(77)
    head = lines(rng, 300)[:-1] + b"\nxx" + C + b"yy\n"
    S = len(head)
    body = bytearray(filler()[:50 + 16384 + 100])
    if has_c:
        body[50 + 8192:50 + 8192 + len(C)] = C
    if has_a:
        body[50 + 16384:50 + 16384 + len(A)] = A
    tail = b"\nq" + C + b"\n" + lines(rng, 200, b"abc") + b"\n" + A + b"\nlast"
    return case("seam_turns", head + bytes(body) + tail, FS, ABC, S=S, big=(S, len(body)))


# ---- 3
@_once
def one_trip():
    """Records of 3 .. 10 bytes: a trip of 64 lanes holds six to sixteen delimiters. In the first half (letters a and b, both one-byte
    patterns) every position hits: the segmented scan. In the second half (eight letters, four two-byte patterns over two of them) a
    trip has a handful of hits: the per-pattern ballots. 12 random clause lists."""
    rng = np.random.RandomState(3)
    out = bytearray()
    half = 10 << 10
    while len(out) < 2 * half:
        alphabet = b"ab" if len(out) < half else b"cduvwxyz"
        out += bytes(rng.choice(list(alphabet), size=int(rng.randint(3, 11))).astype(np.uint8)) + b"\n"
    pats = [b"a", b"b", b"ab", b"ba", b"cc", b"cd", b"dc", b"dd"]
    return case("one_trip", out, FS, pats, half=half, wheres=[random_clauses(rng, len(pats), 4) for _ in range(12)])


# ---- 4
@_once
def wide():
    """40 KiB of lines over a..h and 64 patterns of 2 .. 4 bytes; ranges that cut records, an empty one and one of one byte"""
    rng = np.random.RandomState(64)
    data = lines(rng, 40 << 10, b"abcdefgh", 60)
    pats = []
    while len(pats) < 64:
        p = bytes(rng.choice(list(b"abcdefgh"), size=int(rng.randint(2, 5))).astype(np.uint8))
        if p not in pats:
            pats.append(p)
    nl = [p for p in range(len(data)) if data[p] == NL]
    cut = [p for p in nl if data[p + 1:p + 2] != b"\n" and data[p - 1:p] != b"\n"]
    ranges = [(0, None), (cut[3] + 5, cut[-3] - 4), (cut[40] - 3, cut[300] + 1), (9000, 9100), (cut[7] + 2, cut[7] + 2), (cut[9] + 3, cut[9] + 4)]
    return case("wide", data, 4096, pats, ranges=ranges, wheres=[random_clauses(rng, 64) for _ in range(10)])


# ---- 6
LANES_WHERE = ([(0b0011, 0, 0b0100), (0, 0b1000, 0b0100)], [(0, 0, 0b0100), (0b0101, 0, 0)])   # over [A, B, C, D]; the second is NONMONO


@_once
def lanes():
    """1,030 tiles in one pass: a lane of the one-workgroup scan walks two tiles. Three stretches without a delimiter:
    three whole tiles (A at the head, B at the tail: selected by all = {A, B}), four whole tiles (C at the head, A at the tail: under
    NONMONO unselected, then selected), and a record across a workgroup's whole group of 8 tiles with C alone. D is a two-byte
    pattern of the ordinary lines."""
    U = 1029 * TILE + 5000
    rng = np.random.RandomState(66)
    a = rng.randint(32, 127, size=U).astype(np.uint8)
    a[rng.randint(0, U, size=U // 200)] = NL
    stretches = []
    for start, tiles, first, last in ((300 * TILE - 700, 3, A, B), (601 * TILE - 100, 4, C, A), (800 * TILE - 3000, 8, C, None)):
        end = start + (tiles + 1) * TILE + 1500                                 # (the record, without its delimiters)
        seg = a[start:end]
        seg[seg == NL] = 32
        a[start - 1] = a[end] = NL
        a[start + 20:start + 20 + len(first)] = np.frombuffer(first, dtype=np.uint8)
        if last:
            a[end - 40:end - 40 + len(last)] = np.frombuffer(last, dtype=np.uint8)
        stretches.append((start, end - start))
    data = a.tobytes()
    D = data[123456:123458]
    assert NL not in D
    return case("lanes", data, 65536, [A, B, C, D], stretches=stretches)


# ---- 7
@_once
def delimiters(kind):
    """Three tiles and a bit over a b c d z. `last`: delimiters at the last lane of a trip, a wave and a tile (63, 2,047, 8,191), at the
    first byte, and the content ends with one. `first`: at the first lane of the next (64, 2,048, 8,192), none at byte 0, and the
    content ends without one. `both`: at all six, two delimiters side by side. `only`: delimiters only. `none`: not one."""
    rng = np.random.RandomState(7)
    U = 3 * TILE + 777
    a = rng.choice(list(b"abcdz"), size=U).astype(np.uint8)
    spots = {"last": [0, 63, 2047, 8191, TILE + 63, TILE + 2047, 2 * TILE - 1, U - 1], "first": [64, 2048, 8192, TILE + 64, TILE + 2048, 2 * TILE],
             "both": [0, 63, 64, 2047, 2048, 8191, 8192, 2 * TILE - 1, 2 * TILE, U - 1], "only": list(range(U)), "none": []}[kind]
    if kind in ("last", "first", "both"):
        a[rng.randint(0, U, size=U // 40)] = NL
        for p in (0, 63, 64, 2047, 2048, 8191, 8192, TILE + 63, TILE + 64, TILE + 2047, TILE + 2048, 2 * TILE - 1, 2 * TILE, U - 1):
            if a[p] == NL:
                a[p] = ord("z")
    a[spots] = NL
    return case("delimiters_" + kind, a.tobytes(), FS, [b"ab", b"cd", b"zz"], spots=spots)


DELIM_WHERE = ([(0b001, 0, 0b010)], [(0b011, 0, 0), (0, 0, 0b111)])


# ---- 9
@_once
def expressions():
    """log lines for the expressions error (any case), status=5xx and id=....: tests/test_gpu_grep_where.py's sixth case"""
    rng = np.random.RandomState(6)
    words = [b"error", b"ERROR", b"Error", b"warn", b"info"]
    out = []
    for _ in range(400):
        out.append(b"%s status=%d id=%s %s" % (words[rng.randint(5)], rng.choice([200, 404, 500, 503, 5, 50]),
                                               bytes(rng.choice(list(b"abxyz0123"), size=rng.randint(2, 6)).astype(np.uint8)), b"x" * int(rng.randint(0, 20))))
    return case("expressions", b"\n".join(out)[:16 << 10], FS, [b"error", b"status=5[0-9][0-9]", b"id=...."])
