"""The inputs of tests/test_gpu_tally.py, generated here by fixed seeds so that a CPU test (tests/test_tally_abi.py) can hold them to
the seams they are built for without a GPU. A shape is a dict: name, text, and what its test needs beside them. T is the tally
kernels' tile: a workgroup takes the records that START among T consecutive positions of the text, so the seams are at T - 1, T and
T + 1; MAX_KEY is the longest record that is a key."""
import numpy as np

import tally_model as TM

NL = 10
T = 4096
MAX_KEY = TM.MAX_KEY


def shape(name, text, **more):
    return dict(name=name, text=bytes(text), **more)


def _filler(rng, size, lo=3, hi=12):
    """lower-case records of lo .. hi bytes, each with its delimiter, exactly `size` bytes in all (the last one may be shorter)"""
    out = bytearray()
    while len(out) < size:
        left = size - len(out)
        n = left - 1 if left <= hi + 1 else int(rng.randint(lo, hi + 1))
        out += bytes(rng.randint(97, 123, size=n).astype(np.uint8)) + b"\n"
    assert len(out) == size
    return bytes(out)


# ---- degenerate text
DEGENERATE = ("one_with", "one_without", "delimiters", "one_byte", "one_delimiter", "tile", "tile_plus_1")


def degenerate(kind):
    rng = np.random.RandomState(3)
    text = {"one_with": b"status=200\n", "one_without": b"status=200", "delimiters": b"\n" * 7, "one_byte": b"x", "one_delimiter": b"\n"}.get(kind)
    if kind == "tile":
        text = _filler(rng, T)
    if kind == "tile_plus_1":
        text = _filler(rng, T) + b"z"
    return shape("degenerate_" + kind, text)


# ---- tile seams
SEAMS = ("straddle", "bare_tile", "delimiter_last", "delimiter_first", "mirror")


def seam(kind):
    rng = np.random.RandomState(5)
    if kind == "straddle":                                                     # starts at T - 3, ends at T + 5; once more in tile 1
        big = b"STRADDLE"
        return shape("seam_straddle", _filler(rng, T - 3) + big + b"\n" + _filler(rng, 200) + big + b"\n", big=(T - 3, len(big)))
    if kind == "bare_tile":                                                    # starts at T - 10, covers tile 1, ends in tile 2: longer than MAX_KEY
        n = T + 30
        return shape("seam_bare_tile", _filler(rng, T - 10) + b"B" * n + b"\n" + _filler(rng, 300), big=(T - 10, n))
    if kind == "delimiter_last":                                               # a delimiter at T - 1: a record starts at T
        return shape("seam_delimiter_last", _filler(rng, T) + b"FIRSTOFTILE\n" + _filler(rng, 100), big=(T, 11))
    if kind == "delimiter_first":                                              # a delimiter at T: the record in front ends at the seam, the next starts at T + 1
        return shape("seam_delimiter_first", _filler(rng, T - 6) + b"ENDSAT\n" + b"NEXT\n" + _filler(rng, 100), big=(T - 6, 6))
    if kind == "mirror":                                                       # the first occurrence in tile 0, three repeats in tiles 1, 2 and 3
        key = b"MIRRORED\n"
        parts = [_filler(rng, 1000) + key + _filler(rng, T - 1000 - len(key))]
        for at in (17, T - len(key), 2000):
            parts.append(_filler(rng, at) + key + _filler(rng, T - at - len(key)))
        return shape("seam_mirror", b"".join(parts), big=(1000, len(key) - 1), repeats=[T + 17, 3 * T - len(key), 3 * T + 2000])
    raise KeyError(kind)


# ---- key length
KEY_LENGTHS = ("sizes", "last_byte", "first_byte", "prefix")


def key_length(kind):
    rng = np.random.RandomState(7)
    body = bytes(rng.randint(97, 123, size=MAX_KEY + 1).astype(np.uint8))
    if kind == "sizes":                                                        # MAX_KEY - 1, MAX_KEY, MAX_KEY + 1 (skipped), each twice
        recs = [body[:MAX_KEY - 1], body[:MAX_KEY], body, b"short", body[:MAX_KEY], body, body[:MAX_KEY - 1]]
    elif kind == "last_byte":
        recs = [body[:MAX_KEY - 1] + b"A", body[:MAX_KEY - 1] + b"B", body[:MAX_KEY - 1] + b"A"]
    elif kind == "first_byte":
        recs = [b"A" + body[:MAX_KEY - 1], b"B" + body[:MAX_KEY - 1], b"B" + body[:MAX_KEY - 1]]
    else:                                                                      # a key that is a proper prefix of another, and the empty key
        recs = [b"abcd", b"abc", b"", b"abcd", b"ab", b"abc", b"", b"abcde"]
    return shape("key_length_" + kind, b"".join(r + b"\n" for r in recs), recs=recs)


# ---- skew
SKEWS = ("one", "three", "distinct")
SKEW_RECORDS = 50000


def skew(kind):
    rng = np.random.RandomState(9)
    if kind == "one":
        recs = [b"200"] * SKEW_RECORDS
    elif kind == "three":                                                      # 98 / 1.9 / 0.1 %
        pick = rng.choice(3, size=SKEW_RECORDS, p=[0.98, 0.019, 0.001])
        recs = [(b"200", b"404", b"500")[i] for i in pick]
    else:
        recs = [b"req-%06d" % i for i in rng.permutation(SKEW_RECORDS)]
    return shape("skew_" + kind, b"".join(r + b"\n" for r in recs), n=SKEW_RECORDS)


# ---- collisions, determinism
def collisions(seed=21, keys=300):
    """300 distinct keys of mixed lengths (1 .. 40 bytes, every tenth 500 .. 700), each 1 to 5 times, shuffled; no final delimiter"""
    rng = np.random.RandomState(seed)
    distinct = set()
    while len(distinct) < keys:
        n = int(rng.randint(500, 701)) if len(distinct) % 10 == 9 else int(rng.randint(1, 41))
        distinct.add(bytes(rng.randint(48, 123, size=n).astype(np.uint8)))
    recs = [k for k in sorted(distinct) for _ in range(int(rng.randint(1, 6)))]
    rng.shuffle(recs)
    return shape("collisions", b"\n".join(recs), keys=keys)


# ---- maxDistinct
def promised(D=200):
    rng = np.random.RandomState(23)
    recs = [b"key%03d" % i for i in range(D)] * 3
    rng.shuffle(recs)
    return shape("promised", b"".join(r + b"\n" for r in recs), D=D)
