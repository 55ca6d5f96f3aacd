"""The yardstick of the signature tests: XXH64 with a seed in pure Python (cross-checked against the oracle's zo_xxh64 in
tests/test_sign_abi.py), the signature ZraHipSignArchive writes (include/zra_hip.h), computed from an archive's bytes and the plaintext
the test generated itself, and the signature diff as "a grain is dirty when its words differ". No GPU, no library."""
import struct

import numpy as np

M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, x):
    return (_rotl((acc + x * P2) & M64, 31) * P1) & M64


def _merge(h, v):
    return (((h ^ _round(0, v)) * P1) + P4) & M64


def xxh64(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed & M64, (seed - P1) & M64]
        stripes = n // 32
        if stripes >= 64:                                                      # long inputs: the four lanes as numpy columns
            w = np.frombuffer(data, dtype="<u8", count=4 * stripes).reshape(stripes, 4)
            for row in w.tolist():
                v = [_round(v[k], row[k]) for k in range(4)]
        else:
            for s in range(stripes):
                x = struct.unpack_from("<4Q", data, 32 * s)
                v = [_round(v[k], x[k]) for k in range(4)]
        p = 32 * stripes
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for k in range(4):
            h = _merge(h, v[k])
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27) * P1 + P4) & M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ ((struct.unpack_from("<I", data, p)[0] * P1) & M64), 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h = (_rotl(h ^ ((data[p] * P5) & M64), 11) * P1) & M64
        p += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    h ^= h >> 32
    return h


def gpf(fs, grain):
    return -(-fs // grain)


def words(content_size, fs, grain):
    return -(-content_size // fs) * (1 + gpf(fs, grain))


def grain_words(plaintext, fs, grain, seed=0):
    """[[grain words of frame f]]: gpf words per frame, grains counted from the frame's first byte and clipped to the frame and to the
    content; 0 for a grain without a byte."""
    out = []
    for lo in range(0, len(plaintext), fs):
        hi = min(len(plaintext), lo + fs)
        out.append([xxh64(plaintext[g:min(g + grain, hi)], seed) if g < hi else 0 for g in range(lo, lo + gpf(fs, grain) * grain, grain)])
    return out


def signature(arc_bytes, plaintext, fs, grain, seed=0):
    """The words of the signature as a flat list: per frame the XXH64 of its compressed bytes (the archive's own seek-table span),
    then its grain words."""
    hs = int.from_bytes(arc_bytes[4:8], "little") + 8
    t = 38 + int.from_bytes(arc_bytes[34:38], "little")
    F = -(-len(plaintext) // fs)
    e = [int.from_bytes(arc_bytes[t + 5 * i:t + 5 * i + 5], "little") for i in range(F + 1)]
    out = []
    for f, gw in enumerate(grain_words(plaintext, fs, grain, seed)):
        out.append(xxh64(arc_bytes[hs + e[f]:hs + e[f + 1]], seed))
        out += gw
    assert len(out) == words(len(plaintext), fs, grain)
    return out


def patch(grains_a, a_len, b, fs, grain, seed=0):
    """diff_model.patch's (writes, data, append_offset, append_size) from A's grain words alone (grain_words of A, a_len = A's content
    size) and B's plaintext: a grain is dirty when its word differs from the word of B's bytes of the same clipped grain."""
    assert len(b) >= a_len
    gb = grain_words(b[:a_len], fs, grain, seed)
    d = np.zeros(a_len, dtype=bool)
    for f, (wa, wb) in enumerate(zip(grains_a, gb)):
        for g, (x, y) in enumerate(zip(wa, wb)):
            if x != y:
                lo = f * fs + g * grain
                d[lo:min(lo + grain, (f + 1) * fs, a_len)] = True
    edge = np.diff(np.concatenate(([0], d.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    packed = np.frombuffer(bytes(b[:a_len]), dtype=np.uint8)[d].tobytes()
    return [(int(s), int(e - s)) for s, e in zip(starts, ends)], packed + bytes(b[a_len:]), len(packed), len(b) - a_len
