"""The yardstick of the compare tests: the differing ranges of ZraHipCompareArchives (include/zra_hip.h), computed on the CPU from the
two plaintexts a test generated itself."""
import numpy as np


def ranges(a, b, lo=0, hi=None):
    """The ascending list of (offset, size) of the maximal runs [s, e) inside [lo, hi) with a[p] != b[p] for every p in them; hi None
    (or beyond it): the end of the shorter of the two."""
    c = min(len(a), len(b))
    hi = c if hi is None else min(hi, c)
    if hi <= lo:
        return []
    x = np.frombuffer(bytes(a[lo:hi]), dtype=np.uint8) != np.frombuffer(bytes(b[lo:hi]), dtype=np.uint8)
    edge = np.diff(np.concatenate(([0], x.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    return [(lo + int(s), int(e - s)) for s, e in zip(starts, ends)]


def stats(a, b, fs, lo=0, hi=None, decoded=None, slots=None, cap=1 << 16):
    """What ZraHipGetCompareStats reports for that compare when the frames `decoded` (a set of frame indices; None: every frame of the
    range) are the ones that are decoded, with `slots` frames per pass (None: one pass)."""
    c = min(len(a), len(b))
    hi = c if hi is None else hi
    r = ranges(a, b, lo, hi)
    if hi <= lo:
        return dict(frames=0, equal_compressed=0, decoded=0, content_bytes=0, ranges=0, listed=0, passes=0)
    f0, f1 = lo // fs, (hi - 1) // fs
    n = f1 - f0 + 1
    dec = [f for f in range(f0, f1 + 1) if decoded is None or f in decoded]
    nbytes = sum(min(hi, (f + 1) * fs) - max(lo, f * fs) for f in dec)
    return dict(frames=n, equal_compressed=n - len(dec), decoded=len(dec), content_bytes=nbytes, ranges=len(r), listed=min(len(r), cap),
                passes=1 if slots is None else -(-n // slots))
