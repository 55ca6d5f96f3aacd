"""The yardstick of the diff tests: the patch of ZraHipDiffArchives (include/zra_hip.h), computed on the CPU from the two plaintexts a
test generated itself."""
import numpy as np


def _dirty(a, b, fs, grain):
    """(dirty positions of [0, len(a)) as a bool array, number of dirty grains): frame f is cut into grains counted from its own
    first byte, clipped to the frame and to len(a); a grain with a differing position is dirty as a whole."""
    c = len(a)
    x = np.frombuffer(bytes(a), dtype=np.uint8) != np.frombuffer(bytes(b[:c]), dtype=np.uint8)
    d = np.zeros(c, dtype=bool)
    grains = 0
    for lo in range(0, c, fs):
        hi = min(c, lo + fs)
        for g in range(lo, hi, grain):
            if x[g:min(g + grain, hi)].any():
                d[g:min(g + grain, hi)] = True
                grains += 1
    return d, grains


def patch(a, b, fs, grain=1):
    """(writes, data, append_offset, append_size) that turn content a into content b (len(b) >= len(a)): writes = the ascending
    [(offset, size)] of the maximal runs of dirty positions, data = b's bytes of those runs, packed, then b[len(a):]."""
    assert len(b) >= len(a)
    d, _ = _dirty(a, b, fs, grain)
    edge = np.diff(np.concatenate(([0], d.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    writes = [(int(s), int(e - s)) for s, e in zip(starts, ends)]
    packed = np.frombuffer(bytes(b[:len(a)]), dtype=np.uint8)[d].tobytes()
    return writes, packed + bytes(b[len(a):]), len(packed), len(b) - len(a)


def apply(a, writes, data, append_offset, append_size):
    """content a with the patch applied as ZraHipUpdateArchive applies it: write i replaces its bytes by data at the sum of the sizes
    in front of it, and data[append_offset : append_offset + append_size] is added at the end."""
    out, at = bytearray(a), 0
    for off, n in writes:
        out[off:off + n] = data[at:at + n]
        at += n
    return bytes(out) + bytes(data[append_offset:append_offset + append_size])


def stats(a, b, fs, grain=1, decoded=None, slots=None, tail_slots=None):
    """What ZraHipGetDiffStats reports for that diff when the frames `decoded` (a set of frame indices; None: every frame of [0, C))
    are the pairs that are decoded, with `slots` frame pairs per pair pass and `tail_slots` frames per tail pass (None: one pass)."""
    c = len(a)
    n = -(-c // fs)
    tail = -(-len(b) // fs) - c // fs if len(b) > c else 0
    w, _, dirty, _ = patch(a, b, fs, grain)
    dec = n if decoded is None else len([f for f in range(n) if f in decoded])
    passes = (0 if n == 0 else 1 if slots is None else -(-n // slots)) + (0 if tail == 0 else 1 if tail_slots is None else -(-tail // tail_slots))
    return dict(frames=n, equal_compressed=n - dec, decoded=dec, tail_decoded=tail, writes=len(w), dirty_bytes=dirty, passes=passes,
                dirty_grains=_dirty(a, b, fs, grain)[1])
