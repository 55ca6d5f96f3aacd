"""The inputs of tests/test_gpu_cut.py, generated here by fixed seeds so that a CPU test (tests/test_cut_abi.py) can hold them to the
seams they are built for without a GPU. A case is a dict: name, data, fs (the archive's frame size), pats, sep, and what its test needs
beside them; model() answers a call of a case from tests/cut_model.py, once per argument set. Positions are content offsets: with
lo = 0 a pass of the whole range has its trips, waves, tiles and workgroups at multiples of 64, 2,048, 8,192 and 65,536."""
import numpy as np

import cut_model as CM

NL = 10
COMMA = 0x2C
FS = 1024
TRIP, WAVE, TILE, GROUP = 64, 2048, 8192, 65536
SEAMS = (TRIP, WAVE, TILE, GROUP)
NEEDLE = b"ERR"
ALL = (1 << 64) - 1


def bits(*fields):
    m = 0
    for j in fields:
        m |= 1 << (min(j, 64) - 1)
    return m


def case(name, data, fs, pats, sep=COMMA, **more):
    return dict(name=name, data=bytes(data), fs=fs, pats=pats, sep=sep, _memo={}, **more)


def model(c, mask, inv=False, lo=0, hi=None, pats=None, syntax=0):
    key = (mask, inv, lo, hi, None if pats is None else tuple(pats), syntax)
    if key not in c["_memo"]:
        c["_memo"][key] = CM.cut(c["data"], c["pats"] if pats is None else pats, c["sep"], mask, NL, inv, lo, hi, syntax)
    return c["_memo"][key]


# ---- 1
TINY_MASKS = [bits(1), bits(2), bits(1, 3), bits(2, 4), ALL, bits(64)]


def frame_size_4():
    """Frames of 4 bytes: with one slot of staging every record and most fields cross passes. `late` holds its only match in its last
    field: it is copied provisionally by many passes and selected passes later. `dropped` holds none and is followed by a selected
    record, whose kept bytes land where dropped's lay."""
    late = b"late,one,two,three,four,five,six," + NEEDLE
    dropped = b"dropped,alpha,beta,gamma,delta,epsilon,zeta"
    lines = [b"a,b,c,d", b"x" + NEEDLE + b",y", b"", b",,", late, b"n,o", dropped, b"k," + NEEDLE + b",m,,q", b"plain", b",x,,y", b"tail," + NEEDLE + b",no,newline"]
    data = b"\n".join(lines)
    at = {ln: data.index(ln) for ln in (late, dropped)}
    return case("fs4", data, 4, [NEEDLE], late=(at[late], len(late)), dropped=(at[dropped], len(dropped)),
                after_dropped=(at[dropped] + len(dropped) + 1, len(lines[7])))


# ---- 2
def _tail(rng, n=6):
    """a few short records behind the one a case is about, some with the needle"""
    out = []
    for k in range(n):
        f = [bytes(rng.randint(97, 123, size=rng.randint(0, 6)).astype(np.uint8)) for _ in range(rng.randint(1, 6))]
        if k % 2 == 0:
            f[rng.randint(len(f))] += NEEDLE
        out.append(b",".join(f))
    return b"\n".join(out) + b"\n"


def seam_separator(B, side):
    """One record from offset 0 with a separator at P = B - 1 + side: ',' 'x' * (P - 1) ',' ',' 'z' * 9 NEEDLE. Under fields {1, 3} the
    separator at P is the record's only kept byte (field 1 and field 3 are empty, the separator in front of field 3 is kept because field
    1 is chosen); under fields {1, 2, 4} it is the only dropped one (field 3 is not chosen, every other byte's field is)."""
    P = B - 1 + side
    rec = b"," + b"x" * (P - 1) + b",," + b"z" * 9 + NEEDLE
    assert rec[P] == COMMA and rec[P - 1] != COMMA
    data = rec + b"\n" + _tail(np.random.RandomState(B + side))
    return case("seam_sep_%d_%d" % (B, side), data, FS, [NEEDLE], P=P, big=(0, len(rec)), only_kept=bits(1, 3), only_dropped=bits(1, 2, 4))


def seam_field(B, side):
    """One record from offset 0 whose field 2 is the single byte 'F' at P = B - 1 + side: 'x' * (P - 1) ',' 'F' ',' 'z' * 9 NEEDLE. Under
    fields {2} that byte is the only kept one; under every field but 2 it is dropped, with the separator in front of it."""
    P = B - 1 + side
    rec = b"x" * (P - 1) + b",F," + b"z" * 9 + NEEDLE
    assert rec[P] == 0x46
    data = rec + b"\n" + _tail(np.random.RandomState(B + side + 7))
    return case("seam_field_%d_%d" % (B, side), data, FS, [NEEDLE], P=P, big=(0, len(rec)), only_kept=bits(2), only_dropped=ALL & ~bits(2))


def three_tiles(k):
    """Short records, then one record that gathers k separators in its first tile, runs across a whole tile with neither separator nor
    delimiter and ends, behind three more separators, in a third."""
    rng = np.random.RandomState(k)
    head = _tail(rng, 4)
    first = b",".join([b"f%d" % j for j in range(k)]) + b","                  # k separators, all inside tile 0
    assert len(head) + len(first) < TILE
    body = b"y" * (2 * TILE + 100 - len(head) - len(first))                     # field k + 1 reaches into tile 2
    rec = first + body + b",p,q" + NEEDLE + b",r"
    data = head + rec + b"\n" + _tail(rng)
    return case("three_tiles_%d" % k, data, FS, [NEEDLE], big=(len(head), len(rec)), k=k,
                masks=[bits(k + 1), bits(k + 2), bits(k, k + 2), bits(1, k + 4), ALL & ~bits(k + 1)])


# ---- 3
SAT_COUNTS = (62, 63, 64, 65, 130)
SAT_MASKS = [1 << 62, 1 << 63, (1 << 62) | (1 << 63), 1 | (1 << 63)]


def saturation():
    """records with 62, 63, 64, 65 and 130 separators: fields 63, 64 and the ones bit 63 stands for"""
    lines = []
    for n in SAT_COUNTS:
        lines.append(b",".join(b"%d" % (j % 10) for j in range(n + 1)) + NEEDLE)
        lines.append(b"," * n)
        lines.append(b",".join(b"ab" for j in range(n + 1)))
    return case("saturation", b"\n".join(lines) + b"\n", FS, [NEEDLE])


def saturation_at(B, field):
    """field `field` (64 or 65) of one record from offset 0 starts exactly at position B: field 1 is padded so that separator
    field - 1 is the byte at B - 1"""
    small = b"".join(b",%d" % (j % 10) for j in range(2, field))               # fields 2 .. field - 1 with their separators
    pad = B - 1 - len(small)
    rec = b"p" * pad + small + b"," + b"G" + b",H,I" + NEEDLE
    assert rec[B - 1] == COMMA and rec[B] == 0x47 and rec[:B].count(b",") == field - 1
    data = rec + b"\n" + _tail(np.random.RandomState(B + field))
    return case("sat_%d_%d" % (B, field), data, FS, [NEEDLE], big=(0, len(rec)))


# ---- 4
def degenerate(kind):
    rng = np.random.RandomState(3)
    if kind == "separators":
        data = b"\n".join(b"," * int(n) for n in rng.randint(0, 200, size=40)) + b"\n"
    elif kind == "no_separator":
        data = b"\n".join(bytes(rng.randint(97, 123, size=int(n)).astype(np.uint8)) + (NEEDLE if n % 3 == 0 else b"") for n in rng.randint(0, 300, size=40))
    elif kind == "empty_records":
        data = b"\n\n\n,\n\n" + NEEDLE + b"\n\n,,\n\n\n" + b"a,b\n" + b"\n" * 70 + NEEDLE + b",x\n\n"
    elif kind == "delimiters":
        data = b"\n" * 2500
    else:
        data = b"one,single" + NEEDLE + b",record," + b"w" * 3000 + b",without,a,final,delimiter"
    return case("degenerate_" + kind, data, FS, [NEEDLE])


# ---- 5, 7, 9: CSV-like lines
def csv_lines(seed, size, lo_fields=3, hi_fields=12, every=3):
    rng = np.random.RandomState(seed)
    out = bytearray()
    k = 0
    while len(out) < size:
        f = [bytes(rng.randint(97, 123, size=rng.randint(0, 9)).astype(np.uint8)) for _ in range(rng.randint(lo_fields, hi_fields + 1))]
        if k % every == 0:
            f[rng.randint(len(f))] += NEEDLE
        out += b",".join(f) + b"\n"
        k += 1
    return bytes(out[:size])


def log_lines(seed, size):
    """log-like lines cut at spaces: a date, a time, a level, a component, a message of several words"""
    rng = np.random.RandomState(seed)
    levels = [b"INFO", b"WARN", b"ERROR", b"DEBUG"]
    words = [b"request", b"took", b"ms", b"user", b"id", b"failed", b"ok", b"retry", b"cache", b"miss"]
    out = bytearray()
    while len(out) < size:
        msg = b" ".join(words[i] for i in rng.randint(0, len(words), size=rng.randint(1, 9)))
        out += b"2026-10-%02d %02d:%02d:%02d %s svc%d %s\n" % (rng.randint(1, 29), rng.randint(24), rng.randint(60), rng.randint(60), levels[rng.randint(4)],
                                                              rng.randint(9), msg)
    return bytes(out[:size])


def table():
    """20 KiB of CSV-like lines in frames of 1,024 bytes: the ranges, the capacities, the handle"""
    return case("table", csv_lines(11, 20 * FS + 300), FS, [NEEDLE, b"qz"])


def expressions():
    data = csv_lines(5, 12 * FS).replace(b"ERR", b"eRr", 40).replace(b"ERR", b"Err", 40)
    return case("expressions", data, FS, [b"err"], fold=[b"err"], classes=[b"[Ee][Rr]R", b",[a-c][a-c],"])


# ---- 11
SWEEP_SEEDS = range(6)


def sweep(seed):
    """(case, [(mask, lo, hi, staging)]): CSV-like or log-like text, at most 1 MiB, with random masks, ranges and a staging window
    that gives at least 3 passes"""
    rng = np.random.RandomState(100 + seed)
    fs = (4096, 16384)[seed & 1]
    size = int(rng.randint(40 * fs, 60 * fs))
    if seed % 2 == 0:
        c = case("sweep_csv_%d" % seed, csv_lines(seed, size), fs, [NEEDLE])
        nf = 12
    else:
        c = case("sweep_log_%d" % seed, log_lines(seed, size), fs, [b"ERROR", b"failed"], sep=0x20)
        nf = 14
    calls = []
    for k in range(3):
        mask = 0
        for j in rng.choice(np.arange(1, nf + 1), size=rng.randint(1, 5), replace=False):
            mask |= 1 << (int(j) - 1)
        if k == 2:
            mask |= 1 << 63                                                    # cut's `64-`: nothing on these lines, chosen all the same
        lo = int(rng.randint(0, size // 4))
        hi = int(rng.randint(3 * size // 4, size + 1))
        slots = max(1, -(-(hi - lo) // fs) // int(rng.randint(3, 7)))
        calls.append((mask, lo, hi, slots * fs))
    return c, calls
