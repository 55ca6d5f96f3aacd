"""Pure-Python model of the STRUCTURE stage of ZraHipVerifyArchive, written from the table of causes and codes in include/zra_hip.h
(not from the kernel), plus the small archive-editing helpers the verify tests share. No GPU, no library."""
import zlib

STRUCTURE, CONTENT = 1, 2


def fields(arc):
    """(header size, table offset, frames, frame size, uncompressed size) of an archive"""
    hs = int.from_bytes(arc[4:8], "little") + 8
    ts = int.from_bytes(arc[26:30], "little")
    meta = int.from_bytes(arc[34:38], "little")
    return hs, 38 + meta, max(ts - 1, 0), int.from_bytes(arc[30:34], "little"), int.from_bytes(arc[18:26], "little")


def entries(arc):
    hs, t, F, fs, U = fields(arc)
    return [int.from_bytes(arc[t + 5 * i:t + 5 * i + 5], "little") for i in range(F + 1)]


def fix_crc(arc):
    """the archive with the header CRC-32 recomputed: CRC over [0, 14) || [18, header size)"""
    a = bytearray(arc)
    hs = int.from_bytes(a[4:8], "little") + 8
    a[14:18] = zlib.crc32(bytes(a[18:hs]), zlib.crc32(bytes(a[0:14]))).to_bytes(4, "little")
    return bytes(a)


def crc_ok(arc):
    return fix_crc(arc) == bytes(arc)


def set_entry(arc, k, v):
    a = bytearray(arc)
    t = fields(arc)[1]
    a[t + 5 * k:t + 5 * k + 5] = int(v).to_bytes(5, "little")
    return fix_crc(a)


def with_fcs(arc, f, value):
    """the archive with a 4-byte Frame_Content_Size field of `value` put into the header of frame f, which has none (the encoder
    writes frames without one): descriptor flag set, 4 bytes inserted, the table entries behind the frame moved, the CRC-32 redone"""
    hs, t, F, fs, U = fields(arc)
    e = entries(arc)
    fr = bytearray(arc[hs + e[f]:hs + e[f + 1]])
    assert fr[4] >> 6 == 0 and not (fr[4] >> 5) & 1 and fr[4] & 3 == 0
    fr[4] |= 0x80
    fr[6:6] = int(value).to_bytes(4, "little")
    a = bytearray(arc[:hs + e[f]] + bytes(fr) + arc[hs + e[f + 1]:])
    for k in range(f + 1, F + 1):
        a[t + 5 * k:t + 5 * k + 5] = (e[k] + 4).to_bytes(5, "little")
    return fix_crc(a)


def header_layout(frame):
    """(frame header size, offset of the Frame_Content_Size field, its size) of a zstd frame"""
    fhd = frame[4]
    did, ss, fcs = fhd & 3, (fhd >> 5) & 1, fhd >> 6
    did_size = 4 if did == 3 else did
    fcs_size = (ss, 2, 4, 8)[fcs]
    return 5 + (0 if ss else 1) + did_size + fcs_size, 5 + (0 if ss else 1) + did_size, fcs_size


def block_headers(frame):
    """offsets of the block headers of a sound frame"""
    pos, out = header_layout(frame)[0], []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        out.append(pos)
        pos += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
        if bh & 1:
            return out


def frame_code(arc, f):
    """the code of frame f by the table of zra_hip.h, 0 if it is sound"""
    hs, t, F, fs, U = fields(arc)
    e = entries(arc)
    body = arc[hs:]
    a, b = e[f], e[f + 1]
    if b < a or b > len(body):
        return 72
    if f + 1 == F and b != len(body):
        return 72
    n = b - a
    if n < 9 or n >= 1 << 32:
        return 72
    p = body[a:b]
    fhd = p[4]
    did, ss = fhd & 3, (fhd >> 5) & 1
    hsz, fcs_at, fcs_size = header_layout(p)
    if n < hsz + 3:
        return 72
    if int.from_bytes(p[0:4], "little") != 0xFD2FB528:
        return 10
    if fhd & 8:
        return 14
    if not ss and 10 + (p[5] >> 3) > 31:
        return 16
    did_size = 4 if did == 3 else did
    if did_size and int.from_bytes(p[fcs_at - did_size:fcs_at], "little"):
        return 32
    if fcs_size:
        v = int.from_bytes(p[fcs_at:fcs_at + fcs_size], "little") + (256 if fcs_size == 2 else 0)
        expect = 0 if f * fs >= U else min(fs, U - f * fs)
        if v > expect:
            return 70
        if v < expect:
            return 20
    pos = hsz
    while True:
        if n - pos < 3:
            return 72
        bh = int.from_bytes(p[pos:pos + 3], "little")
        pos += 3
        btype = (bh >> 1) & 3
        if btype == 3:
            return 20
        payload = 1 if btype == 1 else bh >> 3
        if payload > n - pos:
            return 72
        pos += payload
        if bh & 1:
            break
    if fhd & 4:
        pos += 4
    return 0 if pos == n else 72


def structure_faults(arc, first=0, count=None):
    """{frame: code} of the faulty frames of [first, first + count)"""
    F = fields(arc)[2]
    last = F if count is None else first + count
    return {f: c for f in range(first, last) for c in [frame_code(arc, f)] if c}
