"""The yardstick of the record-index tests (include/zra_hip.h: ZraHipIndexRecords, ZraHipLocateRecords, ZraHipReadRecords), computed
on the CPU from the plaintext a test generated itself, straight from the definitions: the delimiters t_0 < ... < t_(D-1) are the
positions whose byte equals the delimiter; record k < D is [s_k, t_k) with s_0 = 0 and s_k = t_(k-1) + 1; record D is [s_D, U) iff
s_D < U."""
BIT63 = 1 << 63


def delimiters(plain, delim):
    return [i for i, b in enumerate(bytes(plain)) if b == delim]


def counts(plain, delim):
    """(D, R)"""
    t = delimiters(plain, delim)
    s_d = t[-1] + 1 if t else 0
    return len(t), len(t) + (1 if s_d < len(plain) else 0)


def index_words(plain, fs, delim):
    """One word per frame of fs bytes: bits 0..62 the delimiter bytes of the frame, bit 63 set iff its last byte is not the delimiter."""
    plain = bytes(plain)
    out = []
    for lo in range(0, len(plain), fs):
        frame = plain[lo:lo + fs]
        out.append(sum(1 for b in frame if b == delim) | (BIT63 if frame[-1] != delim else 0))
    return out


def locate(plain, delim, numbers):
    """[(s_r, n_r)] for r in numbers; None for the whole list when a number is >= R"""
    plain = bytes(plain)
    t = delimiters(plain, delim)
    D, R = counts(plain, delim)
    out = []
    for r in numbers:
        if r >= R:
            return None
        s = 0 if r == 0 else t[r - 1] + 1
        e = t[r] if r < D else len(plain)
        out.append((s, e - s))
    return out


def packed(plain, delim, numbers):
    """the records' bytes in request order, each followed by one delimiter byte"""
    plain = bytes(plain)
    return b"".join(plain[s:s + n] + bytes([delim]) for s, n in locate(plain, delim, numbers))
