"""The yardstick of the tests of ZraHipTallyRecords and ZraHipTallyFields (include/zra_hip.h): the distinct records of a packed text
and their counts, computed on the CPU: a dict in insertion order over text.split(delimiter), with the trailing-record rule (bytes
behind the last delimiter form one more record iff there are any) and the skip rule (a record longer than MAX_KEY is counted in
n_skipped and nowhere else). The composite is tests/cut_model.py's packed text, tallied."""
import cut_model as CM

MAX_KEY = 4096                                                                 # ZRA_HIP_TALLY_MAX_KEY
NL = 10


def records(text, delimiter=NL):
    """[(offset, size)] of every record of the text, without its delimiter"""
    parts = bytes(text).split(bytes([delimiter]))
    if parts[-1] == b"":
        parts.pop()                                                            # (the text ends with a delimiter, or is empty)
    out, at = [], 0
    for p in parts:
        out.append((at, len(p)))
        at += len(p) + 1
    return out


def tally(text, delimiter=NL, max_key=MAX_KEY):
    """(n_records, n_skipped, [(offset, size, count)] in order of first appearance, the keys as text: each with one delimiter)"""
    text = bytes(text)
    seen, skipped = {}, 0
    recs = records(text, delimiter)
    for o, n in recs:
        if n > max_key:
            skipped += 1
            continue
        k = text[o:o + n]
        if k in seen:
            seen[k][2] += 1
        else:
            seen[k] = [o, n, 1]
    entries = [tuple(v) for v in seen.values()]
    return len(recs), skipped, entries, b"".join(k + bytes([delimiter]) for k in seen)


def slots(n_records, max_distinct=0):
    """the table the call sizes: the power of two at or above 1.5 * min(maxDistinct, records) + 64"""
    bound = min(max_distinct, n_records) if max_distinct else n_records
    s = 64
    while s < bound + bound // 2 + 64:
        s <<= 1
    return s


def lines(text, entries, delimiter=NL):
    """what `zratool_amd tally` prints: per entry the count, a space, the key, the delimiter"""
    text = bytes(text)
    return b"".join(b"%d " % c + text[o:o + n] + bytes([delimiter]) for o, n, c in entries)


def tally_fields(data, patterns, separator, mask, delimiter=NL, invert=False, lo=0, hi=None, syntax=0):
    """(the cut's packed text, tally() of it)"""
    packed = CM.cut(data, patterns, separator, mask, delimiter, invert, lo, hi, syntax)[3]
    return packed, tally(packed, delimiter)
