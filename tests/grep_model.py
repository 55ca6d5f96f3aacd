"""The yardstick of the grep tests: the records of a content range and the selected ones of ZraHipGrepArchive (include/zra_hip.h),
computed on the CPU from the plaintext a test generated itself."""
import msearch_model


def records(data, delimiter=0x0A, lo=0, hi=None):
    """The records of [lo, hi) as (offset, size), ascending: one in front of every delimiter of the range, from lo or from behind the
    previous delimiter, and a last one up to hi when bytes are left behind the last delimiter (or there is none and lo < hi). A record
    never holds its delimiter and may be empty; content that ends in a delimiter has no trailing empty record."""
    data = bytes(data)
    hi = len(data) if hi is None else min(hi, len(data))
    out, s = [], lo
    p = data.find(bytes([delimiter]), lo, hi)
    while p >= 0:
        out.append((s, p - s))
        s = p + 1
        p = data.find(bytes([delimiter]), s, hi)
    if s < hi:
        out.append((s, hi - s))
    return out


def grep(data, patterns, delimiter=0x0A, invert=False, lo=0, hi=None):
    """(records of the range, the selected ones, matches): a record is selected iff a match (p, i) of the multi search on [lo, hi)
    starts inside it; inverted, iff none does. matches = the number of (p, i) pairs."""
    recs = records(data, delimiter, lo, hi)
    starts = sorted({p for p, _ in msearch_model.matches_multi(data, patterns, lo, hi)})
    sel, k = [], 0
    for off, size in recs:
        while k < len(starts) and starts[k] < off:
            k += 1
        hit = k < len(starts) and starts[k] < off + size
        if hit != bool(invert):
            sel.append((off, size))
    return recs, sel, len(msearch_model.matches_multi(data, patterns, lo, hi))
