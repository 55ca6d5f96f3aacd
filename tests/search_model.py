"""The yardstick of the search tests: the matches of ZraHipSearchArchive (include/zra_hip.h), computed on the CPU from the plaintext a
test generated itself."""


def matches(data, pattern, lo=0, hi=None):
    """The ascending list of p with lo <= p, p + m <= hi and data[p:p + m] == pattern, overlapping occurrences included."""
    data, pattern = bytes(data), bytes(pattern)
    hi = len(data) if hi is None else min(hi, len(data))
    out = []
    p = data.find(pattern, lo, hi) if pattern else -1
    while p >= 0:
        out.append(p)
        p = data.find(pattern, p + 1, hi)
    return out
