"""The yardstick of the multi-pattern search tests: the matches and the filter survivors of ZraHipSearchArchiveMulti
(include/zra_hip.h), computed on the CPU from the plaintext a test generated itself."""
import search_model


def matches_multi(data, patterns, lo=0, hi=None):
    """The list of (p, i), sorted, with lo <= p, p + m_i <= hi and data[p:p + m_i] == patterns[i]: overlapping occurrences, several
    patterns at one offset and equal patterns included."""
    return sorted((p, i) for i, pat in enumerate(patterns) for p in search_model.matches(data, pat, lo, hi))


def survivors(data, patterns, lo=0, hi=None):
    """The positions p of [lo, hi) that pass the two-byte filter: with p + 1 < hi, some pattern begins with data[p] and is one byte
    long or goes on with data[p + 1]; at p = hi - 1, a 1-byte pattern equals data[p]. 0 when the range is shorter than the shortest
    pattern (nothing is scanned then)."""
    data, patterns = bytes(data), [bytes(p) for p in patterns]
    hi = len(data) if hi is None else min(hi, len(data))
    if hi - lo < min(len(p) for p in patterns):
        return 0
    ones = {p[0] for p in patterns if len(p) == 1}
    pairs = {(p[0], p[1]) for p in patterns if len(p) > 1}
    return sum(1 for p in range(lo, hi) if data[p] in ones or (p + 1 < hi and (data[p], data[p + 1]) in pairs))
