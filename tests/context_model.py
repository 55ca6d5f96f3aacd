"""The yardstick of the context-grep tests: the output records of ZraHipGrepArchiveContext (include/zra_hip.h), computed on the CPU
from the plaintext a test generated itself, on top of the grep's model (tests/grep_model.py)."""
import grep_model as GM


def context(data, patterns, delimiter=0x0A, invert=False, before=0, after=0, lo=0, hi=None):
    """(records of O as (offset, size, selected), |S|, groups, records of the range, matches): R_0 .. R_(n-1) are grep_model.records of
    [lo, hi), S the indices grep_model.grep selects, O = { k : some j in S has j - before <= k <= j + after }, clipped to the range;
    a group is a maximal run of consecutive indices of O."""
    recs, sel, matches = GM.grep(data, patterns, delimiter, invert, lo, hi)
    chosen = set(sel)                                                          # (records of a range are distinct pairs)
    n = len(recs)
    out = [False] * n
    for j, r in enumerate(recs):
        if r in chosen:
            for k in range(max(0, j - before), min(n, j + after + 1)):
                out[k] = True
    groups = sum(1 for k in range(n) if out[k] and (k == 0 or not out[k - 1]))
    listed = [(recs[k][0], recs[k][1], recs[k] in chosen) for k in range(n) if out[k]]
    return listed, len(sel), groups, recs, matches
