"""The yardstick of the regex-grep-with-context tests: the output records of ZraHipGrepArchiveRegexContext (include/zra_hip.h), computed
on the CPU from the plaintext a test generated itself: tests/context_model.py's context with the regex grep's model
(tests/regex_model.py) in the place of the literal grep's."""
import regex_model as RM


def context(data, patterns, delimiter=0x0A, invert=False, fold=False, before=0, after=0, lo=0, hi=None, matcher=None):
    """(records of O as (offset, size, selected), |S|, groups, records of the range, matches): R_0 .. R_(n-1) are grep_model.records of
    [lo, hi), S the indices regex_model.grep_regex selects, O = { k : some j in S has j - before <= k <= j + after }, clipped to the
    range; a group is a maximal run of consecutive indices of O. matcher: a regex_model.Matcher or TableMatcher built for the
    expressions (TableMatcher for long records)."""
    recs, sel, matches = RM.grep_regex(data, patterns, delimiter, invert, fold, lo, hi, matcher)
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
