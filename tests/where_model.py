"""The yardstick of the tests of ZraHipGrepArchiveWhere (include/zra_hip.h): per record the set of patterns with a match that starts
inside it, from the multi search's matches (tests/msearch_model.py, or any other list of (p, i) pairs) and the grep's records
(tests/grep_model.py), then the predicate: a list of clauses (all, any, none), each term a 64-bit mask over the pattern indices."""
import grep_model
import msearch_model


def full(n_patterns):
    """the patterns 0 .. n - 1 as a mask"""
    return (1 << n_patterns) - 1


def mask(indices):
    m = 0
    for i in indices:
        m |= 1 << i
    return m


def clause_holds(clause, H):
    a, y, n = clause
    return (H & a) == a and (y == 0 or (H & y) != 0) and (H & n) == 0


def selected(clauses, H, invert=False):
    """is a record with hit set H selected: some clause holds; invert complements that"""
    return any(clause_holds(c, H) for c in clauses) != bool(invert)


def hit_sets(recs, matches):
    """per record of the ascending list `recs` the mask of the patterns i with a match (p, i), p inside the record. `matches` is
    sorted by p; a match's p never is a delimiter's position, so it lies in exactly one record."""
    out, k = [], 0
    for off, size in recs:
        H = 0
        while k < len(matches) and matches[k][0] < off:
            k += 1
        while k < len(matches) and matches[k][0] < off + size:
            H |= 1 << matches[k][1]
            k += 1
        out.append(H)
    return out


def grep_where(data, patterns, clauses, delimiter=0x0A, invert=False, lo=0, hi=None, matches=None):
    """(records of the range, the selected ones, matches = the number of (p, i) pairs). matches: the (p, i) list to use in the place
    of the literal multi search's (the expression tests pass tests/expr_model.py's)."""
    recs = grep_model.records(data, delimiter, lo, hi)
    if matches is None:
        matches = msearch_model.matches_multi(data, patterns, lo, hi)
    matches = sorted(matches)
    sets = hit_sets(recs, matches)
    return recs, [r for r, H in zip(recs, sets) if selected(clauses, H, invert)], len(matches)
