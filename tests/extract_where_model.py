"""The yardstick of the tests of ZraHipExtractRecordsWhere (include/zra_hip.h): the packed text of the records a predicate selects,
computed on the CPU from the plaintext a test generated itself. Nothing new defines truth here: the selection is
tests/where_model.py's grep_where (held against the plain grep's model in tests/test_grep_where_abi.py), the packing is
tests/extract_model.py's (every selected record's bytes, then one delimiter byte, in ascending order; held against a naive loop in
tests/test_extract_abi.py)."""
import where_model as WM
from extract_model import starts  # noqa: F401  (d_i of every selected record)


def extract_where(data, patterns, clauses, delimiter=0x0A, invert=False, lo=0, hi=None, matches=None):
    """(records of the range, the selected ones, matches = the number of (p, i) pairs, the packed bytes)"""
    data = bytes(data)
    recs, sel, nm = WM.grep_where(data, patterns, clauses, delimiter, invert, lo, hi, matches=matches)
    return recs, sel, nm, b"".join(data[o:o + n] + bytes([delimiter]) for o, n in sel)


def prefix_selection(record, patterns, clauses, invert=False):
    """the selection of every prefix record[:k], k = 0 .. len(record), as a list of bools: what a scan that tested the predicate in
    front of the record's end would see. The hit set of a prefix holds the patterns with a match that STARTS inside it, as a record
    cut by hi there would not: the match may end behind k, as it does for a position whose record goes on in the next trip."""
    import msearch_model
    record = bytes(record)
    at = msearch_model.matches_multi(record, patterns)
    out, H, j = [], 0, 0
    for k in range(len(record) + 1):
        while j < len(at) and at[j][0] < k:
            H |= 1 << at[j][1]
            j += 1
        out.append(WM.selected(clauses, H, invert))
    return out
