"""The yardstick of the extract tests: the packed text of ZraHipExtractRecords (include/zra_hip.h), computed on the CPU from the
plaintext a test generated itself. It is the grep's selection (tests/grep_model.py) joined: every selected record's bytes, then one
delimiter byte, in ascending order."""
import grep_model as GM


def extract(data, patterns, delimiter=0x0A, invert=False, lo=0, hi=None):
    """(records of the range, the selected ones, matches, the packed bytes)"""
    data = bytes(data)
    recs, sel, matches = GM.grep(data, patterns, delimiter, invert, lo, hi)
    return recs, sel, matches, b"".join(data[o:o + n] + bytes([delimiter]) for o, n in sel)


def starts(sel):
    """d_i of every selected record: the sum of (n_j + 1) over the records in front of it"""
    out, d = [], 0
    for _, n in sel:
        out.append(d)
        d += n + 1
    return out
