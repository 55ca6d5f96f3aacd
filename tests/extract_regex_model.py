"""The yardstick of the regex extract tests: the packed text of ZraHipExtractRecordsRegex (include/zra_hip.h), computed on the CPU
from the plaintext a test generated itself. Nothing new defines truth here: the selection is tests/regex_model.py's grep_regex (held
against Python's `re` in tests/test_regex_abi.py), the packing is tests/extract_model.py's (every selected record's bytes, then one
delimiter byte, in ascending order; held against a naive loop in tests/test_extract_abi.py)."""
import regex_model as RM
from extract_model import starts  # noqa: F401  (d_i of every selected record)


def extract_regex(data, patterns, delimiter=0x0A, invert=False, fold=False, lo=0, hi=None, matcher=None):
    """(records of the range, the selected ones, matched records, the packed bytes)"""
    data = bytes(data)
    recs, sel, matched = RM.grep_regex(data, patterns, delimiter, invert, fold, lo, hi, matcher=matcher)
    return recs, sel, matched, b"".join(data[o:o + n] + bytes([delimiter]) for o, n in sel)
