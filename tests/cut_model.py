"""The yardstick of the tests of ZraHipCutRecords (include/zra_hip.h): the chosen fields of the selected records, packed, computed on
the CPU from the plaintext a test generated itself. The selection is tests/extract_model.py's (with a syntax word
tests/expr_model.py's); no pattern selects every record. The field rule is written with true field numbers and Python ints: nothing
saturates here."""
import expr_model as EM
import grep_model as GM

MAX_FIELD = 64                                                                 # ZRA_HIP_CUT_MAX_FIELD


def chosen(mask, j):
    """is field j (from 1) chosen: bit min(j, 64) - 1, bit 63 standing for field 64 and every later one"""
    return (mask >> (min(j, MAX_FIELD) - 1)) & 1 == 1


def cut_record(record, separator, mask):
    """the kept bytes of one record, without its delimiter: a content byte iff its field is chosen; the separator in front of field k
    iff field k is chosen and some field in front of it is"""
    out, j, some = bytearray(), 1, chosen(mask, 1)
    for b in bytes(record):
        if b == separator:
            j += 1
            if chosen(mask, j) and some:
                out.append(b)
            some = some or chosen(mask, j)
        elif chosen(mask, j):
            out.append(b)
    return bytes(out)


def field_mask(text):
    """cut's LIST as ZraHipFieldMask reads it, or None where it refuses"""
    mask = 0
    if not text:
        return None
    for item in text.split(","):
        if item.count("-") > 1 or not item or item == "-" or not all(ch in "0123456789-" for ch in item):
            return None
        if "-" in item:
            a, b = item.split("-")
            a, b = (int(a) if a else 1), (int(b) if b else None)
        else:
            a = b = int(item)
            if a > MAX_FIELD:
                return None
        if a == 0 or b == 0 or (b is not None and b < a):
            return None
        for j in range(min(a, MAX_FIELD), min(MAX_FIELD if b is None else b, MAX_FIELD) + 1):
            mask |= 1 << (j - 1)
    return mask


def cut(data, patterns, separator, mask, delimiter=0x0A, invert=False, lo=0, hi=None, syntax=0):
    """(records of the range, the selected ones, matches = the number of (p, i) pairs, the packed bytes)"""
    data = bytes(data)
    if patterns:
        recs, sel, nm, _ = EM.extract(data, patterns, syntax, delimiter, invert, lo, hi)
    else:
        assert not invert
        recs = GM.records(data, delimiter, lo, hi)
        sel, nm = list(recs), 0
    return recs, sel, nm, b"".join(cut_record(data[o:o + n], separator, mask) + bytes([delimiter]) for o, n in sel)
