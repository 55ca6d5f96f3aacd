"""CPU tests of the extract's boundary (include/zra_hip.h: ZraHipExtractRecords, ZraHipGetExtractStats, ZraHipDebugExtractMs):
declared, exported and bound, every rule-1 refusal before anything touches a device, no CPU result without a GPU, the zra_extract_*
kernels compiled inside their budget, and the model the GPU tests use as their yardstick (tests/extract_model.py) agrees with a naive
per-position loop that emits bytes as it goes, with bytes.split and with answers pinned by hand."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import extract_model as XM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipExtractRecords", "ZraHipGetExtractStats", "ZraHipDebugExtractMs"]
MAXU64 = (1 << 64) - 1


def test_extract_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert zra.EXTRACT_STATS == ("frames", "decoded", "content_bytes", "records", "selected", "packed_bytes", "passes", "matches")
    assert callable(zra.Engine.extract) and callable(zra.Engine.extract_stats) and callable(zra.Engine.extract_ms)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_extract_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42}; *nRecords and *dataSize are zeroed when they are there and the record array is left alone. (The same cases
    with an engine: tests/test_gpu_extract.py.)"""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 5000)
    nl = ctypes.create_string_buffer(b"ab\ncd")
    # (patterns, sizes, count, delimiter, mode)
    cases = [(pats, _sizes(3), 1, 10, 2), (pats, _sizes(3), 1, 10, 3), (pats, _sizes(3), 1, 10, 0x80000000),    # mode bits
             (nl, _sizes(5), 1, 10, 0), (nl, _sizes(2, 3), 2, 10, 1), (pats, _sizes(3), 1, 7, 0),                # a pattern holds the delimiter
             (pats, _sizes(3, 4), 2, 7, 0),
             (pats, _sizes(3, 0), 2, 10, 0), (pats, _sizes(257), 1, 10, 0), (pats, _sizes(*([1] * 65)), 65, 10, 0),   # the multi search's
             (pats, _sizes(*([256] * 17)), 17, 10, 0), (pats, _sizes(3), 0, 10, 0), (None, _sizes(3), 1, 10, 0), (pats, None, 1, 10, 0)]
    ok = (pats, _sizes(3), 1, 10, 0)
    for hp, hs, k, delim, mode in cases + [ok]:
        for arc in ((None, 0), (P(64), 100), (None, 100)):
            arr = (ctypes.c_uint64 * 8)()
            ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
            nn, dd = ctypes.byref(n), ctypes.byref(ds)
            # (hRecords, recordCapacity, nRecords, dData, dataCapacity, dataSize)
            outs = [(arr, 4, nn, P(4096), 64, dd), (None, 0, None, P(4096), 64, dd), (arr, 4, nn, P(4096), 64, None), (None, 4, nn, P(4096), 64, dd),
                    (arr, 4, nn, None, 64, dd), (None, 0, None, None, 0, None)]
            if (hp, hs, k, delim, mode) == ok:
                outs = outs[1:]                                                # (the good patterns: only what the outputs themselves break)
            for out in outs:
                n.value, ds.value = 0x1234, 0x5678
                tag = (k, delim, mode, arc, out[1], out[4])
                assert L.ZraHipExtractRecords(None, *arc, hp, hs, k, delim, mode, 0, MAXU64, 0, *out).tup() == (1, 42), tag
                assert n.value == (0 if out[2] is not None else 0x1234) and ds.value == (0 if out[5] is not None else 0x5678), tag
                assert bytes(arr) == b"\xEE" * 64, tag
    assert L.ZraHipDebugExtractMs(None) == 0.0


def test_extract_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetExtractStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetExtractStats(None, None)                                        # no-op


def test_extract_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_extract.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).extract(64, 100, [b"abc", b"d"], 4096, 64)               # no engine without a GPU: never a CPU result


def test_extract_kernels_stay_inside_their_budget():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_extract.hip")).read()
    kernels = [k for k in res if k.startswith("zra_extract_")]
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_extract_\w+)\s*\(", src))) and len(kernels) >= 3, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_extract.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes"] <= 65536, (k, res[k])


def _naive(data, pats, delim, invert, lo, end):
    """(selected, packed bytes) of [lo, end), one position at a time: the bytes of the open record are kept as they go by and emitted,
    with one delimiter, when the record ends selected"""
    sel, out = [], bytearray()
    start, hit, cur = lo, False, bytearray()
    for p in range(lo, end):
        if data[p] == delim:
            if hit != invert:
                sel.append((start, p - start))
                out += cur
                out.append(delim)
            start, hit, cur = p + 1, False, bytearray()
            continue
        cur.append(data[p])
        for pat in pats:
            if p + len(pat) <= end and all(data[p + j] == pat[j] for j in range(len(pat))):
                hit = True
    if start < end and hit != invert:
        sel.append((start, end - start))
        out += cur
        out.append(delim)
    return sel, bytes(out)


def test_model_agrees_with_a_naive_per_position_loop():
    rng = np.random.RandomState(19)
    empty_sel = first_cut = last_cut = ends_delim = inverted = 0
    for case in range(600):
        k = int(rng.randint(3, 5))
        delim = k - 1                                                          # one symbol of the alphabet is the delimiter
        data = bytes(rng.randint(0, k, size=int(rng.randint(0, 41))).astype(np.uint8))
        pats = [bytes(rng.randint(0, k - 1, size=int(rng.randint(1, 4))).astype(np.uint8)) for _ in range(int(rng.randint(1, 4)))]
        if case % 3 == 0:
            lo, hi = 0, None
        else:
            lo = int(rng.randint(0, len(data) + 1)); hi = int(rng.randint(lo, len(data) + 1))
        end = len(data) if hi is None else hi
        invert = bool(case & 1)
        want = _naive(data, pats, delim, invert, lo, end)
        recs, sel, matches, packed = XM.extract(data, pats, delim, invert, lo, hi)
        assert (sel, packed) == want, (data, pats, delim, invert, lo, hi, sel, packed, want)
        assert len(packed) == sum(n + 1 for _, n in sel) and packed.count(bytes([delim])) == len(sel)
        for (o, n), d in zip(sel, XM.starts(sel)):
            assert packed[d:d + n] == data[o:o + n] and packed[d + n] == delim
        other = XM.extract(data, pats, delim, not invert, lo, hi)
        assert len(packed) + len(other[3]) == sum(n + 1 for _, n in recs)      # the two modes split the records
        empty_sel += any(n == 0 for _, n in sel)
        first_cut += bool(sel) and lo > 0 and data[lo - 1] != delim and sel[0][0] == lo
        last_cut += bool(sel) and end < len(data) and data[end] != delim and sel[-1][0] + sel[-1][1] == end
        ends_delim += end > lo and data[end - 1] == delim and bool(sel)
        inverted += invert and bool(sel)
    assert min(empty_sel, first_cut, last_cut, ends_delim, inverted) > 40, (empty_sel, first_cut, last_cut, ends_delim, inverted)


def test_model_agrees_with_bytes_split():
    rng = np.random.RandomState(20)
    for case in range(100):
        data = bytes(rng.choice([10, 10, 97, 98, 99], size=int(rng.randint(0, 60))).astype(np.uint8))
        parts = data.split(b"\n")
        if parts[-1] == b"":
            parts.pop()                                                        # (no trailing empty record; b"" has none at all)
        for pat in (b"ab", b"c"):
            assert XM.extract(data, [pat])[3] == b"".join(x + b"\n" for x in parts if pat in x), data
            assert XM.extract(data, [pat], invert=True)[3] == b"".join(x + b"\n" for x in parts if pat not in x), data


def test_answers_pinned_by_hand():
    d = b"ab\ncd\n\nab"
    assert XM.extract(d, [b"ab"])[3] == b"ab\nab\n"
    assert XM.extract(d, [b"ab"], invert=True)[3] == b"cd\n\n"
    assert XM.extract(d, [b"ab"], invert=True, lo=0, hi=8)[3] == b"cd\n\na\n"
    assert XM.extract(d, [b"zz"])[3] == b"" and XM.extract(b"", [b"a"], invert=True)[3] == b""
    assert XM.extract(b"\n\n", [b"a"], invert=True)[3] == b"\n\n" and XM.starts([(0, 2), (3, 0), (7, 2)]) == [0, 3, 4]
