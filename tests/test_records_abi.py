"""CPU tests of the record index's boundary (include/zra_hip.h: ZraHipIndexRecords, ZraHipLocateRecords, ZraHipReadRecords, their
stats and bring-up times): declared and exported, the Python binding exists, without an engine every call is refused before anything
touches a device, the zra_rec_ kernels compiled without scratch, and the model the GPU tests use as their yardstick
(tests/records_model.py) cuts the records the grep's and the extract's models cut."""
import ctypes
import json
import os
import re

import corpus as C
import extract_model as EM
import grep_model as GM
import records_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipIndexRecords", "ZraHipGetIndexRecordsStats", "ZraHipDebugIndexRecordsMs", "ZraHipLocateRecords", "ZraHipGetLocateRecordsStats",
         "ZraHipDebugLocateRecordsMs", "ZraHipReadRecords", "ZraHipGetReadRecordsStats", "ZraHipDebugReadRecordsMs"]
EDGES = [b"", b"\n", b"a", b"a\n", b"\na", b"\n\n", b"a\n\nb", b"a\nb\n", b"\n\n\n", b"abc", b"ab\ncd\n\nef", bytes(20), b"x" + bytes(5) + b"y"]


def test_record_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert ctypes.sizeof(zra.ZraHipRecordIndex) == 40
    assert [f[0] for f in zra.ZraHipRecordIndex._fields_] == ["contentSize", "frameSize", "delimiter", "frames", "delimiters", "records"]
    assert re.search(r"typedef struct ZraHipRecordIndex \{ uint64_t contentSize; uint32_t frameSize; uint32_t delimiter; uint64_t frames; "
                     r"uint64_t delimiters; uint64_t records; \} ZraHipRecordIndex;", txt)
    assert "INDEX IS NOT VERIFY" in txt and "Not covered: record numbers" not in txt


def test_record_binding_exists(zra):
    for name in ("index_records", "index_records_stats", "index_records_ms", "locate_records", "locate_records_stats", "locate_records_ms",
                 "read_records", "read_records_stats", "read_records_ms"):
        assert callable(getattr(zra.Engine, name)), name
    assert zra.RecordIndex._fields == ("content_size", "frame_size", "delimiter", "frames", "delimiters", "records")
    assert zra.INDEX_RECORDS_STATS == ("frames", "indexed", "content_bytes", "delimiters", "passes")
    assert zra.LOCATE_RECORDS_STATS == ("frames", "records", "boundaries", "decoded", "content_bytes", "passes")
    assert zra.READ_RECORDS_STATS == ("frames", "records", "packed_bytes", "locate_decoded", "read_decoded", "locate_passes")


def test_calls_without_an_engine_are_refused(zra):
    """{ZStdError, 42} for every combination of the other arguments; the outputs are zeroed and the host arrays are left alone (the
    remaining refusals need an engine: tests/test_gpu_records.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for arc in ((None, 0), (P(64), 100), (None, 100)):
        for delim in (0, 10, 255, 256):
            for idx in ((None, 0), (P(4096), 8), (None, 8)):
                info = zra.ZraHipRecordIndex(1, 2, 3, 4, 5, 6)
                st = L.ZraHipIndexRecords(None, *arc, delim, 0, 0xFFFFFFFFFFFFFFFF, 0, *idx, ctypes.byref(info))
                assert st.tup() == (1, 42) and bytes(info) == bytes(40), (arc, delim, idx)
                assert L.ZraHipIndexRecords(None, *arc, delim, 0, 1, 0, *idx, None).tup() == (1, 42)
    good = zra.ZraHipRecordIndex(2000, 1000, 10, 2, 5, 6)
    for info in (None, good, zra.ZraHipRecordIndex(2000, 1000, 10, 3, 5, 6)):
        ref = ctypes.byref(info) if info is not None else None
        for arc in ((None, 0), (P(64), 100)):
            for idx in ((None, 0), (P(4096), 2), (None, 2)):
                for n in (0, 3):
                    nums = (ctypes.c_uint64 * 3)(0, 1, 2)
                    ranges = (ctypes.c_uint64 * 6)()
                    ctypes.memset(ranges, 0xEE, 48)
                    assert L.ZraHipLocateRecords(None, *arc, ref, *idx, nums, n, 0, ranges).tup() == (1, 42)
                    assert L.ZraHipLocateRecords(None, *arc, ref, *idx, None, n, 0, None).tup() == (1, 42)
                    for data in ((None, 0), (P(8192), 64), (None, 64)):
                        size = ctypes.c_uint64(0x1234)
                        st = L.ZraHipReadRecords(None, *arc, ref, *idx, nums, n, 0, ranges, *data, ctypes.byref(size))
                        assert st.tup() == (1, 42) and size.value == 0, (arc, idx, n, data)
                        assert L.ZraHipReadRecords(None, *arc, ref, *idx, nums, n, 0, None, *data, None).tup() == (1, 42)
                    assert bytes(ranges) == b"\xEE" * 48
    assert L.ZraHipDebugIndexRecordsMs(None) == 0.0 and L.ZraHipDebugLocateRecordsMs(None) == 0.0 and L.ZraHipDebugReadRecordsMs(None) == 0.0


def test_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    for f in (L.ZraHipGetIndexRecordsStats, L.ZraHipGetLocateRecordsStats, L.ZraHipGetReadRecordsStats):
        out = (ctypes.c_uint64 * 8)(*([7] * 8))
        f(None, out)
        assert list(out) == [0] * 8
        f(None, None)                                                          # no-op


def test_rec_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    kernels = [k for k in res if k.startswith("zra_rec_")]
    for k in ("zra_rec_count_kernel", "zra_rec_bounds_kernel", "zra_rec_jobs_kernel", "zra_rec_select_kernel"):
        assert k in kernels, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_records.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])


def _contents():
    log = C.gen_loglike(30000)
    return [(log, 0x0A), (log, 0x00), (log[:12345], 0x20), (log + b"\n", 0x0A)] + [(e, d) for e in EDGES for d in (0x0A, 0x00)]


def test_model_locates_the_greps_records():
    seen = 0
    for plain, d in _contents():
        D, R = RM.counts(plain, d)
        want = GM.records(plain, d)
        assert R == len(want) and D == bytes(plain).count(bytes([d])), (len(plain), d)
        assert RM.locate(plain, d, range(R)) == want, (len(plain), d)
        assert RM.locate(plain, d, [R]) is None and RM.locate(plain, d, [0, R + 5]) is None
        if R:
            assert RM.locate(plain, d, [R - 1, 0, R - 1]) == [want[-1], want[0], want[-1]]
        seen += R
    assert seen > 500


def test_model_packs_what_the_extract_packs():
    for plain, d in _contents():
        _, R = RM.counts(plain, d)
        never = bytes([d]) + b"\x01never\x02" + bytes([d])                     # holds the delimiter: inside no record, and here in no content
        assert never not in bytes(plain)
        want = EM.extract(plain, [never], d, invert=True)
        assert len(want[1]) == R
        assert RM.packed(plain, d, range(R)) == want[3], (len(plain), d)
    assert RM.packed(b"ab\ncd", 0x0A, [1, 0, 1]) == b"cd\nab\ncd\n"


def test_model_index_words():
    B = RM.BIT63
    assert RM.index_words(b"", 4, 10) == []
    assert RM.index_words(b"ab\ncd\n\nef", 4, 10) == [1 | B, 2 | B, B]
    assert RM.index_words(b"\n\n\n\n", 4, 10) == [4]
    assert RM.index_words(b"\n\n\n\nx", 4, 10) == [4, B]
    for plain, d in _contents():
        for fs in (7, 1000):
            w = RM.index_words(plain, fs, d)
            D, R = RM.counts(plain, d)
            assert len(w) == -(-len(plain) // fs) and sum(x & (B - 1) for x in w) == D
            assert R == D + (w[-1] >> 63 if w else 0)
