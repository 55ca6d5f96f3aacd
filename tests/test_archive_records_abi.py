"""CPU tests of the boundary of the record index through an archive handle (include/zra_hip.h: ZraHipArchiveIndexRecords,
ZraHipArchiveLocateRecords, ZraHipArchiveReadRecords, ZraHipArchiveGetRecordStats, ZraHipDebugArchiveRecordStageMs): declared and
exported, the Python binding exists, without a handle every call is refused before anything touches a device, the list-split kernel
compiled without scratch, and the header points at the handle's calls where it used to name them as not covered."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipArchiveIndexRecords", "ZraHipArchiveLocateRecords", "ZraHipArchiveReadRecords", "ZraHipArchiveGetRecordStats",
         "ZraHipDebugArchiveRecordStageMs"]
MAXU64 = (1 << 64) - 1


def _header():
    return open(os.path.join(ROOT, "include", "zra_hip.h")).read()


def _doc(txt, call):
    return txt[:txt.index("ZRA_EXPORT ZraStatus %s(" % call)].rsplit("/**", 1)[1]


def test_record_calls_are_declared_and_exported(zra):
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", _header()))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s


def test_record_binding_exists(zra):
    for name in ("index_records", "locate_records", "read_records", "record_stats", "record_stage_ms"):
        assert callable(getattr(zra.Archive, name)), name
    assert zra.ARCHIVE_RECORD_STATS == ("calls", "staged", "decoded", "passes", "staged_total", "decoded_total")


def test_calls_without_a_handle_are_refused(zra):
    """{ZStdError, 42} in front of everything, whatever the other arguments are (the loops of tests/test_records_abi.py, without the
    archive's): *info is zeroed, *dataSize is 0 and sentinel-filled host arrays are left alone (the remaining refusals need a handle:
    tests/test_gpu_archive_records.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    for delim in (0, 10, 255, 256):
        for idx in ((None, 0), (P(4096), 8), (None, 8)):
            for rng in ((0, MAXU64), (0, 1), (MAXU64, 7)):
                for staging in (0, 4096):
                    info = zra.ZraHipRecordIndex(1, 2, 3, 4, 5, 6)
                    st = L.ZraHipArchiveIndexRecords(None, delim, *rng, staging, *idx, ctypes.byref(info))
                    assert st.tup() == (1, 42) and bytes(info) == bytes(40), (delim, idx, rng, staging)
                    assert L.ZraHipArchiveIndexRecords(None, delim, *rng, staging, *idx, None).tup() == (1, 42)
    good = zra.ZraHipRecordIndex(2000, 1000, 10, 2, 5, 6)
    for info in (None, good, zra.ZraHipRecordIndex(2000, 1000, 10, 3, 5, 6)):
        ref = ctypes.byref(info) if info is not None else None
        for idx in ((None, 0), (P(4096), 2), (None, 2)):
            for n in (0, 3):
                for staging in (0, 4096):
                    nums = (ctypes.c_uint64 * 3)(0, 1, 2)
                    ranges = (ctypes.c_uint64 * 6)()
                    ctypes.memset(ranges, 0xEE, 48)
                    assert L.ZraHipArchiveLocateRecords(None, ref, *idx, nums, n, staging, ranges).tup() == (1, 42)
                    assert L.ZraHipArchiveLocateRecords(None, ref, *idx, None, n, staging, None).tup() == (1, 42)
                    for data in ((None, 0), (P(8192), 64), (None, 64)):
                        size = ctypes.c_uint64(0x1234)
                        st = L.ZraHipArchiveReadRecords(None, ref, *idx, nums, n, staging, ranges, *data, ctypes.byref(size))
                        assert st.tup() == (1, 42) and size.value == 0, (idx, n, data)
                        assert L.ZraHipArchiveReadRecords(None, ref, *idx, nums, n, staging, None, *data, None).tup() == (1, 42)
                    assert bytes(ranges) == b"\xEE" * 48
                    assert bytes(nums) == bytes((ctypes.c_uint64 * 3)(0, 1, 2))
        if info is not None:
            assert bytes(info)[:8] == (2000).to_bytes(8, "little")              # the caller's *info of locate and read is only read


def test_getters_of_no_handle_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipArchiveGetRecordStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipArchiveGetRecordStats(None, None)                                  # no-op
    assert L.ZraHipDebugArchiveRecordStageMs(None) == 0.0


def test_split_kernel_compiles_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    k = res["zra_rec_split_kernel"]
    assert k["source"] == "zra_records.hip", k
    assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_header_points_at_the_handle_calls():
    """The three plain calls name their handle call and no longer list a handle variant as not covered; the scans' section keeps its
    list, without the record index; the handle's section names the follow-ups instead."""
    txt = _header()
    for call, handle in (("ZraHipIndexRecords", "ZraHipArchiveIndexRecords"), ("ZraHipLocateRecords", "ZraHipArchiveLocateRecords"),
                         ("ZraHipReadRecords", "ZraHipArchiveReadRecords")):
        doc = _doc(txt, call)
        assert handle + " " in doc or handle + "," in doc, call
        covered = doc.split("Not covered:", 1)[1] if "Not covered:" in doc else ""
        assert "handle variant" not in covered and "ZraHipArchive handles" not in covered, call
    doc = _doc(txt, "ZraHipArchiveSearch")
    covered = doc.split("Not covered:", 1)[1]
    assert "ZraHipVerifyArchive" in covered and "ZraHipSignArchive" in covered
    assert "the same view of the cache will serve them" not in covered and not re.search(r"and the record index \(the follow-up", covered)
    doc = _doc(txt, "ZraHipArchiveIndexRecords")
    assert "Index and locate are not reads" in doc and "no damage is laundered" in doc
    covered = doc.split("Not covered:", 1)[1]
    assert "read the arena in place" in covered and "fusing the two sweeps" in covered
    doc = _doc(txt, "ZraHipArchiveReadRecords")
    assert "THE BYTE FETCH IS A READ" in doc and "ZraHipArchiveRead" in doc
    assert txt.index("ZraHipDebugArchiveScanStageMs(") < txt.index("ZRA_EXPORT ZraStatus ZraHipArchiveIndexRecords(") < txt.index("ZRA_EXPORT ZraStatus ZraHipUpdateArchive(")
