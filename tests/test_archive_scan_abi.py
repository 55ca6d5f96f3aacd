"""CPU tests of the boundary of the range scans through an archive handle (include/zra_hip.h: ZraHipArchiveSearch,
ZraHipArchiveSearchMulti, ZraHipArchiveGrep, ZraHipArchiveExtractRecords, ZraHipArchiveGetScanStats, ZraHipDebugArchiveScanStageMs):
declared and exported, the Python binding exists, without a handle every call is refused before anything touches a device, the job-split
kernel compiled without scratch, and the header points at the handle's calls where it used to name them as not covered."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipArchiveSearch", "ZraHipArchiveSearchMulti", "ZraHipArchiveGrep", "ZraHipArchiveExtractRecords", "ZraHipArchiveGetScanStats",
         "ZraHipDebugArchiveScanStageMs"]
MAXU64 = (1 << 64) - 1


def _header():
    return open(os.path.join(ROOT, "include", "zra_hip.h")).read()


def test_scan_calls_are_declared_and_exported(zra):
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", _header()))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s


def test_scan_binding_exists(zra):
    for name in ("search", "search_multi", "grep", "extract", "scan_stats", "scan_stage_ms"):
        assert callable(getattr(zra.Archive, name)), name
    assert zra.ARCHIVE_SCAN_STATS == ("scans", "staged", "decoded", "passes", "staged_total", "decoded_total")


def test_calls_without_a_handle_are_refused(zra):
    """{ZStdError, 42} in front of everything, whatever the other arguments are: the output words are zeroed and sentinel-filled host
    arrays are left alone (the remaining refusals need a handle: tests/test_gpu_archive_scan.py)."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = b"abcxy"
    sizes = (ctypes.c_uint32 * 2)(3, 2)
    for pat in (None, pats):
        for rng in ((0, MAXU64), (5, 0), (MAXU64, 7)):
            for staging in (0, 4096):
                for cap in (0, 4):
                    arr = (ctypes.c_uint64 * 12)()
                    per = (ctypes.c_uint64 * 3)()
                    ctypes.memset(arr, 0xEE, 96); ctypes.memset(per, 0xEE, 24)
                    tag = (pat, rng, staging, cap)
                    n = ctypes.c_uint64(0x1234)
                    assert L.ZraHipArchiveSearch(None, pat, 3, *rng, staging, arr, cap, ctypes.byref(n)).tup() == (1, 42) and n.value == 0, tag
                    assert L.ZraHipArchiveSearch(None, pat, 3, *rng, staging, None, cap, None).tup() == (1, 42), tag
                    n = ctypes.c_uint64(0x1234)
                    st = L.ZraHipArchiveSearchMulti(None, pat, sizes, 2, *rng, staging, ctypes.cast(arr, ctypes.POINTER(zra.ZraHipPatternMatch)), cap,
                                                    ctypes.byref(n), per)
                    assert st.tup() == (1, 42) and n.value == 0, tag
                    assert L.ZraHipArchiveSearchMulti(None, pat, None, 2, *rng, staging, None, cap, None, None).tup() == (1, 42), tag
                    for mode in (0, 1, 7):
                        n = ctypes.c_uint64(0x1234)
                        assert L.ZraHipArchiveGrep(None, pat, sizes, 2, 10, mode, *rng, staging, arr, cap, ctypes.byref(n)).tup() == (1, 42) and n.value == 0, tag
                        assert L.ZraHipArchiveGrep(None, pat, sizes, 2, 10, mode, *rng, staging, None, cap, None).tup() == (1, 42), tag
                        for data in ((None, 0), (P(8192), 64), (None, 64)):
                            n, ds = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x5678)
                            st = L.ZraHipArchiveExtractRecords(None, pat, sizes, 2, 10, mode, *rng, staging, arr, cap, ctypes.byref(n), *data, ctypes.byref(ds))
                            assert st.tup() == (1, 42) and n.value == 0 and ds.value == 0, (tag, mode, data)
                            assert L.ZraHipArchiveExtractRecords(None, pat, sizes, 2, 10, mode, *rng, staging, None, cap, None, *data, None).tup() == (1, 42)
                    assert bytes(arr) == b"\xEE" * 96 and bytes(per) == b"\xEE" * 24, tag


def test_getters_of_no_handle_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipArchiveGetScanStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipArchiveGetScanStats(None, None)                                    # no-op
    assert L.ZraHipDebugArchiveScanStageMs(None) == 0.0


def test_split_kernel_compiles_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    k = res["zra_scan_split_kernel"]
    assert k["source"] == "zra_archive.hip", k
    assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_header_points_at_the_handle_calls():
    """The four scans no longer name a handle variant as not covered; the handle's section names the follow-up instead."""
    txt = _header()
    assert not re.search(r"handle variant (that scans|on resident)", txt)
    for call, handle in (("ZraHipSearchArchive", "ZraHipArchiveSearch"), ("ZraHipSearchArchiveMulti", "ZraHipArchiveSearchMulti"),
                         ("ZraHipGrepArchive", "ZraHipArchiveGrep"), ("ZraHipExtractRecords", "ZraHipArchiveExtractRecords")):
        doc = txt[:txt.index("ZRA_EXPORT ZraStatus %s(" % call)].rsplit("/**", 1)[1]
        assert handle + "," in doc or handle + " " in doc, call
        covered = doc.split("Not covered:", 1)[1] if "Not covered:" in doc else ""
        assert "handle variant" not in covered and "ZraHipArchive handles" not in covered, call
    doc = txt[:txt.index("ZRA_EXPORT ZraStatus ZraHipArchiveSearch(")].rsplit("/**", 1)[1]
    assert "A scan is not a read" in doc and "this launders no damage" in doc
    assert "Not covered:" in doc and "ZraHipVerifyArchive" in doc.split("Not covered:", 1)[1]
