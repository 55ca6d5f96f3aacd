"""CPU tests of the boundary of the update through an archive handle (include/zra_hip.h: ZraHipArchiveUpdate,
ZraHipArchiveGetUpdateStats): declared and exported, the Python binding exists, a NULL handle is refused before anything touches a
device, and the kernels the call adds or changes compiled without scratch."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipArchiveUpdate", "ZraHipArchiveGetUpdateStats"]
KERNELS = ["zra_upd_stage_cached_kernel", "zra_upd_plan_kernel", "zra_upd_patch_kernel", "zra_upd_gather_kernel"]


def test_archive_update_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s


def test_archive_update_binding_exists(zra):
    assert callable(zra.Archive.update) and callable(zra.Archive.update_stats)
    assert zra.ARCHIVE_UPDATE_STATS == ("updates", "frames", "archive_bytes", "staged", "refreshed", "staged_total", "refreshed_total")


def test_archive_update_refuses_a_null_handle(zra):
    """{ZStdError, 42} whatever the other arguments are; *outSize is left alone, and outSize may be NULL."""
    L = zra.load()
    one = (ctypes.c_uint64 * 1)(0)
    P = ctypes.c_void_p
    for args in ((None, None, None, None, 0, None, 0, None, 0),
                 (P(64), one, one, one, 1, P(64), 1, P(4096), 100),
                 (None, None, None, None, 1, None, 1, P(4096), 100)):
        osz = ctypes.c_size_t(0x1234)
        assert L.ZraHipArchiveUpdate(None, *args, ctypes.byref(osz), 3, True).tup() == (1, 42), args
        assert osz.value == 0x1234
        assert L.ZraHipArchiveUpdate(None, *args, None, 3, True).tup() == (1, 42), args


def test_archive_update_stats_of_no_handle_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipArchiveGetUpdateStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipArchiveGetUpdateStats(None, None)                                  # no-op


def test_archive_update_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    for k in KERNELS:
        assert k in res, k
        assert res[k]["source"] == "zra_update.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
