"""CPU tests of the update call's boundary (include/zra_hip.h: ZraHipUpdateArchive, ZraHipGetUpdateStats): declared and exported, the
Python binding exists, NULL arguments are refused before anything touches a device, no CPU result without a GPU, and the update's
kernels compiled without scratch."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE_CALLS = ["ZraHipUpdateArchive", "ZraHipGetUpdateStats"]
UPDATE_KERNELS = ["zra_upd_mark_kernel", "zra_upd_plan_kernel", "zra_upd_patch_kernel", "zra_upd_sizes_kernel", "zra_upd_scan_kernel",
                  "zra_upd_offsets_kernel", "zra_upd_gather_kernel"]


def test_update_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in UPDATE_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s


def test_update_binding_exists(zra):
    assert callable(zra.Engine.update) and callable(zra.Engine.update_stats)
    assert zra.UPDATE_STATS == ("frames", "touched", "decoded", "compressed", "carried_bytes", "encoded_bytes", "content_bytes", "passes")


def test_update_refuses_null_arguments(zra):
    """{ZStdError, 42}, the refusal of the archive and comm calls; *outSize is left alone. Without an engine every combination of the
    other arguments is refused alike (the remaining NULL cases need an engine: tests/test_gpu_update.py)."""
    L = zra.load()
    one = (ctypes.c_uint64 * 1)(0)
    P = ctypes.c_void_p
    for args in ((None, 0, None, None, None, None, 0, None, 0, None, 0),
                 (P(64), 100, P(64), one, one, one, 1, P(64), 1, P(4096), 100),
                 (None, 100, None, None, None, None, 1, None, 1, P(4096), 100)):
        osz = ctypes.c_size_t(0x1234)
        assert L.ZraHipUpdateArchive(None, *args, ctypes.byref(osz), 3, True).tup() == (1, 42), args
        assert osz.value == 0x1234
        assert L.ZraHipUpdateArchive(None, *args, None, 3, True).tup() == (1, 42), args


def test_update_stats_of_no_engine_are_zero(zra):
    L = zra.load()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipGetUpdateStats(None, out)
    assert list(out) == [0] * 8
    L.ZraHipGetUpdateStats(None, None)                                         # no-op


def test_update_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        pytest.skip("a GPU is present; covered by tests/test_gpu_update.py")
    with pytest.raises(zra.ZraError):
        zra.Engine(0).update(64, 100, 4096, 100)                              # no engine without a GPU: never a CPU result


def test_update_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    for k in UPDATE_KERNELS:
        assert k in res, k
        assert res[k]["source"] == "zra_update.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
