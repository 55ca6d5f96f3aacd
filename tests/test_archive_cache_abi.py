"""CPU tests of the archive handle's boundary (include/zra_hip.h: ZraHipArchive*): the five calls are declared and exported, the Python
binding exists, opening without a usable engine fails loudly (no CPU fallback), and the handle's kernels compiled without scratch."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHIVE_CALLS = ["ZraHipArchiveOpen", "ZraHipArchiveClose", "ZraHipArchiveRead", "ZraHipArchiveDropCache", "ZraHipArchiveGetStats"]
CACHE_KERNELS = ["zra_cache_lookup_kernel", "zra_cache_victims_kernel", "zra_cache_commit_kernel"]


def test_archive_calls_are_declared_and_exported(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in ARCHIVE_CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s


def test_archive_binding_exists(zra):
    A = zra.Archive
    for m in ("read", "stats", "drop_cache", "close", "__enter__", "__exit__"):
        assert callable(getattr(A, m)), m
    assert zra.ARCHIVE_STATS == ("slots", "resident", "reads", "hits", "misses", "evictions", "uncompressed_size", "frame_size")


def test_archive_refuses_null_arguments(zra):
    """NULL engine / handle / out-pointer: {ZStdError, 42}, the refusal of the comm calls; no handle is written. Close(NULL) is a no-op."""
    L = zra.load()
    h = ctypes.c_void_p(0x1234)
    assert L.ZraHipArchiveOpen(None, None, 0, 1 << 20, ctypes.byref(h)).tup() == (1, 42)
    assert h.value == 0x1234
    assert L.ZraHipArchiveRead(None, None, None, None, None, 0).tup() == (1, 42)
    assert L.ZraHipArchiveDropCache(None).tup() == (1, 42)
    L.ZraHipArchiveClose(None)
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    L.ZraHipArchiveGetStats(None, out)
    assert list(out) == [0] * 8


def test_archive_open_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        pytest.skip("a GPU is present; covered by tests/test_gpu_archive_cache.py")
    with pytest.raises(zra.ZraError):
        zra.Archive(zra.Engine(0), 0, 0, 1 << 20)       # no engine without a GPU, so no handle: never a CPU result


def test_cache_kernels_compile_without_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    for k in CACHE_KERNELS:
        assert k in res, k
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
