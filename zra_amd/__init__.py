"""zra_amd — Python binding of libzra_amd.so, the MI355X-native ZRA engine.

This module is plumbing only: it loads the in-tree C-ABI shared library (HIP kernels + C++ host engine)
with ctypes and mirrors the reference's interface names (include/zra.h of zraorg/ZRA: ZraCompressBuffer,
ZraDecompressBuffer, ZraDecompressRA, ... + the additive device-pointer calls of include/zra_hip.h).
There is NO CPU codec here: without the built extension or without a GPU the compute calls raise.
"""
import collections
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzra_amd.so")
if os.environ.get("ZRA_AMD_LIB") and os.environ.get("ZRA_AMD_BRINGUP") == "1":   # bring-up A/B of two builds on one box (tools/ab_lib.sh): both variables, never in production
    LIB_PATH = os.environ["ZRA_AMD_LIB"]

STATUS_NAMES = ["Success", "ZStdError", "ZraVersionLow", "HeaderInvalid", "HeaderIncomplete", "OutOfBoundsAccess",
                "OutputBufferTooSmall", "CompressedSizeTooLarge", "InputFrameSizeMismatch"]


class ZraStatus(ctypes.Structure):
    _fields_ = [("zra", ctypes.c_int), ("zstd", ctypes.c_int)]

    def tup(self):
        return (self.zra, self.zstd)


class ZraError(RuntimeError):
    def __init__(self, status, what=""):
        self.zra, self.zstd = status
        name = STATUS_NAMES[self.zra] if 0 <= self.zra < len(STATUS_NAMES) else str(self.zra)
        super().__init__("%s (zra=%d, zstd=%d) %s" % (name, self.zra, self.zstd, what))


READ_FN = ctypes.CFUNCTYPE(None, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p)


class ZraHipSlice(ctypes.Structure):
    """include/zra_hip.h: one piece of a query cut at ownership boundaries"""
    _fields_ = [("owner", ctypes.c_uint32), ("query", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("size", ctypes.c_uint64), ("within", ctypes.c_uint64)]


class ZraHipFrameFault(ctypes.Structure):
    """include/zra_hip.h: one faulty frame of ZraHipVerifyArchive"""
    _fields_ = [("frame", ctypes.c_uint64), ("code", ctypes.c_uint32), ("stage", ctypes.c_uint32)]


VERIFY_STRUCTURE, VERIFY_CONTENT = 1, 2      # ZRA_HIP_VERIFY_*


class ZraHipPatternMatch(ctypes.Structure):
    """include/zra_hip.h: one match of ZraHipSearchArchiveMulti"""
    _fields_ = [("offset", ctypes.c_uint64), ("pattern", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                               ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t))


class ZraHipHostTransport(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allgather", ALLGATHER_FN), ("exchange", EXCHANGE_FN)]


class ZraHipSignature(ctypes.Structure):
    _fields_ = [("contentSize", ctypes.c_uint64), ("frameSize", ctypes.c_uint32), ("grain", ctypes.c_uint32), ("seed", ctypes.c_uint64),
                ("frames", ctypes.c_uint64), ("words", ctypes.c_uint64)]


Signature = collections.namedtuple("Signature", "content_size frame_size grain seed frames words")


class ZraHipRecordIndex(ctypes.Structure):
    _fields_ = [("contentSize", ctypes.c_uint64), ("frameSize", ctypes.c_uint32), ("delimiter", ctypes.c_uint32), ("frames", ctypes.c_uint64),
                ("delimiters", ctypes.c_uint64), ("records", ctypes.c_uint64)]


RecordIndex = collections.namedtuple("RecordIndex", "content_size frame_size delimiter frames delimiters records")

_lib = None


def load():
    """Loads libzra_amd.so. Raises (loudly) if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("zra_amd: %s is missing — run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)" % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64 with the same soname as /opt/rocm's: whichever is loaded first serves both.
    # torch only finds its GPUs through its own copy, so when torch is installed it goes first (tests and bench.py use both).
    if "torch" not in sys.modules and not os.environ.get("ZRA_NO_TORCH_PRELOAD"):
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH)
    sz, vp, u32, u64p = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)
    szp = ctypes.POINTER(ctypes.c_size_t)
    S = ZraStatus
    sig = {
        "ZraGetVersion": (ctypes.c_uint16, []),
        "ZraGetErrorString": (ctypes.c_char_p, [S]),
        "ZraCreateHeader": (S, [ctypes.POINTER(vp), READ_FN]),
        "ZraCreateHeader2": (S, [ctypes.POINTER(vp), vp, sz]),
        "ZraDeleteHeader": (None, [vp]),
        "ZraGetVersionWithHeader": (sz, [vp]),
        "ZraGetHeaderSizeWithHeader": (sz, [vp]),
        "ZraGetUncompressedSizeWithHeader": (sz, [vp]),
        "ZraGetFrameSizeWithHeader": (sz, [vp]),
        "ZraGetMetadataSize": (sz, [vp]),
        "ZraGetMetadata": (None, [vp, vp]),
        "ZraGetCompressedOutputBufferSize": (sz, [sz, sz]),
        "ZraCompressBuffer": (S, [vp, sz, vp, szp, ctypes.c_int8, u32, ctypes.c_bool, vp, sz]),
        "ZraDecompressBuffer": (S, [vp, sz, vp]),
        "ZraDecompressRA": (S, [vp, sz, vp, sz, sz]),
        "ZraCreateCompressor": (S, [ctypes.POINTER(vp), sz, ctypes.c_int8, u32, ctypes.c_bool, vp, sz]),
        "ZraDeleteCompressor": (None, [vp]),
        "ZraGetOutputBufferSizeWithCompressor": (sz, [vp, sz]),
        "ZraCompressWithCompressor": (S, [vp, vp, sz, vp, szp]),
        "ZraGetHeaderSizeWithCompressor": (sz, [vp]),
        "ZraGetHeaderWithCompressor": (S, [vp, vp]),
        "ZraCreateDecompressor": (S, [ctypes.POINTER(vp), READ_FN, sz]),
        "ZraDeleteDecompressor": (None, [vp]),
        "ZraGetHeaderWithDecompressor": (vp, [vp]),
        "ZraDecompressWithDecompressor": (S, [vp, sz, sz, vp]),
        "ZraCreateFullDecompressor": (S, [ctypes.POINTER(vp), READ_FN, sz]),
        "ZraDeleteFullDecompressor": (None, [vp]),
        "ZraGetHeaderWithFullDecompressor": (vp, [vp]),
        "ZraDecompressWithFullDecompressor": (S, [vp, vp, sz, szp]),
        # zra_hip.h
        "ZraHipDeviceCount": (ctypes.c_int, []),
        "ZraHipCreateEngine": (S, [ctypes.POINTER(vp), ctypes.c_int]),
        "ZraHipDestroyEngine": (None, [vp]),
        "ZraHipSynchronize": (S, [vp]),
        "ZraHipGetStream": (vp, [vp]),
        "ZraHipWaitStream": (S, [vp, vp]),
        "ZraHipReleaseScratch": (S, [vp]),
        "ZraHipLastKernelMs": (ctypes.c_double, [vp]),
        "ZraHipGetKernelStats": (None, [vp, ctypes.POINTER(ctypes.c_double)]),
        "ZraHipGetDecodeStageStats": (None, [vp, ctypes.POINTER(ctypes.c_double)]),
        "ZraHipGetLaunchTelemetry": (sz, [vp, u64p, sz]),
        "ZraHipCompressBuffer": (S, [vp, vp, sz, vp, szp, ctypes.c_int8, u32, ctypes.c_bool]),
        "ZraHipDecompressBuffer": (S, [vp, vp, sz, vp, sz]),
        "ZraHipDecompressRABatch": (S, [vp, vp, sz, vp, u64p, u64p, u64p, sz]),
        "ZraHipCompressFrames": (S, [vp, vp, sz, vp, vp, szp, ctypes.c_int8, u32, ctypes.c_bool]),
        "ZraHipStitchHeader": (S, [u64p, sz, ctypes.c_uint64, u32, vp, szp]),
        # archive handle
        "ZraHipArchiveOpen": (S, [vp, vp, sz, sz, ctypes.POINTER(vp)]),
        "ZraHipArchiveClose": (None, [vp]),
        "ZraHipArchiveRead": (S, [vp, vp, u64p, u64p, u64p, sz]),
        "ZraHipArchiveDropCache": (S, [vp]),
        "ZraHipArchiveGetStats": (None, [vp, u64p]),
        "ZraHipArchiveUpdate": (S, [vp, vp, u64p, u64p, u64p, sz, vp, sz, vp, sz, szp, ctypes.c_int8, ctypes.c_bool]),
        "ZraHipArchiveGetUpdateStats": (None, [vp, u64p]),
        # the range scans through the handle: the engine calls' arguments without (engine, dArchive, archiveSize)
        "ZraHipArchiveSearch": (S, [vp, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipArchiveSearchMulti": (S, [vp, vp, ctypes.POINTER(u32), sz, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(ZraHipPatternMatch), sz, u64p, u64p]),
        "ZraHipArchiveGrep": (S, [vp, vp, ctypes.POINTER(u32), sz, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipArchiveExtractRecords": (S, [vp, vp, ctypes.POINTER(u32), sz, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp, sz, u64p]),
        "ZraHipArchiveGetScanStats": (None, [vp, u64p]),
        "ZraHipDebugArchiveScanStageMs": (ctypes.c_double, [vp]),
        "ZraHipDebugArchiveArena": (None, [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]),
        # the record index through the handle: likewise
        "ZraHipArchiveIndexRecords": (S, [vp, u32, ctypes.c_uint64, ctypes.c_uint64, sz, vp, sz, ctypes.POINTER(ZraHipRecordIndex)]),
        "ZraHipArchiveLocateRecords": (S, [vp, ctypes.POINTER(ZraHipRecordIndex), vp, sz, u64p, sz, sz, u64p]),
        "ZraHipArchiveReadRecords": (S, [vp, ctypes.POINTER(ZraHipRecordIndex), vp, sz, u64p, sz, sz, u64p, vp, sz, u64p]),
        "ZraHipArchiveGetRecordStats": (None, [vp, u64p]),
        "ZraHipDebugArchiveRecordStageMs": (ctypes.c_double, [vp]),
        # update
        "ZraHipUpdateArchive": (S, [vp, vp, sz, vp, u64p, u64p, u64p, sz, vp, sz, vp, sz, szp, ctypes.c_int8, ctypes.c_bool]),
        "ZraHipGetUpdateStats": (None, [vp, u64p]),
        "ZraHipDebugUpdateStageMs": (ctypes.c_double, [vp]),
        # verify
        "ZraHipVerifyArchive": (S, [vp, vp, sz, u32, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(ZraHipFrameFault), sz, szp]),
        "ZraHipGetVerifyStats": (None, [vp, u64p]),
        # search
        "ZraHipSearchArchive": (S, [vp, vp, sz, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipGetSearchStats": (None, [vp, u64p]),
        "ZraHipDebugSearchScanMs": (ctypes.c_double, [vp]),
        "ZraHipSearchArchiveMulti": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(ZraHipPatternMatch), sz,
                                         u64p, u64p]),
        "ZraHipGetSearchMultiStats": (None, [vp, u64p]),
        "ZraHipDebugSearchMultiScanMs": (ctypes.c_double, [vp]),
        # grep
        "ZraHipGrepArchive": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipGetGrepStats": (None, [vp, u64p]),
        "ZraHipDebugGrepScanMs": (ctypes.c_double, [vp]),
        # extract
        "ZraHipExtractRecords": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp, sz,
                                     u64p]),
        "ZraHipGetExtractStats": (None, [vp, u64p]),
        "ZraHipDebugExtractMs": (ctypes.c_double, [vp]),
        # pattern expressions: the six multi-pattern scans with a syntax word behind nPatterns, and the host-only checker
        "ZraHipCheckPatternExpr": (S, [vp, ctypes.POINTER(u32), sz, u32, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "ZraHipSearchArchiveMultiExpr": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(ZraHipPatternMatch),
                                             sz, u64p, u64p]),
        "ZraHipGrepArchiveExpr": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipExtractRecordsExpr": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp,
                                         sz, u64p]),
        "ZraHipArchiveSearchMultiExpr": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(ZraHipPatternMatch), sz, u64p,
                                             u64p]),
        "ZraHipArchiveGrepExpr": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipArchiveExtractRecordsExpr": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp, sz,
                                                u64p]),
        # the grep with a record predicate: clauses of ZraHipRecordClause {all, any, none} behind `mode`
        "ZraHipCheckRecordClauses": (S, [vp, sz, sz]),
        "ZraHipGrepArchiveWhere": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipArchiveGrepWhere": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        # the extract with a record predicate: ZraHipGrepArchiveWhere's arguments, then the extract's three
        "ZraHipExtractRecordsWhere": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p,
                                          vp, sz, u64p]),
        "ZraHipArchiveExtractRecordsWhere": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, vp, sz, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p,
                                                 vp, sz, u64p]),
        # cut records: ZraHipExtractRecordsExpr's arguments with the separator and the field mask behind `mode`; the LIST parser is host only
        "ZraHipFieldMask": (S, [ctypes.c_char_p, u64p]),
        "ZraHipCutRecords": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz,
                                 u64p, sz, u64p, vp, sz, u64p]),
        "ZraHipArchiveCutRecords": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz,
                                        u64p, sz, u64p, vp, sz, u64p]),
        # tally records: the primitive over packed text in device memory; the composites take the cut's arguments up to stagingBytes, then the workspace, then
        # the primitive's from maxDistinct on
        "ZraHipTallyRecords": (S, [vp, vp, sz, ctypes.c_uint8, ctypes.c_uint64, u64p, sz, vp, sz, u64p, u64p, u64p, u64p]),
        "ZraHipTallyFields": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz,
                                  vp, sz, u64p, ctypes.c_uint64, u64p, sz, vp, sz, u64p, u64p, u64p, u64p]),
        "ZraHipArchiveTallyFields": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz,
                                         vp, sz, u64p, ctypes.c_uint64, u64p, sz, vp, sz, u64p, u64p, u64p, u64p]),
        "ZraHipGetTallyStats": (None, [vp, u64p]),
        "ZraHipDebugTallyMs": (ctypes.c_double, [vp]),
        "ZraHipDebugTallyHashBits": (None, [vp, u32]),
        # the grep with context records: before and after behind `mode`, |S| and the groups behind nRecords
        "ZraHipGrepArchiveContext": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, u32, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p,
                                         u64p, u64p]),
        "ZraHipArchiveGrepContext": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, u32, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, u64p,
                                         u64p]),
        # the grep with regular expressions: the syntax word behind nPatterns; ZraHipRegexInfo is five 32-bit words
        "ZraHipCheckRegex": (S, [vp, ctypes.POINTER(u32), sz, u32, ctypes.c_int, ctypes.POINTER(u32)]),
        "ZraHipGrepArchiveRegex": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        "ZraHipArchiveGrepRegex": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p]),
        # the extract with regular expressions: ZraHipExtractRecordsExpr's arguments
        "ZraHipExtractRecordsRegex": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp,
                                          sz, u64p]),
        "ZraHipArchiveExtractRecordsRegex": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, vp, sz,
                                                 u64p]),
        # the regex grep with context records: ZraHipGrepArchiveContext's arguments
        "ZraHipGrepArchiveRegexContext": (S, [vp, vp, sz, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, u32, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz,
                                              u64p, u64p, u64p]),
        "ZraHipArchiveGrepRegexContext": (S, [vp, vp, ctypes.POINTER(u32), sz, u32, ctypes.c_uint8, u32, u32, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p,
                                              u64p, u64p]),
        # compare
        "ZraHipCompareArchives": (S, [vp, vp, sz, vp, sz, u32, ctypes.c_uint64, ctypes.c_uint64, sz, u64p, sz, u64p, u64p]),
        "ZraHipGetCompareStats": (None, [vp, u64p]),
        "ZraHipGetCompareSizes": (None, [vp, u64p]),
        "ZraHipDebugCompareMs": (ctypes.c_double, [vp]),
        # diff
        "ZraHipDiffArchives": (S, [vp, vp, sz, vp, sz, u32, u32, sz, u64p, u64p, u64p, sz, u64p, vp, sz, u64p, u64p, u64p]),
        "ZraHipGetDiffStats": (None, [vp, u64p]),
        "ZraHipDebugDiffMs": (ctypes.c_double, [vp]),
        # content signatures
        "ZraHipSignArchive": (S, [vp, vp, sz, u32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz, vp, sz, ctypes.POINTER(ZraHipSignature)]),
        "ZraHipGetSignStats": (None, [vp, u64p]),
        "ZraHipDebugSignMs": (ctypes.c_double, [vp]),
        "ZraHipDiffSignature": (S, [vp, ctypes.POINTER(ZraHipSignature), vp, sz, vp, sz, u32, sz, u64p, u64p, u64p, sz, u64p, vp, sz, u64p, u64p, u64p]),
        "ZraHipGetDiffSignatureStats": (None, [vp, u64p]),
        "ZraHipDebugDiffSignatureMs": (ctypes.c_double, [vp]),
        # record index
        "ZraHipIndexRecords": (S, [vp, vp, sz, u32, ctypes.c_uint64, ctypes.c_uint64, sz, vp, sz, ctypes.POINTER(ZraHipRecordIndex)]),
        "ZraHipGetIndexRecordsStats": (None, [vp, u64p]),
        "ZraHipDebugIndexRecordsMs": (ctypes.c_double, [vp]),
        "ZraHipLocateRecords": (S, [vp, vp, sz, ctypes.POINTER(ZraHipRecordIndex), vp, sz, u64p, sz, sz, u64p]),
        "ZraHipGetLocateRecordsStats": (None, [vp, u64p]),
        "ZraHipDebugLocateRecordsMs": (ctypes.c_double, [vp]),
        "ZraHipReadRecords": (S, [vp, vp, sz, ctypes.POINTER(ZraHipRecordIndex), vp, sz, u64p, sz, sz, u64p, vp, sz, u64p]),
        "ZraHipGetReadRecordsStats": (None, [vp, u64p]),
        "ZraHipDebugReadRecordsMs": (ctypes.c_double, [vp]),
        # distributed archive
        "ZraHipShardRange": (None, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u64p, u64p]),
        "ZraHipOwnerOfFrame": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64]),
        "ZraHipRouteQueries": (S, [ctypes.c_uint64, u32, ctypes.c_int, u64p, u64p, sz, ctypes.POINTER(ZraHipSlice), sz, szp, u64p]),
        "ZraHipCommGetUniqueId": (S, [vp]),
        "ZraHipCommCreateRccl": (S, [ctypes.POINTER(vp), vp, vp, ctypes.c_int, ctypes.c_int]),
        "ZraHipCommCreateHost": (S, [ctypes.POINTER(vp), vp, ctypes.POINTER(ZraHipHostTransport), ctypes.c_int, ctypes.c_int]),
        "ZraHipCommLoopback": (S, [vp, vp, vp, sz]),
        "ZraHipCommDestroy": (None, [vp]),
        "ZraHipCommCompress": (S, [vp, vp, sz, ctypes.c_uint64, ctypes.c_int8, u32, ctypes.c_bool, ctypes.POINTER(vp)]),
        "ZraHipShardDestroy": (None, [vp]),
        "ZraHipShardHeaderSize": (sz, [vp]),
        "ZraHipShardGetHeader": (None, [vp, vp]),
        "ZraHipShardArchiveSize": (ctypes.c_uint64, [vp]),
        "ZraHipShardGetBody": (None, [vp, ctypes.POINTER(vp), u64p, u64p]),
        "ZraHipCommGatherArchive": (S, [vp, vp, ctypes.c_int, vp, sz, szp]),
        "ZraHipCommUseOwnStream": (S, [vp]),
        "ZraHipCommGatherArchiveBegin": (S, [vp, vp, ctypes.c_int, vp, sz]),
        "ZraHipCommGatherArchiveEnd": (S, [vp, szp]),
        "ZraHipCommServe": (S, [vp, vp, u64p, u64p, u64p, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == a symbol include/*.h declares is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


C_ABI_SYMBOLS = [
    "ZraGetVersion", "ZraGetErrorString", "ZraCreateHeader", "ZraCreateHeader2", "ZraDeleteHeader", "ZraGetVersionWithHeader",
    "ZraGetHeaderSizeWithHeader", "ZraGetUncompressedSizeWithHeader", "ZraGetFrameSizeWithHeader", "ZraGetMetadataSize", "ZraGetMetadata",
    "ZraGetCompressedOutputBufferSize", "ZraCompressBuffer", "ZraDecompressBuffer", "ZraDecompressRA", "ZraCreateCompressor",
    "ZraDeleteCompressor", "ZraGetOutputBufferSizeWithCompressor", "ZraCompressWithCompressor", "ZraGetHeaderSizeWithCompressor",
    "ZraGetHeaderWithCompressor", "ZraCreateDecompressor", "ZraDeleteDecompressor", "ZraGetHeaderWithDecompressor",
    "ZraDecompressWithDecompressor", "ZraCreateFullDecompressor", "ZraDeleteFullDecompressor", "ZraGetHeaderWithFullDecompressor",
    "ZraDecompressWithFullDecompressor",
]
HIP_ABI_SYMBOLS = ["ZraHipDeviceCount", "ZraHipCreateEngine", "ZraHipDestroyEngine", "ZraHipSynchronize", "ZraHipGetStream", "ZraHipWaitStream", "ZraHipReleaseScratch", "ZraHipLastKernelMs", "ZraHipGetKernelStats", "ZraHipGetDecodeStageStats", "ZraHipGetLaunchTelemetry",
                   "ZraHipCompressBuffer", "ZraHipDecompressBuffer", "ZraHipDecompressRABatch", "ZraHipCompressFrames", "ZraHipStitchHeader", "ZraHipDebugReadSeqs", "ZraHipSetOptions", "ZraHipGetOptions",
                   "ZraHipShardRange", "ZraHipOwnerOfFrame", "ZraHipRouteQueries", "ZraHipCommGetUniqueId", "ZraHipCommCreateRccl", "ZraHipCommCreateHost", "ZraHipCommLoopback", "ZraHipCommDestroy",
                   "ZraHipCommCompress", "ZraHipCommStitchSizes", "ZraHipShardDestroy", "ZraHipShardHeaderSize", "ZraHipShardGetHeader", "ZraHipShardArchiveSize", "ZraHipShardGetBody",
                   "ZraHipCommGatherArchive", "ZraHipCommUseOwnStream", "ZraHipCommGatherArchiveBegin", "ZraHipCommGatherArchiveEnd", "ZraHipCommServe",
                   "ZraHipArchiveOpen", "ZraHipArchiveClose", "ZraHipArchiveRead", "ZraHipArchiveDropCache", "ZraHipArchiveGetStats",
                   "ZraHipArchiveUpdate", "ZraHipArchiveGetUpdateStats", "ZraHipDebugUpdateStageMs",
                   "ZraHipArchiveSearch", "ZraHipArchiveSearchMulti", "ZraHipArchiveGrep", "ZraHipArchiveExtractRecords", "ZraHipArchiveGetScanStats",
                   "ZraHipDebugArchiveScanStageMs", "ZraHipDebugArchiveArena",
                   "ZraHipArchiveIndexRecords", "ZraHipArchiveLocateRecords", "ZraHipArchiveReadRecords", "ZraHipArchiveGetRecordStats",
                   "ZraHipDebugArchiveRecordStageMs",
                   "ZraHipUpdateArchive", "ZraHipGetUpdateStats", "ZraHipVerifyArchive", "ZraHipGetVerifyStats",
                   "ZraHipSearchArchive", "ZraHipGetSearchStats", "ZraHipDebugSearchScanMs",
                   "ZraHipSearchArchiveMulti", "ZraHipGetSearchMultiStats", "ZraHipDebugSearchMultiScanMs",
                   "ZraHipGrepArchive", "ZraHipGetGrepStats", "ZraHipDebugGrepScanMs",
                   "ZraHipExtractRecords", "ZraHipGetExtractStats", "ZraHipDebugExtractMs",
                   "ZraHipCheckPatternExpr", "ZraHipSearchArchiveMultiExpr", "ZraHipGrepArchiveExpr", "ZraHipExtractRecordsExpr",
                   "ZraHipArchiveSearchMultiExpr", "ZraHipArchiveGrepExpr", "ZraHipArchiveExtractRecordsExpr",
                   "ZraHipCheckRecordClauses", "ZraHipGrepArchiveWhere", "ZraHipArchiveGrepWhere", "ZraHipExtractRecordsWhere", "ZraHipArchiveExtractRecordsWhere",
                   "ZraHipFieldMask", "ZraHipCutRecords", "ZraHipArchiveCutRecords",
                   "ZraHipTallyRecords", "ZraHipTallyFields", "ZraHipArchiveTallyFields", "ZraHipGetTallyStats", "ZraHipDebugTallyMs", "ZraHipDebugTallyHashBits",
                   "ZraHipGrepArchiveContext", "ZraHipArchiveGrepContext",
                   "ZraHipCheckRegex", "ZraHipGrepArchiveRegex", "ZraHipArchiveGrepRegex",
                   "ZraHipExtractRecordsRegex", "ZraHipArchiveExtractRecordsRegex",
                   "ZraHipGrepArchiveRegexContext", "ZraHipArchiveGrepRegexContext",
                   "ZraHipCompareArchives", "ZraHipGetCompareStats", "ZraHipGetCompareSizes", "ZraHipDebugCompareMs",
                   "ZraHipDiffArchives", "ZraHipGetDiffStats", "ZraHipDebugDiffMs",
                   "ZraHipSignArchive", "ZraHipGetSignStats", "ZraHipDebugSignMs",
                   "ZraHipDiffSignature", "ZraHipGetDiffSignatureStats", "ZraHipDebugDiffSignatureMs",
                   "ZraHipIndexRecords", "ZraHipGetIndexRecordsStats", "ZraHipDebugIndexRecordsMs",
                   "ZraHipLocateRecords", "ZraHipGetLocateRecordsStats", "ZraHipDebugLocateRecordsMs",
                   "ZraHipReadRecords", "ZraHipGetReadRecordsStats", "ZraHipDebugReadRecordsMs"]


def _chk(st, what=""):
    if st.zra != 0:
        raise ZraError(st.tup(), what)


def _cbuf(b):
    return (ctypes.c_char * max(len(b), 1)).from_buffer_copy(bytes(b) if len(b) else b"\0")


# ---------------------------------------------------------------------------------------------------------------
# host-pointer calls — same names and argument meaning as the reference's zra:: free functions (zra.hpp:139-194)
def GetOutputBufferSize(input_size, frame_size):
    return load().ZraGetCompressedOutputBufferSize(input_size, frame_size)


def CompressBuffer(data, compressionLevel=0, frameSize=16384, checksum=True, meta=b""):
    L = load()
    cap = L.ZraGetCompressedOutputBufferSize(len(data), frameSize)
    out = ctypes.create_string_buffer(cap)
    osz = ctypes.c_size_t(0)
    mb = _cbuf(meta)
    _chk(L.ZraCompressBuffer(_cbuf(data), len(data), out, ctypes.byref(osz), compressionLevel, frameSize, checksum, mb if len(meta) else None, len(meta)))
    return out.raw[: osz.value]


def DecompressBuffer(archive):
    L = load()
    n = int.from_bytes(bytes(archive[18:26]), "little") if len(archive) >= 26 else 0
    out = ctypes.create_string_buffer(max(n, 1))
    _chk(L.ZraDecompressBuffer(_cbuf(archive), len(archive), out))
    return out.raw[:n]


def DecompressRA(archive, offset, size):
    L = load()
    out = ctypes.create_string_buffer(max(size, 1))
    _chk(L.ZraDecompressRA(_cbuf(archive), len(archive), out, offset, size))
    return out.raw[:size]


# ---------------------------------------------------------------------------------------------------------------
class Engine:
    """Device-pointer engine (include/zra_hip.h). Pointers are plain integers (e.g. torch tensor .data_ptr())."""

    def __init__(self, device=0):
        self.L = load()
        h = ctypes.c_void_p()
        _chk(self.L.ZraHipCreateEngine(ctypes.byref(h), device), "ZraHipCreateEngine")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.L.ZraHipDestroyEngine(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        return self.L.ZraHipGetStream(self.h)

    def wait_stream(self, stream_handle=None):
        """Orders the engine's streams behind work queued on `stream_handle` (a hipStream_t as int; None = the null stream)."""
        _chk(self.L.ZraHipWaitStream(self.h, ctypes.c_void_p(stream_handle or 0)))

    def release_scratch(self):
        """Hands the engine's (grow-only) scratch back to the device."""
        _chk(self.L.ZraHipReleaseScratch(self.h))

    def _order(self):
        # inputs are usually torch tensors produced asynchronously on torch's current stream: make the engine wait for that stream
        # (event wait, no host sync). Plumbing only; C callers use ZraHipWaitStream / their own synchronisation (zra_hip.h).
        t = sys.modules.get("torch")
        if t is not None and t.cuda.is_available():
            self.wait_stream(t.cuda.current_stream(device=self.device).cuda_stream)      # the ENGINE's device, whatever torch's current one is

    def last_kernel_ms(self):
        return self.L.ZraHipLastKernelMs(self.h)

    def kernel_stats(self):
        """{mf_ms, mf_launches, ent_ms, ent_launches, dec_ms, dec_launches} of the last call (HIP events on the engine stream)."""
        a = (ctypes.c_double * 6)()
        self.L.ZraHipGetKernelStats(self.h, a)
        return dict(mf_ms=a[0], mf_launches=int(a[1]), ent_ms=a[2], ent_launches=int(a[3]), dec_ms=a[4], dec_launches=int(a[5]))

    def launch_telemetry(self):
        """What the waves of the last persistent level-3/4 match-finder launch recorded (zra_hip.h: ZraHipGetLaunchTelemetry), reduced:
        effective shader MHz, waves per compute unit (min / max / histogram), waves, frames and frames per wave-second per XCD, the stagger
        of the wave starts and ends. None when the last call took another path."""
        cap = 32 + 2048 + 8 + 2048
        a = (ctypes.c_uint64 * cap)()
        n = self.L.ZraHipGetLaunchTelemetry(self.h, a, cap)
        if n < 32 or a[2] == 0:
            return None
        M = (1 << 64) - 1
        cuw = [int(v) for v in a[32:32 + 2048] if v]
        simd = [[(v >> (16 * k)) & 0xFFFF for k in range(4)] for v in cuw]        # a CU's word: four 16-bit counts, one per SIMD
        cu = [sum(q) for q in simd]
        shist = {}
        for q in simd:
            k = "/".join(str(x) for x in sorted(q, reverse=True)); shist[k] = shist.get(k, 0) + 1
        ent = None
        if n >= 2080 + 8:
            ecu = [int(v) for v in a[2088:n] if v]
            ent = dict(workgroups=int(a[2080]), cus=len(ecu), workgroups_per_cu_max=max(ecu) if ecu else 0, frames=int(a[2083]),
                       resident_ms_mean=round(a[2081] / max(1, a[2080]) / 1e5, 3), waiting_frac=round(a[2082] / max(1, a[2081]), 4),
                       ms_per_frame=round((a[2081] - a[2082]) / max(1, a[2083]) / 1e5, 4))
        hist = {}
        for v in cu:
            hist[v] = hist.get(v, 0) + 1
        first_start, last_end, last_start, first_end = M - a[4], a[5], a[6], M - a[7]
        return dict(shader_mhz=round(a[0] / max(1, a[1]) * 100.0, 1), waves=int(a[2]), cus=len(cu),
                    waves_per_cu_min=min(cu) if cu else 0, waves_per_cu_max=max(cu) if cu else 0,
                    waves_per_cu_hist={str(k): hist[k] for k in sorted(hist)}, waves_per_simd_hist=shist,
                    waves_per_xcd=[int(v) for v in a[8:16]], frames_per_xcd=[int(v) for v in a[16:24]],
                    frames_per_wave_ms_per_xcd=[round(a[16 + i] / (a[24 + i] / 1e5), 4) if a[24 + i] else 0.0 for i in range(8)],
                    span_ms=round((last_end - first_start) / 1e5, 3), start_stagger_ms=round((last_start - first_start) / 1e5, 3),
                    end_stagger_ms=round((last_end - first_end) / 1e5, 3), longest_wave_ms=round(a[3] / 1e5, 3), entropy=ent)

    def decode_stage_stats(self):
        """{parse_ms, huf_ms, chain_ms, exec_ms, rounds, small_ms, small_launches} of the last decode / random-access call."""
        a = (ctypes.c_double * 8)()
        self.L.ZraHipGetDecodeStageStats(self.h, a)
        return dict(parse_ms=a[0], huf_ms=a[1], chain_ms=a[2], exec_ms=a[3], rounds=int(a[4]), small_ms=a[5], small_launches=int(a[6]))

    def debug_read_seqs(self, frame, cap=65536):
        """bring-up: [(litLength, matchLength, offsetValue)] of `frame` in the last batch + (nbSeq, lastLL, skip)."""
        buf = (ctypes.c_uint64 * cap)(); meta = (ctypes.c_uint32 * 3)()
        self.L.ZraHipDebugReadSeqs.restype = ctypes.c_uint32
        n = self.L.ZraHipDebugReadSeqs(self.h, ctypes.c_uint32(frame), buf, ctypes.c_uint32(cap), meta)
        return [(int(v) & 0xFFFFF, (int(v) >> 20) & 0xFFFFF, int(v) >> 40) for v in buf[:n]], tuple(meta)

    def compress(self, d_in, in_size, d_out, level=3, frame_size=65536, checksum=True):
        osz = ctypes.c_size_t(0)
        self._order()
        _chk(self.L.ZraHipCompressBuffer(self.h, d_in, in_size, d_out, ctypes.byref(osz), level, frame_size, checksum))
        return osz.value

    def decompress(self, d_in, in_size, d_out, out_cap):
        self._order()
        _chk(self.L.ZraHipDecompressBuffer(self.h, d_in, in_size, d_out, out_cap))

    def decompress_ra_batch(self, d_in, in_size, d_out, offsets, sizes, out_offsets):
        import numpy as np
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        s = np.ascontiguousarray(sizes, dtype=np.uint64)
        oo = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        self._order()
        _chk(self.L.ZraHipDecompressRABatch(self.h, d_in, in_size, d_out, p(o), p(s), p(oo), len(o)))

    def compress_frames(self, d_in, in_size, d_body, d_sizes, level=3, frame_size=65536, checksum=True):
        bsz = ctypes.c_size_t(0)
        self._order()
        _chk(self.L.ZraHipCompressFrames(self.h, d_in, in_size, d_body, d_sizes, ctypes.byref(bsz), level, frame_size, checksum))
        return bsz.value

    def update(self, d_archive, size, d_out, out_cap, *, writes=None, d_data=0, d_append=0, append_size=0, level=3, checksum=True):
        """ZraHipUpdateArchive: the archive at d_archive (size bytes) with `writes` = (offsets, sizes, data_offsets) applied (bytes of the
        content replaced by d_data + data_offset) and append_size bytes from d_append added, written to d_out. Returns the new size.
        OutputBufferTooSmall carries the size needed in ZraError.needed."""
        import numpy as np
        o, s, do = (np.ascontiguousarray(a, dtype=np.uint64) for a in (writes if writes is not None else ((), (), ())))
        if not (len(o) == len(s) == len(do)):
            raise ValueError("writes: offsets, sizes and data_offsets differ in length")
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if len(a) else None
        osz = ctypes.c_size_t(0)
        self._order()
        st = self.L.ZraHipUpdateArchive(self.h, d_archive or None, size, d_data or None, p(o), p(s), p(do), len(o), d_append or None, append_size,
                                        d_out or None, out_cap, ctypes.byref(osz), level, checksum)
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipUpdateArchive")
            e.needed = osz.value
            raise e
        return osz.value

    def update_stats(self):
        """Counters of the last update() on this engine (all zero unless it succeeded), keyed by UPDATE_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetUpdateStats(self.h, a)
        return dict(zip(UPDATE_STATS, (int(v) for v in a)))

    def verify(self, d_archive, size, *, content=True, first_frame=0, frame_count=None, staging_bytes=0, max_faults=1 << 16):
        """ZraHipVerifyArchive over frames [first_frame, first_frame + frame_count) (None: to the end) of the archive at d_archive:
        header CRC-32, seek table and block walk of every frame, and with `content` every sound frame decoded and its checksum verified.
        Returns (n_faults, [(frame, code, stage), ...]): every faulty frame is counted, the first max_faults are listed, in frame order.
        Faulty frames are data; ZraError is a call that could not verify (bad header, range outside the archive, no memory)."""
        arr = (ZraHipFrameFault * max_faults)() if max_faults else None
        n = ctypes.c_size_t(0)
        self._order()
        _chk(self.L.ZraHipVerifyArchive(self.h, d_archive or None, size, VERIFY_CONTENT if content else VERIFY_STRUCTURE, first_frame,
                                        (1 << 64) - 1 if frame_count is None else frame_count, staging_bytes, arr, max_faults, ctypes.byref(n)),
             "ZraHipVerifyArchive")
        return n.value, [(int(arr[i].frame), int(arr[i].code), int(arr[i].stage)) for i in range(min(n.value, max_faults))]

    def verify_stats(self):
        """Counters of the last verify() on this engine (all zero unless it succeeded), keyed by VERIFY_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetVerifyStats(self.h, a)
        return dict(zip(VERIFY_STATS, (int(v) for v in a[:7])))

    def search(self, d_archive, size, pattern, *, offset=0, length=None, staging_bytes=0, max_matches=1 << 20):
        """ZraHipSearchArchive: the content offsets at which `pattern` (1 .. SEARCH_MAX_PATTERN bytes, literal) occurs whole inside
        [offset, offset + length) (None: to the end) of the content of the archive at d_archive. Returns (n_matches, [offsets]): every
        match is counted, overlapping ones included, and the first max_matches are listed in ascending order. ZraError is a call that
        could not search (bad header, range outside the content, a frame of the range that does not decode, no memory)."""
        pattern = bytes(pattern)
        arr = (ctypes.c_uint64 * max_matches)() if max_matches else None
        n = ctypes.c_uint64(0)
        self._order()
        _chk(self.L.ZraHipSearchArchive(self.h, d_archive or None, size, _cbuf(pattern), len(pattern), offset,
                                        (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_matches, ctypes.byref(n)),
             "ZraHipSearchArchive")
        return n.value, [int(v) for v in arr[:min(n.value, max_matches)]] if arr is not None else []

    def search_stats(self):
        """Counters of the last search() on this engine (all zero unless it succeeded), keyed by SEARCH_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetSearchStats(self.h, a)
        return dict(zip(SEARCH_STATS, (int(v) for v in a[:6])))

    def search_scan_ms(self):
        """bring-up: HIP-event time of the last search()'s scan launches, summed over its passes (its decode: kernel_stats()['dec_ms'])."""
        return self.L.ZraHipDebugSearchScanMs(self.h)

    def search_multi(self, d_archive, size, patterns, *, offset=0, length=None, staging_bytes=0, max_matches=1 << 20, syntax=0):
        """ZraHipSearchArchiveMulti: where each of `patterns` (1 .. SEARCH_MAX_PATTERNS byte strings of 1 .. SEARCH_MAX_PATTERN bytes,
        SEARCH_MAX_PATTERN_BYTES in all, literal) occurs whole inside [offset, offset + length) (None: to the end) of the content of
        the archive at d_archive, in one decode of the range. Returns (n_matches, [(offset, pattern index)], per_pattern): every match
        is counted, the first max_matches are listed in ascending (offset, pattern index) order, and per_pattern[i] counts the matches
        of patterns[i], listed or not. syntax: PATTERN_FOLD_CASE | PATTERN_CLASSES (ZraHipSearchArchiveMultiExpr; lengths are then
        counted in elements). ZraError is a call that could not search."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ZraHipPatternMatch * max_matches)() if max_matches else None
        per = (ctypes.c_uint64 * max(len(patterns), 1))()
        n = ctypes.c_uint64(0)
        self._order()
        fn, sx = _scan_call(self.L, "ZraHipSearchArchiveMulti", syntax)
        _chk(fn(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, offset,
                (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_matches, ctypes.byref(n), per), fn.__name__)
        listed = [(int(arr[i].offset), int(arr[i].pattern)) for i in range(min(n.value, max_matches))] if arr is not None else []
        return n.value, listed, [int(v) for v in per[:len(patterns)]]

    def search_multi_stats(self):
        """Counters of the last search_multi() on this engine (all zero unless it succeeded), keyed by SEARCH_MULTI_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetSearchMultiStats(self.h, a)
        return dict(zip(SEARCH_MULTI_STATS, (int(v) for v in a)))

    def search_multi_scan_ms(self):
        """bring-up: HIP-event time of the last search_multi()'s scan launches, summed over its passes."""
        return self.L.ZraHipDebugSearchMultiScanMs(self.h)

    def grep(self, d_archive, size, patterns, *, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=1 << 20, syntax=0,
             where=None):
        """ZraHipGrepArchive: the records of [offset, offset + length) (None: to the end) of the content of the archive at d_archive,
        cut at the byte `delimiter`, in which one of `patterns` (search_multi's, none holding the delimiter) occurs; invert: those in
        which none does. Returns (n_records, [(offset, size)]): every selected record is counted and the first max_records are listed
        in ascending order, without their delimiter. max_records=0 is `grep -c`. syntax: search_multi's (ZraHipGrepArchiveExpr).
        where: a non-empty list of clauses (all, any, none), each term an int mask or an iterable of pattern indices
        (ZraHipGrepArchiveWhere): a record is selected when some clause holds for the set of patterns that occur in it; invert
        complements that. ZraError is a call that could not grep."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n = ctypes.c_uint64(0)
        self._order()
        fn, sx, wx = _grep_call(self.L, "ZraHipGrepArchive", syntax, where)
        _chk(fn(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, delimiter,
                GREP_INVERT if invert else 0, *wx, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                max_records, ctypes.byref(n)), fn.__name__)
        k = min(n.value, max_records)
        return n.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def grep_context(self, d_archive, size, patterns, *, before=0, after=0, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0,
                     max_records=1 << 20, syntax=0):
        """ZraHipGrepArchiveContext: grep()'s selected records (patterns, syntax, delimiter, invert and the range as there) with the
        `before` records in front of and the `after` records behind each of them (`grep -B -A`; each at most GREP_MAX_CONTEXT), inside the
        range. Returns (n_records, n_selected, n_groups, [(offset, size, selected)]): every output record is counted, the first
        max_records are listed in ascending order, each once; a group is a run of consecutive output records (what grep separates by
        `--`). Writes grep_stats(), whose `selected` is n_records. ZraError is a call that could not grep."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ns, ng = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._order()
        _chk(self.L.ZraHipGrepArchiveContext(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), syntax, delimiter,
                                             GREP_INVERT if invert else 0, before, after, offset, (1 << 64) - 1 if length is None else length, staging_bytes,
                                             arr, max_records, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(ng)), "ZraHipGrepArchiveContext")
        return n.value, ns.value, ng.value, _context_list(arr, min(n.value, max_records))

    def grep_regex(self, d_archive, size, patterns, *, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None, staging_bytes=0,
                   max_records=1 << 20):
        """ZraHipGrepArchiveRegex: grep()'s records of the range that one of `patterns` matches: POSIX extended regular expressions
        over bytes (check_regex), alternatives as with grep -e A -e B; invert: the records none matches; fold_case: grep -i. Returns
        (n_records, [(offset, size)]) as grep() does and writes grep_stats(), whose `matches` is the number of matched records.
        ZraError is a call that could not grep."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n = ctypes.c_uint64(0)
        self._order()
        _chk(self.L.ZraHipGrepArchiveRegex(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0,
                                           delimiter, GREP_INVERT if invert else 0, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                                           max_records, ctypes.byref(n)), "ZraHipGrepArchiveRegex")
        k = min(n.value, max_records)
        return n.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def grep_regex_context(self, d_archive, size, patterns, *, before=0, after=0, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None,
                           staging_bytes=0, max_records=1 << 20):
        """ZraHipGrepArchiveRegexContext: grep_regex()'s selected records (expressions, delimiter, invert, fold_case and the range as
        there) with the `before` records in front of and the `after` records behind each of them (`grep -E -B -A`; each at most
        GREP_MAX_CONTEXT), inside the range. Returns what grep_context() returns, (n_records, n_selected, n_groups,
        [(offset, size, selected)]), and writes grep_stats(), whose `selected` is n_records and whose `matches` is the number of
        matched records. ZraError is a call that could not grep."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ns, ng = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._order()
        _chk(self.L.ZraHipGrepArchiveRegexContext(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns),
                                                  PATTERN_FOLD_CASE if fold_case else 0, delimiter, GREP_INVERT if invert else 0, before, after, offset,
                                                  (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records, ctypes.byref(n), ctypes.byref(ns),
                                                  ctypes.byref(ng)), "ZraHipGrepArchiveRegexContext")
        return n.value, ns.value, ng.value, _context_list(arr, min(n.value, max_records))

    def grep_stats(self):
        """Counters of the last grep() on this engine (all zero unless it succeeded), keyed by GREP_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetGrepStats(self.h, a)
        return dict(zip(GREP_STATS, (int(v) for v in a)))

    def grep_scan_ms(self):
        """bring-up: HIP-event time of the last grep()'s scan launches, summed over its passes."""
        return self.L.ZraHipDebugGrepScanMs(self.h)

    def extract(self, d_archive, size, patterns, d_data, data_cap, *, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=0,
                syntax=0, where=None):
        """ZraHipExtractRecords: grep()'s selected records with their bytes, from one decode pass. For each selected record, in ascending
        order, its content and then one `delimiter` byte lie packed at d_data (data_cap bytes, device memory): the text `grep` prints.
        Returns (n_records, data_size, [(offset, size)]); the list is filled iff max_records != 0. OutputBufferTooSmall (more than
        max_records records when a list is wanted, or more than data_cap bytes) carries what the call needs in ZraError.needed_records
        and ZraError.needed_data; d_data=0, data_cap=0 is the sizing call. syntax: search_multi's (ZraHipExtractRecordsExpr). where:
        grep()'s clauses (ZraHipExtractRecordsWhere): the records grep(where=...) selects, the text `grep A | grep B | grep -v C`
        prints. ZraError otherwise is a call that could not extract."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._order()
        fn, sx, wx = _grep_call(self.L, "ZraHipExtractRecords", syntax, where)
        st = fn(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, delimiter,
                GREP_INVERT if invert else 0, *wx, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                max_records, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), fn.__name__)
            e.needed_records, e.needed_data = n.value, ds.value
            raise e
        k = n.value if max_records else 0
        return n.value, ds.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def cut(self, d_archive, size, patterns, d_data, data_cap, *, separator, fields, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0,
            max_records=0, syntax=0):
        """ZraHipCutRecords: extract()'s selected records, of each only the chosen fields: the text `grep -F patterns | cut -d SEP -f LIST`
        prints, packed at d_data from one decode pass. separator: the byte that ends a field; fields: cut's LIST as a string ("1,3,5-7,9-")
        or a mask (field_mask()). No pattern selects every record, plain cut. Returns and raises as extract() does."""
        return _cut_call(self.L, self.L.ZraHipCutRecords, (self.h, d_archive or None, size), self._order, patterns, d_data, data_cap, separator, fields, delimiter,
                         invert, offset, length, staging_bytes, max_records, syntax)

    def tally_text(self, d_text, size, *, delimiter=0x0A, max_distinct=0, d_keys=0, key_cap=0, max_entries=1 << 16):
        """ZraHipTallyRecords: the distinct records of `size` bytes of packed text at d_text (device memory; what extract() and cut() write),
        cut at `delimiter`, in order of first appearance, each with its count: `sort | uniq -c` in the order of `awk '!seen[$0]++'`.
        Returns (n_records, n_skipped, [(offset, size, count)]): offset and size locate the key's first occurrence in the text; a record
        longer than TALLY_MAX_KEY is skipped. d_keys / key_cap (optional): the keys as text, each with its delimiter; its size and the other
        words of the call are in self.last_tally. max_distinct: a promise that sizes the hash table (0: none). ZraError for a refused call;
        OutputBufferTooSmall carries n_records, n_skipped, needed_entries and needed_keys."""
        return _tally_call(self, lambda tail: self.L.ZraHipTallyRecords(self.h, d_text or None, size, delimiter, *tail), "ZraHipTallyRecords", None, max_distinct,
                           d_keys, key_cap, max_entries)

    def tally(self, d_archive, size, patterns, d_work, work_cap, *, separator, fields, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, syntax=0,
              max_distinct=0, d_keys=0, key_cap=0, max_entries=1 << 16):
        """ZraHipTallyFields: cut() into the workspace d_work (device memory, work_cap bytes), then tally_text() of what it packed: the counts
        `grep -F patterns | cut -d SEP -f LIST | sort | uniq -c` prints. Arguments as cut() and tally_text(); fields=(1 << 64) - 1 tallies
        whole records. Returns as tally_text(), the offsets pointing into d_work; self.last_tally["work_size"] is the cut's packed size,
        also when it says what d_work needs (ZraError.needed_work)."""
        return _tally_call(self, None, "ZraHipTallyFields", (self.L.ZraHipTallyFields, (self.h, d_archive or None, size), patterns, separator, fields, delimiter, invert,
                                                             offset, length, staging_bytes, syntax, d_work, work_cap), max_distinct, d_keys, key_cap, max_entries)

    def tally_stats(self):
        """Counters of the last tally_text() / tally() on this engine (all zero unless it succeeded), keyed by TALLY_STATS. longest_probe
        and table_inserts depend on the order in which lanes arrive; nothing else does."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetTallyStats(self.h, a)
        return dict(zip(TALLY_STATS, (int(v) for v in a)))

    def tally_ms(self):
        """bring-up: HIP-event time of the last tally's own launches."""
        return self.L.ZraHipDebugTallyMs(self.h)

    def debug_tally_hash_bits(self, bits):
        """bring-up (ZraHipDebugTallyHashBits): the next tallies keep only the low `bits` bits of the key hash; 0 keeps none (every key
        starts probing at slot 0), None restores the full hash."""
        self.L.ZraHipDebugTallyHashBits(self.h, 0 if bits is None else (TALLY_HASH_NONE if bits == 0 else bits))

    def extract_regex(self, d_archive, size, patterns, d_data, data_cap, *, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None,
                      staging_bytes=0, max_records=0):
        """ZraHipExtractRecordsRegex: grep_regex()'s selected records with their bytes, packed at d_data as extract() packs them: the
        text `grep -E` prints, from one decode pass. Returns what extract() returns and writes extract_stats(), whose `matches` is the
        number of matched records; OutputBufferTooSmall carries ZraError.needed_records and ZraError.needed_data."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._order()
        st = self.L.ZraHipExtractRecordsRegex(self.h, d_archive or None, size, _cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0,
                                              delimiter, GREP_INVERT if invert else 0, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                                              max_records, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipExtractRecordsRegex")
            e.needed_records, e.needed_data = n.value, ds.value
            raise e
        k = n.value if max_records else 0
        return n.value, ds.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def extract_stats(self):
        """Counters of the last extract() on this engine (all zero unless it succeeded), keyed by EXTRACT_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetExtractStats(self.h, a)
        return dict(zip(EXTRACT_STATS, (int(v) for v in a)))

    def extract_ms(self):
        """bring-up: HIP-event time of the last extract()'s own launches, summed over its passes."""
        return self.L.ZraHipDebugExtractMs(self.h)

    def compare(self, d_a, size_a, d_b, size_b, *, decode_all=False, offset=0, length=None, staging_bytes=0, max_ranges=1 << 16):
        """ZraHipCompareArchives: the maximal runs of content positions inside [offset, offset + length) (None: to the end of the
        shorter content) at which the archives at d_a and d_b differ. Returns (n_ranges, differing_bytes, [(offset, size)]): every
        range is counted, and the first max_ranges are listed in ascending order. Frames whose compressed bytes agree are equal
        without a decode unless decode_all. The two content sizes: compare_sizes(). ZraError is a call that could not compare (bad
        header, different frame sizes, range outside the common content, a frame that had to be decoded and does not, no memory)."""
        arr = (ctypes.c_uint64 * (2 * max_ranges))() if max_ranges else None
        n, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._order()
        _chk(self.L.ZraHipCompareArchives(self.h, d_a or None, size_a, d_b or None, size_b, COMPARE_DECODE_ALL if decode_all else 0, offset,
                                          (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_ranges, ctypes.byref(n),
                                          ctypes.byref(nb)), "ZraHipCompareArchives")
        k = min(n.value, max_ranges)
        return n.value, nb.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def compare_stats(self):
        """Counters of the last compare() on this engine (all zero unless it succeeded), keyed by COMPARE_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetCompareStats(self.h, a)
        return dict(zip(COMPARE_STATS, (int(v) for v in a[:7])))

    def compare_sizes(self):
        """(UA, UB): the content sizes of the two archives of the last compare() (zero unless it succeeded)."""
        a = (ctypes.c_uint64 * 2)()
        self.L.ZraHipGetCompareSizes(self.h, a)
        return int(a[0]), int(a[1])

    def compare_ms(self):
        """bring-up: HIP-event time of the last compare()'s own launches, summed over its passes (its decode: kernel_stats()['dec_ms'])."""
        return self.L.ZraHipDebugCompareMs(self.h)

    def diff(self, d_a, size_a, d_b, size_b, d_data, data_cap, *, grain=1, decode_all=False, staging_bytes=0, max_writes=1 << 16):
        """ZraHipDiffArchives: the patch that gives the archive at d_a the content of the archive at d_b. Returns ((offsets, sizes,
        data_offsets), append_offset, append_size, data_size): three numpy u64 arrays, one entry per write (a maximal run of dirty
        grains of `grain` bytes), to be passed as `writes=` of update() with d_data=d_data; B's bytes of the writes lie packed at
        d_data (data_cap bytes, device memory), and B's append_size bytes behind A's content at d_data + append_offset.
        OutputBufferTooSmall (more than max_writes writes, or more than data_cap bytes) carries what the patch needs in
        ZraError.needed_writes and ZraError.needed_data. ZraError otherwise is a call that could not diff (bad header, different frame
        sizes, B shorter than A, a frame that had to be decoded and does not, no memory)."""
        import numpy as np
        o, s, do = (np.zeros(max_writes, dtype=np.uint64) for _ in range(3))
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if max_writes else None
        n, ds, ao, asz = (ctypes.c_uint64(0) for _ in range(4))
        self._order()
        st = self.L.ZraHipDiffArchives(self.h, d_a or None, size_a, d_b or None, size_b, DIFF_DECODE_ALL if decode_all else 0, grain, staging_bytes,
                                       p(o), p(s), p(do), max_writes, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds), ctypes.byref(ao),
                                       ctypes.byref(asz))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipDiffArchives")
            e.needed_writes, e.needed_data = n.value, ds.value
            raise e
        k = n.value
        return (o[:k].copy(), s[:k].copy(), do[:k].copy()), ao.value, asz.value, ds.value

    def diff_stats(self):
        """Counters of the last diff() on this engine (all zero unless it succeeded), keyed by DIFF_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetDiffStats(self.h, a)
        return dict(zip(DIFF_STATS, (int(v) for v in a)))

    def diff_ms(self):
        """bring-up: HIP-event time of the last diff()'s own launches, summed over its passes (its decodes: kernel_stats()['dec_ms'])."""
        return self.L.ZraHipDebugDiffMs(self.h)

    def sign(self, d_archive, size, d_sig, sig_cap_words, *, grain=4096, seed=0, first_frame=0, frame_count=None, staging_bytes=0):
        """ZraHipSignArchive: the XXH64 words of frames [first_frame, first_frame + frame_count) (None: to the last frame) of the
        archive at d_archive go into their records of the signature at d_sig (sig_cap_words 64-bit words, device memory): per frame
        one word over its compressed bytes and one per grain of its content. Returns the Signature of the WHOLE archive
        (content_size, frame_size, grain, seed, frames, words), which is what diff_signature() takes and what travels with the
        words. OutputBufferTooSmall (sig_cap_words < words) carries the words needed in ZraError.needed_words. ZraError otherwise
        is a call that could not sign (bad header, range outside the frames, a frame that does not decode, no memory)."""
        info = ZraHipSignature()
        self._order()
        st = self.L.ZraHipSignArchive(self.h, d_archive or None, size, grain, seed, first_frame, 0xFFFFFFFFFFFFFFFF if frame_count is None else frame_count,
                                      staging_bytes, d_sig or None, sig_cap_words, ctypes.byref(info))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipSignArchive")
            e.needed_words = info.words
            raise e
        return Signature(info.contentSize, info.frameSize, info.grain, info.seed, info.frames, info.words)

    def sign_stats(self):
        """Counters of the last sign() on this engine (all zero unless it succeeded), keyed by SIGN_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetSignStats(self.h, a)
        return dict(zip(SIGN_STATS, (int(v) for v in a)))

    def sign_ms(self):
        """bring-up: HIP-event time of the last sign()'s own launches (span hash, grain hash), summed over its passes."""
        return self.L.ZraHipDebugSignMs(self.h)

    def diff_signature(self, sig, d_sig, sig_words, d_b, size_b, d_data, data_cap, *, decode_all=False, staging_bytes=0, max_writes=1 << 16):
        """ZraHipDiffSignature: diff() of the archive at d_b against the SIGNATURE (sig: a Signature, d_sig: its sig_words words in
        device memory) of an archive that lies elsewhere, at the signature's grain. Returns what diff() returns and raises what it
        raises; equal 64-bit words are taken as equal content."""
        import numpy as np
        o, s, do = (np.zeros(max_writes, dtype=np.uint64) for _ in range(3))
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if max_writes else None
        n, ds, ao, asz = (ctypes.c_uint64(0) for _ in range(4))
        info = ZraHipSignature(*sig)
        self._order()
        st = self.L.ZraHipDiffSignature(self.h, ctypes.byref(info), d_sig or None, sig_words, d_b or None, size_b, SIGDIFF_DECODE_ALL if decode_all else 0,
                                        staging_bytes, p(o), p(s), p(do), max_writes, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds),
                                        ctypes.byref(ao), ctypes.byref(asz))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipDiffSignature")
            e.needed_writes, e.needed_data = n.value, ds.value
            raise e
        k = n.value
        return (o[:k].copy(), s[:k].copy(), do[:k].copy()), ao.value, asz.value, ds.value

    def diff_signature_stats(self):
        """Counters of the last diff_signature() on this engine (all zero unless it succeeded), keyed by SIGDIFF_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetDiffSignatureStats(self.h, a)
        return dict(zip(SIGDIFF_STATS, (int(v) for v in a)))

    def diff_signature_ms(self):
        """bring-up: HIP-event time of the last diff_signature()'s own launches, summed over its passes."""
        return self.L.ZraHipDebugDiffSignatureMs(self.h)

    def index_records(self, d_archive, size, d_index, index_cap_words, *, delimiter=0x0A, first_frame=0, frame_count=None, staging_bytes=0):
        """ZraHipIndexRecords: the record-index words of frames [first_frame, first_frame + frame_count) (None: to the last frame) of
        the archive at d_archive go into their places of the index at d_index (index_cap_words 64-bit words, device memory): per
        frame its delimiter count, bit 63 set when its last byte is no delimiter. Returns the RecordIndex of the WHOLE archive
        (content_size, frame_size, delimiter, frames, delimiters, records), the totals taken from all words as they lie at d_index:
        meaningful once every frame has been indexed. OutputBufferTooSmall (index_cap_words < frames) carries the words needed in
        ZraError.needed_words."""
        info = ZraHipRecordIndex()
        self._order()
        st = self.L.ZraHipIndexRecords(self.h, d_archive or None, size, delimiter, first_frame, 0xFFFFFFFFFFFFFFFF if frame_count is None else frame_count,
                                       staging_bytes, d_index or None, index_cap_words, ctypes.byref(info))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipIndexRecords")
            e.needed_words = info.frames
            raise e
        return RecordIndex(info.contentSize, info.frameSize, info.delimiter, info.frames, info.delimiters, info.records)

    def index_records_stats(self):
        """Counters of the last index_records() on this engine (all zero unless it succeeded), keyed by INDEX_RECORDS_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetIndexRecordsStats(self.h, a)
        return dict(zip(INDEX_RECORDS_STATS, (int(v) for v in a)))

    def index_records_ms(self):
        """bring-up: HIP-event time of the last index_records()'s own launches (tile counts, frame words, totals), summed over its passes."""
        return self.L.ZraHipDebugIndexRecordsMs(self.h)

    def locate_records(self, d_archive, size, index, d_index, index_words, numbers, *, staging_bytes=0):
        """ZraHipLocateRecords: [(offset, size)] of the records `numbers` (any order, duplicates allowed) of the archive at d_archive,
        in request order, by the RecordIndex `index` and its index_words words at d_index. Only the frames that hold a boundary
        are decoded, and each is checked against its word: ZraError (1, 20) is a stale word, OutOfBoundsAccess a number >= records."""
        import numpy as np
        nums = np.ascontiguousarray(np.asarray(numbers, dtype=np.uint64))
        n = int(nums.size)
        out = np.zeros(2 * max(n, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        info = ZraHipRecordIndex(*index)
        self._order()
        _chk(self.L.ZraHipLocateRecords(self.h, d_archive or None, size, ctypes.byref(info), d_index or None, index_words, p(nums) if n else None, n,
                                        staging_bytes, p(out) if n else None), "ZraHipLocateRecords")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def locate_records_stats(self):
        """Counters of the last locate_records() on this engine (all zero unless it succeeded), keyed by LOCATE_RECORDS_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetLocateRecordsStats(self.h, a)
        return dict(zip(LOCATE_RECORDS_STATS, (int(v) for v in a)))

    def locate_records_ms(self):
        """bring-up: HIP-event time of the last locate_records()'s own launches, summed over its passes."""
        return self.L.ZraHipDebugLocateRecordsMs(self.h)

    def read_records(self, d_archive, size, index, d_index, index_words, numbers, d_data, data_cap, *, staging_bytes=0, ranges=True):
        """ZraHipReadRecords: locate_records(), then the records' bytes packed at d_data (data_cap bytes, device memory) in request
        order, each followed by one delimiter byte. Returns (data_size, [(offset, size)] or None without `ranges`).
        OutputBufferTooSmall (data_cap too small) carries the bytes needed in ZraError.needed_data."""
        import numpy as np
        nums = np.ascontiguousarray(np.asarray(numbers, dtype=np.uint64))
        n = int(nums.size)
        out = np.zeros(2 * max(n, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        info = ZraHipRecordIndex(*index)
        ds = ctypes.c_uint64(0)
        self._order()
        st = self.L.ZraHipReadRecords(self.h, d_archive or None, size, ctypes.byref(info), d_index or None, index_words, p(nums) if n else None, n,
                                      staging_bytes, p(out) if ranges and n else None, d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipReadRecords")
            e.needed_data = ds.value
            raise e
        return ds.value, ([(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)] if ranges else None)

    def read_records_stats(self):
        """Counters of the last read_records() on this engine (all zero unless it succeeded), keyed by READ_RECORDS_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipGetReadRecordsStats(self.h, a)
        return dict(zip(READ_RECORDS_STATS, (int(v) for v in a)))

    def read_records_ms(self):
        """bring-up: HIP-event time of the last read_records()'s locate-sweep launches, summed over its passes."""
        return self.L.ZraHipDebugReadRecordsMs(self.h)


ARCHIVE_STATS = ("slots", "resident", "reads", "hits", "misses", "evictions", "uncompressed_size", "frame_size")

ARCHIVE_UPDATE_STATS = ("updates", "frames", "archive_bytes", "staged", "refreshed", "staged_total", "refreshed_total")

ARCHIVE_SCAN_STATS = ("scans", "staged", "decoded", "passes", "staged_total", "decoded_total")

ARCHIVE_RECORD_STATS = ("calls", "staged", "decoded", "passes", "staged_total", "decoded_total")


UPDATE_STATS = ("frames", "touched", "decoded", "compressed", "carried_bytes", "encoded_bytes", "content_bytes", "passes")

VERIFY_STATS = ("frames", "checked", "structure_faults", "content_faults", "decoded", "content_bytes", "passes")

SEARCH_MAX_PATTERN = 256                     # ZRA_HIP_SEARCH_MAX_PATTERN
SEARCH_STATS = ("frames", "decoded", "content_bytes", "matches", "listed", "passes")
SEARCH_MAX_PATTERNS = 64                     # ZRA_HIP_SEARCH_MAX_PATTERNS
SEARCH_MAX_PATTERN_BYTES = 4096              # ZRA_HIP_SEARCH_MAX_PATTERN_BYTES
SEARCH_MULTI_STATS = ("frames", "decoded", "content_bytes", "matches", "listed", "passes", "patterns", "survivors")
GREP_INVERT = 1                              # ZRA_HIP_GREP_INVERT
GREP_MAX_CONTEXT = 64                        # ZRA_HIP_GREP_MAX_CONTEXT: records before, and records after
CONTEXT_SELECTED = 1 << 63                   # ZRA_HIP_CONTEXT_SELECTED, in a listed record's size
PATTERN_FOLD_CASE = 1                        # ZRA_HIP_PATTERN_FOLD_CASE: ASCII letters match either case
PATTERN_CLASSES = 2                          # ZRA_HIP_PATTERN_CLASSES: patterns are expressions: . [set] [^set] \escape
PATTERN_MAX_SETS = 32                        # ZRA_HIP_PATTERN_MAX_SETS
PATTERN_MAX_EXPR_BYTES = 16384               # ZRA_HIP_PATTERN_MAX_EXPR_BYTES


def _scan_call(L, name, syntax):
    """the entry point of a multi-pattern scan and what goes behind nPatterns: the literal call for syntax 0, else its ...Expr twin"""
    return (getattr(L, name), ()) if not syntax else (getattr(L, name + "Expr"), (syntax,))


def check_pattern_expr(patterns, syntax=PATTERN_CLASSES, delimiter=None):
    """ZraHipCheckPatternExpr: the pattern checks of the scans' `syntax` keyword, on the host alone (no engine, no device).
    delimiter: the grep's and the extract's byte, None for the multi search. Returns (lengths in elements, counted sets); ZraError is
    a refused pattern list."""
    patterns = [bytes(p) for p in patterns]
    sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
    lens = (ctypes.c_uint32 * max(len(patterns), 1))()
    ns = ctypes.c_uint32(0)
    _chk(load().ZraHipCheckPatternExpr(_cbuf(b"".join(patterns)), sizes, len(patterns), syntax, -1 if delimiter is None else delimiter, lens, ctypes.byref(ns)),
         "ZraHipCheckPatternExpr")
    return [int(v) for v in lens[:len(patterns)]], int(ns.value)
GREP_STATS = ("frames", "decoded", "content_bytes", "records", "selected", "listed", "passes", "matches")
WHERE_MAX_CLAUSES = 8                        # ZRA_HIP_WHERE_MAX_CLAUSES


def _context_list(arr, k):
    """the first k entries of a context grep's record array as (offset, size, selected)"""
    return [(int(arr[2 * i]), int(arr[2 * i + 1]) & ~CONTEXT_SELECTED, bool(int(arr[2 * i + 1]) & CONTEXT_SELECTED)) for i in range(k)]


def _pattern_set(term):
    """a clause's term as a 64-bit mask: an int mask as it is, else the indices of an iterable"""
    if isinstance(term, int):
        mask = term
    else:
        mask = 0
        for i in term:
            if not 0 <= int(i) < 64:
                raise ValueError("pattern index %r outside 0 .. 63" % (i,))
            mask |= 1 << int(i)
    if not 0 <= mask < 1 << 64:
        raise ValueError("pattern mask %r does not fit 64 bits" % (term,))
    return mask


def _clauses(where):
    """[(all, any, none)] as a ZraHipRecordClause array (three 64-bit words per clause) and its length"""
    where = [tuple(_pattern_set(t) for t in c) for c in where]
    if any(len(c) != 3 for c in where):
        raise ValueError("a clause is (all, any, none)")
    flat = [w for c in where for w in c]
    return (ctypes.c_uint64 * max(len(flat), 3))(*flat), len(where)


def field_mask(text):
    """ZraHipFieldMask: cut's LIST ("1,3,5-7,9-", "-3") as the field mask of Engine.cut: bit j - 1 for field j, bit 63 for field 64 and
    every later one. ZraError for a list the call refuses."""
    m = ctypes.c_uint64(0)
    st = load().ZraHipFieldMask(text.encode() if isinstance(text, str) else bytes(text), ctypes.byref(m))
    if st.zra != 0:
        raise ZraError(st.tup(), "ZraHipFieldMask")
    return m.value


def _cut_call(L, fn, head, order, patterns, d_data, data_cap, separator, fields, delimiter, invert, offset, length, staging_bytes, max_records, syntax):
    """Engine.cut and Archive.cut: `head` is what stands in front of hPatterns"""
    patterns = [bytes(p) for p in patterns]
    sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
    mask = fields if isinstance(fields, int) else field_mask(fields)
    sep = separator if isinstance(separator, int) else bytes(separator)[0]
    arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
    n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
    order()
    st = fn(*head, _cbuf(b"".join(patterns)) if patterns else None, sizes if patterns else None, len(patterns), syntax, delimiter, GREP_INVERT if invert else 0, sep, mask,
            offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds))
    if st.zra != 0:
        e = ZraError(st.tup(), fn.__name__)
        e.needed_records, e.needed_data = n.value, ds.value
        raise e
    k = n.value if max_records else 0
    return n.value, ds.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]


def _tally_call(engine, plain, name, composite, max_distinct, d_keys, key_cap, max_entries):
    """Engine.tally_text (plain: the call with the primitive's tail), Engine.tally and Archive.tally (composite: the cut's arguments)"""
    arr = (ctypes.c_uint64 * (3 * max_entries))() if max_entries else None
    w = [ctypes.c_uint64(0) for _ in range(5)]                               # records, distinct, skipped, key size; the workspace's size
    tail = (max_distinct, arr, max_entries, d_keys or None, key_cap) + tuple(ctypes.byref(x) for x in w[:4])
    engine._order()
    if composite is None:
        st = plain(tail)
    else:
        fn, head, patterns, separator, fields, delimiter, invert, offset, length, staging_bytes, syntax, d_work, work_cap = composite
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        mask = fields if isinstance(fields, int) else field_mask(fields)
        sep = separator if isinstance(separator, int) else bytes(separator)[0]
        st = fn(*head, _cbuf(b"".join(patterns)) if patterns else None, sizes if patterns else None, len(patterns), syntax, delimiter, GREP_INVERT if invert else 0, sep,
                mask, offset, (1 << 64) - 1 if length is None else length, staging_bytes, d_work or None, work_cap, ctypes.byref(w[4]), *tail)
    engine.last_tally = {"records": w[0].value, "distinct": w[1].value, "skipped": w[2].value, "key_size": w[3].value, "work_size": w[4].value}
    if st.zra != 0:
        e = ZraError(st.tup(), name)
        e.n_records, e.needed_entries, e.n_skipped, e.needed_keys, e.needed_work = (x.value for x in w)
        raise e
    k = w[1].value if max_entries else 0
    return w[0].value, w[2].value, [(int(arr[3 * i]), int(arr[3 * i + 1]), int(arr[3 * i + 2])) for i in range(k)]


def _grep_call(L, name, syntax, where):
    """the entry point of a grep, what goes behind nPatterns and what goes behind mode: _scan_call's without `where`, else the
    ...Where call, which takes the syntax word always and the clauses"""
    if not where:
        return _scan_call(L, name, syntax) + ((),)
    return getattr(L, name + "Where"), (syntax,), _clauses(where)


def check_record_clauses(where, n_patterns):
    """ZraHipCheckRecordClauses: the clause checks of grep(where=...), on the host alone (no engine, no device). ZraError is a refused
    clause list."""
    arr, k = _clauses(where)
    _chk(load().ZraHipCheckRecordClauses(arr if k else None, k, n_patterns), "ZraHipCheckRecordClauses")
REGEX_MAX_STATES = 64                        # ZRA_HIP_REGEX_MAX_STATES
REGEX_MAX_POSITIONS = 4096                   # ZRA_HIP_REGEX_MAX_POSITIONS
REGEX_INFO = ("states", "classes", "positions", "why", "pattern")


def check_regex(patterns, fold_case=False, delimiter=0x0A):
    """ZraHipCheckRegex: the expression checks of grep_regex(), on the host alone (no engine, no device). Returns ZraHipRegexInfo as a
    dict keyed by REGEX_INFO; ZraError is a refused expression list, with the same dict in ZraError.info."""
    patterns = [bytes(p) for p in patterns]
    sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
    info = (ctypes.c_uint32 * 5)()
    st = load().ZraHipCheckRegex(_cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0, delimiter, info)
    d = dict(zip(REGEX_INFO, (int(v) for v in info)))
    if st.zra != 0:
        e = ZraError(st.tup(), "ZraHipCheckRegex")
        e.info = d
        raise e
    return d
TALLY_MAX_KEY = 4096                         # ZRA_HIP_TALLY_MAX_KEY
TALLY_HASH_NONE = 0xFFFFFFFF                 # ZRA_HIP_TALLY_HASH_NONE
TALLY_STATS = ("records", "distinct", "skipped", "key_bytes", "table_slots", "longest_probe", "table_inserts")
EXTRACT_STATS = ("frames", "decoded", "content_bytes", "records", "selected", "packed_bytes", "passes", "matches")

COMPARE_DECODE_ALL = 1                       # ZRA_HIP_COMPARE_DECODE_ALL
COMPARE_STATS = ("frames", "equal_compressed", "decoded", "content_bytes", "ranges", "listed", "passes")

DIFF_DECODE_ALL = 1                          # ZRA_HIP_DIFF_DECODE_ALL
DIFF_MAX_GRAIN = 8192                        # ZRA_HIP_DIFF_MAX_GRAIN
DIFF_STATS = ("frames", "equal_compressed", "decoded", "tail_decoded", "writes", "dirty_bytes", "passes", "dirty_grains")

SIGN_MIN_GRAIN = 64                          # ZRA_HIP_SIGN_MIN_GRAIN
SIGN_MAX_GRAIN = 8192                        # ZRA_HIP_SIGN_MAX_GRAIN
SIGDIFF_DECODE_ALL = 1                       # ZRA_HIP_SIGDIFF_DECODE_ALL
SIGN_STATS = ("frames", "signed", "grain_words", "content_bytes", "compressed_bytes", "passes")
INDEX_RECORDS_STATS = ("frames", "indexed", "content_bytes", "delimiters", "passes")
LOCATE_RECORDS_STATS = ("frames", "records", "boundaries", "decoded", "content_bytes", "passes")
READ_RECORDS_STATS = ("frames", "records", "packed_bytes", "locate_decoded", "read_decoded", "locate_passes")
SIGDIFF_STATS = DIFF_STATS                   # the diff's shape; equal_compressed: frames whose span hashes to A's frame word


def signature_words(content_size, frame_size, grain):
    """64-bit words of the signature of content_size bytes in frames of frame_size at `grain`: frames x (1 + ceil(frame_size / grain))."""
    return -(-content_size // frame_size) * (1 + -(-frame_size // grain))


class Archive:
    """Archive handle (include/zra_hip.h: ZraHipArchive*): a device-resident archive opened once on `engine`, with a cache of whole
    decoded frames in an HBM arena of `cache_bytes` (0: no cache, reads are ZraHipDecompressRABatch). The archive's bytes must stay
    valid and unchanged until close() or until update() binds the handle to its result. d_archive and size are the archive the handle
    serves now. Keeps its Engine alive: the engine is not destroyed before the handle."""

    def __init__(self, engine, d_archive_ptr, size, cache_bytes=0):
        self.engine = engine
        self.L = engine.L
        self.h = None
        h = ctypes.c_void_p()
        engine._order()
        _chk(self.L.ZraHipArchiveOpen(engine.h, d_archive_ptr, size, cache_bytes, ctypes.byref(h)), "ZraHipArchiveOpen")
        self.h = h
        self.d_archive, self.size = d_archive_ptr, size

    def read(self, d_out, offsets, sizes, out_offsets):
        import numpy as np
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        s = np.ascontiguousarray(sizes, dtype=np.uint64)
        oo = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        self.engine._order()
        _chk(self.L.ZraHipArchiveRead(self.h, d_out, p(o), p(s), p(oo), len(o)), "ZraHipArchiveRead")

    def stats(self):
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipArchiveGetStats(self.h, a)
        return dict(zip(ARCHIVE_STATS, (int(v) for v in a)))

    def update(self, d_out, out_cap, *, writes=None, d_data=0, d_append=0, append_size=0, level=3, checksum=True):
        """ZraHipArchiveUpdate: Engine.update of the archive the handle serves, written to d_out; old plaintext comes from the cache where
        it is resident, the handle serves the result afterwards and its resident frames hold the new bytes. Returns the new size.
        OutputBufferTooSmall carries the size needed in ZraError.needed; after any error the handle is as it was."""
        import numpy as np
        o, s, do = (np.ascontiguousarray(a, dtype=np.uint64) for a in (writes if writes is not None else ((), (), ())))
        if not (len(o) == len(s) == len(do)):
            raise ValueError("writes: offsets, sizes and data_offsets differ in length")
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if len(a) else None
        osz = ctypes.c_size_t(0)
        self.engine._order()
        st = self.L.ZraHipArchiveUpdate(self.h, d_data or None, p(o), p(s), p(do), len(o), d_append or None, append_size, d_out or None, out_cap,
                                        ctypes.byref(osz), level, checksum)
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipArchiveUpdate")
            e.needed = osz.value
            raise e
        self.d_archive, self.size = d_out, osz.value
        return osz.value

    def update_stats(self):
        """Counters of the updates through this handle, keyed by ARCHIVE_UPDATE_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipArchiveGetUpdateStats(self.h, a)
        return dict(zip(ARCHIVE_UPDATE_STATS, (int(v) for v in a[:7])))

    # ---- the range scans through the handle: Engine.search / search_multi / grep / extract of the archive the handle serves, with their
    # keyword arguments and results. A pass copies its resident frames out of the cache and decodes only the others; a scan is not a
    # read: the cache and stats() do not change. The call overwrites the engine's counters of its kind (engine.search_stats() ...).
    def search(self, pattern, *, offset=0, length=None, staging_bytes=0, max_matches=1 << 20):
        """ZraHipArchiveSearch: Engine.search through the handle. Returns (n_matches, [offsets])."""
        pattern = bytes(pattern)
        arr = (ctypes.c_uint64 * max_matches)() if max_matches else None
        n = ctypes.c_uint64(0)
        self.engine._order()
        _chk(self.L.ZraHipArchiveSearch(self.h, _cbuf(pattern), len(pattern), offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                                        max_matches, ctypes.byref(n)), "ZraHipArchiveSearch")
        return n.value, [int(v) for v in arr[:min(n.value, max_matches)]] if arr is not None else []

    def search_multi(self, patterns, *, offset=0, length=None, staging_bytes=0, max_matches=1 << 20, syntax=0):
        """ZraHipArchiveSearchMulti (syntax != 0: ...Expr): Engine.search_multi through the handle. Returns (n_matches, [(offset, pattern index)], per_pattern)."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ZraHipPatternMatch * max_matches)() if max_matches else None
        per = (ctypes.c_uint64 * max(len(patterns), 1))()
        n = ctypes.c_uint64(0)
        self.engine._order()
        fn, sx = _scan_call(self.L, "ZraHipArchiveSearchMulti", syntax)
        _chk(fn(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, offset, (1 << 64) - 1 if length is None else length,
                staging_bytes, arr, max_matches, ctypes.byref(n), per), fn.__name__)
        listed = [(int(arr[i].offset), int(arr[i].pattern)) for i in range(min(n.value, max_matches))] if arr is not None else []
        return n.value, listed, [int(v) for v in per[:len(patterns)]]

    def grep(self, patterns, *, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=1 << 20, syntax=0, where=None):
        """ZraHipArchiveGrep (syntax != 0: ...Expr; a non-empty where: ZraHipArchiveGrepWhere): Engine.grep through the handle.
        Returns (n_records, [(offset, size)])."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n = ctypes.c_uint64(0)
        self.engine._order()
        fn, sx, wx = _grep_call(self.L, "ZraHipArchiveGrep", syntax, where)
        _chk(fn(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, delimiter, GREP_INVERT if invert else 0, *wx, offset,
                (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records, ctypes.byref(n)), fn.__name__)
        k = min(n.value, max_records)
        return n.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def grep_context(self, patterns, *, before=0, after=0, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=1 << 20, syntax=0):
        """ZraHipArchiveGrepContext: Engine.grep_context through the handle. Returns (n_records, n_selected, n_groups, [(offset, size, selected)])."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ns, ng = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.engine._order()
        _chk(self.L.ZraHipArchiveGrepContext(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), syntax, delimiter, GREP_INVERT if invert else 0, before, after,
                                             offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records, ctypes.byref(n), ctypes.byref(ns),
                                             ctypes.byref(ng)), "ZraHipArchiveGrepContext")
        return n.value, ns.value, ng.value, _context_list(arr, min(n.value, max_records))

    def grep_regex(self, patterns, *, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None, staging_bytes=0, max_records=1 << 20):
        """ZraHipArchiveGrepRegex: Engine.grep_regex through the handle. Returns (n_records, [(offset, size)])."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n = ctypes.c_uint64(0)
        self.engine._order()
        _chk(self.L.ZraHipArchiveGrepRegex(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0, delimiter,
                                           GREP_INVERT if invert else 0, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records,
                                           ctypes.byref(n)), "ZraHipArchiveGrepRegex")
        k = min(n.value, max_records)
        return n.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def grep_regex_context(self, patterns, *, before=0, after=0, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None, staging_bytes=0,
                           max_records=1 << 20):
        """ZraHipArchiveGrepRegexContext: Engine.grep_regex_context through the handle. Returns (n_records, n_selected, n_groups, [(offset, size, selected)])."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ns, ng = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.engine._order()
        _chk(self.L.ZraHipArchiveGrepRegexContext(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0, delimiter,
                                                  GREP_INVERT if invert else 0, before, after, offset, (1 << 64) - 1 if length is None else length, staging_bytes,
                                                  arr, max_records, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(ng)), "ZraHipArchiveGrepRegexContext")
        return n.value, ns.value, ng.value, _context_list(arr, min(n.value, max_records))

    def extract(self, patterns, d_data, data_cap, *, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=0, syntax=0, where=None):
        """ZraHipArchiveExtractRecords (syntax != 0: ...Expr; a non-empty where: ZraHipArchiveExtractRecordsWhere): Engine.extract through the handle; d_data must overlap neither the archive nor the cache. Returns
        (n_records, data_size, [(offset, size)]); OutputBufferTooSmall carries ZraError.needed_records and ZraError.needed_data."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.engine._order()
        fn, sx, wx = _grep_call(self.L, "ZraHipArchiveExtractRecords", syntax, where)
        st = fn(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), *sx, delimiter, GREP_INVERT if invert else 0, *wx, offset,
                (1 << 64) - 1 if length is None else length, staging_bytes, arr, max_records, ctypes.byref(n),
                d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), fn.__name__)
            e.needed_records, e.needed_data = n.value, ds.value
            raise e
        k = n.value if max_records else 0
        return n.value, ds.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def cut(self, patterns, d_data, data_cap, *, separator, fields, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, max_records=0, syntax=0):
        """ZraHipArchiveCutRecords: Engine.cut through the handle; d_data must overlap neither the archive nor the cache. Returns and raises as
        extract() does."""
        return _cut_call(self.L, self.L.ZraHipArchiveCutRecords, (self.h,), self.engine._order, patterns, d_data, data_cap, separator, fields, delimiter, invert,
                         offset, length, staging_bytes, max_records, syntax)

    def tally(self, patterns, d_work, work_cap, *, separator, fields, delimiter=0x0A, invert=False, offset=0, length=None, staging_bytes=0, syntax=0, max_distinct=0,
              d_keys=0, key_cap=0, max_entries=1 << 16):
        """ZraHipArchiveTallyFields: Engine.tally through the handle; d_work and d_keys must overlap neither the archive nor the cache. Returns
        and raises as Engine.tally; the words of the call are in self.engine.last_tally."""
        return _tally_call(self.engine, None, "ZraHipArchiveTallyFields", (self.L.ZraHipArchiveTallyFields, (self.h,), patterns, separator, fields, delimiter, invert,
                                                                           offset, length, staging_bytes, syntax, d_work, work_cap), max_distinct, d_keys, key_cap,
                           max_entries)

    def extract_regex(self, patterns, d_data, data_cap, *, delimiter=0x0A, invert=False, fold_case=False, offset=0, length=None, staging_bytes=0, max_records=0):
        """ZraHipArchiveExtractRecordsRegex: Engine.extract_regex through the handle; d_data must overlap neither the archive nor the cache. Returns
        (n_records, data_size, [(offset, size)]); OutputBufferTooSmall carries ZraError.needed_records and ZraError.needed_data."""
        patterns = [bytes(p) for p in patterns]
        sizes = (ctypes.c_uint32 * max(len(patterns), 1))(*(len(p) for p in patterns))
        arr = (ctypes.c_uint64 * (2 * max_records))() if max_records else None
        n, ds = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.engine._order()
        st = self.L.ZraHipArchiveExtractRecordsRegex(self.h, _cbuf(b"".join(patterns)), sizes, len(patterns), PATTERN_FOLD_CASE if fold_case else 0, delimiter,
                                                     GREP_INVERT if invert else 0, offset, (1 << 64) - 1 if length is None else length, staging_bytes, arr,
                                                     max_records, ctypes.byref(n), d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipArchiveExtractRecordsRegex")
            e.needed_records, e.needed_data = n.value, ds.value
            raise e
        k = n.value if max_records else 0
        return n.value, ds.value, [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(k)]

    def scan_stats(self):
        """Counters of the scans through this handle, keyed by ARCHIVE_SCAN_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipArchiveGetScanStats(self.h, a)
        return dict(zip(ARCHIVE_SCAN_STATS, (int(v) for v in a[:6])))

    def scan_stage_ms(self):
        """bring-up: HIP-event time of the last accepted scan's job-split and stage-from-cache launches, summed over its passes."""
        return self.L.ZraHipDebugArchiveScanStageMs(self.h)

    def arena_range(self):
        """bring-up: (base, bytes) of the handle's arena in device memory, (0, 0) without a cache: for tests of the arena check."""
        base, n = ctypes.c_void_p(0), ctypes.c_size_t(0)
        self.L.ZraHipDebugArchiveArena(self.h, ctypes.byref(base), ctypes.byref(n))
        return base.value or 0, n.value

    # ---- the record index through the handle: Engine.index_records / locate_records / read_records of the archive the handle serves,
    # without d_archive and size. A whole-frame sweep copies the resident frames it needs out of the cache and decodes only the others.
    # Index and locate are not reads: the cache and stats() do not change. The read's byte fetch is a read of the handle: it counts in
    # stats() and keeps the frames it decoded. The call overwrites the engine's counters of its kind (engine.index_records_stats() ...).
    def index_records(self, d_index, index_cap_words, *, delimiter=0x0A, first_frame=0, frame_count=None, staging_bytes=0):
        """ZraHipArchiveIndexRecords: Engine.index_records through the handle; d_index must overlap neither the archive nor the cache.
        Returns the RecordIndex of the whole archive; OutputBufferTooSmall carries the words needed in ZraError.needed_words."""
        info = ZraHipRecordIndex()
        self.engine._order()
        st = self.L.ZraHipArchiveIndexRecords(self.h, delimiter, first_frame, 0xFFFFFFFFFFFFFFFF if frame_count is None else frame_count, staging_bytes,
                                              d_index or None, index_cap_words, ctypes.byref(info))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipArchiveIndexRecords")
            e.needed_words = info.frames
            raise e
        return RecordIndex(info.contentSize, info.frameSize, info.delimiter, info.frames, info.delimiters, info.records)

    def locate_records(self, index, d_index, index_words, numbers, *, staging_bytes=0):
        """ZraHipArchiveLocateRecords: Engine.locate_records through the handle. Returns [(offset, size)] in request order."""
        import numpy as np
        nums = np.ascontiguousarray(np.asarray(numbers, dtype=np.uint64))
        n = int(nums.size)
        out = np.zeros(2 * max(n, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        info = ZraHipRecordIndex(*index)
        self.engine._order()
        _chk(self.L.ZraHipArchiveLocateRecords(self.h, ctypes.byref(info), d_index or None, index_words, p(nums) if n else None, n, staging_bytes,
                                               p(out) if n else None), "ZraHipArchiveLocateRecords")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def read_records(self, index, d_index, index_words, numbers, d_data, data_cap, *, staging_bytes=0, ranges=True):
        """ZraHipArchiveReadRecords: Engine.read_records through the handle; d_data must overlap neither the archive, the index nor the
        cache. Returns (data_size, [(offset, size)] or None without `ranges`); OutputBufferTooSmall carries ZraError.needed_data."""
        import numpy as np
        nums = np.ascontiguousarray(np.asarray(numbers, dtype=np.uint64))
        n = int(nums.size)
        out = np.zeros(2 * max(n, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        info = ZraHipRecordIndex(*index)
        ds = ctypes.c_uint64(0)
        self.engine._order()
        st = self.L.ZraHipArchiveReadRecords(self.h, ctypes.byref(info), d_index or None, index_words, p(nums) if n else None, n, staging_bytes,
                                             p(out) if ranges and n else None, d_data or None, data_cap, ctypes.byref(ds))
        if st.zra != 0:
            e = ZraError(st.tup(), "ZraHipArchiveReadRecords")
            e.needed_data = ds.value
            raise e
        return ds.value, ([(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)] if ranges else None)

    def record_stats(self):
        """Counters of the record calls through this handle, keyed by ARCHIVE_RECORD_STATS."""
        a = (ctypes.c_uint64 * 8)()
        self.L.ZraHipArchiveGetRecordStats(self.h, a)
        return dict(zip(ARCHIVE_RECORD_STATS, (int(v) for v in a[:6])))

    def record_stage_ms(self):
        """bring-up: HIP-event time of the last accepted record call's job-split and stage-from-cache launches, summed over its passes."""
        return self.L.ZraHipDebugArchiveRecordStageMs(self.h)

    def drop_cache(self):
        _chk(self.L.ZraHipArchiveDropCache(self.h), "ZraHipArchiveDropCache")

    def close(self):
        if self.h:
            self.L.ZraHipArchiveClose(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stitch_header(frame_sizes, uncompressed_size, frame_size):
    """Host-side seek-table stitch for sharded compression: all ranks' frame sizes -> full ZRA header."""
    import numpy as np
    L = load()
    fs = np.ascontiguousarray(frame_sizes, dtype=np.uint64)
    out = ctypes.create_string_buffer(38 + 5 * (len(fs) + 1))
    hsz = ctypes.c_size_t(0)
    _chk(L.ZraHipStitchHeader(fs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(fs), uncompressed_size, frame_size, out, ctypes.byref(hsz)))
    return out.raw[: hsz.value]
