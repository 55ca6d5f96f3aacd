/* zra_amd — additive device-side C ABI of the MI355X-native ZRA engine.
 *
 * NOT part of the reference. The 29 reference entry points (include/zra.h) keep their host-pointer
 * semantics; one kernel launch per call cannot serve BASELINE config C3 (1M random-access queries), and
 * callers that already hold data in HBM should not bounce it through the host. These calls take DEVICE
 * pointers (hipMalloc / torch.cuda tensors: plain addresses, no torch types) and are what bench.py times.
 *
 * Reference interfaces they accelerate:
 *   ZraHipCompressBuffer      <- zra::CompressBuffer    (zra.cpp:194-234, zra.h:138)
 *   ZraHipDecompressBuffer    <- zra::DecompressBuffer  (zra.cpp:243-250, zra.h:146)
 *   ZraHipDecompressRABatch   <- zra::DecompressRA      (zra.cpp:258-296, zra.h:156), batched
 *   ZraHipCompressFrames / ZraHipStitch <- the per-frame loop zra.cpp:216-225 split for multi-GPU sharding
 */
#ifndef ZRA_HIP_H
#define ZRA_HIP_H
#include "zra.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ZraHipEngine ZraHipEngine;

/** Number of visible HIP devices (0 when there is no GPU / no driver). Never throws. */
ZRA_EXPORT int ZraHipDeviceCount(void);

/** Creates an engine bound to `device` (its own stream + scratch pool). Fails with ZStdError/GENERIC(1) when no GPU is usable. */
ZRA_EXPORT ZraStatus ZraHipCreateEngine(ZraHipEngine** engine, int device);
ZRA_EXPORT void ZraHipDestroyEngine(ZraHipEngine* engine);
/** Blocks until all work queued on the engine's stream is complete. */
ZRA_EXPORT ZraStatus ZraHipSynchronize(ZraHipEngine* engine);
/** STREAM ORDERING. The engine works on two private non-blocking HIP streams; they are not ordered against the caller's
 *  streams (nor against the null stream). Inputs (dIn / the archive / device-resident query arrays) must be complete before a
 *  ZraHip* compute call starts reading them: either synchronise the producing stream, or call ZraHipWaitStream(engine, stream)
 *  first — it records an event on `producerStream` (a hipStream_t; NULL = the null stream) and makes the engine's streams wait
 *  for it, with no host synchronisation. Every ZraHip* compute call is host-synchronous on return: its outputs are complete and
 *  visible to any stream. */
ZRA_EXPORT ZraStatus ZraHipWaitStream(ZraHipEngine* engine, void* producerStream);
/** Returns the engine's scratch allocations to the device. Scratch is grow-only between calls (a level-9 compression of a large
 *  buffer keeps tens of GiB for its hash-chain tables); a long-running host that is done with such a phase can hand it back. */
ZRA_EXPORT ZraStatus ZraHipReleaseScratch(ZraHipEngine* engine);
/** The engine's hipStream_t, as an opaque pointer (for event timing on the stream kernels run on). */
ZRA_EXPORT void* ZraHipGetStream(ZraHipEngine* engine);

/** CompressBuffer with device-resident input/output. dOut must hold ZraGetCompressedOutputBufferSize(inSize, frameSize) bytes.
 *  Output is byte-identical to the reference at the same level (zstd 1.4.9 semantics). Synchronous. *outSize is written on Success
 *  only: on any other status ({ZStdError, 64} when scratch cannot be allocated) it is not touched. */
ZRA_EXPORT ZraStatus ZraHipCompressBuffer(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut, size_t* outSize,
                                          int8_t compressionLevel, uint32_t frameSize, bool checksum);

/** DecompressBuffer with a device-resident archive; dOut must hold the archive's uncompressedSize bytes. Synchronous.
 *  Frame boundaries come from the archive's own seek table (the body stays on the device, nothing walks it on the host): on a valid
 *  archive the result is the reference's; on a damaged one the frames' own errors are reported like libzstd's, but a seek table
 *  that does not match the frames is an error here (srcSize_wrong / corruption_detected) where zra::DecompressBuffer — one
 *  multi-frame zstd call that never looks at the table, zra.cpp:249 — may still succeed. The host-pointer ZraDecompressBuffer /
 *  ZraDecompressRA of include/zra.h reproduce the reference on such archives too. The same holds for ZraHipDecompressRABatch. */
ZRA_EXPORT ZraStatus ZraHipDecompressBuffer(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut, size_t outCapacity);

/** Batched DecompressRA: query i returns bytes [hOffsets[i], hOffsets[i]+hSizes[i]) of the original data at dOut + hOutOffsets[i].
 *  hOffsets/hSizes/hOutOffsets are HOST arrays of nQueries entries. Bounds rule per query is the reference's
 *  (offset+size >= uncompressedSize -> OutOfBoundsAccess, zra.cpp:260). Synchronous.
 *  The frames a batch touches are found and scheduled on the device from the archive's own seek table; every touched frame is
 *  decoded once, and only as far as the last byte any query needs from it (the reference decodes whole frames, zra.cpp:279-295).
 *  For a valid archive the bytes are identical. What differs is damage detection: bytes of a frame behind the last one needed, and
 *  the frame's content checksum, are not looked at. ZRA_HIP_OPT_RA_WHOLE_FRAMES restores whole-frame decode + checksum. */
ZRA_EXPORT ZraStatus ZraHipDecompressRABatch(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut,
                                             const uint64_t* hOffsets, const uint64_t* hSizes, const uint64_t* hOutOffsets, size_t nQueries);

/* ---- archive handle: a device-resident archive opened once, with a cache of whole decoded frames in HBM ----
 * The reference's Decompressor holds the parsed header and takes a maxCacheSize (zra.h); this is its device-pointer counterpart.
 * A read whose frames are all resident costs one query upload, one copy kernel and one small read-back — no decode. */
typedef struct ZraHipArchive ZraHipArchive;

/** Opens the archive at dArchive (archiveSize bytes, device memory) on `engine`.
 *  - Validation and statuses are ZraHipDecompressRABatch's: archiveSize <= 38 or < the header size -> OutOfBoundsAccess; a fixed-header
 *    problem -> that status (HeaderInvalid / ZraVersionLow); a seek table outside the header or ceil(uncompressedSize / frameSize) !=
 *    frames -> HeaderInvalid.
 *  - The header is read from the device here, once; no read copies it again.
 *  - Slots = min(cacheBytes / frameSize, frames), each one frame of frameSize bytes in an arena of the handle's own (not engine scratch:
 *    ZraHipReleaseScratch does not touch it). An arena or tables that cannot be allocated -> {ZStdError, 64} (memory_allocation); no
 *    handle is written and nothing is kept.
 *  - engine NULL, dArchive NULL with archiveSize != 0, or archive NULL -> {ZStdError, 42}.
 *  - The archive's bytes must stay valid and unchanged until ZraHipArchiveClose; a caller that rewrites them calls ZraHipArchiveDropCache.
 *  Threading is the engine's: one call at a time per engine. Several handles may share one engine, each with its own arena; close every
 *  handle before destroying its engine. */
ZRA_EXPORT ZraStatus ZraHipArchiveOpen(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, size_t cacheBytes,
                                       ZraHipArchive** archive);
/** Releases the handle and its arena. NULL is a no-op. */
ZRA_EXPORT void ZraHipArchiveClose(ZraHipArchive* archive);
/** Query i returns bytes [hOffsets[i], hOffsets[i] + hSizes[i]) of the content at dOut + hOutOffsets[i] (host arrays, as
 *  ZraHipDecompressRABatch). Synchronous.
 *  - Bounds: the reference's rule, offset + size >= uncompressedSize -> OutOfBoundsAccess (zra.cpp:260). A refused call changes no
 *    counter and no resident frame.
 *  - 0 slots: exactly ZraHipDecompressRABatch on the same archive (bytes, statuses, partial decode, the ZRA_HIP_OPT_RA_WHOLE_FRAMES
 *    opt-in); only the header read is gone.
 *  - At least 1 slot: every frame the handle decodes is decoded whole and its content checksum verified if it has one. On a valid archive
 *    the answers equal ZraHipDecompressRABatch's, and dOut bytes outside them are not touched. On a damaged archive the status is that of
 *    ZraHipDecompressRABatch under ZRA_HIP_OPT_RA_WHOLE_FRAMES, whatever the process-wide option says.
 *  - Residency: a frame becomes resident only if it decoded with status 0 and regenerated exactly min(frameSize, uncompressedSize -
 *    f * frameSize) bytes. A read that returns an error leaves every slot it claimed for decoding empty; frames resident before it that it
 *    did not claim stay. A frame that failed is never served from the cache: the next read decodes it again and fails again alike.
 *  - Counting: for each accepted read, hits + misses = the distinct frames its non-empty queries touch (duplicate and overlapping queries
 *    share a frame). When the missed frames outnumber the slots they are decoded in passes of at most `slots` frames into the same slots:
 *    every answer is still right, and at most `slots` frames are resident afterwards.
 *  - Eviction is CLOCK (second chance): a frame is inserted with its reference bit clear and a hit sets it; the hand clears set bits and
 *    passes those slots, and takes clear or empty slots as victims, in hand order. So with S slots, if every read touches one hot frame
 *    H and K < S/2 frames never touched before, H is a hit on every read after the first.
 *  - ZraHipGetKernelStats / ZraHipGetDecodeStageStats describe the read afterwards, like any call on the engine; a read whose frames were
 *    all resident reports 0 decode launches. */
ZRA_EXPORT ZraStatus ZraHipArchiveRead(ZraHipArchive* archive, void* dOut, const uint64_t* hOffsets, const uint64_t* hSizes,
                                       const uint64_t* hOutOffsets, size_t nQueries);
/** Forgets every resident frame (the counters stay). */
ZRA_EXPORT ZraStatus ZraHipArchiveDropCache(ZraHipArchive* archive);
/** out8 = {cache slots, frames resident now, reads accepted, frame hits, frame misses (= frames decoded), evictions,
 *  uncompressed size, frame size}; counters 2-5 are cumulative since the handle was opened. A read refused with OutOfBoundsAccess is
 *  not accepted; nor is, on a handle without slots, one refused with {ZStdError, 64}: it decoded and wrote nothing. */
ZRA_EXPORT void ZraHipArchiveGetStats(const ZraHipArchive* archive, uint64_t* out8);
/** ZraHipUpdateArchive (below) through the handle: the archive the handle is bound to is updated into dOut, the handle is bound to the
 *  result, and its cache stays coherent and warm. Synchronous; stream ordering as the other compute calls (ZraHipWaitStream).
 *  - Result: dOut and *outSize are byte for byte what ZraHipUpdateArchive(the handle's engine, the bytes the handle is bound to, the same
 *    arguments) writes, with its statuses 1-9 in its order. Two checks come in front: archive NULL -> {ZStdError, 42}; and, joined to
 *    check 2, [dOut, dOut + outCapacity) overlapping the handle's arena -> {ZStdError, 42}. Header problems cannot occur beyond those
 *    a handle can be opened with (a frame size of 0: HeaderInvalid): the handle holds a checked header, which is not read again.
 *  - Re-binding: on Success the handle serves the archive at dOut (*outSize bytes, U' and F'). The buffer it was bound to before is no
 *    longer referenced: the caller may free it, or pass it as dOut of the next update (ping-pong). The new bytes must stay valid and
 *    unchanged until close, the rule of ZraHipArchiveOpen. The header the handle keeps is built from the host copy the update wrote.
 *  - Failure: on every refusal (statuses 1-9 of ZraHipUpdateArchive and the two checks above) nothing has changed: dOut is untouched,
 *    the handle is bound as before, and every resident frame, reference bit, the hand and all counters are as before. When F' exceeds
 *    what the frame table of the cache holds, a larger one (with headroom for further appends) is allocated behind check 4 and swapped
 *    in on Success; if it cannot be had -> {ZStdError, 64}. The one exception is a HIP runtime error ({ZStdError, 1}) behind check 8,
 *    while the result is being written: dOut and the touched resident frames are then undefined and the handle is still bound to the
 *    old archive; close it, or ZraHipArchiveDropCache before reading on.
 *  - Cache (at least 1 slot; TOUCHED as in ZraHipUpdateArchive): an untouched resident frame stays resident in its slot. A touched frame
 *    that keeps some old bytes and is resident is not decoded: its old plaintext is copied from the arena into the update's staging
 *    (this launders no damage: a frame is resident only after a whole decode with status 0, checksum verified, exact size); one that
 *    is not resident is decoded exactly as by ZraHipUpdateArchive. Every touched resident frame, one replaced whole included, stays
 *    resident and its slot holds the new plaintext after the call; the old last frame grown by an append stays resident with its new
 *    length. A touched frame that was not resident and every appended frame are not inserted. The update inserts and evicts nothing,
 *    moves no hand and sets no reference bit: it is not a read. Slots and arena stay as opened. hits, misses, reads and evictions of
 *    ZraHipArchiveGetStats do not change; uncompressed size becomes U'.
 *  - 0 slots: ZraHipUpdateArchive plus the re-binding.
 *  - ZraHipGetUpdateStats(engine) describes the call; "frames decoded" counts decode jobs, so not the frames staged from the cache. */
ZRA_EXPORT ZraStatus ZraHipArchiveUpdate(ZraHipArchive* archive,
    const void* dData, const uint64_t* hOffsets, const uint64_t* hSizes, const uint64_t* hDataOffsets, size_t nWrites,
    const void* dAppend, size_t appendSize,
    void* dOut, size_t outCapacity, size_t* outSize, int8_t compressionLevel, bool checksum);
/** out8 = {updates accepted, frames now, archive size now, frames staged from the cache in the last accepted update, resident frames
 *  refreshed (holding new bytes) in it, frames staged (cumulative), frames refreshed (cumulative), 0}. Refreshed >= staged: a resident
 *  frame replaced whole is refreshed, not staged. archive NULL: all zero; out8 NULL: no-op. */
ZRA_EXPORT void ZraHipArchiveGetUpdateStats(const ZraHipArchive* archive, uint64_t* out8);

/* ---- the range scans through the handle: resident frames are staged from the cache, not decoded ----
 * ZraHipSearchArchive, ZraHipSearchArchiveMulti, ZraHipGrepArchive and ZraHipExtractRecords (below) decode every frame of their range
 * on every call. A server that keeps its hot frames resident and greps them again and again holds that plaintext already: through the
 * handle a pass copies the resident frames of its range out of the arena, at HBM bandwidth, and decodes only the others. */
struct ZraHipPatternMatch;   /* defined with ZraHipSearchArchiveMulti */
struct ZraHipContentRange;   /* defined with ZraHipGrepArchive */

/** ZraHipSearchArchive on the archive the handle is bound to: its arguments without engine, dArchive and archiveSize. Synchronous; stream
 *  ordering as the other compute calls (ZraHipWaitStream). What is said here holds for the three calls behind it as well, each against
 *  its engine-level counterpart.
 *  - Result: hMatches and *nMatches are byte for byte what ZraHipSearchArchive(the handle's engine, the bytes the handle is bound to, the
 *    same arguments) gives, on every status: nothing reaches the host before the last pass, the early returns (the empty range, a
 *    range shorter than the shortest pattern) decode nothing, and the extract's OutputBufferTooSmall sizes as it does there.
 *  - Statuses: the plain call's, in its order, with three differences. archive NULL -> {ZStdError, 42} in front of everything. Header
 *    problems cannot occur beyond those a handle can be opened with (a frame size of 0: HeaderInvalid): the handle holds a checked
 *    header, which is not read from the device again; that is the one saving a handle with 0 slots still has. And the extract's rule 2
 *    additionally refuses [dData, dData + dataCapacity) overlapping the handle's arena with {ZStdError, 42}, the arena check of
 *    ZraHipArchiveUpdate.
 *  - Where the plaintext of a pass comes from (at least 1 slot): a frame of the pass that is resident is copied from its arena slot
 *    into its slot of the staging window, min(frameSize, U - f * frameSize) bytes, and is not decoded (this launders no damage: a frame
 *    is resident only after a whole decode with status 0, checksum verified, exact size); one that is not resident is decoded whole,
 *    its checksum verified, exactly as by the plain call. The window a pass scans holds the same bytes either way, and the scan
 *    kernels are the plain call's.
 *  - A scan is not a read: it inserts, evicts and refreshes nothing, sets no reference bit and moves no hand, and never writes the
 *    arena. reads, hits, misses, evictions and resident of ZraHipArchiveGetStats do not change, on success or on failure: a scan of a
 *    whole archive cannot flush the hot set. A caller who wants frames resident reads them (ZraHipArchiveRead).
 *  - A frame that fails is by construction not resident; the status is the plain call's rule 5: the lowest failing frame of the first
 *    failing pass. On failure the handle and its cache are exactly as before the call.
 *  - 0 slots: the plain call minus the header read; the same kernels are launched.
 *  - Stats: the call is a ZraHipSearchArchive on the handle's engine: it overwrites ZraHipGetSearchStats and ZraHipDebugSearchScanMs
 *    (the other three: their own kind's) under their rules, zero on every outcome other than Success. Through a handle word [1]
 *    counts decode jobs ("frames decoded") and word [2] the bytes the decoder regenerated: both leave out the frames staged from the
 *    arena; every other word is the plain call's. ZraHipGetKernelStats reports 0 decode launches for a scan whose frames were all
 *    resident.
 *  - Scratch: the plain call's rule 4, plus, with at least 1 slot, 16 bytes per frame of a pass for the copy entries and the pass's two
 *    counts, which come to the host through a page-locked word of the handle, one small read-back per pass.
 *  Not covered: populating or refreshing the cache from a scan, scan kernels that read the arena in place, and handle variants of
 *  ZraHipVerifyArchive, ZraHipCompareArchives, ZraHipDiffArchives and ZraHipSignArchive (the record index has them: below), shards,
 *  the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipArchiveSearch(ZraHipArchive* archive,
    const void* hPattern, size_t patternSize,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    uint64_t* hMatches, size_t matchCapacity, uint64_t* nMatches);
/** ZraHipSearchArchiveMulti through the handle: see ZraHipArchiveSearch. Overwrites ZraHipGetSearchMultiStats. This call and the two
 *  below take their patterns literally; with case folding and byte classes: the ZraHipArchive...Expr calls, further below. Not
 *  covered by either: quantifiers, alternation, anchors. */
ZRA_EXPORT ZraStatus ZraHipArchiveSearchMulti(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    struct ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern);
/** ZraHipGrepArchive through the handle: see ZraHipArchiveSearch. Overwrites ZraHipGetGrepStats. */
ZRA_EXPORT ZraStatus ZraHipArchiveGrep(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    struct ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
/** ZraHipExtractRecords through the handle: see ZraHipArchiveSearch. dData must overlap neither the archive nor the handle's arena
 *  ({ZStdError, 42}, joined to rule 2). Overwrites ZraHipGetExtractStats. */
ZRA_EXPORT ZraStatus ZraHipArchiveExtractRecords(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    struct ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** out8 = {scans accepted, frames staged from the cache in the last accepted scan, frames decoded in it, passes of it, frames staged
 *  (cumulative), frames decoded (cumulative), 0, 0}, over the four calls above. A scan is accepted when it returns Success; the early
 *  returns that decode nothing count, with zeros for the three last-scan words. A scan that is not accepted changes none of the words.
 *  archive NULL: all zero; out8 NULL: no-op. */
ZRA_EXPORT void ZraHipArchiveGetScanStats(const ZraHipArchive* archive, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugUpdateStageMs: HIP-event time of the last accepted scan's job-split and stage-from-cache launches,
 *  summed over its passes; 0 when none ran. archive NULL: 0. */
ZRA_EXPORT double ZraHipDebugArchiveScanStageMs(const ZraHipArchive* archive);
/** Bring-up aid: where the handle's arena lies, [*base, *base + *bytes) in device memory, so that a test can aim a buffer at it and
 *  see the arena check of the calls above, of ZraHipArchiveUpdate and of the extracts through a handle refuse it. The arena is the
 *  handle's own: nothing but the handle may write it, and the range holds until ZraHipArchiveClose. A handle without a cache, and
 *  archive NULL, give NULL and 0; base or bytes NULL: no-op. */
ZRA_EXPORT void ZraHipDebugArchiveArena(const ZraHipArchive* archive, const void** base, size_t* bytes);

/* ---- the record index through the handle: index, locate and read records from the frame cache ----
 * ZraHipIndexRecords, ZraHipLocateRecords and ZraHipReadRecords (below) are the one read path whose caller comes back to the same frames
 * again and again: a server that hands out records by number draws its batches from a hot set, and every plain call decodes every frame
 * that holds a boundary, the read a second time for the bytes. Through the handle the resident ones are not decoded. It also closes the
 * handle's own workflow: after ZraHipArchiveUpdate the touched resident frames hold their new plaintext, and the sub-range call that
 * refreshes their index words takes it from there. */
struct ZraHipRecordIndex;    /* defined with ZraHipIndexRecords */

/** ZraHipIndexRecords on the archive the handle is bound to: its arguments without engine, dArchive and archiveSize. Synchronous; stream
 *  ordering as the other compute calls (ZraHipWaitStream). What is said here holds for ZraHipArchiveLocateRecords and
 *  ZraHipArchiveReadRecords as well, each against its engine-level counterpart, run on the handle's engine, on the bytes the handle is
 *  bound to, with the same arguments.
 *  - Result: the words at dIndex, *info, hRanges, dData and *dataSize are byte for byte the plain call's, and so is what stays
 *    untouched on failure.
 *  - Statuses: the plain call's, in its order, with four differences. archive NULL -> {ZStdError, 42} in front of everything; the
 *    output words are zeroed as the plain call zeroes them. The header is the handle's checked one and is not read from the device: a
 *    frame size of 0 -> HeaderInvalid is the only header status left. Locate and read check the archive against *info (rule 3,
 *    {ZStdError, 40}) by the handle's header. And the overlap rule (rule 2 of the index, the read's dData rule) additionally refuses a
 *    dIndex or dData range that overlaps the handle's arena with {ZStdError, 42}, the arena check of ZraHipArchiveUpdate.
 *  - Where the plaintext of a whole-frame sweep comes from (at least 1 slot): the sweep needs the frames of the index range, or the
 *    boundary frames of the locate sweep. One that is resident is copied from its arena slot into its slot of the staging window,
 *    min(frameSize, U - f * frameSize) bytes, and is not decoded (no damage is laundered by this: a frame is resident only after a whole
 *    decode with status 0, checksum verified, exact size); one that is not resident is decoded whole, its checksum verified, exactly as
 *    by the plain call. The tile-count, frame-word, stale-word and select kernels run over the same window and are the plain call's: a
 *    stale word of a staged resident frame is found like any other ({ZStdError, 20}).
 *  - Index and locate are not reads: they insert, evict and refresh nothing, set no reference bit and move no hand, and never write
 *    the arena. Every word of ZraHipArchiveGetStats stays as it was, on success and on failure. A frame that fails is by construction
 *    not resident; the status is the plain rule: the lowest failing frame of the first failing pass.
 *  - 0 slots: the plain call minus the header read; the same kernels are launched.
 *  - Stats: the call is one of its kind on the handle's engine: it overwrites ZraHipGetIndexRecordsStats and ZraHipDebugIndexRecordsMs
 *    (locate, read: their own kind's) under their rules. The index's words are the plain call's. Through a handle the locate's words
 *    [3] and [4] and the read's word [3] count decode jobs and the bytes those regenerated: they leave out the frames staged from the
 *    arena; the read's word [4] is the frames its byte fetch decoded. ZraHipGetKernelStats reports 0 decode launches for a call
 *    whose frames were all resident.
 *  - Scratch: the plain call's, plus, with at least 1 slot, 16 bytes per frame of a pass for the copy entries and the pass's counts,
 *    which come to the host through a page-locked word of the handle, one small read-back per pass.
 *  Not covered: populating the cache from the index or the locate, sweep kernels that read the arena in place (they address frames
 *  slot by slot, so they could), fusing the two sweeps of the read, shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipArchiveIndexRecords(ZraHipArchive* archive, uint32_t delimiter, uint64_t firstFrame, uint64_t frameCount,
    size_t stagingBytes, uint64_t* dIndex, size_t indexCapacityWords, struct ZraHipRecordIndex* info);
/** ZraHipLocateRecords through the handle: see ZraHipArchiveIndexRecords. Overwrites ZraHipGetLocateRecordsStats. */
ZRA_EXPORT ZraStatus ZraHipArchiveLocateRecords(ZraHipArchive* archive, const struct ZraHipRecordIndex* info, const uint64_t* dIndex,
    size_t indexWords, const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes, struct ZraHipContentRange* hRanges);
/** ZraHipReadRecords through the handle: a composition, as the plain call is. The locate sweep runs as described with
 *  ZraHipArchiveIndexRecords; then the located ranges are fetched with the semantics of ZraHipArchiveRead on this handle (record k < D
 *  as [s_k, t_k + 1), the end bound inclusive; an open last record gets its delimiter byte stored separately).
 *  THE BYTE FETCH IS A READ: it counts one read, hits plus misses are the distinct frames the located ranges touch, misses are
 *  decoded whole, checksums verified, into CLOCK victims, more misses than slots go in passes, and a failing fetch leaves its
 *  claimed slots empty.
 *  Statuses: the locate sweep's, then OutputBufferTooSmall, then those of ZraHipArchiveRead for the located ranges. On a damaged
 *  archive the one difference from the plain call is the one ZraHipArchiveRead has: with at least 1 slot a frame that only the fetch
 *  decodes (an interior frame of a record longer than a frame) is decoded whole and its checksum looked at.
 *  The sizing call (dataCapacity 0) runs the locate sweep only and changes no word of ZraHipArchiveGetStats. A second identical call
 *  with every touched frame resident launches the decoder in neither sweep. dData must overlap neither the archive, the index nor the
 *  handle's arena. Overwrites ZraHipGetReadRecordsStats. */
ZRA_EXPORT ZraStatus ZraHipArchiveReadRecords(ZraHipArchive* archive, const struct ZraHipRecordIndex* info, const uint64_t* dIndex,
    size_t indexWords, const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes, struct ZraHipContentRange* hRanges,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** out8 = {record calls accepted, frames staged from the cache in the last accepted call's whole-frame sweep, frames decoded by that
 *  sweep, its passes, frames staged (cumulative), frames decoded (cumulative), 0, 0}, over the three calls above; the read's byte fetch
 *  is in ZraHipArchiveGetStats. A call is accepted when it returns Success; the early returns that decode nothing count, with zeros
 *  for the three last-call words. A call that is not accepted changes none of the words. archive NULL: all zero; out8 NULL: no-op. */
ZRA_EXPORT void ZraHipArchiveGetRecordStats(const ZraHipArchive* archive, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugArchiveScanStageMs: HIP-event time of the last accepted record call's job-split and stage-from-cache
 *  launches, summed over its passes; 0 when none ran. archive NULL: 0. */
ZRA_EXPORT double ZraHipDebugArchiveRecordStageMs(const ZraHipArchive* archive);

/* ---- update: a new archive from an old one, on the device ----
 * The reference's Compressor only ever starts from nothing. Frames are independent zstd frames tied together by the seek table alone,
 * so a change re-encodes the frames it lands in and carries every other frame over byte for byte. */

/** dOut receives an archive whose content is that of the archive at dArchive with
 *    - bytes [hOffsets[i], hOffsets[i] + hSizes[i]) replaced by dData + hDataOffsets[i], for every write i (host arrays of nWrites
 *      entries, as ZraHipDecompressRABatch; dArchive, dData, dAppend and dOut are device pointers), and
 *    - appendSize bytes from dAppend added at the end.
 *  The frame size is the archive's own: U' = U + appendSize, F' = ceil(U' / frameSize). Synchronous; stream ordering as the other
 *  compute calls (ZraHipWaitStream).
 *  - A frame is TOUCHED if a non-empty write intersects it or an appended byte lands in it (the old last frame when U is not a multiple
 *    of frameSize and appendSize > 0; every new frame). Each touched frame is encoded from its new content with compressionLevel and
 *    checksum, exactly as ZraHipCompressBuffer encodes a frame of that content: at the level and checksum flag the archive was written
 *    with, the result is byte-identical (header, table and CRC-32 included) to ZraHipCompressBuffer of the patched content.
 *  - Every other frame's compressed bytes are CARRIED OVER unchanged. They are neither decoded nor verified: damage in an untouched
 *    frame survives the update, exactly as it was (ZraHipVerifyArchive below finds it).
 *  - A touched frame that keeps some of its old bytes is first decoded whole and its content checksum verified (an update does not
 *    launder damage); a touched frame whose every byte is replaced is not decoded at all.
 *  - Header: the 38 fixed bytes are rewritten (U', the new table size), the meta section of a streaming-Compressor archive is copied
 *    verbatim, the new seek table and the CRC-32 follow. The table and the CRC pass through the host (5 bytes per frame); the body
 *    never leaves the device.
 *  Statuses, checked in this order; on every status other than Success no byte of dOut is written:
 *   1. engine, outSize or dOut NULL; dArchive NULL with archiveSize != 0; an h* array NULL with nWrites != 0; dData NULL while a write is
 *      non-empty; dAppend NULL with appendSize != 0 -> {ZStdError, 42}, the refusal of the archive and comm calls.
 *   2. [dOut, dOut + outCapacity) overlaps [dArchive, dArchive + archiveSize) -> {ZStdError, 42}.
 *   3. Header problems: the statuses of ZraHipArchiveOpen (a frame size of 0, or a table that does not cover the content: HeaderInvalid).
 *   4. A non-empty write with offset + size > U (or a sum that overflows) -> OutOfBoundsAccess. The bound is inclusive on purpose: the
 *      reference's ">=" (zra.cpp:260) is a quirk of its reads, and a write must be able to reach the last byte. Two non-empty writes that
 *      share a byte -> {ZStdError, 42}: there is no "last one wins" between copies that run side by side. Empty writes are ignored
 *      wherever they point.
 *   5. An old seek table that runs backwards over a frame that is carried over, or ends beyond the body -> {ZStdError, 20}.
 *   6. A touched frame that has to be decoded and fails: the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for
 *      a query inside that frame; of several failing frames, the one with the lowest index.
 *   7. header + body >= 2^40 -> CompressedSizeTooLarge (ZraHipCompressBuffer's rule).
 *   8. outCapacity smaller than the result -> OutputBufferTooSmall, and *outSize holds the size needed. (ZraGetCompressedOutputBufferSize(U',
 *      frameSize) + the meta size is always enough for the touched frames; carried frames keep the size they have.)
 *  *outSize is written on Success and by rule 8 and on no other status: it is not touched then (the same through ZraHipArchiveUpdate).
 *   9. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's: plaintext staging of at most 65,536 frames or 4 GiB
 *      (more touched frames go through several decode / encode passes), the newly encoded frames, 29 bytes per frame of tables;
 *      ZraHipReleaseScratch returns it.
 *  An open ZraHipArchive handle requires unchanged archive bytes: update into a new buffer and open a new handle on it, or update
 *  through the handle (ZraHipArchiveUpdate), which keeps its cache. */
ZRA_EXPORT ZraStatus ZraHipUpdateArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* dData, const uint64_t* hOffsets, const uint64_t* hSizes, const uint64_t* hDataOffsets, size_t nWrites,
    const void* dAppend, size_t appendSize,
    void* dOut, size_t outCapacity, size_t* outSize,
    int8_t compressionLevel, bool checksum);
/** What the last ZraHipUpdateArchive on the engine did (all zero after any outcome other than Success; engine NULL: all zero):
 *  out8 = {frames in the result, frames touched, frames decoded, frames compressed, compressed bytes carried over, compressed bytes
 *  newly encoded, content bytes replaced or appended, decode / encode passes}. Counters, not timings. */
ZRA_EXPORT void ZraHipGetUpdateStats(ZraHipEngine* engine, uint64_t* out8);

/* ---- verify: every faulty frame of a device-resident archive, without an output buffer ----
 * The counterpart of `zstd -t` for an archive that lives in HBM through many updates. ZraHipDecompressBuffer needs room for the whole
 * content and stops at the first failing frame; this call needs a bounded staging window and reports every bad frame. */
#define ZRA_HIP_VERIFY_STRUCTURE 1u   /* header, CRC-32, seek table, every frame's zstd frame header and block-header walk; nothing decoded */
#define ZRA_HIP_VERIFY_CONTENT   2u   /* the above, then every structurally sound frame decoded whole, content checksum verified */

/** One faulty frame. code: zstd error code; stage: the ZRA_HIP_VERIFY_* bit that found it. */
typedef struct ZraHipFrameFault { uint64_t frame; uint32_t code; uint32_t stage; } ZraHipFrameFault;

/** Checks frames [firstFrame, firstFrame + frameCount) of the archive at dArchive (archiveSize bytes, device memory); frameCount =
 *  UINT64_MAX: to the last frame. Synchronous; stream ordering as the other compute calls (ZraHipWaitStream). The archive is only read.
 *  Result:
 *  - Success whenever the verification ran, however many frames are bad: bad frames are data, not a failure of the call.
 *  - *nFaults = the faulty frames of the range; it may exceed faultCapacity. The first min(*nFaults, faultCapacity) of them are written
 *    to hFaults (a HOST array) in ascending frame order, at most one entry per frame. hFaults may be NULL when faultCapacity is 0.
 *  - On any status other than Success nothing is written to hFaults and *nFaults is 0.
 *  Statuses, checked in this order:
 *   1. engine or nFaults NULL; dArchive NULL with archiveSize != 0; hFaults NULL with faultCapacity != 0; mode 0 or with bits other than
 *      the two above -> {ZStdError, 42}.
 *   2. Header problems: the statuses of ZraHipArchiveOpen.
 *   3. The stored header CRC-32 differs from the one computed over the header as it lies on the device (fixed part, meta section, seek
 *      table) -> HeaderInvalid, the status of the host-pointer option ZRA_HIP_OPT_VERIFY_HEADER_CRC. The header travels to the host
 *      once for this, 5 bytes per frame; no other byte of the archive leaves the device.
 *   4. firstFrame > frames, or frameCount != UINT64_MAX and firstFrame + frameCount > frames -> OutOfBoundsAccess. An empty range is
 *      Success with 0 faults.
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's (ZraHipReleaseScratch returns it): 28 bytes of
 *      tables per frame of the RANGE, 16 bytes per listed fault, the staging window, the decoder's own scratch for one pass.
 *  STRUCTURE stage (always): one lane per frame, nothing decoded; it reads the frame's two table entries, its frame header and three
 *  bytes per block. With [a, b) = the frame's seek-table span and n = b - a, the first rule of this table that holds gives the code:
 *      b < a, or b > body size                                                              72  (the span convention of the decoder)
 *      the archive's last frame: b != body size                                             72
 *      n < 9, n >= 4 GiB, or n < frame header size + 3                                      72
 *      magic != 0xFD2FB528                                                                  10
 *      reserved bit of the frame header descriptor set                                      14
 *      window descriptor with a window log above 31 (frames without Single_Segment)         16
 *      a dictionary id other than 0                                                         32
 *      a declared Frame_Content_Size != min(frameSize, uncompressedSize - frame * frameSize): larger 70, smaller 20
 *      block walk from the end of the frame header, a 3-byte block header at a time (raw and compressed blocks advance by
 *      Block_Size, RLE blocks by 1), up to and including the block with Last_Block set:
 *        fewer than 3 bytes left for a block header                                         72
 *        reserved block type 3                                                              20
 *        a block body running past the span                                                 72
 *      the end of the last block, plus 4 when the checksum flag is set, != n                72
 *  These are the decoder's own rules, restated (a frame flagged here also fails when it is decoded); the decoder may name another
 *  code for the same frame where it meets a second problem first.
 *  CONTENT stage (only with ZRA_HIP_VERIFY_CONTENT): the frames of the range that passed the structure stage — the others are not
 *  decoded — are decoded whole, in frame order, into a staging window of stagingBytes (0: min(65,536 frames, 4 GiB), the update's
 *  bound) in passes of max(1, min(65,536, stagingBytes / frameSize)) frames, and their content checksums are verified. A frame's code is
 *  the one ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it (a frame that regenerates another size
 *  than its slot: 20). A failing frame does not disturb another frame of its pass. After each pass the per-frame statuses are compacted
 *  into the fault list on the device, in order; the list comes to the host once, at the end.
 *  Not covered: the shards of a distributed archive (ZraHipShard), repair, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipVerifyArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t mode,
                                         uint64_t firstFrame, uint64_t frameCount, size_t stagingBytes,
                                         ZraHipFrameFault* hFaults, size_t faultCapacity, size_t* nFaults);
/** The last ZraHipVerifyArchive on the engine (all zero after any outcome other than Success; engine NULL: all zero):
 *  out8 = {frames in the archive, frames checked, structure faults, content faults, frames decoded, content bytes regenerated, decode
 *  passes, 0}. Counters, not timings. */
ZRA_EXPORT void ZraHipGetVerifyStats(ZraHipEngine* engine, uint64_t* out8);

/* ---- search: where a byte pattern occurs in the content of a device-resident archive, without an output buffer ----
 * The counterpart of `zstdgrep`. Random access answers "give me bytes [a, b)"; a caller who does not know the offset yet would have to
 * ZraHipDecompressBuffer the whole content into a second buffer and scan it with code of their own. This call decodes the frames of a
 * content range into a bounded staging window, a pass at a time, and scans the plaintext where it lies. */
#define ZRA_HIP_SEARCH_MAX_PATTERN 256u

/** Finds the patternSize bytes at hPattern (HOST memory, 1 .. ZRA_HIP_SEARCH_MAX_PATTERN bytes, taken literally) in the content range
 *  [offset, offset + size) of the archive at dArchive (archiveSize bytes, device memory); size = UINT64_MAX: to the end of the content.
 *  Synchronous; stream ordering as the other compute calls (ZraHipWaitStream). The archive is only read.
 *  Result, with m = patternSize and [lo, hi) = the range:
 *  - A match is a content offset p with lo <= p, p + m <= hi and content[p, p + m) == pattern: the whole occurrence lies inside the
 *    range. Overlapping occurrences are all matches (00 00 00 in 1,000 zero bytes has 998).
 *  - *nMatches = the number of matches; it may exceed matchCapacity. The first min(*nMatches, matchCapacity) offsets are written to
 *    hMatches (a HOST array) in ascending order, each exactly once; nothing is written behind them. hMatches may be NULL when
 *    matchCapacity is 0: a count-only search.
 *  - On any status other than Success nothing is written to hMatches and *nMatches is 0. No offset reaches the host before the last
 *    pass is done: a search never reports matches from an archive it could not decode.
 *  Statuses, checked in this order:
 *   1. engine, nMatches or hPattern NULL; dArchive NULL with archiveSize != 0; hMatches NULL with matchCapacity != 0; patternSize 0 or
 *      above ZRA_HIP_SEARCH_MAX_PATTERN -> {ZStdError, 42}.
 *   2. Header problems: the statuses of ZraHipArchiveOpen (content without frames, i.e. a frame size of 0: HeaderInvalid). The stored
 *      header CRC-32 is NOT checked here: that is ZraHipVerifyArchive's job.
 *   3. offset > U, or size != UINT64_MAX and offset + size > U (or a sum that overflows) -> OutOfBoundsAccess. The bound is inclusive, as
 *      the update's rule 4: a search must be able to reach the last byte. A range shorter than the pattern, the empty range included, is
 *      Success with 0 matches, and nothing is decoded.
 *   4. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's (ZraHipReleaseScratch returns it): the staging
 *      window, a carry area of ZRA_HIP_SEARCH_MAX_PATTERN bytes in front of it, 8 bytes per listed match, 12 bytes per 8 KiB of window
 *      for the tile tables, the decoder's own scratch for one pass.
 *   5. A decoded frame that fails: the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside that
 *      frame; of several failing frames, the one with the lowest index (passes run in frame order and the call stops behind the first
 *      pass with a failing frame).
 *  Only the frames that intersect [lo, hi) are decoded, each whole, its content checksum verified, in frame order, into a staging
 *  window of stagingBytes (0: min(65,536 frames, 4 GiB)) in passes of max(1, min(65,536, stagingBytes / frameSize)) frames: the rules
 *  of ZraHipVerifyArchive. Frames outside the range are not touched; damage there does not disturb the search. Occurrences that
 *  straddle frames or passes are found: the last m - 1 bytes of a pass are carried in front of the next one, and an occurrence is
 *  reported by the pass that holds its last byte.
 *  Cost: the scan reads every decoded byte once from HBM and a few times from LDS; a position whose first min(m, 4) bytes differ from
 *  the pattern's costs one word compare. The worst case is a pattern that matches everywhere (zeros in zeros): every position then runs
 *  the full m-byte compare, and every listed match is compared twice. That is accepted; there is no machinery for it.
 *  Several patterns per call: ZraHipSearchArchiveMulti, below.
 *  Resident frames of a ZraHipArchive are staged from its cache, not decoded, by the handle's call: ZraHipArchiveSearch, above.
 *  Not covered: regular
 *  expressions, the shards of a distributed archive (ZraHipShard), the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipSearchArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPattern, size_t patternSize,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    uint64_t* hMatches, size_t matchCapacity, uint64_t* nMatches);
/** The last ZraHipSearchArchive on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, frames decoded, content bytes regenerated, matches, matches listed, decode passes, 0, 0}. Counters,
 *  not timings. */
ZRA_EXPORT void ZraHipGetSearchStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugUpdateStageMs: HIP-event time of the last search's scan launches (count, prefix scan, fill, carry),
 *  summed over its passes; the decode of the same call is in ZraHipGetKernelStats. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugSearchScanMs(ZraHipEngine* engine);

/* ---- search for several patterns in one pass: what `grep -F -f patterns` is to `grep` ----
 * The cost of a search is the decode of every frame of its range. A caller with K strings (request ids, a keyword list) would pay K
 * decodes of the same frames with ZraHipSearchArchive and merge K lists on the host; this call decodes once and scans for all K. */
#define ZRA_HIP_SEARCH_MAX_PATTERNS      64u
#define ZRA_HIP_SEARCH_MAX_PATTERN_BYTES 4096u   /* sum of all pattern lengths */
typedef struct ZraHipPatternMatch { uint64_t offset; uint32_t pattern; uint32_t reserved; } ZraHipPatternMatch;  /* reserved = 0 */

/** Finds nPatterns byte patterns in the content range [offset, offset + size) of the archive at dArchive (size = UINT64_MAX: to the end
 *  of the content). hPatterns (HOST memory) holds the patterns one after the other; pattern i has hPatternSizes[i] bytes, 1 ..
 *  ZRA_HIP_SEARCH_MAX_PATTERN each, taken literally. Equal patterns are allowed and reported independently. Synchronous; the archive
 *  is only read.
 *  Result, with m_i the length of pattern i, M = max m_i and [lo, hi) = the range:
 *  - A match is a pair (p, i) with lo <= p, p + m_i <= hi and content[p, p + m_i) == pattern i. Overlapping occurrences are all
 *    matches, and so are several patterns at one p.
 *  - *nMatches = the number of matches; it may exceed matchCapacity. The first min(*nMatches, matchCapacity) matches are written to
 *    hMatches (a HOST array) in ascending (offset, pattern index) order, each exactly once, reserved = 0; nothing is written behind
 *    them. A capacity that ends between two matches at one offset cuts there. hMatches may be NULL when matchCapacity is 0.
 *  - hPerPattern may be NULL; otherwise a HOST array of nPatterns entries that receives the matches of each pattern, listed or not.
 *  - On any status other than Success nothing is written to hMatches or hPerPattern, *nMatches is 0 and all stats are zero. No match
 *    reaches the host before the last pass is done.
 *  Statuses, checked in this order:
 *   1. engine, nMatches, hPatterns or hPatternSizes NULL; dArchive NULL with archiveSize != 0; hMatches NULL with matchCapacity != 0;
 *      nPatterns 0 or above ZRA_HIP_SEARCH_MAX_PATTERNS; a pattern size of 0 or above ZRA_HIP_SEARCH_MAX_PATTERN; a sum of the sizes
 *      above ZRA_HIP_SEARCH_MAX_PATTERN_BYTES -> {ZStdError, 42}.
 *   2. Header problems: ZraHipSearchArchive's rule 2.
 *   3. The range: ZraHipSearchArchive's rule 3, inclusive bound. A range shorter than the shortest pattern is Success with 0 matches:
 *      nothing is decoded and hPerPattern is all zero.
 *   4. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's: the staging window with its carry area, 16 bytes
 *      per listed match, 28 bytes per 8 KiB of window, 14 KiB for the pattern table, the decoder's own scratch for one pass.
 *   5. A decoded frame that fails: ZraHipSearchArchive's rule 5.
 *  Passes, staging window, stagingBytes, "only the frames of the range", whole frames and verified checksums: ZraHipSearchArchive.
 *  The last M - 1 bytes of a pass are carried in front of the next one, and a start position p is tested, for all patterns, by the
 *  pass that holds content byte min(p + M - 1, hi - 1); the list ascends whatever the pattern lengths are.
 *  Cost: one decode of the range. The scan tests every position's first two bytes against a 65,536-bit table made of the patterns'
 *  first two bytes (a 1-byte pattern sets all 256 bits of its byte); only a position whose bit is set, a "filter survivor", is compared
 *  against the patterns that begin with its first byte. The worst case is patterns that match everywhere (64 patterns of zeros in
 *  zeros): every position then runs 64 full compares, and every listed match is compared twice. That is accepted.
 *  Through a ZraHipArchive handle, resident frames staged from its cache: ZraHipArchiveSearchMulti, above.
 *  Case folding and byte classes: ZraHipSearchArchiveMultiExpr, below.
 *  Not covered: quantifiers, alternation, anchors, patterns in device memory, shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipSearchArchiveMulti(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern);
/** The last ZraHipSearchArchiveMulti on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL:
 *  no-op): out8 = {frames in the archive, frames decoded, content bytes regenerated, matches, matches listed, decode passes, patterns,
 *  filter survivors}. A multi search does not touch ZraHipGetSearchStats, and the other way round. */
ZRA_EXPORT void ZraHipGetSearchMultiStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugSearchScanMs: HIP-event time of the scan launches of the last multi search. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugSearchMultiScanMs(ZraHipEngine* engine);

/* ---- grep: the records of a device-resident archive that hold a match, without an output buffer for the content ----
 * What `grep` itself returns: the lines. The searches above return byte offsets, and a caller who wants the record around a hit has to
 * find the delimiter in front of it and the one behind it, which means decoding the content a second time into a buffer of their own.
 * "How many lines match", "which lines hold any of these 40 request ids" and "which lines hold none of them" all need one pass over
 * the plaintext, and the multi search already pays for that pass. This call adds the delimiter to it. */
#define ZRA_HIP_GREP_INVERT 1u   /* select the records that hold NO match (grep -v) */

typedef struct ZraHipContentRange { uint64_t offset; uint64_t size; } ZraHipContentRange;

/** Lists the records of the content range [offset, offset + size) of the archive at dArchive in which one of nPatterns byte patterns
 *  occurs. Patterns and their limits (ZRA_HIP_SEARCH_MAX_PATTERNS, _MAX_PATTERN, _MAX_PATTERN_BYTES), the range [lo, hi) with its
 *  inclusive bound and size = UINT64_MAX, stagingBytes, passes, whole frames with verified checksums, "only the frames of the range",
 *  host synchrony and stream ordering: ZraHipSearchArchiveMulti's, word for word.
 *  Records. Let t_0 < t_1 < ... be the positions of [lo, hi) whose byte equals `delimiter`.
 *  - For every t_k there is a record [s_k, t_k), with s_0 = lo and s_k = t_(k-1) + 1.
 *  - A last record [s_last, hi) follows iff s_last < hi. With no delimiter at all that is the one record [lo, hi) iff lo < hi.
 *  - A record never contains its delimiter, and may be empty (two delimiters in a row). Content that ends in a delimiter has no
 *    trailing empty record. lo and hi act as record boundaries: a record the range cuts is reported clipped.
 *  Selection. A match is the multi search's: (p, i) with lo <= p, p + m_i <= hi and content[p, p + m_i) == pattern i. No pattern may
 *  contain the delimiter (rule 1), so an occurrence lies inside one record.
 *  - Without ZRA_HIP_GREP_INVERT a record is selected iff a match starts in it.
 *  - With ZRA_HIP_GREP_INVERT a record is selected iff none does. Empty records are then selected.
 *  Result.
 *  - *nRecords = the number of selected records; it may exceed recordCapacity. The first min(*nRecords, recordCapacity) selected
 *    records are written to hRecords (a HOST array) as {offset, size}, ascending, each exactly once; nothing is written behind them.
 *    hRecords may be NULL when recordCapacity is 0: that is `grep -c`.
 *  - On any status other than Success nothing is written to hRecords, *nRecords is 0 and all stats are zero. No entry reaches the
 *    host before the last pass is done.
 *  Statuses, checked in this order:
 *   1. ZraHipSearchArchiveMulti's rule 1 (hRecords, recordCapacity and nRecords in the place of hMatches, matchCapacity and nMatches);
 *      mode with bits other than ZRA_HIP_GREP_INVERT; a pattern that contains `delimiter` -> {ZStdError, 42}.
 *   2. Header problems: ZraHipSearchArchive's rule 2.
 *   3. The range: ZraHipSearchArchive's rule 3. The empty range is Success with 0 records in both modes. Without INVERT a range shorter
 *      than the shortest pattern is Success with 0 records: nothing is decoded, and the stats are {frames, 0, ...}, as the multi
 *      search's same shortcut. With INVERT that range is scanned like any other, and every record of it is selected.
 *   4. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's: the staging window with its carry area, 16 bytes
 *      per listed record, 32 bytes per 8 KiB of window for the per-tile tables, 14 KiB for the pattern table, 128 bytes for the
 *      carried record state and the totals, the decoder's own scratch for one pass.
 *   5. A decoded frame that fails: ZraHipSearchArchive's rule 5.
 *  A record is attributed to the delimiter that ends it (the last one to hi), by the pass that owns that position under the multi
 *  search's rule; a record that spans frames or passes is one record.
 *  Cost: one decode of the range and the multi search's filter; on top of it one byte compare per position and a segmented reduction
 *  over the positions between delimiters (profiles/grep_scan.md).
 *  Not covered: the BYTES of the records (ZraHipExtractRecords below keeps them from the same pass; with this call alone, fetch them
 *  with ZraHipDecompressRABatch or ZraHipArchiveRead from the listed ranges, under those calls' own bound rule), quantifiers, alternation, anchors (ZraHipGrepArchiveRegex, below; case folding and byte classes: ZraHipGrepArchiveExpr, below), multi-byte delimiters, shards, the
 *  host-pointer API. Through a ZraHipArchive handle, resident frames staged from its cache: ZraHipArchiveGrep, above. */
ZRA_EXPORT ZraStatus ZraHipGrepArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
/** The last ZraHipGrepArchive on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, frames decoded, content bytes regenerated, records of the range (selected or not), records selected,
 *  records listed, decode passes, matches}. matches = the (p, i) pairs, *nMatches of ZraHipSearchArchiveMulti on the same range, in
 *  both modes. A grep touches neither ZraHipGetSearchStats nor ZraHipGetSearchMultiStats, and the other way round. */
ZRA_EXPORT void ZraHipGetGrepStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugSearchMultiScanMs: HIP-event time of the scan launches of the last grep. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugGrepScanMs(ZraHipEngine* engine);

/** The grep that returns the lines: the selected records of ZraHipGrepArchive AND their bytes, from the same decode pass. Patterns and
 *  their limits, `delimiter`, `mode` (ZRA_HIP_GREP_INVERT only), the range [lo, hi) with its inclusive bound, stagingBytes, passes,
 *  "only the frames of the range", whole frames with verified checksums, the records and the selection: ZraHipGrepArchive's, word for
 *  word. The archive is only read.
 *  Result. Let the selected records be r_0 < r_1 < ..., r_i = [o_i, o_i + n_i).
 *  - *nRecords = their number, *dataSize = the sum of (n_i + 1).
 *  - dData (DEVICE memory, any alignment) receives, for each i in order, the n_i content bytes of r_i and then one byte `delimiter`.
 *    The last record, which hi ends rather than a delimiter, gets its delimiter too; an empty selected record is the one delimiter
 *    byte. Record i starts at d_i = the sum of (n_j + 1) over j < i: the host derives that from the list, there is no offsets array.
 *    The result is the text `grep -F` prints, and can go straight into ZraHipCompressBuffer.
 *  - A list is wanted iff recordCapacity != 0: it is written to hRecords (a HOST array) as the grep's list is, after the last pass,
 *    once. With recordCapacity == 0, hRecords may be NULL and only the bytes come back.
 *  - After Success the bytes of dData in [*dataSize, dataCapacity) are undefined. No byte in front of dData or at or behind dData +
 *    dataCapacity is ever written, whatever the outcome.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchive's rule 1; dataSize NULL; hRecords NULL with recordCapacity != 0; dData NULL with dataCapacity != 0
 *      -> {ZStdError, 42}.
 *   2. [dData, dData + dataCapacity) overlaps [dArchive, dArchive + archiveSize) -> {ZStdError, 42}.
 *   3. Header problems: ZraHipGrepArchive's rule 2.
 *   4. The range: ZraHipGrepArchive's rule 3, with the same two shortcuts (the empty range: Success, 0 records, 0 bytes; without
 *      INVERT a range shorter than the shortest pattern: Success with nothing decoded).
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the grep's with 64 bytes per 8 KiB of window for the per-tile
 *      tables, and 16 bytes per listed record up to recordCapacity; never an array per record of the pass.
 *   6. A decoded frame that fails: ZraHipGrepArchive's rule 5.
 *   7. OutputBufferTooSmall when recordCapacity != 0 && *nRecords > recordCapacity, or when *dataSize > dataCapacity. The two words
 *      hold what the call needs: the one outcome other than Success that sets them. Capacities 0 / 0 is the sizing call (Success
 *      when nothing is selected). Nothing is written to hRecords; the first dataCapacity bytes of dData are undefined.
 *  On every status other than Success the stats are zero and hRecords is untouched; apart from rule 7, *nRecords = *dataSize = 0.
 *  Cost: the grep's, plus one byte store per copied position (profiles/extract_scan.md).
 *  Through a ZraHipArchive handle, resident frames staged from its cache: ZraHipArchiveExtractRecords, above.
 *  Not covered: context lines, output without the delimiter bytes, and what ZraHipGrepArchive does not cover (case folding and byte
 *  classes: ZraHipExtractRecordsExpr, below). Records BY NUMBER are
 *  the record index's: ZraHipIndexRecords, ZraHipLocateRecords and ZraHipReadRecords below. */
ZRA_EXPORT ZraStatus ZraHipExtractRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** The last ZraHipExtractRecords on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, frames decoded, content bytes regenerated, records of the range, records selected, packed bytes
 *  (= *dataSize), decode passes, matches}. An extract touches neither the grep's stats nor the searches', and the other way round. */
ZRA_EXPORT void ZraHipGetExtractStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugGrepScanMs: HIP-event time of the last extract's own launches, summed over its passes. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugExtractMs(ZraHipEngine* engine);

/* ---- pattern expressions for the multi-pattern scans: case folding and byte classes ----
 * The six calls above that take several patterns (ZraHipSearchArchiveMulti, ZraHipGrepArchive, ZraHipExtractRecords and their
 * ZraHipArchive... twins) have a twin with one more word, `syntax`, behind nPatterns. Every ELEMENT of a pattern matches exactly one
 * byte: a literal, a case-folded letter or a byte set. A pattern therefore keeps a fixed length, counted in elements, and everything
 * the literal calls say about lengths, ranges, passes, ownership, records, capacities, statuses and stats holds word for word with
 * m_i = the number of elements of pattern i. Quantifiers, alternation and anchors need another scan and are not part of this; their
 * characters are reserved, so that adding them later changes the meaning of no expression accepted now. */
#define ZRA_HIP_PATTERN_FOLD_CASE 1u   /* ASCII letters match either case (grep -i) */
#define ZRA_HIP_PATTERN_CLASSES   2u   /* patterns are expressions: . [set] [^set] \escape */
#define ZRA_HIP_PATTERN_MAX_SETS        32u     /* distinct byte sets per call, see below */
#define ZRA_HIP_PATTERN_MAX_EXPR_BYTES  16384u  /* sum of the expression sizes */

/** Rule 1's pattern checks of the ...Expr calls, on the host alone: no engine, no device. hPatterns / hPatternSizes / nPatterns as
 *  for the calls; delimiter: the grep's and the extract's byte, or -1 for the multi search, which has none. On Success hLengths[i]
 *  (may be NULL) is pattern i's length in elements and *nSets (may be NULL) the number of counted sets. Any refusal -> {ZStdError, 42},
 *  the outputs untouched.
 *
 *  syntax == 0: literal bytes, as the literal calls take them. The two bits combine; any other bit is refused.
 *  Without ZRA_HIP_PATTERN_CLASSES the pattern bytes are literals and hPatternSizes[i] = m_i; FOLD_CASE still applies to them.
 *  With ZRA_HIP_PATTERN_CLASSES hPatternSizes[i] is the size of expression i in bytes (1 and up, ZRA_HIP_PATTERN_MAX_EXPR_BYTES in
 *  all); the limits of the literal calls apply to elements: 1 .. ZRA_HIP_SEARCH_MAX_PATTERN per pattern, _MAX_PATTERN_BYTES in all.
 *   .            any byte
 *   [items]      a byte set; [^items] its complement. An item is a byte, an escape, or a range a-b of two single bytes, a <= b.
 *                ] directly behind [ or [^ is a literal; - first or last is a literal; [ followed by : is refused, at the head of
 *                a set and inside one (POSIX classes are reserved). An unterminated set is refused.
 *   \xHH         the byte HH (hex digits of either case); \n \t \r
 *   \d \w \s     [0-9], [0-9A-Za-z_], space and \t \n \v \f \r; allowed inside a set, but not as either end of a range
 *   \c           the byte c, for c one of . [ ] \ * + ? { } ( ) | ^ $ -
 *                Any other byte behind \, and a \ at the end, is refused.
 *   ] * + ? { } ( ) | ^ $ unescaped outside a set are refused: reserved.
 *   Every other byte, NUL and bytes >= 0x80 included, is a literal. Bytes are bytes: nothing is UTF-8 aware.
 *  An element whose final set is empty is refused.
 *  ZRA_HIP_PATTERN_FOLD_CASE: a literal A-Z or a-z matches both cases; a set is closed under the case swap of its ASCII letters
 *  BEFORE a ^ complements it (grep -i '[^a]'). No other byte folds: not @ [ ` {, not 0xC0 .. 0xFF.
 *  The delimiter (grep and extract): no element may match it, so that an occurrence stays inside one record. `.` and [^...] lose it
 *  silently, as . never matches a newline in grep; a literal, a positive set or a fold that contains it is refused.
 *  ZRA_HIP_PATTERN_MAX_SETS bounds the distinct final sets of a call. A set of one byte does not count, nor does a set that is one
 *  letter in its two cases; equal sets count once. */
ZRA_EXPORT ZraStatus ZraHipCheckPatternExpr(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint32_t syntax, int delimiter, uint32_t* hLengths, uint32_t* nSets);

/** ZraHipSearchArchiveMulti with a syntax word: a match is (p, i) with lo <= p, p + m_i <= hi and element q of pattern i admitting
 *  content[p + q] for every q < m_i. Rule 1 gains ZraHipCheckPatternExpr's refusals (delimiter -1: `.` matches all 256 bytes).
 *  Everything else is the literal call's definition with m_i counted in elements, the shortcut "range shorter than the shortest
 *  pattern" included. Writes ZraHipGetSearchMultiStats and ZraHipDebugSearchMultiScanMs; "filter survivors" are the positions whose
 *  first two elements admit their bytes for some pattern. With syntax == 0 the call IS the literal one: the same kernels.
 *  Cost: a position is tested against the patterns whose first two elements admit its first two bytes, element by element from the
 *  third. A pattern that begins `..` makes every position a candidate (as 64 patterns of zeros in a content of zeros do for the
 *  literal call); the work per position is bounded by 64 patterns x 256 elements (profiles/pattern_expr.md).
 *  Not covered: quantifiers, alternation, anchors (for the grep: ZraHipGrepArchiveRegex, below), POSIX classes, UTF-8 awareness, patterns in device memory, shards, the host-pointer
 *  API, the single-pattern ZraHipSearchArchive (one expression goes through this call). */
ZRA_EXPORT ZraStatus ZraHipSearchArchiveMultiExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern);
/** ZraHipGrepArchive with a syntax word, as ZraHipSearchArchiveMultiExpr is to its twin; `delimiter` enters the pattern checks as
 *  described at ZraHipCheckPatternExpr. `mode` is the literal call's (ZRA_HIP_GREP_INVERT only). Writes ZraHipGetGrepStats and
 *  ZraHipDebugGrepScanMs. */
ZRA_EXPORT ZraStatus ZraHipGrepArchiveExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
/** ZraHipExtractRecords with a syntax word: see ZraHipGrepArchiveExpr. Writes ZraHipGetExtractStats and ZraHipDebugExtractMs. */
ZRA_EXPORT ZraStatus ZraHipExtractRecordsExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** The three through a ZraHipArchive handle: ZraHipArchiveSearchMulti, ZraHipArchiveGrep and ZraHipArchiveExtractRecords with the
 *  syntax word; resident frames are staged from the cache as for their twins, and the handle's counters move as for them. */
ZRA_EXPORT ZraStatus ZraHipArchiveSearchMultiExpr(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint64_t offset, uint64_t size,
    size_t stagingBytes,
    ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern);
ZRA_EXPORT ZraStatus ZraHipArchiveGrepExpr(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
ZRA_EXPORT ZraStatus ZraHipArchiveExtractRecordsExpr(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);

/* ---- grep with a record predicate: AND, OR and NOT of the patterns, per record, in one pass ----
 * ZraHipGrepArchive selects a record when ANY pattern occurs in it. "Lines with ERROR and user=42 but not healthcheck" is
 * `grep A | grep B | grep -v C`: one grep per term, each decoding the range again, and an intersection of the lists on the host.
 * The scan already knows WHICH patterns hit at a position; this call keeps that set per record and tests a predicate on it. */
#define ZRA_HIP_WHERE_MAX_CLAUSES 8

typedef struct ZraHipRecordClause { uint64_t all, any, none; } ZraHipRecordClause;  /* bit i = pattern i */

/** Rule 1 of ZraHipGrepArchiveWhere as far as the clauses go, on the host alone: no engine, no device. {ZStdError, 42} when hClauses
 *  is NULL, nClauses is 0 or above ZRA_HIP_WHERE_MAX_CLAUSES, nPatterns is 0 or above ZRA_HIP_SEARCH_MAX_PATTERNS, a clause has a bit
 *  at or above nPatterns, or a clause has all & none != 0 or any & none != 0 (it demands and forbids one pattern). Else Success. */
ZRA_EXPORT ZraStatus ZraHipCheckRecordClauses(const ZraHipRecordClause* hClauses, size_t nClauses, size_t nPatterns);

/** ZraHipGrepArchiveExpr with a predicate over the patterns in the place of "any pattern". Patterns with their `syntax` word (0:
 *  literal bytes; ZRA_HIP_PATTERN_FOLD_CASE, ZRA_HIP_PATTERN_CLASSES), `delimiter`, the range, stagingBytes, passes, ownership, the
 *  records and the matches are that call's, word for word.
 *  Selection. The hit set of a record is H = { i : a match (p, i) of the multi search on [lo, hi) starts inside the record }.
 *  A clause {all, any, none} holds for H when (H & all) == all, and any == 0 or (H & any) != 0, and (H & none) == 0. A record is
 *  selected when one of the nClauses clauses holds; ZRA_HIP_GREP_INVERT in `mode` complements that answer.
 *  - {0, all patterns, 0} is the plain grep; {0, 0, all patterns} is grep -v; {0, 0, 0} selects every record.
 *  - "A and B and not C" is {A|B, 0, C}; "(A and B) or not C" is the two clauses {A|B, 0, 0}, {0, 0, C}.
 *  Result, capacity 0 as `grep -c`, "nothing reaches the host before the last pass" and the stats: ZraHipGrepArchive's. The call
 *  writes ZraHipGetGrepStats (matches = the (p, i) pairs, whatever the predicate) and ZraHipDebugGrepScanMs.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchiveExpr's rule 1, then ZraHipCheckRecordClauses' refusals -> {ZStdError, 42}. Nothing is decoded.
 *   2. Header problems: ZraHipSearchArchive's rule 2.
 *   3. The range: ZraHipSearchArchive's rule 3. The empty range is Success with 0 records. In a non-empty range shorter than the
 *      shortest pattern every record has H = {}: when the predicate, INVERT applied, is false on the empty set, the call is Success
 *      with 0 records, nothing decoded and stats {frames, 0, ...}; otherwise the range is scanned and every record of it is selected.
 *   4. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the grep's, with 64 bytes per 8 KiB of window for the per-tile
 *      tables in the place of 32: a tile's summary and its head carry a 64-bit pattern set each.
 *   5. A decoded frame that fails: ZraHipSearchArchive's rule 5.
 *  Cost: the grep's; a trip of 64 positions in which something hit pays one lane read per hitting lane and one ballot per distinct
 *  pattern that hit in it, or, from 8 hitting lanes on, a six-step scan over the lanes: 1.01 to 1.04 times the grep's scan time on
 *  log text, 1.35 times with a hit at nearly every position (profiles/grep_where.md). The plain entry points keep their own kernels.
 *  The selected records' bytes: ZraHipExtractRecordsWhere, below. Not covered: per-pattern record counts, quantifiers, alternation inside a pattern, anchors (ZraHipGrepArchiveRegex, below),
 *  context lines, shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipGrepArchiveWhere(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    const ZraHipRecordClause* hClauses, size_t nClauses,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
/** ZraHipGrepArchiveWhere through a ZraHipArchive handle: resident frames are staged from the cache as for ZraHipArchiveGrep, the
 *  cache is not changed, and the handle's scan counters (ZraHipArchiveGetScanStats) move as for that call. */
ZRA_EXPORT ZraStatus ZraHipArchiveGrepWhere(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    const ZraHipRecordClause* hClauses, size_t nClauses,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);

/** The records ZraHipGrepArchiveWhere selects WITH their bytes, packed: the text `grep A | grep B | grep -v C` prints, from the one
 *  decode pass that selects the records. The meaning is the composition of two contracts, word for word.
 *  Selection: ZraHipGrepArchiveWhere's. 1 .. 64 patterns with their `syntax` word (0: literal bytes; ZRA_HIP_PATTERN_FOLD_CASE,
 *  ZRA_HIP_PATTERN_CLASSES); the hit set of a record is H = { i : a match (p, i) of the multi search on [lo, hi) starts inside the
 *  record }; a clause {all, any, none} holds for H when (H & all) == all, and any == 0 or (H & any) != 0, and (H & none) == 0; a
 *  record is selected when one of the 1 .. ZRA_HIP_WHERE_MAX_CLAUSES clauses holds, and ZRA_HIP_GREP_INVERT, the only bit of `mode`,
 *  complements that answer. lo and hi cut records the way delimiters do.
 *  Result: ZraHipExtractRecordsExpr's. *nRecords = the selected records; *dataSize = the sum of (n_i + 1) over them; dData (device
 *  memory) receives each selected record's bytes followed by one `delimiter` byte, in ascending order, the last record, which hi
 *  ends, included. The list goes to hRecords once, after the last pass, only on Success and only when recordCapacity != 0. The
 *  bytes of dData in [*dataSize, dataCapacity) are undefined after Success (a record open at the end of a pass is copied before its
 *  selection is known: under a predicate that can change up to the record's last byte); no byte outside [dData, dData +
 *  dataCapacity) is ever written, whatever the outcome.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchiveWhere's rule 1 (ZraHipGrepArchiveExpr's, then every refusal of ZraHipCheckRecordClauses); dataSize NULL;
 *      hRecords NULL with recordCapacity != 0; dData NULL with dataCapacity != 0 -> {ZStdError, 42}. Nothing is decoded.
 *   2. dData overlaps the archive (through a handle: or the handle's arena) -> {ZStdError, 42}.
 *   3. Header problems: ZraHipGrepArchive's rule 2.
 *   4. The range: ZraHipGrepArchiveWhere's rule 3. The empty range is Success with 0 records and 0 bytes. In a non-empty range
 *      shorter than the shortest pattern every record has H = {}: when the predicate, INVERT applied, is false on the empty set, the
 *      call is Success with 0 records and 0 bytes, nothing decoded and stats {frames, 0, ...}; otherwise the range is scanned and
 *      every record of it is selected.
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the extract's with 96 bytes per 8 KiB of window for the
 *      per-tile tables in the place of 64.
 *   6. A decoded frame that fails: ZraHipGrepArchive's rule 5.
 *   7. OutputBufferTooSmall: ZraHipExtractRecords's rule 7, word for word: *nRecords and *dataSize then hold what the call needs,
 *      hRecords is not written. recordCapacity 0 and dataCapacity 0 make the sizing call, which launches no copy kernel.
 *  Zeroing of the outputs and the stats on every other status: ZraHipExtractRecords's rules.
 *  The call writes ZraHipGetExtractStats and ZraHipDebugExtractMs as ZraHipExtractRecordsExpr does; word 7, matches, is the number
 *  of (p, i) pairs, whatever the predicate. The grep's and the searches' stats are left alone.
 *  Cost: ZraHipGrepArchiveWhere's, plus a second walk of the tiles that hold a copied byte: measured on 1 GiB of log lines, the call's
 *  launches take 1.20 to 1.46 times the predicate grep's scan and 1.12 to 1.21 times ZraHipExtractRecords' under the plain predicate,
 *  and the call 0.72 to 0.78 of the wall time of the predicate grep followed by a ZraHipDecompressRABatch of the listed ranges once
 *  thousands of records are selected (profiles/extract_where.md).
 *  Not covered: context records with the predicate, the predicate over regular expressions, per-pattern record counts, shards, the
 *  host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipExtractRecordsWhere(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    const ZraHipRecordClause* hClauses, size_t nClauses,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** ZraHipExtractRecordsWhere through a ZraHipArchive handle: resident frames are staged from the cache as for
 *  ZraHipArchiveExtractRecords, the cache is not changed, dData must overlap neither the archive nor the handle's arena (rule 2),
 *  and the handle's scan counters (ZraHipArchiveGetScanStats) move as for ZraHipArchiveExtractRecords. */
ZRA_EXPORT ZraStatus ZraHipArchiveExtractRecordsWhere(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    const ZraHipRecordClause* hClauses, size_t nClauses,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);

/* ---- cut records: the chosen fields of the selected records, packed ----
 * `grep -F A | cut -d SEP -f LIST`. A log or CSV archive is rarely queried for whole lines; the extract packs whole records, and the
 * plaintext, the record boundaries and the selection all lie in the staging window when it runs. This call adds "which field is
 * this byte in" and packs only the chosen fields of each selected record. */
#define ZRA_HIP_CUT_MAX_FIELD 64
/** cut's LIST (`1,3,5-7,9-`, `-3`) as a field mask, on the host: bit j - 1 stands for field j, bit 63 for field 64 AND every later one
 *  (cut's `64-`). Items are separated by commas; an item is N, N-M, N- or -M, numbers from 1. A range whose end lies above 64, and
 *  N- with N >= 64, set bit 63 (and the bits of the fields below 64 they cover); a lone field above 64 is refused, because it cannot
 *  be told from `64-`. {ZStdError, 42} with *mask = 0 (where mask is not NULL): list or mask NULL, an empty list or item, a 0, a
 *  decreasing range, any other character. */
ZRA_EXPORT ZraStatus ZraHipFieldMask(const char* list, uint64_t* mask);
/** The records ZraHipExtractRecordsExpr selects, of each only the chosen fields, packed: the text `grep -F -f patterns | cut -d SEP
 *  -f LIST` prints, from the one decode pass that selects the records.
 *  Selection: ZraHipExtractRecordsExpr's, word for word: the patterns with their `syntax` word (0: literal bytes), `delimiter`,
 *  `mode` (ZRA_HIP_GREP_INVERT only), the range with lo and hi cutting records the way delimiters do, stagingBytes and the passes,
 *  whole frames with verified checksums. One addition: nPatterns == 0 selects every record, plain `cut`; hPatterns and hPatternSizes
 *  may then be NULL, and word 7 of the stats, matches, is 0.
 *  Fields: inside a record as reported (for a record that lo cuts: from lo) field 1 starts at the record's start; every `separator`
 *  byte ends a field and starts the next; fields may be empty. Field j is chosen iff bit min(j, 64) - 1 of fieldMask is set. A
 *  content byte is kept iff its field is chosen; the separator in front of field k (k >= 2) is kept iff field k is chosen and some
 *  field j < k is. A selected record contributes its kept bytes in order and then one `delimiter` byte: the record that hi ends
 *  included, and a record that keeps nothing, which contributes the delimiter alone.
 *  Against `cut -d SEP -f LIST`: on every record that holds a separator the output is GNU cut's; on a record without one it is
 *  cut's as well when field 1 is chosen, and an empty line otherwise, where cut prints the record whole (and `cut -s` nothing).
 *  Result: *nRecords = the selected records; hRecords receives their {offset, size} in the content, exactly the extract's list (only
 *  on Success and when recordCapacity != 0); *dataSize = the packed size; dData (device memory) holds the packed text. The bytes of
 *  dData in [*dataSize, dataCapacity) are undefined after Success; no byte outside [dData, dData + dataCapacity) is ever written.
 *  Statuses, checked in this order:
 *   1. ZraHipExtractRecordsExpr's rule 1 (with nPatterns == 0 allowed); separator == delimiter; fieldMask == 0; INVERT with
 *      nPatterns == 0 -> {ZStdError, 42}. Nothing is decoded.
 *   2. dData overlaps the archive (through a handle: or the handle's arena) -> {ZStdError, 42}.
 *   3. to 6. ZraHipExtractRecordsExpr's: header, range (the empty range, and without INVERT a range shorter than the shortest
 *      pattern, are Success with 0 records, 0 bytes and nothing decoded), scratch (1,104 bytes per 8 KiB of window for the per-tile
 *      tables: the keep flags of every position lie there), a decoded frame that fails.
 *   7. OutputBufferTooSmall: ZraHipExtractRecords's rule 7, word for word: *nRecords and *dataSize then hold what the call needs,
 *      hRecords is not written. recordCapacity 0 and dataCapacity 0 make the sizing call, which launches no copy kernel.
 *  Zeroing of the outputs and the stats on every other status: ZraHipExtractRecords's rules.
 *  The call writes ZraHipGetExtractStats (word 5: *dataSize) and ZraHipDebugExtractMs as the extracts do. The grep's and the
 *  searches' stats are left alone.
 *  Cost: five launches per pass (count, one-workgroup scan, keep flags, one-workgroup placement, copy); DESIGN.md §33 and
 *  profiles/cut_scan.md say what was measured.
 *  Not covered: regex and predicate selection; `cut -s` and cut's whole-line rule for records without a separator; `--complement`
 *  (the caller inverts the mask); `--output-delimiter`; multi-byte separators; byte or character positions (`-b`, `-c`); shards; the
 *  host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipCutRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** ZraHipCutRecords through a ZraHipArchive handle: resident frames are staged from the cache as for ZraHipArchiveExtractRecords,
 *  the cache is not changed, dData must overlap neither the archive nor the handle's arena (rule 2), and the handle's scan counters
 *  (ZraHipArchiveGetScanStats) move as for ZraHipArchiveExtractRecords. */
ZRA_EXPORT ZraStatus ZraHipArchiveCutRecords(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);

/* ---- tally records: the distinct records of a packed text and their counts ----
 * `grep A | cut -d' ' -f9 | sort | uniq -c`. The calls above return records; the question a log archive is asked next is an aggregate:
 * how many lines per status code, per host, per user. The packed text of an extract or a cut lies in device memory when the call
 * returns; these calls group it there and hand back a few entries where the caller would copy the text to the host and count. */
/** the longest record that is a key; a longer one is skipped and counted in *nSkipped. It bounds every lane's loops over a record */
#define ZRA_HIP_TALLY_MAX_KEY 4096
/** ZraHipDebugTallyHashBits: keep no bit of the hash, every key starts probing at slot 0 */
#define ZRA_HIP_TALLY_HASH_NONE 0xFFFFFFFFu
/** one distinct key: where its first occurrence lies in the tallied text (without its delimiter), and how often it occurs */
typedef struct ZraHipTallyEntry {
  uint64_t offset;
  uint64_t size;
  uint64_t count;
} ZraHipTallyEntry;
/** The distinct records of textSize bytes at dText (device memory) and the count of each.
 *  Records: dText is cut at `delimiter`; bytes behind the last delimiter form one more record iff there are any; empty records count,
 *  with the empty key: the format ZraHipExtractRecords* and ZraHipCutRecords write.
 *  Keys: two records are the same key iff their bytes are equal; the comparison is of the bytes, never of a hash. A record longer than
 *  ZRA_HIP_TALLY_MAX_KEY is skipped: counted in *nSkipped, in no entry and in no count. *nRecords counts every record, skipped ones
 *  included.
 *  Result: *nDistinct = the distinct keys; hEntries[k], k < *nDistinct, is the k-th key in order of first appearance: offset and size
 *  of its first occurrence in dText without the delimiter, and the number of its occurrences; the counts sum to *nRecords - *nSkipped.
 *  dKeys (device memory) receives the keys in entry order, each followed by one `delimiter` byte, the text `awk '!seen[$0]++'` prints;
 *  *keySize = its size. hEntries and dKeys may each be NULL with capacity 0. The result is a function of the input alone, byte for
 *  byte, run after run. The bytes of dKeys in [*keySize, keyCapacity) are undefined after Success; no byte outside [dKeys, dKeys +
 *  keyCapacity) is ever written, and dText is only read.
 *  Statuses, checked in this order:
 *   1. engine or one of the four result words NULL; dText NULL with textSize != 0; hEntries NULL with entryCapacity != 0; dKeys NULL
 *      with keyCapacity != 0; [dKeys, dKeys + keyCapacity) overlaps the text; textSize >= 2^40 - 1 -> {ZStdError, 42}. Nothing is
 *      launched.
 *   2. textSize == 0 -> Success with four zeros.
 *   3. scratch that cannot be allocated -> {ZStdError, 64}. The call takes 16 bytes per 4 KiB tile, a quarter of the text's size for two
 *      bitmaps of its positions, and 24 bytes per table slot: the power of two at or above 1.5 * min(maxDistinct, *nRecords) + 64.
 *   4. more than maxDistinct distinct keys -> OutputBufferTooSmall; *nRecords and *nSkipped are set, *nDistinct = *nRecords -
 *      *nSkipped, a bound that is certain to suffice, *keySize = 0, and nothing is written to the buffers. maxDistinct == 0 makes no
 *      promise: the table is sized by the record count and this status cannot occur.
 *   5. *nDistinct > entryCapacity with entryCapacity != 0, or *keySize > keyCapacity with keyCapacity != 0 -> OutputBufferTooSmall
 *      with the four exact words; hEntries and dKeys are not written. Both capacities 0 make the sizing call, which is Success.
 *  On every status but Success and rules 4 and 5 the four words are zeroed.
 *  The call writes ZraHipGetTallyStats and ZraHipDebugTallyMs and no other call's stats.
 *  Cost: seven launches and two synchronisations (the record count sizes the table; the totals decide rules 4 and 5); DESIGN.md §34
 *  and profiles/tally_scan.md say what was measured.
 *  Not covered: the bytewise-sorted order and the top-k by count (the host derives both from the entries); regex and predicate
 *  selection in the composite; sums and extrema of numeric fields; a tally that streams pass by pass without a workspace; shards; the
 *  host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipTallyRecords(ZraHipEngine* engine, const void* dText, size_t textSize, uint8_t delimiter,
    uint64_t maxDistinct,
    ZraHipTallyEntry* hEntries, size_t entryCapacity,
    void* dKeys, size_t keyCapacity,
    uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize);
/** ZraHipCutRecords into a workspace, then ZraHipTallyRecords of it, on the engine's stream: `grep -F A | cut -d SEP -f LIST | sort |
 *  uniq -c` (in first-appearance order). The selection and field arguments are ZraHipCutRecords', word for word; a fieldMask of all
 *  ones tallies whole selected records. dWork (device memory, workCapacity bytes) receives the cut's packed text, *workSize its size,
 *  and the entries' offsets point into it. The tally's arguments and results are ZraHipTallyRecords'.
 *  Statuses: engine, workSize or a tally result word NULL, the tally's other rule-1 refusals (with dWork's capacity as the text), and
 *  dKeys overlapping the archive -> {ZStdError, 42}; then the cut's, in its order, with the five words zeroed as the cut zeroes its
 *  own; its rule 7 reads "*workSize says what dWork needs" (workCapacity 0 is that sizing call), the tally's words are then zero. After
 *  a successful cut the tally's rules 2 to 5 follow.
 *  The cut writes ZraHipGetExtractStats as it does on its own; the tally writes ZraHipGetTallyStats, zeroed when the cut fails. */
ZRA_EXPORT ZraStatus ZraHipTallyFields(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    void* dWork, size_t workCapacity, uint64_t* workSize,
    uint64_t maxDistinct,
    ZraHipTallyEntry* hEntries, size_t entryCapacity,
    void* dKeys, size_t keyCapacity,
    uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize);
/** ZraHipTallyFields through a ZraHipArchive handle: the cut is ZraHipArchiveCutRecords (resident frames staged from the cache, the
 *  cache not changed, the handle's scan counters moved); dWork and dKeys must overlap neither the archive nor the handle's arena. */
ZRA_EXPORT ZraStatus ZraHipArchiveTallyFields(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    void* dWork, size_t workCapacity, uint64_t* workSize,
    uint64_t maxDistinct,
    ZraHipTallyEntry* hEntries, size_t entryCapacity,
    void* dKeys, size_t keyCapacity,
    uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize);
/** the last tally of this engine: {records, distinct keys, skipped records, key bytes, table slots, longest probe (the most slots one insert
 *  looked at, its own included), inserts into the table in device memory (the rest were combined in LDS), 0}; all zero unless it
 *  succeeded. Words 5 and 6 depend on the order in which lanes arrive, nothing else does. */
ZRA_EXPORT void ZraHipGetTallyStats(ZraHipEngine* engine, uint64_t* out8);
/** bring-up: HIP-event milliseconds of the last tally's own launches */
ZRA_EXPORT double ZraHipDebugTallyMs(ZraHipEngine* engine);
/** bring-up, for tests: the next tallies of this engine keep only the low `bits` (1 .. 63) of the key hash; 0 restores the full hash;
 *  ZRA_HIP_TALLY_HASH_NONE keeps no bit. With 0 to 2 bits kept every key starts probing at one of at most four slots, so that claim
 *  races, byte-compare mismatches, long probe chains and the wrap at the table's end happen at a few hundred keys. Results do not
 *  change, only the time. Any other value is ignored. */
ZRA_EXPORT void ZraHipDebugTallyHashBits(ZraHipEngine* engine, uint32_t bits);

/* ---- grep with context records: the records in front of and behind each selected one ----
 * `grep -A`, `-B`, `-C`. A log search wants the lines around a hit; with the calls above a caller decodes the neighbourhood of every
 * hit a second time and cuts it at delimiters on the host. The grep pass sees every delimiter and every selection in order: this call
 * keeps a summary that counts in records as well as in hits. */
#define ZRA_HIP_GREP_MAX_CONTEXT   64u             /* records before, and records after: the width of a wave */
#define ZRA_HIP_CONTEXT_SELECTED   (1ull << 63)    /* in ZraHipContentRange.size: the record itself is selected */

/** ZraHipGrepArchiveExpr with `before` records in front of and `after` records behind every selected record. The patterns with their
 *  `syntax` word (0, ZRA_HIP_PATTERN_FOLD_CASE, ZRA_HIP_PATTERN_CLASSES) and `delimiter`, `mode` (ZRA_HIP_GREP_INVERT only), the
 *  range with its inclusive bound and size = UINT64_MAX, stagingBytes, the passes and ownership, "only the frames of the range" (whole
 *  frames with verified checksums), host synchrony and the definition of the records of [lo, hi) are that call's, word for word.
 *  Meaning. R_0 .. R_(n-1) are the records of [lo, hi), S the set of indices ZraHipGrepArchiveExpr selects (INVERT applied). The
 *  output set is O = { k : some j in S has j - before <= k <= j + after }. Context never reaches outside the range: lo and hi end
 *  the world as the file's ends do for grep. A group is a maximal run of consecutive indices in O: what grep separates by `--`.
 *  Result. *nRecords = |O| (it may exceed the capacity); *nSelected = |S| and *nGroups = the number of groups (either pointer may be
 *  NULL). The first min(|O|, recordCapacity) records of O go to hRecords, ascending, each once, as {offset, size} with
 *  ZRA_HIP_CONTEXT_SELECTED set in size iff the record is in S (content sizes are 40-bit). Nothing is written behind them, and
 *  nothing reaches the host before the last pass. recordCapacity 0 with hRecords NULL is the counting call. On any status but
 *  Success hRecords is untouched, the three counts are 0 and the stats are zero. before == after == 0 is ZraHipGrepArchiveExpr's
 *  list with the bit set in every entry. Every group is one contiguous content range (its first record's offset to its last
 *  record's end), so ZraHipDecompressRABatch over the groups fetches the bytes.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchiveExpr's rule 1, then before or after above ZRA_HIP_GREP_MAX_CONTEXT -> {ZStdError, 42}.
 *   2. to 5. Rules 2 to 5 of that call, both shortcuts included (the empty range, and without INVERT a range shorter than the
 *      shortest pattern: Success, 0 records, nothing decoded, stats {frames, 0, ...}). Scratch is the grep's with 48 bytes per
 *      8 KiB of window for the per-tile tables in the place of 32, and 16 * before bytes behind the list for the ranges that
 *      wait for a later pass to select a record.
 *  Stats: the call writes ZraHipGetGrepStats {frames, decoded, content bytes, records of the range, |O|, listed, passes, matches as
 *  the grep counts them} and ZraHipDebugGrepScanMs.
 *  Cost: profiles/grep_context.md.
 *  Not covered: context with ZraHipGrepArchiveWhere and with the two extracts (with regular expressions:
 *  ZraHipGrepArchiveRegexContext, below); the packed bytes (see
 *  above); more than ZRA_HIP_GREP_MAX_CONTEXT records of context; shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipGrepArchiveContext(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    uint64_t* nSelected, uint64_t* nGroups);
/** ZraHipGrepArchiveContext through a ZraHipArchive handle: resident frames are staged from the cache as for ZraHipArchiveGrepExpr,
 *  the cache is not changed, and the handle's scan counters (ZraHipArchiveGetScanStats) move as for that call. */
ZRA_EXPORT ZraStatus ZraHipArchiveGrepContext(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    uint64_t* nSelected, uint64_t* nGroups);

/* ---- grep with regular expressions: quantifiers, alternation and anchors ----
 * The calls above take patterns of fixed length, tested per position. A regular expression is a state machine over the bytes of a
 * record: this call compiles the expressions into one deterministic automaton on the host and carries its STATE through the scan
 * where the grep carries one bit. The expressions use the characters that the pattern expressions reserved; no expression accepted
 * by the ...Expr calls changes its meaning there, and those calls go on refusing every syntax bit but their two. */
#define ZRA_HIP_REGEX_MAX_STATES     64u    /* states of the minimal automaton of a call */
#define ZRA_HIP_REGEX_MAX_POSITIONS  4096u  /* atoms of all expressions after counted repetitions are expanded */

typedef struct ZraHipRegexInfo { uint32_t states, classes, positions, why, pattern; } ZraHipRegexInfo;

/** Rule 1 of ZraHipGrepArchiveRegex as far as the expressions go, on the host alone: no engine, no device. hPatterns /
 *  hPatternSizes / nPatterns: 1 .. ZRA_HIP_SEARCH_MAX_PATTERNS expressions laid end to end, each of 1 byte or more,
 *  ZRA_HIP_PATTERN_MAX_EXPR_BYTES in all (the sizes are summed in 64 bits before a byte is read); they are alternatives, as with
 *  `grep -e A -e B`. syntax: 0 or ZRA_HIP_PATTERN_FOLD_CASE. delimiter: 0 .. 255. Success, or {ZStdError, 42}; `info` (may be NULL)
 *  is filled on both outcomes: why = 0 accepted, 1 arguments or a size limit, 2 syntax, 3 an atom whose set is empty once the
 *  delimiter is removed, 4 more than ZRA_HIP_REGEX_MAX_STATES states or the construction bound; pattern = the index of the refused
 *  expression for reasons 2 and 3, else 0; states, classes and positions are valid on Success and 0 otherwise.
 *
 *  Grammar: POSIX ERE over bytes.
 *   atoms        ZraHipCheckPatternExpr's elements, unchanged: a literal byte, . [items] [^items] \xHH \n \t \r \d \w \s, and \c for
 *                c one of . [ ] \ * + ? { } ( ) | ^ $ -. FOLD_CASE closes an atom's set under the ASCII case swap before a ^
 *                complements it. [: stays refused (POSIX classes are reserved).
 *   delimiter    removed silently from EVERY atom (a record never holds it, so no answer changes; `\s+` and `[ \n]` can be written
 *                with the newline as delimiter). Only an atom whose set is then empty is refused (reason 3): the literal delimiter,
 *                `[\n]`. ZRA_HIP_PATTERN_MAX_SETS does not apply.
 *   x* x+ x?     x{n} x{n,} x{n,m}, 0 <= n <= m <= 255, behind an atom or a group. {0} and {0,0} are legal; {,m} is refused.
 *   ( )          groups; nothing is captured.      |   alternation.      ^ $   anchors, anywhere.
 *  Refused (reason 2): a quantifier with nothing in front of it (at the start, behind ( or |), directly behind a quantifier (`*?`
 *  `+?` `*+` stay reserved) or on an anchor; an empty group; an empty branch (`a|`, `|a`, `(a|)`); unbalanced ( or ); a { that does
 *  not begin a valid bound; an unescaped ] or } outside a set or a bound; everything ZraHipCheckPatternExpr refuses in an atom.
 *  Reason 1: more than 64 expressions, an expression of 0 bytes, more than ZRA_HIP_PATTERN_MAX_EXPR_BYTES bytes, more than
 *  ZRA_HIP_REGEX_MAX_POSITIONS positions. A position is an atom or an anchor; x* x+ x? count as x, x{n,m} as m times x, x{n,} as
 *  max(n, 1) times x. Syntax is checked for every expression before the positions are counted.
 *  Meaning. BOL and EOL are two symbols that no atom admits; ^ reads BOL and $ reads EOL. With S = any byte but the delimiter, BOL
 *  or EOL, a record r is matched iff BOL r EOL is in S* (e_1 | ... | e_K) S*. So ^ holds at the start of a record and $ at its end,
 *  `^$` and `a*` match the empty record, and an expression that can match nothing (`a^b`, `^^a`) is legal and selects nothing.
 *  states = the states of the minimal complete DFA over the non-delimiter bytes for the set of matched records, restricted to the
 *  states reachable from its start (the dead state included if reachable): a defined number. classes = the classes of non-delimiter
 *  bytes with identical columns in it. The subset construction stops at 4,096 distinct position sets (reason 4), which bounds the
 *  host's time on `(a|b)*a(a|b){12}`; the limit of 64 states is the width of a wave: a state map is one lane per state and 64 bytes
 *  in the per-tile tables. */
ZRA_EXPORT ZraStatus ZraHipCheckRegex(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
    uint32_t syntax, int delimiter, ZraHipRegexInfo* info);

/** The records of a content range that a regular expression matches. The records and the range [lo, hi) with its inclusive bound and
 *  size = UINT64_MAX, stagingBytes, the passes, whole frames with verified checksums, "only the frames of the range", `mode`
 *  (ZRA_HIP_GREP_INVERT only), capacity 0 as `grep -c`, *nRecords above the capacity, "nothing reaches the host before the last
 *  pass" and the zeroing of outputs and stats on every status but Success: ZraHipGrepArchive's, word for word.
 *  Selection. A record is selected iff the expression matches somewhere inside the record's bytes (ZraHipCheckRegex, Meaning); with
 *  INVERT iff it does not. lo and hi cut records the way delimiters do: ^ holds at the start of a record as reported and $ at its
 *  end as reported, so a clipped record is anchored at the clip.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchive's rule 1 with its pointer and capacity checks; `syntax` with any bit other than ZRA_HIP_PATTERN_FOLD_CASE
 *      and every refusal of ZraHipCheckRegex -> {ZStdError, 42}. Nothing is decoded.
 *   2. Header problems: ZraHipGrepArchive's rule 2.
 *   3. The range: ZraHipGrepArchive's rule 3. The empty range is Success with 0 records, nothing decoded and stats {frames, 0, ...}.
 *      There is no "shorter than the shortest pattern" shortcut: every non-empty range is scanned.
 *   4. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the grep's with 112 bytes per 8 KiB of window for the
 *      per-tile tables: a summary, a head and a 64-byte state map.
 *   5. A decoded frame that fails: ZraHipGrepArchive's rule 5.
 *  The call writes ZraHipGetGrepStats and ZraHipDebugGrepScanMs as ZraHipGrepArchiveWhere does. Word 7, matches, is the number of
 *  records of the range that the expression matches, before INVERT: with INVERT, selected = records - matches.
 *  Cost: one dependent table step per byte. A record inside a tile is one lane's walk; the bytes in front of a tile's first
 *  delimiter are stepped for all 64 states at once by one wave. Content without delimiters makes every tile one such head: 8,192
 *  dependent steps per tile on one wave. The cost does not depend on the expression, only on the bytes and on how the delimiters
 *  fall.
 *  Not covered: match offsets, leftmost-longest spans, captures; ZraHipGrepArchiveWhere with regular expressions (the selected
 *  records' bytes: ZraHipExtractRecordsRegex, below); more than ZRA_HIP_REGEX_MAX_STATES states; backreferences, lazy or possessive quantifiers, look-around, word
 *  boundaries, POSIX classes, UTF-8 awareness; multi-byte delimiters, shards, the host-pointer API. (Context lines:
 *  ZraHipGrepArchiveRegexContext, below.) */
ZRA_EXPORT ZraStatus ZraHipGrepArchiveRegex(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);
/** ZraHipGrepArchiveRegex through a ZraHipArchive handle: resident frames are staged from the cache as for ZraHipArchiveGrep, the
 *  cache is not changed, and the handle's scan counters (ZraHipArchiveGetScanStats) move as for ZraHipArchiveGrepWhere. */
ZRA_EXPORT ZraStatus ZraHipArchiveGrepRegex(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords);

/** The records ZraHipGrepArchiveRegex selects WITH their bytes, packed: the text `grep -E` (with INVERT: `grep -E -v`) prints, from
 *  the one decode pass that selects the records. The meaning is the composition of two contracts, word for word.
 *  Selection: ZraHipGrepArchiveRegex's. 1 .. 64 expressions are alternatives, `syntax` is 0 or ZRA_HIP_PATTERN_FOLD_CASE, lo and hi
 *  cut records the way delimiters do (^ and $ hold at a clip), `mode` is ZRA_HIP_GREP_INVERT only, and every non-empty range is
 *  scanned.
 *  Result: ZraHipExtractRecords's. *nRecords = the selected records; *dataSize = the sum of (n_i + 1) over them; dData (device
 *  memory) receives each selected record's bytes followed by one `delimiter` byte, in ascending order, the last record, which hi
 *  ends, included. The list goes to hRecords once, after the last pass, and only when recordCapacity != 0. The bytes of dData in
 *  [*dataSize, dataCapacity) are undefined after Success (a record open at the end of a pass is copied before its selection is
 *  known); no byte outside [dData, dData + dataCapacity) is ever written, whatever the outcome.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchiveRegex's rule 1 (every refusal of ZraHipCheckRegex, every foreign `syntax` bit); dataSize NULL; hRecords
 *      NULL with recordCapacity != 0; dData NULL with dataCapacity != 0 -> {ZStdError, 42}. Nothing is decoded.
 *   2. dData overlaps the archive (through a handle: or the handle's arena) -> {ZStdError, 42}.
 *   3. Header problems: ZraHipGrepArchive's rule 2.
 *   4. The range: ZraHipGrepArchive's rule 3. The empty range is Success with 0 records and 0 bytes, nothing decoded and stats
 *      {frames, 0, ...}.
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the regex grep's with 128 bytes per 8 KiB of window.
 *   6. A decoded frame that fails: ZraHipGrepArchive's rule 5.
 *   7. OutputBufferTooSmall: ZraHipExtractRecords's rule 7, word for word: *nRecords and *dataSize then hold what the call needs,
 *      hRecords is not written. recordCapacity 0 and dataCapacity 0 make the sizing call, which launches no copy kernel.
 *  Zeroing of the outputs and the stats on every other status: ZraHipExtractRecords's rules.
 *  The call writes ZraHipGetExtractStats and ZraHipDebugExtractMs as ZraHipExtractRecordsExpr does; word 7, matches, is
 *  ZraHipGrepArchiveRegex's: the records of the range that the expression matches, before INVERT. The grep's and the searches' stats
 *  are left alone.
 *  Cost: ZraHipGrepArchiveRegex's, plus a second walk of the tiles that hold a copied byte: measured on 1 GiB of log lines, the
 *  call's launches take 1.10 to 1.63 times the regex grep's scan, and the call 0.68 to 0.78 of the wall time of the regex grep
 *  followed by a ZraHipDecompressRABatch of the listed ranges (profiles/extract_regex.md).
 *  Not covered: ZraHipGrepArchiveWhere with regular expressions; match offsets, spans, captures; more than
 *  ZRA_HIP_REGEX_MAX_STATES states; context lines, output without delimiter bytes; multi-byte delimiters, shards, the host-pointer
 *  API. */
ZRA_EXPORT ZraStatus ZraHipExtractRecordsRegex(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);
/** ZraHipExtractRecordsRegex through a ZraHipArchive handle: resident frames are staged from the cache as for
 *  ZraHipArchiveExtractRecords, the cache is not changed, dData must overlap neither the archive nor the handle's arena (rule 2),
 *  and the handle's scan counters (ZraHipArchiveGetScanStats) move as for ZraHipArchiveExtractRecords. */
ZRA_EXPORT ZraStatus ZraHipArchiveExtractRecordsRegex(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    void* dData, size_t dataCapacity, uint64_t* dataSize);

/** The records ZraHipGrepArchiveRegex selects with `before` records in front of and `after` records behind each of them: what
 *  `grep -E -A after -B before` prints, `--` lines counted, from one decode pass. The meaning is the composition of two contracts.
 *  Selection: ZraHipGrepArchiveRegex's. 1 .. 64 expressions are alternatives, `syntax` is 0 or ZRA_HIP_PATTERN_FOLD_CASE, every
 *  refusal of ZraHipCheckRegex applies, `mode` is ZRA_HIP_GREP_INVERT only, lo and hi cut records the way delimiters do (^ and $
 *  hold at a clip), and every non-empty range is scanned: there is no "shorter than the shortest pattern" shortcut.
 *  Result: ZraHipGrepArchiveContext's, with S the set of indices ZraHipGrepArchiveRegex selects (INVERT applied). O, the groups,
 *  *nRecords = |O| (it may exceed the capacity), *nSelected = |S| and *nGroups (either pointer may be NULL); the first
 *  min(|O|, recordCapacity) records of O in hRecords, ascending, ZRA_HIP_CONTEXT_SELECTED set in the size of the records of S.
 *  Context never leaves [lo, hi). recordCapacity 0 with hRecords NULL is the counting call. Nothing is written behind the list,
 *  nothing reaches the host before the last pass, and on every status but Success hRecords is untouched, the three counts are 0 and
 *  the stats are zero. before == after == 0 gives ZraHipGrepArchiveRegex's list with the bit set in every entry.
 *  Statuses, checked in this order:
 *   1. ZraHipGrepArchiveRegex's rule 1, then before or after above ZRA_HIP_GREP_MAX_CONTEXT -> {ZStdError, 42}.
 *   2. to 5. Rules 2 to 5 of ZraHipGrepArchiveRegex. Scratch is the grep's with 128 bytes per 8 KiB of window for the per-tile
 *      tables (a 16-byte summary, a 48-byte head and a 64-byte state map), and 16 * before bytes behind the list for the ranges that
 *      wait for a later pass to select a record.
 *  Stats: the call writes ZraHipGetGrepStats {frames, decoded, content bytes, records of the range, |O|, listed, passes, matches} and
 *  ZraHipDebugGrepScanMs; matches is ZraHipGrepArchiveRegex's: the records of the range that the expression matches, before INVERT.
 *  Cost: ZraHipGrepArchiveRegex's dependent walk per byte, unchanged; the context adds a reduction of the selection bits per tile, a
 *  walk backwards in the one-workgroup scan and a second walk of the tiles that hold a listed record. Measured on 1 GiB of log lines
 *  with a capacity of 2^20, the call's launches take 0.86 to 1.20 times the regex grep's scan: 1.08 to 1.20 at 0.1 % selected with 0
 *  to 64 records each way, 1.09 down to 0.86 at 17.7 % (wider context reaches the capacity in fewer tiles), 1.09 with every record
 *  selected (profiles/grep_regex_context.md).
 *  Not covered: context with ZraHipGrepArchiveWhere and with the two extracts; match spans; more than ZRA_HIP_GREP_MAX_CONTEXT
 *  records of context; shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipGrepArchiveRegexContext(ZraHipEngine* engine, const void* dArchive, size_t archiveSize,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    uint64_t* nSelected, uint64_t* nGroups);
/** ZraHipGrepArchiveRegexContext through a ZraHipArchive handle: resident frames are staged from the cache as for
 *  ZraHipArchiveGrepRegex, the cache is not changed, and the handle's scan counters (ZraHipArchiveGetScanStats) move as for that call. */
ZRA_EXPORT ZraStatus ZraHipArchiveGrepRegexContext(ZraHipArchive* archive,
    const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
    uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after,
    uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords,
    uint64_t* nSelected, uint64_t* nGroups);

/* ---- compare: where the contents of two device-resident archives differ, without an output buffer for either ----
 * The `cmp` of the family. After an update there are two archives side by side, and a replica, or a checker, wants the changed byte
 * ranges; the same content written at two levels raises the same question. A caller would have to ZraHipDecompressBuffer both contents
 * into two buffers and compare them with code of their own. This call uses what the container has and a plain zstd stream lacks,
 * independent frames: identical compressed bytes of a frame mean identical content, decided at the bandwidth of the compressed data. */
#define ZRA_HIP_COMPARE_DECODE_ALL 1u   /* no compressed-bytes shortcut: every frame of the range is decoded on both sides */

/* ZraHipContentRange {offset, size}: declared above, with ZraHipGrepArchive, which lists records in the same shape. */

/** Compares the content of the archive at dA (sizeA bytes, device memory) with that of the archive at dB (sizeB bytes, device memory)
 *  inside the content range [offset, offset + size); size = UINT64_MAX: to C = min(UA, UB), the end of the shorter content.
 *  Synchronous; stream ordering as the other compute calls (ZraHipWaitStream). Both archives are only read.
 *  Result, with [lo, hi) = the range:
 *  - A differing range is a MAXIMAL run [s, e) inside [lo, hi) with A[p] != B[p] for every p in it: a run that continues from one frame
 *    into the next, or from one pass into the next, is one range; a run that the range cuts is reported clipped.
 *  - *nRanges = the number of differing ranges; it may exceed rangeCapacity. The first min(*nRanges, rangeCapacity) ranges are written
 *    to hRanges (a HOST array) in ascending order, each exactly once; nothing is written behind them. hRanges may be NULL when
 *    rangeCapacity is 0: a count-only compare.
 *  - *differingBytes = the sum of the sizes of all ranges, listed or not. differingBytes may be NULL.
 *  - Content behind C, where the archives have different lengths, is not a range: UA and UB are in ZraHipGetCompareSizes, and the
 *    caller compares them.
 *  - On any status other than Success nothing is written to hRanges, *nRanges and *differingBytes are 0 and all stats are zero. No
 *    range reaches the host before the last pass is done.
 *  Statuses, checked in this order:
 *   1. engine or nRanges NULL; dA or dB NULL with a size other than 0; hRanges NULL with rangeCapacity != 0; mode with bits other than
 *      ZRA_HIP_COMPARE_DECODE_ALL -> {ZStdError, 42}.
 *   2. Header problems of A, then of B: the statuses of ZraHipArchiveOpen (a frame size of 0 on either side: HeaderInvalid). The stored
 *      header CRC-32 is NOT checked here: that is ZraHipVerifyArchive's job.
 *   3. Different frame sizes -> {ZStdError, 40} (parameter_unsupported).
 *   4. offset > C, or size != UINT64_MAX and offset + size > C (or a sum that overflows) -> OutOfBoundsAccess. The bound is inclusive,
 *      as the search's rule 3. The empty range is Success with 0 ranges, and nothing is read.
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's (ZraHipReleaseScratch returns it): the staging
 *      window, 1 byte per slot of a pass, the decoder's job arrays for two archives, 16 bytes per 8 KiB tile of the decoded frames of
 *      a pass, 16 bytes per listed range, the decoder's own scratch for one pass.
 *   6. A frame that has to be decoded and fails: the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query
 *      inside that frame; of several failing frames the one with the lowest index, A before B at the same index (passes run in frame
 *      order and the call stops behind the first pass with a failing frame).
 *  THE SHORTCUT, and what it does not promise. Without ZRA_HIP_COMPARE_DECODE_ALL a frame of the range is EQUAL without being decoded
 *  when its two seek-table spans are well formed (the decoder's convention: a <= b <= body size), equally long and hold the same
 *  bytes. Anything else is decoded on both sides, whole, checksums verified: an odd span, another length, one differing byte; the
 *  decoder's own refusal is then the status. Identical damaged frames are therefore equal and go unnoticed, exactly as the update
 *  carries them over: COMPARE IS NOT VERIFY (ZraHipVerifyArchive is). On archives whose frames all decode, both modes give the same
 *  ranges.
 *  The frames are taken in passes of max(1, min(65,536, stagingBytes / (2 * frameSize))) consecutive frames (stagingBytes 0: 4 GiB in
 *  all): the staging window holds one half per archive. Frames outside the range are not touched.
 *  Cost: every compressed byte of the range is read once (less for a frame that differs early); a frame pair that is decoded is read
 *  once more as plaintext, twice when it holds a listed range boundary.
 *  Not covered: archives of different frame sizes beyond the refusal, a variant on ZraHipArchive handles that uses resident frames,
 *  the shards of a distributed archive (ZraHipShard), the host-pointer API. (The patch that ZraHipUpdateArchive applies:
 *  ZraHipDiffArchives below.) */
ZRA_EXPORT ZraStatus ZraHipCompareArchives(ZraHipEngine* engine,
    const void* dA, size_t sizeA, const void* dB, size_t sizeB,
    uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes,
    ZraHipContentRange* hRanges, size_t rangeCapacity, uint64_t* nRanges, uint64_t* differingBytes);
/** The last ZraHipCompareArchives on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames of the range, frames equal by their compressed bytes, frame pairs decoded, content bytes of the range compared
 *  after a decode, ranges, ranges listed, passes, 0}. Counters, not timings. */
ZRA_EXPORT void ZraHipGetCompareStats(ZraHipEngine* engine, uint64_t* out8);
/** The content sizes of the last ZraHipCompareArchives on the engine: out2 = {UA, UB}, set on every Success, the empty range included
 *  (whose stats are all zero); {0, 0} after any other outcome. engine NULL: {0, 0}; out2 NULL: no-op. */
ZRA_EXPORT void ZraHipGetCompareSizes(ZraHipEngine* engine, uint64_t* out2);
/** Bring-up aid, like ZraHipDebugSearchScanMs: HIP-event time of the last compare's own launches (span compare, job build, count,
 *  prefix scan, fill), summed over its passes; the decode of the same call is in ZraHipGetKernelStats. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugCompareMs(ZraHipEngine* engine);

/* ---- diff: the patch that turns one device-resident archive's content into another's, in the shape ZraHipUpdateArchive takes ----
 * The compare says where two archives differ; a replica needs the bytes as well. The compare has the plaintext of every differing
 * frame pair in its staging window when it finds the ranges: this call keeps B's side of it. One pass over A and B yields the writes
 * and the packed bytes, without a buffer for either content. */
#define ZRA_HIP_DIFF_DECODE_ALL 1u      /* as ZRA_HIP_COMPARE_DECODE_ALL: every frame of [0, C) is decoded on both sides */
#define ZRA_HIP_DIFF_MAX_GRAIN  8192u

/** The writes and the append that give the archive at dA (sizeA bytes, device memory) the content of the archive at dB (sizeB bytes,
 *  device memory). UA and UB are the content sizes, C = min(UA, UB), fs the common frame size. Synchronous; stream ordering as the
 *  other compute calls (ZraHipWaitStream). Both archives are only read.
 *  GRAINS. grain is a power of two from 1 to ZRA_HIP_DIFF_MAX_GRAIN. Frame f is cut into grains of `grain` bytes counted from the
 *  frame's own first byte, so a grain never straddles a frame. A grain is clipped to its frame and to C: the last grain of a frame
 *  may be short. A grain is DIRTY if A and B differ at one or more of its positions.
 *  WRITES. A write is a maximal run of dirty grains that follow each other in content order; the last grain of frame f and the first
 *  grain of frame f + 1 are neighbours, so a run that continues across frames, or across passes, is one write. Its offset and size are
 *  the union of its clipped grains. With grain = 1 the writes are exactly the ranges ZraHipCompareArchives gives for [0, C). A larger
 *  grain trades a few equal bytes in dData for fewer writes (a write costs 24 bytes of host arrays and a tuple in the update;
 *  rewriting an equal byte is harmless).
 *  - *nWrites = the number of writes. hOffsets[i], hSizes[i] (HOST arrays of writeCapacity entries) describe write i, ascending; no
 *    two writes share or touch a byte, so rule 4 of ZraHipUpdateArchive is met.
 *  - dData (device memory, dataCapacity bytes) receives B's bytes of all dirty grains, in content order, packed: hDataOffsets[i] is
 *    the sum of the sizes of the writes in front of write i.
 *  - TAIL. When UB > UA, B's bytes [UA, UB) follow the dirty bytes in dData: *appendOffset is their offset in dData and *appendSize =
 *    UB - UA. When UB == UA, *appendSize = 0 and *appendOffset is the number of dirty bytes.
 *  - *dataSize = dirty bytes + *appendSize.
 *  ZraHipUpdateArchive(engine, dA, sizeA, dData, hOffsets, hSizes, hDataOffsets, *nWrites, (char*)dData + *appendOffset, *appendSize,
 *  ...) then yields an archive with B's content; at the level and checksum flag B was written with, B's bytes.
 *  Statuses, checked in this order:
 *   1. engine, nWrites, dataSize, appendOffset or appendSize NULL; dA or dB NULL with a size other than 0; one of the three host
 *      arrays NULL with writeCapacity != 0; dData NULL with dataCapacity != 0; mode with bits other than ZRA_HIP_DIFF_DECODE_ALL;
 *      grain not a power of two in 1 .. 8192 -> {ZStdError, 42}.
 *   2. [dData, dData + dataCapacity) overlaps either archive -> {ZStdError, 42}.
 *   3. Header problems of A, then of B, as rule 2 of ZraHipCompareArchives.
 *   4. Different frame sizes -> {ZStdError, 40}.
 *   5. UB < UA -> {ZStdError, 40}: an update cannot shorten content, so no patch exists.
 *   6. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's (ZraHipReleaseScratch returns it): the staging
 *      window, 1 byte per slot of a pass, the decoder's job arrays for two archives, 24 bytes per 8 KiB tile of the decoded frames of
 *      a pass, 16 bytes per write up to writeCapacity, the decoder's own scratch for one pass.
 *   7. A frame that has to be decoded and fails, as rule 6 of ZraHipCompareArchives. The tail frames of B come behind all pair passes.
 *   8. *nWrites > writeCapacity or *dataSize > dataCapacity -> OutputBufferTooSmall. The four output words hold what the patch needs:
 *      this is the one outcome other than Success that sets them. A call with capacities 0 / 0 is the sizing call.
 *  On every status other than Success nothing is written to the three host arrays and the stats are zero; apart from rule 8 the
 *  output words are 0. dData is written while the passes run: after a status other than Success its first dataCapacity bytes are
 *  undefined. No byte at or behind dData + dataCapacity is ever written, whatever the outcome. As in the compare, no list entry
 *  reaches the host before the last pass is done.
 *  THE SHORTCUT is the compare's, word for word: a frame with equal compressed spans is clean and is not decoded, so DIFF IS NOT
 *  VERIFY. With ZRA_HIP_DIFF_DECODE_ALL every frame of [0, C) is decoded on both sides. Identical archives give Success with 0 writes,
 *  *dataSize 0 and no decode launch.
 *  Passes: the frames of [0, C) in passes of max(1, min(65,536, stagingBytes / (2 * frameSize))) frame pairs, as the compare; then
 *  B's frames from the one that holds C on, in passes of max(1, min(65,536, stagingBytes / frameSize)) (stagingBytes 0: 4 GiB). When
 *  UA lies inside a frame, that frame of B is decoded in both.
 *  Not covered: a content sub-range, shrinking (UB < UA), a variant on ZraHipArchive handles, the shards of a distributed archive, the
 *  host-pointer API, a gap-merging rule other than grains. */
ZRA_EXPORT ZraStatus ZraHipDiffArchives(ZraHipEngine* engine,
    const void* dA, size_t sizeA, const void* dB, size_t sizeB,
    uint32_t mode, uint32_t grain, size_t stagingBytes,
    uint64_t* hOffsets, uint64_t* hSizes, uint64_t* hDataOffsets, size_t writeCapacity, uint64_t* nWrites,
    void* dData, size_t dataCapacity, uint64_t* dataSize,
    uint64_t* appendOffset, uint64_t* appendSize);
/** The last ZraHipDiffArchives on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames of [0, C), frames equal by their compressed bytes, frame pairs decoded, tail frames of B decoded, writes, dirty
 *  bytes, passes (pair + tail), dirty grains}. A diff does not touch ZraHipGetCompareStats, and the other way round. */
ZRA_EXPORT void ZraHipGetDiffStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugCompareMs: HIP-event time of the last diff's own launches (span compare, job build, count, prefix
 *  scan, fill with the gather copy, tail jobs and tail copy), summed over its passes; its decodes are in ZraHipGetKernelStats.
 *  engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugDiffMs(ZraHipEngine* engine);

/* ---- content signatures: diff a device-resident archive against a replica that lies elsewhere ----
 * ZraHipDiffArchives needs both archives in one device's memory. A replica on another GPU or host sends a SIGNATURE of its content
 * instead: a few 64-bit words per frame. The side that holds the new archive diffs against the signature and ships the patch.
 * Updates overwrite in place and append (no insertions), so hashes of aligned grains are enough: no rolling hash.
 * THE SIGNATURE. With fs the frame size, grain a power of two from ZRA_HIP_SIGN_MIN_GRAIN to ZRA_HIP_SIGN_MAX_GRAIN and gpf =
 * ceil(fs / grain), the signature of an archive of F frames is F records of 1 + gpf 64-bit words in device memory, record f at word
 * f * (1 + gpf):
 *  - word 0, the frame word: XXH64 with `seed` of the frame's compressed bytes, its seek-table span [a, b) of the body;
 *  - word 1 + g, a grain word: XXH64 with `seed` of grain g of frame f, grains cut as ZraHipDiffArchives cuts them (`grain` bytes
 *    counted from the frame's own first byte, clipped to the frame and to the content size). The grain words of a short last frame
 *    that have no byte are 0.
 * The record stride depends on fs and grain only: when an update appends frames the old records keep their places and new ones
 * follow; the old last frame, grown by the append, is signed again inside its own record. What describes a signature stays on the
 * host (ZraHipSignature, 40 bytes) and travels with the words. */
#define ZRA_HIP_SIGN_MIN_GRAIN 64u
#define ZRA_HIP_SIGN_MAX_GRAIN 8192u
#define ZRA_HIP_SIGDIFF_DECODE_ALL 1u   /* every frame of [0, C) is decoded and its grains hashed, whatever its frame word says */
typedef struct ZraHipSignature { uint64_t contentSize; uint32_t frameSize; uint32_t grain; uint64_t seed; uint64_t frames; uint64_t words; } ZraHipSignature;

/** Signs frames [firstFrame, firstFrame + frameCount) (frameCount UINT64_MAX: to the last frame; ZraHipVerifyArchive's range) of
 *  the archive at dArchive (device memory): their words go into their records of dSig (device memory, sigCapacityWords words).
 *  *info always describes the WHOLE archive (words = frames * (1 + gpf)) and sigCapacityWords is always measured against info->words:
 *  a caller who has just updated signs the touched frames into the signature it already holds. Synchronous; the archive is only
 *  read; stream ordering as the other compute calls (ZraHipWaitStream).
 *  Statuses, checked in this order:
 *   1. engine or info NULL; dArchive NULL with a size other than 0; dSig NULL with sigCapacityWords != 0; grain not a power of two
 *      in 64 .. 8192 -> {ZStdError, 42}.
 *   2. [dSig, dSig + 8 * sigCapacityWords) overlaps the archive -> {ZStdError, 42}.
 *   3. Header problems -> the statuses of ZraHipArchiveOpen; a frame size of 0 -> HeaderInvalid. The header's CRC-32 is not checked.
 *   4. firstFrame > frames, or frameCount != UINT64_MAX and frameCount > frames - firstFrame -> OutOfBoundsAccess. The empty range is
 *      Success.
 *   5. sigCapacityWords < info->words -> OutputBufferTooSmall with *info filled: the sizing call, pure header arithmetic. Nothing is
 *      decoded and nothing is written to dSig.
 *   6. Scratch that cannot be allocated -> {ZStdError, 64}. Scratch is the engine's (ZraHipReleaseScratch returns it): the staging
 *      window, the decoder's job arrays and the decoder's own scratch for one pass.
 *   7. A frame that fails to decode -> the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside
 *      it; of several failing frames the one with the lowest index (passes run in frame order and the call stops behind the first pass
 *      with a failing frame).
 *  *info is set on Success and on OutputBufferTooSmall; on every other status it is zeroed and the stats are zero. After rule 7 the
 *  words of the range's records are undefined. No word outside the records of the range, and none at or behind sigCapacityWords, is
 *  ever written, whatever the outcome.
 *  Passes: max(1, min(65,536, stagingBytes / frameSize)) frames each (stagingBytes 0: 4 GiB). Every frame of the range is decoded
 *  whole with its checksum verified: A SIGNATURE NEVER DESCRIBES CONTENT THAT DOES NOT DECODE. The frame word of a frame whose span is
 *  not well formed (the decoder's convention: a <= b <= body size) is never computed from bytes outside the span: the frame is
 *  skipped there, and its decode then fails the call.
 *  Not covered: a rolling hash for shifted content, a variant on ZraHipArchive handles, the shards of a distributed archive, the
 *  host-pointer API, a signature of a content sub-range other than whole frames. */
ZRA_EXPORT ZraStatus ZraHipSignArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t grain, uint64_t seed,
    uint64_t firstFrame, uint64_t frameCount, size_t stagingBytes, uint64_t* dSig, size_t sigCapacityWords, ZraHipSignature* info);
/** The last ZraHipSignArchive on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, frames signed, grain words written (non-empty grains), content bytes hashed, compressed bytes
 *  hashed, passes, 0, 0}. */
ZRA_EXPORT void ZraHipGetSignStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugDiffMs: HIP-event time of the last sign call's own launches (span hash, grain hash), summed over its
 *  passes; its decodes are in ZraHipGetKernelStats. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugSignMs(ZraHipEngine* engine);

/** ZraHipDiffArchives with A given by its signature (*sigA on the host, its sigWords words at dSigA in device memory) and B by the
 *  archive at dB. The outputs are defined exactly as there at grain = sigA->grain with UA = sigA->contentSize (C = UA): writes are
 *  maximal runs of dirty grains, continuing across frames and passes; B's bytes of the dirty grains are packed into dData; B's tail
 *  [UA, UB) lies behind them; the four output words are the diff's. A grain is DIRTY when its word in dSigA differs from XXH64 with
 *  sigA->seed of B's bytes of the same clipped grain. A call with A's signature gives, word for word and byte for byte, what
 *  ZraHipDiffArchives(A, B, grain) gives, with one exception, the documented limit: equal 64-bit words are taken as equal content, so
 *  SIGNATURE DIFF IS NOT COMPARE. A caller that wants 128 bits signs twice with two seeds and takes the union of the two patches.
 *  Statuses, checked in this order:
 *   1. the NULLs of rule 1 of ZraHipDiffArchives; sigA NULL; dSigA NULL with sigWords != 0; mode with bits other than
 *      ZRA_HIP_SIGDIFF_DECODE_ALL; an inconsistent *sigA (grain not a power of two in 64 .. 8192, frameSize 0, frames !=
 *      ceil(contentSize / frameSize), words != frames * (1 + gpf), sigWords < words) -> {ZStdError, 42}.
 *   2. [dData, dData + dataCapacity) overlaps B or the signature -> {ZStdError, 42}.
 *   3. Header problems of B, as rule 3 of ZraHipSignArchive.
 *   4. B's frame size differs from sigA->frameSize -> {ZStdError, 40}.
 *   5. UB < UA -> {ZStdError, 40}.
 *   6. Scratch that cannot be allocated -> {ZStdError, 64}: the staging window, 1 byte per slot and 1 byte per grain of a pass, 24
 *      bytes per 256 grains of a pass, 16 bytes per write up to writeCapacity, the decoder's job arrays and own scratch.
 *   7. A frame of B that has to be decoded and fails, as rule 7 of ZraHipDiffArchives. The tail frames come behind all other passes.
 *   8. *nWrites > writeCapacity or *dataSize > dataCapacity -> OutputBufferTooSmall with the four words set: the sizing call.
 *  Everything ZraHipDiffArchives promises about untouched host arrays, dData behind dataCapacity and "no list entry before the last
 *  pass" holds here too.
 *  THE SHORTCUT. Without ZRA_HIP_SIGDIFF_DECODE_ALL a frame of [0, ceil(C / fs)) is clean without being decoded when B's span is well
 *  formed and its XXH64 equals A's frame word; anything else is decoded, whole, checksum verified, and its grains are hashed and
 *  compared. After an update every carried-over frame is skipped, so the cost follows the touched frames. A signature against an
 *  identical archive gives 0 writes and no decode launch; the same content at another level decodes every frame and gives 0 writes.
 *  Passes: max(1, min(65,536, stagingBytes / frameSize)) frames each: only B is decoded, the window is not halved. Tail passes are
 *  the diff's. */
ZRA_EXPORT ZraStatus ZraHipDiffSignature(ZraHipEngine* engine, const ZraHipSignature* sigA, const uint64_t* dSigA, size_t sigWords,
    const void* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
    uint64_t* hOffsets, uint64_t* hSizes, uint64_t* hDataOffsets, size_t writeCapacity, uint64_t* nWrites,
    void* dData, size_t dataCapacity, uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize);
/** The last ZraHipDiffSignature on the engine, in the shape of ZraHipGetDiffStats (all zero after any outcome other than Success):
 *  out8 = {frames of [0, C), frames equal by their frame word, frames decoded, tail frames decoded, writes, dirty bytes, passes, dirty
 *  grains}. A signature diff does not touch ZraHipGetDiffStats, and the other way round. */
ZRA_EXPORT void ZraHipGetDiffSignatureStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid: HIP-event time of the last signature diff's own launches (span hash, job build, grain hash, count, scan, fill with
 *  the gather copy, tail jobs and tail copy), summed over its passes. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugDiffSignatureMs(ZraHipEngine* engine);

/* ---- record index: read the records of a device-resident archive by their number ----
 * Every other read path addresses content by byte offset. A caller who keeps line-oriented data in an archive (logs, JSONL samples)
 * addresses it by RECORD: "samples 17, 4,000,000 and 12". The index below makes that a lookup: one 64-bit word per frame.
 * CONTENT AND DELIMITERS. The content is [0, U). The delimiters t_0 < ... < t_(D-1) are the positions whose byte equals `delimiter`.
 * RECORDS. Record k < D is [s_k, t_k), with s_0 = 0 and s_k = t_(k-1) + 1. Record D is [s_D, U) iff s_D < U. R is the number of
 * records; U = 0 gives R = 0. These are the records ZraHipGrepArchive defines for the range [0, U).
 * THE INDEX. F 64-bit words in device memory, F = frames, word f belongs to frame f: bits 0..62 hold the number of delimiter bytes in
 * frame f's content, bit 63 is set iff the frame's last content byte is not the delimiter. A word depends on its own frame only, so
 * an append leaves old words in place and adds new ones behind them; after ZraHipUpdateArchive the words of the touched frames are
 * refreshed with a sub-range call, as ZraHipSignArchive refreshes the records of a signature. D = the sum of the counts,
 * R = D + bit 63 of word F-1. What describes an index stays on the host (ZraHipRecordIndex, 40 bytes) and travels with the words. */
typedef struct ZraHipRecordIndex { uint64_t contentSize; uint32_t frameSize; uint32_t delimiter; uint64_t frames; uint64_t delimiters; uint64_t records; } ZraHipRecordIndex;

/** Writes the words of frames [firstFrame, firstFrame + frameCount) (frameCount UINT64_MAX: to the last frame; ZraHipVerifyArchive's
 *  range) of the archive at dArchive (device memory) into their places in dIndex (device memory, indexCapacityWords words).
 *  Synchronous; the archive is only read; stream ordering as the other compute calls (ZraHipWaitStream).
 *  Statuses, checked in this order:
 *   1. engine or info NULL; dArchive NULL with a size other than 0; dIndex NULL with indexCapacityWords != 0; delimiter > 255
 *      -> {ZStdError, 42}.
 *   2. [dIndex, dIndex + 8 * indexCapacityWords) overlaps the archive -> {ZStdError, 42}.
 *   3. Header problems -> the statuses of ZraHipArchiveOpen; a frame size of 0 -> HeaderInvalid.
 *   4. firstFrame > frames, or frameCount != UINT64_MAX and frameCount > frames - firstFrame -> OutOfBoundsAccess. The empty range is
 *      Success and writes nothing.
 *   5. indexCapacityWords < frames -> OutputBufferTooSmall; *info has its first four fields filled and its totals 0. This is the
 *      sizing call: nothing is decoded and nothing is written.
 *   6. Scratch that cannot be allocated -> {ZStdError, 64}: the staging window, 4 bytes per 8 KiB tile of it, the decoder's job
 *      arrays and own scratch.
 *   7. A frame that does not decode -> the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside
 *      it: the lowest failing frame of the first failing pass. The words of the range are then undefined.
 *  No word outside the range, and none at or behind indexCapacityWords, is ever written, whatever the outcome.
 *  Passes: max(1, min(65,536, stagingBytes / frameSize)) frames each (stagingBytes 0: 4 GiB). Frames are decoded whole, with their
 *  checksums verified.
 *  On Success info->delimiters and info->records are computed on the device from ALL F words as they lie in dIndex after the call
 *  (the empty range included, when indexCapacityWords >= frames): THEY ARE MEANINGFUL ONCE EVERY FRAME HAS BEEN INDEXED, by this call
 *  or by earlier ones into the same buffer. *info is zeroed on every status other than Success and OutputBufferTooSmall.
 *  Through an archive handle, ZraHipArchiveIndexRecords takes the resident frames of the range out of the cache.
 *  Not covered: delimiters of more than one byte, shards, the host-pointer API. */
ZRA_EXPORT ZraStatus ZraHipIndexRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t delimiter,
    uint64_t firstFrame, uint64_t frameCount, size_t stagingBytes, uint64_t* dIndex, size_t indexCapacityWords, ZraHipRecordIndex* info);
/** The last ZraHipIndexRecords on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, frames indexed, content bytes scanned, delimiters in the range, passes, 0, 0, 0}. */
ZRA_EXPORT void ZraHipGetIndexRecordsStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid, like ZraHipDebugSignMs: HIP-event time of the last index call's own launches (tile counts, frame words, totals),
 *  summed over its passes; its decodes are in ZraHipGetKernelStats. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugIndexRecordsMs(ZraHipEngine* engine);

/** hRanges[i] = {s_r, t_r - s_r} for r = hRecordNumbers[i] (record D: {s_D, U - s_D}). Both are host arrays of nRecords entries; the
 *  output is in request order; any order and duplicates are allowed. *info and the indexWords words at dIndex (device memory) are
 *  what ZraHipIndexRecords left. Synchronous; archive and index are only read.
 *  Statuses, checked in this order:
 *   1. engine, info NULL; dArchive NULL with a size other than 0; dIndex NULL with indexWords != 0; hRecordNumbers or hRanges NULL
 *      with nRecords != 0; an inconsistent *info (frameSize 0, frames != ceil(contentSize / frameSize), delimiter > 255, indexWords <
 *      frames) -> {ZStdError, 42}. nRecords above 2^32 - 16 -> {ZStdError, 64}, as the random-access batch.
 *   2. Header problems: rule 3 of ZraHipIndexRecords.
 *   3. The archive's content size, frame size or frame count differs from *info -> {ZStdError, 40}.
 *   4. A record number >= R, R recomputed from the words and not taken from info->records -> OutOfBoundsAccess.
 *   5. Scratch that cannot be allocated -> {ZStdError, 64}: 20 bytes per frame of the archive and 40 bytes per request, the staging
 *      window of the NEEDED frames with 4 bytes per 8 KiB tile, the decoder's job arrays and own scratch.
 *   6. A needed frame that fails to decode: rule 7 of ZraHipIndexRecords.
 *   7. A STALE WORD: a decoded frame whose delimiter count, or whose bit 63, differs from its index word -> {ZStdError, 20}. Locate
 *      never returns a range out of a frame whose word is wrong.
 *  Frames that are not decoded are not checked: INDEX IS NOT VERIFY. A wrong word of a frame that holds no asked boundary shifts the
 *  numbering behind it and goes unnoticed.
 *  Nothing is written to hRanges unless the call succeeds; the list comes to the host once, behind the last pass.
 *  Work, all of it on the device: the exclusive prefix of the counts; per request up to two boundaries, delimiter r - 1 and delimiter r
 *  (the start of record 0 and the end of an open record D need no lookup); a binary search in the prefix gives each boundary's
 *  (frame, ordinal in the frame) and flags the frame; the flagged frames, ascending, are decoded whole in passes of
 *  max(1, min(65,536, stagingBytes / frameSize)) NEEDED frames; per pass the delimiters of each 8 KiB tile are counted, the tiles of a
 *  frame prefixed, total and last byte compared with the word, and every boundary whose frame is in the pass is resolved by reading one
 *  tile. The cost follows the records asked for, not the archive: 100 records in 3 frames decode 3 frames. Every pass launches one wave
 *  per boundary of the call (those of other passes leave at once).
 *  Through an archive handle, ZraHipArchiveLocateRecords decodes only the boundary frames that are not resident. */
ZRA_EXPORT ZraStatus ZraHipLocateRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const ZraHipRecordIndex* info,
    const uint64_t* dIndex, size_t indexWords, const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes,
    ZraHipContentRange* hRanges);
/** The last ZraHipLocateRecords on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, records asked, boundaries looked up, frames decoded, content bytes regenerated, passes, 0, 0}. */
ZRA_EXPORT void ZraHipGetLocateRecordsStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid: HIP-event time of the last locate's own launches (prefix, boundaries, jobs, tile counts, frame check, select),
 *  summed over its passes. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugLocateRecordsMs(ZraHipEngine* engine);

/** ZraHipLocateRecords (hRanges optional: NULL is allowed), then the records' bytes at dData (device memory, dataCapacity bytes) in
 *  request order, each record followed by one `delimiter` byte: the packing of ZraHipExtractRecords. *dataSize = the sum of
 *  (n_i + 1); record i starts at the sum of (n_j + 1) over the requests before it.
 *  Statuses: those of ZraHipLocateRecords in their order, with
 *   - dataSize NULL, dData NULL with dataCapacity != 0 -> {ZStdError, 42} (rule 1);
 *   - directly behind rule 1: [dData, dData + dataCapacity) overlaps the archive or the index -> {ZStdError, 42};
 *   - behind rule 7: *dataSize > dataCapacity -> OutputBufferTooSmall with *dataSize set. The sizing call (capacity 0) costs the
 *     locate sweep only; nothing is written to hRanges or dData;
 *   - then the statuses of ZraHipDecompressRABatch for the read of the located ranges.
 *  On every status other than Success and OutputBufferTooSmall *dataSize = 0; hRanges is written on Success only. No byte in front
 *  of dData or at or behind dData + dataCapacity is ever written.
 *  BUILT AS A COMPOSITION IN THIS VERSION: the locate sweep, then one batched read of the located ranges (record k < D as
 *  [s_k, t_k + 1), so its delimiter comes from the content; only an open last record gets its delimiter byte stored separately).
 *  THE KNOWN COST: a frame that holds a boundary is decoded by both sweeps. The read sweep decodes up to the last byte a record
 *  needs, whatever ZRA_HIP_OPT_RA_WHOLE_FRAMES says (the boundary frames were decoded whole, checksums verified, by the locate sweep).
 *  Fusing the two sweeps when all needed frames fit one window is not done. Through an archive handle, ZraHipArchiveReadRecords serves
 *  both sweeps from the resident frames and keeps the frames it had to decode. */
ZRA_EXPORT ZraStatus ZraHipReadRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const ZraHipRecordIndex* info,
    const uint64_t* dIndex, size_t indexWords, const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes,
    ZraHipContentRange* hRanges, void* dData, size_t dataCapacity, uint64_t* dataSize);
/** The last ZraHipReadRecords on the engine (all zero after any outcome other than Success; engine NULL: all zero; out8 NULL: no-op):
 *  out8 = {frames in the archive, records, packed bytes (= *dataSize), frames decoded by the locate sweep, decode jobs of the read
 *  sweep, locate passes, 0, 0}. None of the three record calls touches another one's stats. */
ZRA_EXPORT void ZraHipGetReadRecordsStats(ZraHipEngine* engine, uint64_t* out8);
/** Bring-up aid: HIP-event time of the last successful read's locate-sweep launches, summed over its passes; its read sweep is in
 *  ZraHipGetKernelStats. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugReadRecordsMs(ZraHipEngine* engine);

/* ---- sharded compression (one process per GPU; frames [firstFrame, firstFrame+nFrames) of a larger input) ---- */
/** Compresses nFrames frames of frameSize bytes (last may be shorter: inSize bytes total) from dIn into a packed body at dBody
 *  (capacity nFrames*ZSTD_compressBound(frameSize)); writes the nFrames local frame sizes (u64, device) to dSizes and the
 *  local body size to *bodySize. No header is produced. */
ZRA_EXPORT ZraStatus ZraHipCompressFrames(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dBody, uint64_t* dSizes,
                                          size_t* bodySize, int8_t compressionLevel, uint32_t frameSize, bool checksum);

/** Builds the complete ZRA header (38 bytes + 5*tableSize) on the HOST from all frame sizes (rank-ordered concatenation),
 *  including the CRC-32 (zra.cpp:128-133). hHeader must hold 38 + 5*(nFramesTotal+1) bytes. */
ZRA_EXPORT ZraStatus ZraHipStitchHeader(const uint64_t* hFrameSizes, size_t nFramesTotal, uint64_t uncompressedSize,
                                        uint32_t frameSize, void* hHeader, size_t* headerSize);

/* ---- distributed archive: one process per GPU, frames sharded by index (zra_amd/csrc/zra_comm.hip) ----
 * The reference has no multi-device mode; its frame loop (zra.cpp:216-225) and its lookup (zra.cpp:265-269) are what is split here.
 * Rank r of `world` owns frames [F*r/world, F*(r+1)/world). All ZraHipComm* calls are COLLECTIVE: every rank of the communicator
 * makes the same call, and every rank returns the same status (the first failing rank's). */
typedef struct ZraHipComm ZraHipComm;
typedef struct ZraHipShard ZraHipShard;

/** Frames [*lo, *hi) owned by `rank`. Pure arithmetic. */
ZRA_EXPORT void ZraHipShardRange(uint64_t nFrames, int rank, int world, uint64_t* lo, uint64_t* hi);
/** The rank that owns `frame`. */
ZRA_EXPORT int ZraHipOwnerOfFrame(uint64_t nFrames, int world, uint64_t frame);

/** One piece of a query after it has been cut at ownership boundaries. */
typedef struct ZraHipSlice {
  uint32_t owner;      /* rank that holds the frames of this piece */
  uint64_t query;      /* index of the query it belongs to */
  uint64_t offset;     /* first uncompressed byte (offset into the whole archive's content) */
  uint64_t size;       /* bytes */
  uint64_t within;     /* where the piece starts inside the query's answer */
} ZraHipSlice;
/** Query router: cuts (offset, size) queries at ownership boundaries; slices are written grouped by owner, query order inside an
 *  owner, and counted per owner in perOwnerCount[world] (may be NULL). Bounds as DecompressRA: any query with
 *  offset + size >= uncompressedSize fails the call with OutOfBoundsAccess (zra.cpp:260). OutputBufferTooSmall: *nSlices tells the
 *  capacity needed. Pure host arithmetic — no engine, no GPU. */
ZRA_EXPORT ZraStatus ZraHipRouteQueries(uint64_t uncompressedSize, uint32_t frameSize, int world, const uint64_t* offsets, const uint64_t* sizes,
                                        size_t nQueries, ZraHipSlice* slices, size_t sliceCapacity, size_t* nSlices, uint64_t* perOwnerCount);

/** RCCL transport (ncclAllGather, grouped ncclSend/ncclRecv over xGMI). Rank 0 creates the 128-byte
 *  id and hands it to the other ranks by the host program's own means. */
ZRA_EXPORT ZraStatus ZraHipCommGetUniqueId(void* id128);
ZRA_EXPORT ZraStatus ZraHipCommCreateRccl(ZraHipComm** comm, ZraHipEngine* engine, const void* id128, int rank, int world);
/** Host transport: the exchange steps are handed to two callbacks of the host program (MPI, sockets, ...) on HOST buffers; device
 *  data is staged. Return 0 for success.
 *    allgather: every rank contributes `bytes` bytes, recv gets world*bytes in rank order.
 *    exchange:  one point-to-point round — all sends and receives of this rank; returns when all of them are complete.
 *  engine may be NULL for a communicator that only stitches (ZraHipCommStitchSizes). */
typedef struct ZraHipHostTransport {
  void* user;
  int (*allgather)(void* user, const void* send, void* recv, size_t bytes);
  int (*exchange)(void* user, int nSend, const int* sendPeer, const void* const* sendBuf, const size_t* sendBytes,
                  int nRecv, const int* recvPeer, void* const* recvBuf, const size_t* recvBytes);
} ZraHipHostTransport;
ZRA_EXPORT ZraStatus ZraHipCommCreateHost(ZraHipComm** comm, ZraHipEngine* engine, const ZraHipHostTransport* transport, int rank, int world);
/** Diagnostic (RCCL transport): bytes from dSrc to dDst through the point-to-point path, this rank sending to itself — what a one-rank
 *  run can exercise of the transport's message chunking (pieces of at most 1 GiB per ncclSend / ncclRecv; ZRA_COMM_CHUNK_MIB). */
ZRA_EXPORT ZraStatus ZraHipCommLoopback(ZraHipComm* comm, const void* dSrc, void* dDst, size_t bytes);
ZRA_EXPORT void ZraHipCommDestroy(ZraHipComm* comm);

/** Sharded CompressBuffer (zra.cpp:194-235): dLocal = the uncompressed bytes of this rank's frames, i.e. bytes
 *  [lo*frameSize, min(totalBytes, hi*frameSize)) of the input with [lo, hi) = ZraHipShardRange(ceil(totalBytes/frameSize), rank, world)
 *  (InputFrameSizeMismatch if localBytes is not exactly that). Only the frame sizes travel (8 bytes per frame, all-gather): every rank
 *  ends up with the complete header + seek table and the compressed body of its own frames — a shard. Byte-identical to the archive
 *  one GPU would write. */
ZRA_EXPORT ZraStatus ZraHipCommCompress(ZraHipComm* comm, const void* dLocal, size_t localBytes, uint64_t totalBytes, int8_t compressionLevel,
                                        uint32_t frameSize, bool checksum, ZraHipShard** shard);
/** The size exchange and stitch alone (zra.cpp:216-230), for frames that were compressed elsewhere: hLocalSizes = the compressed sizes
 *  of this rank's frames [lo, hi) (nLocal = hi - lo, InputFrameSizeMismatch otherwise). Collective; every rank gets the complete
 *  header + seek table (ZraHipShardGetHeader), the shard holds no body (ZraHipShardGetBody: NULL, 0 bytes). Works on a communicator
 *  created without an engine. Engine-less communicators and stitch-only shards must be that on EVERY rank: ZraHipCommCompress /
 *  GatherArchive / Serve return parameter_unsupported on them after one agreement round, and ranks that hold an engine or a body would
 *  go on to larger exchanges. More than 2^32 - 2 frames, or hLocalSizes == NULL with nLocal > 0, are rejected on every rank. */
ZRA_EXPORT ZraStatus ZraHipCommStitchSizes(ZraHipComm* comm, const uint64_t* hLocalSizes, size_t nLocal, uint64_t totalBytes, uint32_t frameSize,
                                           ZraHipShard** shard);
ZRA_EXPORT void ZraHipShardDestroy(ZraHipShard* shard);
ZRA_EXPORT size_t ZraHipShardHeaderSize(const ZraHipShard* shard);
/** Header + seek table of the WHOLE archive (host copy, CRC-32 set). */
ZRA_EXPORT void ZraHipShardGetHeader(const ZraHipShard* shard, void* hHeader);
/** Size of the whole archive (header + all ranks' frames). */
ZRA_EXPORT uint64_t ZraHipShardArchiveSize(const ZraHipShard* shard);
/** This rank's frames: device pointer, their offset inside the archive's body, their length (NULL and 0 for a stitch-only shard). */
ZRA_EXPORT void ZraHipShardGetBody(const ZraHipShard* shard, const void** dBody, uint64_t* bodyBase, uint64_t* bodyBytes);
/** The archive in one piece in dArchive on rank `root` (other ranks pass NULL / 0): world-1 inbound point-to-point messages in one group. */
ZRA_EXPORT ZraStatus ZraHipCommGatherArchive(ZraHipComm* comm, const ZraHipShard* shard, int root, void* dArchive, size_t archiveCapacity,
                                             size_t* archiveSize);
/** The gather beside other work (round 6): a SECOND communicator of the process gets a stream of its own (UseOwnStream); Begin starts
 *  ZraHipCommGatherArchive on it (a worker thread drives the collective; every rank calls Begin and End) and returns at once, so that the
 *  ranks can serve queries from their shards on the first communicator meanwhile (ZraHipCommServe works on the shards, not on the gathered
 *  archive); End joins and returns the gather's status and, on the root, the archive's size. */
ZRA_EXPORT ZraStatus ZraHipCommUseOwnStream(ZraHipComm* comm);
ZRA_EXPORT ZraStatus ZraHipCommGatherArchiveBegin(ZraHipComm* comm, const ZraHipShard* shard, int root, void* dArchive, size_t archiveCapacity);
ZRA_EXPORT ZraStatus ZraHipCommGatherArchiveEnd(ZraHipComm* comm, size_t* archiveSize);
/** Sharded serving (BASELINE config C5): every rank passes its own queries over the WHOLE uncompressed range; slices go to the ranks
 *  that own the frames, are decoded there (ZraHipDecompressRABatch semantics on the shard) and come back; answer q lands at
 *  dOut + hOutOffsets[q]. Bounds as DecompressRA (zra.cpp:260). */
ZRA_EXPORT ZraStatus ZraHipCommServe(ZraHipComm* comm, const ZraHipShard* shard, const uint64_t* hOffsets, const uint64_t* hSizes,
                                     const uint64_t* hOutOffsets, size_t nQueries, void* dOut);

/** Last per-call timing of the dominant kernel on the engine's stream, measured with HIP events (milliseconds; 0 if none). */
ZRA_EXPORT double ZraHipLastKernelMs(ZraHipEngine* engine);
/** HIP-event timings (ms) and launch counts of the kernels of the LAST call on this engine, measured on the engine's stream:
 *  out6 = {match-finder ms, launches, entropy-stage ms, launches, decode ms, launches}. */
ZRA_EXPORT void ZraHipGetKernelStats(ZraHipEngine* engine, double* out6);
/** Decode stages of the LAST decode / random-access call on this engine (HIP events on the engine's stream, summed over its rounds):
 *  out8 = {parse ms, Huffman ms, sequence-chain ms, execute ms, rounds, one-launch small-batch kernel ms, its launches, 0}.
 *  The parse span includes the literal streams its waves decode themselves (blocks whose literals come with a new Huffman tree);
 *  the Huffman span is what is left to that stage's own launch. */
ZRA_EXPORT void ZraHipGetDecodeStageStats(ZraHipEngine* engine, double* out8);
/** Launch telemetry of the LAST persistent level-3/4 compress on this engine, written by every wave of the match-finder launch:
 *  u64 words [0] shader cycles summed over waves, [1] ticks of the constant 100 MHz clock summed over waves (cycles / ticks x 100 = the
 *  effective shader MHz of the launch), [2] waves, [3] longest wave (ticks), [4] ~earliest wave start, [5] latest wave end, [6] latest
 *  wave start, [7] ~earliest wave end, [8..15] waves per XCD, [16..23] frames taken per XCD, [24..31] ticks per XCD, [32 + k] waves on
 *  compute unit k = xcc << 8 | se << 5 | sh << 4 | cu (2048 words, each four 16-bit counts: the unit's four SIMDs); then the entropy stage's persistent workgroups: [2080] workgroups
 *  that took a frame, [2081] their resident ticks, [2082] ticks they spent waiting for a frame or a slot, [2083] frames, [2088 + k]
 *  workgroups on compute unit k. Returns the words written (0: the call took another path). */
ZRA_EXPORT size_t ZraHipGetLaunchTelemetry(ZraHipEngine* engine, uint64_t* out, size_t capWords);

/* ---- opt-in integrity options (default 0: bit- and error-compatible with the reference, quirks included) ---- */
#define ZRA_HIP_OPT_VERIFY_HEADER_CRC 1u     /* Header constructors check the CRC-32 the reference writes but never reads (zra.cpp:128-133) */
#define ZRA_HIP_OPT_INCLUSIVE_RA_BOUND 2u    /* DecompressRA accepts offset+size == uncompressedSize (reference: '>=', zra.cpp:260) */
#define ZRA_HIP_OPT_STORE_META_IN_MEMORY 4u  /* in-memory CompressBuffer stores `meta` like the streaming Compressor (reference: zra.cpp:202-205) */
#define ZRA_HIP_OPT_RA_WHOLE_FRAMES 8u      /* ZraHipDecompressRABatch decodes every touched frame in full and verifies its checksum */
/** Process-wide; affects the zra.h / zra.hpp entry points (and, for the last flag, ZraHipDecompressRABatch). */
ZRA_EXPORT void ZraHipSetOptions(uint32_t mask);
ZRA_EXPORT uint32_t ZraHipGetOptions(void);

/** Bring-up aid (not a product entry point): the match finder's sequences {litLength | matchLength<<20 | offsetValue<<40} left in
 *  scratch for frame `frame` of the last compress call's last batch (last block of the frame); meta3 = {nbSeq, lastLL, skip}. */
ZRA_EXPORT uint32_t ZraHipDebugReadSeqs(ZraHipEngine* engine, uint32_t frame, uint64_t* out, uint32_t cap, uint32_t* meta3);

/** Bring-up aid (not a product entry point): HIP-event time (ms, on the engine's stream) of the stage-from-cache kernel launches of the
 *  last ZraHipArchiveUpdate on this engine, summed over its passes; 0 when none ran. engine NULL: 0. */
ZRA_EXPORT double ZraHipDebugUpdateStageMs(ZraHipEngine* engine);

#ifdef __cplusplus
}
#endif
#endif
