// zra_amd — host engine: owns one HIP device, one stream and a grow-only scratch pool, and drives the
// decode / encode kernels. Internal C++ interface used by the C ABI (zra_capi.cpp) and zra_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "zra_kernels.h"
#include "zra_pass_plan.h"   // pass_slots, the pass geometry of the range scans (zra_scan_plan.h) and of the frame passes (host only)

namespace zra_eng {

struct Status { int zra; int zstd; };   // mirrors ZraStatus (kept free of the public header here)
enum : int { kSuccess = 0, kZStdError = 1, kVersionLow = 2, kHeaderInvalid = 3, kHeaderIncomplete = 4, kOutOfBounds = 5,
             kOutputTooSmall = 6, kCompressedTooLarge = 7, kFrameSizeMismatch = 8 };
inline Status ok() { return {kSuccess, 0}; }
inline Status zerr(int code) { return {kZStdError, (int)(int8_t)code}; }   // i8 narrowing like zra.cpp:440

// grow-only device allocation
struct DevBuf {
  void* p = nullptr; size_t cap = 0;
  // true: cap >= n (the buffer may have MOVED, and its old contents are gone: the old one is freed before the new one is asked for,
  // to keep the peak low). false: no memory, and on `false` the buffer is EMPTY (p == nullptr, cap == 0): every pointer taken from
  // it before is dead, and so is host state that describes its contents. The result decides the caller's status ({ZStdError, 64}).
  [[nodiscard]] bool reserve(size_t n);
  void release();
  template <typename T> T* as() const { return (T*)p; }
};

// device scratch held by all engines of the process (DevBuf reservations), in bytes
uint64_t scratch_bytes_in_use();

// parsed fixed header (host side; zra.cpp:141-163 semantics)
struct HeaderInfo {
  uint16_t version; uint32_t size; uint64_t uncompressedSize; uint32_t frameSize, metaOffset, metaSize, seekTableOffset, seekTableSize;
  uint32_t frames() const { return seekTableSize / 5 ? seekTableSize / 5 - 1 : 0; }
};
// parse the 38 fixed bytes; returns a ZRA status code (0 ok)
int parse_fixed_header(const uint8_t* fixed38, HeaderInfo* h);
// A device-resident archive as the device-archive calls see it (random access, handle, update, verify, search, grep, extract, compare, diff, sign): the checked header and
// where its parts lie. Built once per call, by Engine::archive_view or, from a header checked before (a handle's), by `over`. A shard of
// a distributed archive (zra_comm.hip) overrides body / bodyBytes with the bytes [bodyBase, bodyBase + bodyBytes) of the body it holds.
struct ArchiveView {
  HeaderInfo h{};
  const uint8_t* table = nullptr, * body = nullptr;   // seek table (frames + 1 entries of 5 bytes), compressed frames
  uint64_t bodyBytes = 0, bodyBase = 0;
  uint32_t frames = 0;
  uint64_t fs = 0, U = 0;            // frame size, uncompressed size
  static ArchiveView over(const HeaderInfo& h, const uint8_t* dArc, size_t arcSize) {
    ArchiveView a;
    a.h = h; a.table = dArc + h.seekTableOffset; a.body = dArc + h.size; a.bodyBytes = arcSize - h.size; a.frames = h.frames(); a.fs = h.frameSize; a.U = h.uncompressedSize;
    return a;
  }
};
// The index of a device-archive call's counters and milliseconds (Engine::callStats_, callMs_): the range scans (search, multi-pattern
// search, grep, extract; one host driver, zra_scan.h) first, then the calls on whole frames (zra_framepass.h, zra_verify.hip)
enum : int { kScanSearch = 0, kScanMulti, kScanGrep, kScanExtract, kScanCalls,
             kCallCompare = kScanCalls, kCallDiff, kCallSign, kCallSigDiff, kCallIndex, kCallLocate, kCallRead, kCallVerify, kCallTally, kCalls };
// the tally (zra_tally.hip): the positions of one workgroup, and ZRA_HIP_TALLY_MAX_KEY, the longest record that is a key
constexpr uint32_t kTallyTile = 4096, kTallyMaxKey = 4096;
// the code a failing frame is reported with: 255 (the decoder's own "regenerated another size than its slot") is corruption_detected
__host__ __device__ inline int reported_code(unsigned long long firstError) { const int c = (int)(firstError & 0xFF); return c == 255 ? 20 : c; }
// An update through an archive handle (zra_archive.hip, ZraHipArchiveUpdate): what the handle lends to Engine::update_archive and what
// comes back.
struct UpdCacheView {
  HeaderInfo h{};                    // the handle's checked header, taken in place of a read from the device
  uint8_t* arena = nullptr;          // slots x frameSize: old plaintext is read from it, and new bytes are laid over it after the last check
  uint32_t slots = 0;                // 0: a handle without a cache (table is not called)
  // frame -> arena slot (0xFFFFFFFF: not resident), readable for `frames` frames, those behind the old frames not resident. Called once,
  // behind the host-side checks of the update (statuses 1-4), with the frames of the RESULT: the handle grows its table here, on the
  // engine's stream. nullptr: no memory ({ZStdError, 64})
  const uint32_t* (*table)(void* ctx, uint32_t frames) = nullptr;
  void* ctx = nullptr;
  // on Success: the header of the archive at dOut (from the host copy the update wrote), frames staged from the arena in place of a
  // decode, resident frames that hold new bytes
  HeaderInfo newHeader{};
  uint32_t staged = 0, refreshed = 0;
};
// A range scan or a record call through an archive handle (zra_archive.hip, ZraHipArchiveSearch .. ZraHipArchiveExtractRecords,
// ZraHipArchiveIndexRecords .. ZraHipArchiveReadRecords): what the handle lends to the scans' driver (zra_scan.h), to the frame-pass
// driver (zra_framepass.h) and to the locate sweep (zra_records.hip), and what comes back. They only READ the arena and the table: a
// scan, an index and a locate are not reads.
struct ScanCacheView {
  HeaderInfo h{};                    // the handle's checked header, taken in place of a read from the device
  const uint8_t* arena = nullptr;    // slots x frameSize: the plaintext of the resident frames
  const uint32_t* slotOf = nullptr;  // device: frame -> arena slot (0xFFFFFFFF: not resident), `frames` entries
  uint32_t slots = 0, frames = 0;    // slots 0: a handle without a cache (the plain call's passes, minus the header read)
  uint32_t* pin = nullptr;           // four page-locked words: the counts of a pass come back here (zra_scan_split_kernel)
  // what the call did, on any status: frames staged from the arena, decode jobs, bytes those regenerated, passes; HIP-event time of
  // the job-split and stage-from-cache launches, summed over the passes
  uint64_t staged = 0, decoded = 0, decodedBytes = 0, passes = 0;
  double stageMs = 0;
};
// A record scan (Engine::record_scan, zra_record_scan.h): the arguments the entry points of zra_hip.h share, as the caller gave them.
// The records of [offset, offset + size), cut at `delimiter`, that the kind selects, ascending, in ONE decode of the range's frames;
// kind picks what selects a record and the kernels (a file each). Statuses and their order: zra_hip.h, the entry point named.
enum RecordKind : uint32_t {
  kRecGrep,          // ZraHipGrepArchive[Expr] (zra_grep.hip): a match of one of the patterns starts in the record. Writes grep_stats / grep_scan_ms
  kRecGrepWhere,     // ZraHipGrepArchiveWhere (zra_grep_where.hip, zra_where.h): one of the clauses holds for the set of patterns that hit in the
                     // record. Kernels of its own; writes the grep's counters and milliseconds
  kRecGrepRegex,     // ZraHipGrepArchiveRegex (zra_grep_regex.hip, zra_regex.h): the automaton of the expressions (alternatives; syntax: 0 or fold
                     // case) matches inside the record. Kernels of its own; writes the grep's counters (word 7: the matched records) and milliseconds
  kRecExtract,       // ZraHipExtractRecords[Expr] (zra_extract.hip): kRecGrep's selection with the records' bytes. Writes extract_stats / extract_ms
  kRecExtractRegex,  // ZraHipExtractRecordsRegex (zra_extract_regex.hip): kRecGrepRegex's selection, kRecExtract's outputs, in one pass. Kernels of
                     // its own; writes the extract's counters (word 7: the matched records before the mode) and milliseconds
  kRecGrepContext,   // ZraHipGrepArchiveContext (zra_grep_context.hip, zra_context.h): kRecGrep's selection with `before` records in front
                     // of and `after` behind each selected one. Kernels of its own; writes the grep's counters (word 4: |O|) and milliseconds
  kRecGrepRegexContext,   // ZraHipGrepArchiveRegexContext (zra_grep_regex_context.hip, zra_regex_context.h): kRecGrepRegex's selection,
                     // kRecGrepContext's outputs. Kernels of its own; writes the grep's counters (word 4: |O|, word 7: the matched records)
  kRecExtractWhere,  // ZraHipExtractRecordsWhere (zra_extract_where.hip): kRecGrepWhere's selection, kRecExtract's outputs, in one pass. Kernels of
                     // its own; writes the extract's counters and milliseconds
  kRecCut,           // ZraHipCutRecords (zra_cut.hip): kRecExtract's selection (no pattern: every record), of each selected record only the fields
                     // of fieldMask, cut at `separator`. Kernels of its own; writes the extract's counters and milliseconds
};
struct RecordCall {
  RecordKind kind;
  const uint8_t* dArc; size_t arcSize;                 // (through a handle: filled in by it)
  // nPat host patterns laid end to end at hPat, pattern i of hSizes[i] bytes; syntax: the word of the ...Expr, ...Where and ...Regex
  // entry points, 0 for the literal ones
  const uint8_t* hPat; const uint32_t* hSizes; size_t nPat; uint32_t syntax;
  uint8_t delimiter; uint32_t mode;                    // mode 1: the records NOT selected
  uint64_t offset, size; size_t stagingBytes;          // the range (size ~0: to the end), the staging window
  uint64_t* hRecords; size_t recordCap; uint64_t* nRecords;   // the list, {offset, size} pairs, ascending
  // the extracts: each selected record's content and one delimiter byte, packed at dData (device memory); the list goes to hRecords
  // iff recordCap != 0. *dataSize: the packed bytes
  uint8_t* dData = nullptr; size_t dataCap = 0; uint64_t* dataSize = nullptr;
  // kRecGrepWhere, kRecExtractWhere: a record is selected when one of the nClauses clauses {all, any, none} (ZraHipRecordClause) holds for the set of
  // patterns that hit in it
  const void* hClauses = nullptr; size_t nClauses = 0;
  // kRecGrepContext, kRecGrepRegexContext: the context in records (each at most 64), and beside *nRecords = |O| the selected records and the groups (or null)
  uint32_t before = 0, after = 0;
  uint64_t* nSelected = nullptr, * nGroups = nullptr;
  // kRecCut: the byte that ends a field, and the chosen fields: bit min(j, 64) - 1 for field j (no other kind reads them)
  uint8_t separator = 0; uint64_t fieldMask = 0;
};
// The byte fetch of a record read through an archive handle (zra_records.hip): the located ranges as one read of the handle, a query
// allowed to end AT the content's end. *jobs: the frames the fetch decoded.
struct RecordFetch {
  Status (*fn)(void* ctx, uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, uint32_t* jobs) = nullptr;
  void* ctx = nullptr;
};
// chunk length of the pipelined host-pointer calls (zra_hostpipe.hip); ZRA_HOST_CHUNK_MIB, default 1024
size_t host_chunk_bytes();

class Engine {
 public:
  static Status create(Engine** out, int device);
  ~Engine();
  hipStream_t stream() const { return stream_; }
  Status sync();
  // stream-ordering contract of the device-pointer API: the engine runs on two private non-blocking streams, which do not order
  // themselves against the caller's streams. Work queued on `producer` before this call completes before anything the engine
  // launches afterwards (an event wait, no host synchronisation). Outputs are complete when an engine call returns.
  Status wait_stream(hipStream_t producer);
  // gives every scratch allocation of this engine back to the device (they are grow-only otherwise and can reach tens of GiB after a
  // large level-9 compression); the next call allocates again what it needs
  Status release_scratch();
  double last_kernel_ms() const { return lastKernelMs_; }
  // launch telemetry of the last persistent dfast compress (ZraEncArgs::mfTele); empty when the call took another path
  // (fetched from the device here, on demand: the two blocking copies used to be paid by every persistent call, the small ones included)
  size_t launch_telemetry(uint64_t* out, size_t cap);
  // after a whole-archive decode_host(): bytes regenerated when frames had to be packed one after the other (a frame regenerated
  // another size than its slot), ~0 when every frame filled exactly its slot
  uint64_t last_produced_total() const { return lastProducedTotal_; }
  // HIP-event timings of the last call on the engine's stream: {mf ms, mf launches, entropy ms, entropy launches, decode ms, decode launches}
  void kernel_stats(double out[6]) const { for (int i = 0; i < 6; i++) out[i] = kstats_[i]; }
  // decode stages of the last call: {parse ms, Huffman ms, sequence-chain ms, execute ms, rounds, one-launch kernel ms, its launches, 0 (unused)}
  void decode_stage_stats(double out[8]) const { for (int i = 0; i < 8; i++) out[i] = dstats_[i]; }
  // bring-up: sequences {ll | ml<<20 | offVal<<40} the match finder left in scratch context 0 for frame `frame` of the LAST batch
  // (last block of the frame); returns the count, meta = {nbSeq, lastLL, skip}
  uint32_t debug_read_seqs(uint32_t frame, uint64_t* out, uint32_t cap, uint32_t meta[3]);

  // ---- decode
  // Decode nFrames frames described by device job arrays. Synchronises and returns the first failing frame's code.
  // maxFrameBytes: upper bound of what one frame regenerates (sizes the per-pass scratch); ra: optional random-access extras
  // (limit / pieceBase / pieces / raOut of ZraDecodeArgs, indexed like the job arrays)
  Status decode_jobs(const uint8_t* dBody, uint64_t bodySize, const uint64_t* dFrameOff, uint8_t* dOut,
                     const uint64_t* dOutOff, const uint32_t* dExpect, uint32_t nFrames, uint32_t maxFrameBytes, uint32_t offStride = 1,
                     uint64_t seqTotal = 0, const struct ZraDecodeArgs* ra = nullptr);
  // one pass: jobs [0, a.nFrames) of the arrays in `a` through the parse / chain / execute rounds + frame-end checks;
  // *res = min over failing jobs of ((jobBase + job) << 8 | code), untouched when none fails
  Status decode_launch(const struct ZraDecodeArgs& a, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* hResult);
  // the same for few jobs: one launch (zra_ra_small_kernel), one synchronisation; *bailed = jobs that need decode_launch after all
  Status decode_small(const struct ZraDecodeArgs& a, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* hResult, uint32_t* bailed);
  // one pass of decode_jobs over the jobs of `b` (at most one pass's worth): decode_small when they are few, decode_launch when they are
  // many or the small kernel handed one back. result_ must hold ~0 words (decode_jobs' memset). Afterwards status_ / produced_ hold every
  // job's own status and regenerated size, whatever *res says: what the verifier collects (zra_verify.hip).
  Status decode_pass(const struct ZraDecodeArgs& b, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* res);
  Status decode_scratch(struct ZraDecodeArgs& a, uint32_t maxFrameBytes);
  // Whole archive resident on the device (header + body), output on the device.
  Status decompress_device(const uint8_t* dArc, size_t arcSize, uint8_t* dOut, size_t outCap);
  // Batched random access (zra_ra.hip), archive + output on the device, query arrays on the host.
  Status decompress_ra_batch(const uint8_t* dArc, size_t arcSize, uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq) {
    return decompress_ra_batch_shard(dArc, arcSize, nullptr, 0, 0, dOut, hOff, hSize, hOutOff, nq);
  }
  Status decompress_ra_batch_shard(const uint8_t* dArc, size_t arcSize, const uint8_t* dBody, uint64_t bodyBytes, uint64_t bodyBase, uint8_t* dOut,
                                   const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq);
  // pieces of the batch, shared with the other device-archive calls: the header read + checks and the view they give, the walk over the
  // host query arrays (bounds, tuples uploaded to the device), the planner of the decode jobs, the batch behind an already checked header
  Status ra_header(const uint8_t* dArc, size_t arcSize, HeaderInfo* h);
  Status archive_view(const uint8_t* dArc, size_t arcSize, ArchiveView* a) {
    HeaderInfo h; const Status st = ra_header(dArc, arcSize, &h); if (!st.zra) *a = ArchiveView::over(h, dArc, arcSize); return st;
  }
  // endInclusive (internal, the record read alone): a query may end AT the content's end; every other caller keeps the reference's bound
  Status ra_walk_queries(const ArchiveView& a, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, uint64_t* maxPieces,
                         bool endInclusive = false);
  Status ra_plan_fill(uint32_t* plan, size_t nq, const ArchiveView& a, uint32_t passSlots, bool fullFrames, const uint32_t* victim, uint32_t totals[2]);
  // *jobsOut (optional): the decode jobs the batch ran
  Status ra_batch_body(const ArchiveView& a, uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool endInclusive = false,
                       uint32_t* jobsOut = nullptr);
  // tuples [q0, q1) of pinQ_ (pinned_tuples) -> qmeta_, queued on the stream; the caller writes and sends them kTupleChunk at a time
  static constexpr size_t kTupleChunk = 1u << 17;
  Status upload_tuples(size_t q0, size_t q1) {
    if (hipMemcpyAsync(qmeta_.as<uint64_t>() + 4 * q0, pinQ_ + 4 * q0, (q1 - q0) * 32, hipMemcpyHostToDevice, stream_) == hipSuccess) return ok();
    (void)hipGetLastError(); return zerr(1);
  }
  // One staged pass (verify, the range scans, compare, diff, sign): jobs [j0, j0 + n) of frameOff_ / expect_ decoded whole, checksums verified, into `window`, job j0 + k at
  // outOff_[k] (the same slots every pass). *firstError = decode_pass' word (~0: none failed); status_ / produced_: every job's own. Synchronised.
  Status staged_pass(const ArchiveView& a, uint32_t j0, uint32_t n, uint8_t* window, unsigned long long* firstError);
  // Host-walked frame list (reference semantics of DecompressBuffer: seek table not consulted). hFrameOff has nFrames+1 entries
  // relative to dBody; frames are assumed to regenerate frameSize bytes each (last: the remainder of total).
  Status decompress_frames_host_list(const uint8_t* dBody, uint64_t bodySize, const std::vector<uint64_t>& hFrameOff,
                                     uint8_t* dOut, uint64_t total, uint32_t frameSize);

  // ---- encode (zra_encode.hip)
  // Compress frames of `frameSize` from dIn (inSize bytes) into a packed body at dBody; per-frame sizes (u64) to dSizes.
  Status compress_frames(const uint8_t* dIn, size_t inSize, uint8_t* dBody, uint64_t* dSizes, size_t* bodySize,
                         int level, uint32_t frameSize, bool checksum);
  Status compress_persistent(const uint8_t* dIn, size_t inSize, uint8_t* dBody, uint64_t bodyBase0, uint8_t* dEntries, uint64_t* dSizes,
                             size_t* bodySize, uint32_t frameSize, bool checksum, const struct ZraEncParams& full, const struct ZraEncParams& tail,
                             const struct EncPlan& plan);
  Status compress_impl(const uint8_t* dIn, size_t inSize, uint8_t* dBody, uint64_t bodyBase0, uint8_t* dEntries, uint64_t* dSizes,
                       size_t* bodySize, int level, uint32_t frameSize, bool checksum);
  Status compress_impl_body(const uint8_t* dIn, size_t inSize, uint8_t* dBody, uint64_t bodyBase0, uint8_t* dEntries, uint64_t* dSizes,
                            size_t* bodySize, int level, uint32_t frameSize, bool checksum);
  void drain_after_error();
  // Full archive (header + table + body) on the device.
  Status compress_device(const uint8_t* dIn, size_t inSize, uint8_t* dOut, size_t* outSize, int level, uint32_t frameSize, bool checksum);

  // ---- update (zra_update.hip): a new archive at dOut = the one at dArc with nw byte ranges of its content overwritten and appendSize
  // bytes added. Only the frames whose content changes are decoded (when partly replaced) and encoded again; every other frame's
  // compressed bytes are carried over as they are. Statuses and their order: zra_hip.h, ZraHipUpdateArchive.
  Status update_archive(const uint8_t* dArc, size_t arcSize, const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize,
                        const uint64_t* hDataOff, size_t nw, const uint8_t* dAppend, size_t appendSize, uint8_t* dOut, size_t outCap,
                        size_t* outSize, int level, bool checksum, UpdCacheView* cache = nullptr);
  // what the last update_archive did: {frames, touched, decoded, compressed, bytes carried, bytes encoded, content bytes written, passes};
  // all zero unless it succeeded. decoded counts decode jobs: frames staged from a handle's cache are not among them
  void update_stats(uint64_t out[8]) const { for (int i = 0; i < 8; i++) out[i] = ustats_[i]; }
  // bring-up: HIP-event time of the last update's zra_upd_stage_cached_kernel launches, summed over its passes (0: none ran)
  double update_stage_ms() const { return updStageMs_; }

  // ---- verify (zra_verify.hip): header CRC-32, seek table and every frame's block walk of frames [first, first + count) of the archive
  // at dArc, then (content) every structurally sound frame decoded whole into a staging window, checksum verified. Every faulty frame is
  // reported, in frame order. Statuses, codes and their order: zra_hip.h, ZraHipVerifyArchive. hFaults: ZraHipFrameFault's layout.
  Status verify_archive(const uint8_t* dArc, size_t arcSize, uint32_t mode, uint64_t first, uint64_t count, size_t stagingBytes,
                        void* hFaults, size_t faultCap, size_t* nFaults);
  // the last verify_archive: {frames, checked, structure faults, content faults, decoded, content bytes regenerated, passes, 0}; all zero
  // unless it succeeded
  void verify_stats(uint64_t out[8]) const { call_stats(kCallVerify, out); }

  // ---- search (zra_search.hip): every content offset p of [offset, offset + size) (size ~0: to the end) at which the patternSize host
  // bytes at hPattern occur whole inside the range, ascending. Only the frames of the range are decoded, whole, a staging window at a
  // time; the window's plaintext is scanned on the device. Statuses and their order: zra_hip.h, ZraHipSearchArchive.
  Status search_archive(const uint8_t* dArc, size_t arcSize, const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size,
                        size_t stagingBytes, uint64_t* hMatches, size_t matchCap, uint64_t* nMatches);
  // the last search_archive: {frames, decoded, content bytes regenerated, matches, matches listed, passes, 0, 0}; all zero unless it succeeded
  void search_stats(uint64_t out[8]) const { call_stats(kScanSearch, out); }
  // bring-up: HIP-event time of the last search's scan launches (count, scan, fill, carry), summed over its passes
  double search_scan_ms() const { return callMs_[kScanSearch]; }

  // ---- search for several patterns (zra_msearch.hip): every (content offset, pattern index) at which one of the nPatterns host
  // patterns (laid end to end at hPatterns, pattern i of hPatternSizes[i] bytes) occurs whole inside the range, ascending, in ONE
  // decode of the range's frames. hMatches: ZraHipPatternMatch's layout; hPerPattern (optional): the matches of each pattern.
  // Statuses and their order: zra_hip.h, ZraHipSearchArchiveMulti. syntax (here and in the two calls below): the pattern syntax word of
  // the ...Expr entry points (zra_pattern_expr.h; lengths then count elements), 0 for the literal ones.
  Status search_archive_multi(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint64_t offset,
                              uint64_t size, size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern);
  // the last search_archive_multi: {frames, decoded, content bytes regenerated, matches, matches listed, passes, patterns, filter
  // survivors}; all zero unless it succeeded. The single-pattern search and this one leave each other's counters alone
  void search_multi_stats(uint64_t out[8]) const { call_stats(kScanMulti, out); }
  // bring-up: HIP-event time of the last multi search's scan launches (count, scan, fill, carry), summed over its passes
  double search_multi_scan_ms() const { return callMs_[kScanMulti]; }

  // ---- the record scans (zra_record_scan.h): grep, grep with a record predicate, grep with regular expressions, extract, extract with
  // regular expressions, by c.kind; one decode of the range's frames. Patterns, range and passes are search_archive_multi's. Statuses
  // and their order: zra_hip.h, the entry point of the kind. cv: the call goes through an archive handle.
  Status record_scan(const RecordCall& c, ScanCacheView* cv = nullptr);
  // the last grep of any kind: {frames, decoded, content bytes regenerated, records of the range, records selected, records listed,
  // passes, matches}; all zero unless it succeeded. The searches and the grep leave each other's counters alone
  void grep_stats(uint64_t out[8]) const { call_stats(kScanGrep, out); }
  // bring-up: HIP-event time of the last grep's scan launches (count, scan, fill, carry), summed over its passes
  double grep_scan_ms() const { return callMs_[kScanGrep]; }
  // the last extract of either kind: {frames, decoded, content bytes regenerated, records of the range, records selected, packed bytes,
  // passes, matches (with regular expressions: the matched records before the mode)}; all zero unless it succeeded. The searches, the
  // grep and the extract leave each other's counters alone
  void extract_stats(uint64_t out[8]) const { call_stats(kScanExtract, out); }
  // bring-up: HIP-event time of the last extract's own launches (count, scan, copy, carry), summed over its passes
  double extract_ms() const { return callMs_[kScanExtract]; }

  // ---- compare (zra_compare.hip): the maximal runs of content positions of [offset, offset + size) (size ~0: to the end of the common
  // content) at which the archives at dA and dB differ, ascending, as {offset, size} pairs in hRanges. A frame whose compressed bytes are
  // the same in both archives is equal without a decode (mode 1: every frame is decoded); the others are decoded whole on both sides, a
  // staging window of two halves at a time, and compared on the device. Statuses and their order: zra_hip.h, ZraHipCompareArchives.
  Status compare_archives(const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode, uint64_t offset, uint64_t size,
                          size_t stagingBytes, uint64_t* hRanges, size_t rangeCap, uint64_t* nRanges, uint64_t* differingBytes);
  // the last compare_archives: {frames of the range, equal by compressed bytes, frame pairs decoded, content bytes compared after decode,
  // ranges, ranges listed, passes, 0}; all zero unless it succeeded. compare_sizes: the two content sizes, likewise
  void compare_stats(uint64_t out[8]) const { call_stats(kCallCompare, out); }
  void compare_sizes(uint64_t out[2]) const { out[0] = cmpSizes_[0]; out[1] = cmpSizes_[1]; }
  // bring-up: HIP-event time of the last compare's own launches (spans, jobs, count, scan, fill), summed over its passes
  double compare_ms() const { return callMs_[kCallCompare]; }

  // ---- diff (zra_compare.hip): the patch that turns the content of the archive at dA into that of the archive at dB, in the shape
  // update_archive takes: the maximal runs of dirty grains of [0, UA) as writes in three host arrays, B's bytes of those runs packed
  // at dData, B's content behind UA after them. One pass over both archives, the compare's. Statuses and their order: zra_hip.h,
  // ZraHipDiffArchives.
  Status diff_archives(const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode, uint32_t grain, size_t stagingBytes,
                       uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap,
                       uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize);
  // the last diff_archives: {frames of [0, C), equal by compressed bytes, frame pairs decoded, tail frames of B decoded, writes, dirty
  // bytes, passes (pair + tail), dirty grains}; all zero unless it succeeded
  void diff_stats(uint64_t out[8]) const { call_stats(kCallDiff, out); }
  // bring-up: HIP-event time of the last diff's own launches (spans, jobs, count, scan, fill, tail jobs, tail copy), summed over its passes
  double diff_ms() const { return callMs_[kCallDiff]; }

  // ---- content signatures (zra_sign.hip): XXH64 words of the archive at dArc, a record of 1 + ceil(frameSize / grain) words per frame
  // (the frame's compressed span, then its grains as the diff cuts them), written into the records of frames [first, first + count) of
  // dSig. info6 = ZraHipSignature's six words {content size, frame size, grain, seed, frames, words}, of the WHOLE archive. Statuses
  // and their order: zra_hip.h, ZraHipSignArchive.
  Status sign_archive(const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count, size_t stagingBytes,
                      uint64_t* dSig, size_t sigCapWords, uint64_t info6[6]);
  // the last sign_archive: {frames of the archive, frames signed, grain words written, content bytes hashed, compressed bytes hashed,
  // passes, 0, 0}; all zero unless it succeeded
  void sign_stats(uint64_t out[8]) const { call_stats(kCallSign, out); }
  // bring-up: HIP-event time of the last sign's own launches (span hash, grain hash), summed over its passes
  double sign_ms() const { return callMs_[kCallSign]; }
  // The diff of archive B against the SIGNATURE of an archive A that lies elsewhere: diff_archives' outputs at grain sig6[2], a grain
  // dirty when its word differs. sig6: ZraHipSignature's six words; dSigA: its words. Statuses and their order: zra_hip.h,
  // ZraHipDiffSignature.
  Status diff_signature(const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
                        uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap,
                        uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize);
  // the last diff_signature, in diff_stats' shape: {frames of [0, C), equal by their frame word, decoded, tail frames decoded, writes,
  // dirty bytes, passes, dirty grains}; all zero unless it succeeded
  void diff_signature_stats(uint64_t out[8]) const { call_stats(kCallSigDiff, out); }
  double diff_signature_ms() const { return callMs_[kCallSigDiff]; }

  // ---- record index (zra_records.hip): one 64-bit word per frame, bits 0..62 the delimiter bytes of the frame's content, bit 63 set iff
  // its last content byte is not the delimiter. index_records writes the words of frames [first, first + count) into their places in
  // dIndex; info6 = ZraHipRecordIndex's six words {content size, frame size, delimiter, frames, delimiters, records}, the totals from
  // all F words as they lie in dIndex. Statuses and their order: zra_hip.h, ZraHipIndexRecords.
  // cv (here and in the two calls below; a call through an archive handle, zra_archive.hip): the handle's header, and, with slots, the
  // resident frames a whole-frame sweep needs are staged from the arena; dIndex / dData must not overlap the arena either
  Status index_records(const uint8_t* dArc, size_t arcSize, uint32_t delimiter, uint64_t first, uint64_t count, size_t stagingBytes, uint64_t* dIndex,
                       size_t indexCapWords, uint64_t info6[6], ScanCacheView* cv = nullptr);
  // the last index_records: {frames, frames indexed, content bytes scanned, delimiters in the range, passes, 0, 0, 0}; all zero unless it succeeded
  void index_records_stats(uint64_t out[8]) const { call_stats(kCallIndex, out); }
  // bring-up: HIP-event time of the last index's own launches (count, frame words, totals), summed over its passes
  double index_records_ms() const { return callMs_[kCallIndex]; }
  // hRanges[i] = {start, size} of record hNumbers[i], in request order; only the frames that hold a boundary are decoded, and each is
  // checked against its word. Statuses and their order: zra_hip.h, ZraHipLocateRecords.
  Status locate_records(const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n,
                        size_t stagingBytes, uint64_t* hRanges, ScanCacheView* cv = nullptr);
  // the last locate_records: {frames, records asked, boundaries looked up, frames decoded, content bytes regenerated, passes, 0, 0};
  // through a handle "decoded" and "regenerated" count the decode jobs and leave out the frames staged from its arena
  void locate_records_stats(uint64_t out[8]) const { call_stats(kCallLocate, out); }
  // bring-up: HIP-event time of the last locate's own launches (prefix, bounds, jobs, count, frame check, select), summed over its passes
  double locate_records_ms() const { return callMs_[kCallLocate]; }
  // locate_records, then the records' bytes packed at dData in request order, each followed by one delimiter byte (the packing of
  // extract_records); hRanges is optional. Statuses and their order: zra_hip.h, ZraHipReadRecords.
  Status read_records(const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n,
                      size_t stagingBytes, uint64_t* hRanges, uint8_t* dData, size_t dataCap, uint64_t* dataSize, ScanCacheView* cv = nullptr,
                      const RecordFetch* fetch = nullptr);
  // the last read_records: {frames, records, packed bytes, frames decoded by the locate sweep, decode jobs of the read sweep, locate passes, 0, 0}
  void read_records_stats(uint64_t out[8]) const { call_stats(kCallRead, out); }
  // bring-up: HIP-event time of the last read's locate-sweep launches, summed over its passes (its read sweep: kernel_stats)
  double read_records_ms() const { return callMs_[kCallRead]; }

  // ---- tally (zra_tally.hip): the distinct records of textSize bytes of packed text at dText (device memory), cut at `delimiter`, in
  // order of first appearance, as {offset, size, count} triples in hEntries and as text at dKeys (device memory), each key followed by
  // one delimiter byte. A record longer than kTallyMaxKey is skipped. Statuses and their order: zra_hip.h, ZraHipTallyRecords.
  Status tally_records(const uint8_t* dText, size_t textSize, uint32_t delimiter, uint64_t maxDistinct, uint64_t* hEntries, size_t entryCap, uint8_t* dKeys, size_t keyCap,
                       uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize);
  // the last tally_records: {records, distinct keys, skipped records, key bytes, table slots, longest probe, inserts into the table in
  // HBM, 0}; all zero unless it succeeded. Words 5 and 6 depend on the order in which lanes arrive; nothing else does
  void tally_stats(uint64_t out[8]) const { call_stats(kCallTally, out); }
  // bring-up: HIP-event time of the last tally's own launches (count, insert, mark, sum, scan, emit, copy)
  double tally_ms() const { return callMs_[kCallTally]; }
  void tally_clear();                        // the row as a failed tally leaves it (the composite, when its cut fails)
  // bring-up (ZraHipDebugTallyHashBits): the bits of the key hash the next tallies keep; ~0: all
  void set_tally_keep(uint64_t mask) { tallyKeep_ = mask; }

  // ---- host-pointer helpers (H2D -> kernels -> D2H) behind the reference-compatible C/C++ API (zra_hostpipe.hip; compress_frames_host: zra_encode.hip)
  Status compress_host(const uint8_t* hIn, size_t n, uint8_t* hOut, size_t* outSize, int level, uint32_t frameSize, bool checksum);
  Status compress_frames_host(const uint8_t* hIn, size_t n, uint8_t* hBody, std::vector<uint64_t>& sizes, size_t* bodySize,
                              int level, uint32_t frameSize, bool checksum);
  // frames given as (start,end) pairs inside hSpan; frame i regenerates min(frameSize, total - i*frameSize) bytes;
  // bytes [skip, skip+size) of the concatenated output are returned in hOut
  Status decode_host(const uint8_t* hSpan, size_t spanSize, const std::vector<uint64_t>& starts, const std::vector<uint64_t>& ends,
                     uint32_t frameSize, uint64_t total, uint8_t* hOut, size_t skip, size_t size, bool wholeArchive = false);
  // whole archive in ~1 GiB chunks, copies beside the kernels (zra_hostpipe.hip); *fallBack: a frame failed, take decode_host
  Status decode_host_pipelined(const uint8_t* hSpan, const std::vector<uint64_t>& starts, const std::vector<uint64_t>& ends,
                               uint32_t frameSize, uint64_t total, uint8_t* hOut, bool* fallBack);

  // batched random access: false (default) = a frame is decoded up to the last byte a query needs, so damage behind that byte
  // and the frame's content checksum go unnoticed; true = whole frames + checksums, the reference's error behaviour
  void set_ra_verify_whole_frames(bool on) { raVerifyWholeFrames_ = on; }
  bool ra_verify_whole_frames() const { return raVerifyWholeFrames_; }
  int device() const { return device_; }
  int num_cus() const { return numCUs_; }

 private:
  Engine() = default;
  int device_ = 0, numCUs_ = 0;
  hipStream_t stream_ = nullptr;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr, evWait_ = nullptr;
  double lastKernelMs_ = 0;
  std::vector<uint64_t> mfTele_;
  const uint64_t* mfTeleDev_ = nullptr;   // the last persistent launch's telemetry block on the device (inside encScan_), not fetched yet; nullptr: none / fetched
  double kstats_[6] = {0, 0, 0, 0, 0, 0};
  double dstats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<hipEvent_t> stageEv_; size_t stageEvNext_ = 0;
  hipEvent_t stage_event();
  // one parse -> Huffman -> chain -> execute sequence on stream_ between the stage events it hands back in se[]: nJobs sizes the grids
  // of the two middle stages and `mid` is their argument block, nFrames and `a` those of parse and execute (blockPass: the _all kernels)
  Status launch_stages(uint64_t nJobs, const struct ZraDecodeArgs& a, const struct ZraDecodeArgs& mid, uint32_t nFrames, bool blockPass, hipEvent_t se[5]);
  Status launch_chain(uint64_t nJobs, const struct ZraDecodeArgs& mid, hipEvent_t after);
  Status decode_sequential_tail(const struct ZraDecodeArgs& a, const uint64_t* dFrameOff, uint32_t offStride, const uint64_t* dOutOff, uint32_t first,
                                uint32_t nFrames, uint32_t maxFrameBytes, uint64_t seqTotal);
  // job arrays built on the host -> frameOff_ / outOff_ / expect_; synchronises (the host arrays may go out of scope)
  Status upload_jobs(const std::vector<uint64_t>& frameOff, const std::vector<uint64_t>& outOff, const std::vector<uint32_t>& expect);
  Status read_fixed_header(const uint8_t* dArc, size_t arcSize, HeaderInfo* h);   // copy-back + parse_fixed_header + the two size checks
  uint64_t* pinned_tuples(size_t nTuples);   // pinQ_ grown to 4 words per tuple; nullptr: no memory
  void reset_decode_stats() { kstats_[4] = kstats_[5] = 0; for (auto& d : dstats_) d = 0; }
  // milliseconds between two recorded and completed events; 0 (and the runtime's error cleared) when they cannot be had
  static float elapsed_ms(hipEvent_t e0, hipEvent_t e1) { float ms = 0; if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { ms = 0; (void)hipGetLastError(); } return ms; }
  bool call_events() {                       // evCall_ created on first use; false: the runtime refused (error cleared)
    for (auto& ev : evCall_) if (!ev && hipEventCreate(&ev) != hipSuccess) { ev = nullptr; (void)hipGetLastError(); return false; }
    return true;
  }
  void free_scratch();                       // every DevBuf of the engine handed back: release_scratch() and the destructor
  void call_stats(int which, uint64_t out[8]) const { for (int i = 0; i < 8; i++) out[i] = callStats_[which][i]; }
  hipEvent_t evR_[17] = {nullptr};   // per-round events of one encode batch: e[2r] before mf, e[2r+1] between, e[2r+2] after entropy
  // decode scratch
  DevBuf decFrames_, decTables_, decLists_, decCounters_, decLits_, decSeqs_, roundN_;
  DevBuf decBlkRecs_, decBlkTables_, decBlkLists_;   // block-parallel pass (frames of several blocks): per-block records, tables, job lists
  DevBuf raPlan_, raLimit_, raPieceBase_, raPieces_;
  uint8_t* pinSmall_ = nullptr;             // page-locked staging of small host-pointer decodes (decode_host: job arrays + compressed span in, answer out)
  uint64_t* pinQ_ = nullptr; size_t pinQCap_ = 0;   // page-locked query tuples of the running batch (host side of an asynchronous copy)
  int decOccParse_ = 0, decOccExec_ = 0, decOccHuf_ = 0; // resident workgroups per CU of the parse / execute kernels
  bool raVerifyWholeFrames_ = false;     // batched random access decodes every touched frame in full and checks its checksum
  DevBuf status_, produced_, frameMeta_, frameOff_, outOff_, expect_, result_, qmeta_;
  // THE plaintext staging window of the device-archive calls (batch, update, verify, search, multi-pattern search, grep, extract, compare,
  // diff, sign, signature diff): whole frames of one decode pass, slot s at s * frameSize; the range scans keep their carry area in
  // front of slot 0 (zra_scan.h), the compare and the diff two halves of slots (zra_pass_plan.h: pair_half). Every engine call runs on
  // stream_ and returns synchronised, so one window is live at a time. THE RULE: a call reserves the window once, before it takes a
  // pointer into it (reserve may move the buffer), and from there to its last use calls nothing that reserves it. decode_jobs /
  // decode_pass / staged_pass and compress_frames do not (decoder and encoder scratch). The handle's read and update call ra_batch_body
  // / update_archive, which do, but hold no window then. The calls on whole frames reserve it, and their tables (fp_, under the same
  // rule), in one place: FramePasses::open (zra_framepass.h).
  DevBuf stage_;
  // encode scratch (see zra_encode.hip)
  struct EncCtx { DevBuf tables, seqs, lits, work, slots, misc, ck, sizes, rec; };   // rec: the split entropy stage's per-frame records (ZraEntRec)
  EncCtx encCtx_[2];
  DevBuf encScan_;
  DevBuf mfFlags_;                         // bucket-flag masks of the dfast match finder: one slot per resident wave (df_later_flags)
  int lsAttr_ = 0;                  // zra_mf_dfast_ls_kernel's dynamic LDS limit raised: 1 yes, -1 refused
  hipStream_t stream2_ = nullptr;          // entropy stage / gather stream (overlaps the match finder on stream_)
  bool decCountersClean_ = false;          // the decoder's round counters are known to be zero (zeroed behind the last one-launch decode)
  int chainLdsAttr_ = 0;                   // zra_dec_chain_lds_kernel's dynamic LDS size: 0 not asked yet, 1 granted, -1 refused
  hipStream_t pipeStreams_[2] = {nullptr, nullptr};   // side streams: [0] the encoder batch path's second match-finder stream, [1] the decoder's LDS-table chain kernel
  std::vector<hipEvent_t> evPool_;
  DevBuf hostIn_, hostOut_, seqScratch_;
  uint64_t dbgSeqStride_ = 0; uint32_t dbgB_ = 0;
  uint64_t lastProducedTotal_ = ~0ull;     // whole-archive decode that fell back to the sequential tail: bytes actually regenerated
  void* encCounters_ = nullptr; size_t encCountersBytes_ = 0;   // sub-batch counters stream B may be waiting on (drain_after_error)
  int waitValueOk_ = 0;                    // 0 unknown, 1 hipStreamWaitValue32 works on device memory, -1 it does not (batch path)
  // update scratch (zra_update.hip): per-frame plan words, the packed newly encoded frames, their sizes,
  // the per-frame sizes / offsets / source displacements, the new seek table, the frames staged from a handle's cache (4 words each)
  struct UpdScratch { DevBuf plan, packed, encSizes, frames, table, copies; } upd_;
  uint64_t ustats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // around a pass's stage-from-cache kernel (update through a handle), own launches (the range scans; compare, diff, sign, signature diff
  // and index: zra_framepass.h, (time); the locate sweep); they never run inside each other.
  // [2] .. [3] and [4] .. [5]: a range scan or a record call through a handle, around a pass's job split and around its stage-from-cache
  // kernel (zra_scan.h, zra_framepass.h, zra_records.hip)
  hipEvent_t evCall_[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double updStageMs_ = 0;
  // verify scratch (zra_verify.hip): per-frame structure codes and job numbers + totals, the fault list
  struct VerifyScratch { DevBuf plan, faults; } vfy_;
  // range-scan scratch (zra_scan.h: search, multi-pattern search, grep, extract): the call's pattern table + totals + per-tile tables
  // (each call its own layout, uploaded before its first launch), its list. One pair: a call returns synchronised, so one is live at a
  // time
  struct ScanScratch { DevBuf tables, list; } scan_;
  // The counters and the HIP-event time of the own launches of every device-archive call, a row per call (kScanSearch .. kCallVerify),
  // written through entry_call (zra_host.h): a call touches its own row and no other. The verify has no milliseconds
  uint64_t callStats_[kCalls][8] = {};
  double callMs_[kCalls] = {};
  uint64_t cmpSizes_[2] = {0, 0};          // the two content sizes of the last compare
  // frame-pass scratch (zra_framepass.h: compare, diff, sign, signature diff): a decode flag per slot, a dirty flag per grain of a pass
  // (signature diff), the call's header words + per-item table, the starts and ends of the listed ranges or writes. One group: a call
  // returns synchronised, so one is live at a time (THE RULE of stage_)
  struct FramePassScratch { DevBuf flags, dirty, tables, list; } fp_;
  // record index (zra_records.hip): the header words + frame counts, prefix, slots and tile prefixes of a call; the record numbers,
  // boundaries and positions of a locate
  struct RecScratch { DevBuf tables, ranges; } rec_;
  // tally (zra_tally.hip): the call's words; the tiles' table, the two bitmaps of the text's positions and the hash table; the entries
  struct TallyScratch { DevBuf hdr, tables, entries; } tally_;
  uint64_t tallyKeep_ = ~0ull;
  friend struct EncodeImpl;
  friend struct UpdateImpl;        // the update drives the walk's pinned tuples, the decoder's job arrays and the encoder (zra_update.hip)
  friend struct VerifyImpl;        // the verifier drives the decoder's job arrays and reads its per-job status words (zra_verify.hip)
  friend struct ScanImpl;          // the range scans drive the decoder's job arrays as the verifier does (zra_scan.h, zra_record_scan.h and the seven calls' files)
  friend struct FramePasses;       // the one pass driver of compare, diff, sign, signature diff and index: scratch, job arrays, call events (zra_framepass.h)
  friend struct RecordsImpl;       // the locate sweep drives the decoder's job arrays of the needed frames on its own (zra_records.hip)
  friend struct TallyImpl;         // the tally uses the call events (zra_tally.hip)
  friend class ArchiveCache;       // the archive handle drives the random-access scratch and the decoder of its engine (zra_archive.hip)
};

// The range scans' per-pass steps that do not depend on the pattern, launched on stream s (zra_search.hip; the driver in zra_scan.h
// makes the first and the third for all seven calls, the multi-pattern search shares the second; the frame-pass driver, zra_framepass.h,
// makes the first for its plain passes): the decode jobs of frames [first, first + n) into slots 0 .. n - 1; bases[t] = *cntIn + the counts in front of item
// t, *cntOut = *cntIn + all of them; the last n bytes of the run win[.., L) moved to win[-n, 0), n <= 255.
void search_launch_jobs(hipStream_t s, const uint8_t* table, uint64_t fs, uint64_t total, uint64_t first, uint32_t n, uint64_t* frameOff, uint64_t* outOff,
                        uint32_t* expect);
// A pass of a range scan through a handle (zra_scan.h): frames [first, first + n) split by residency (zra_joblist.h,
// split_by_residency) into decode jobs and copy entries of 4 words, counts = {jobs, copies, bytes the jobs regenerate (2 words)};
// and the copy entries [0, n) staged from the arena, entry slot e[0] to stage + (e[0] - s0) * fs (zra_update.hip, the update's
// zra_upd_stage_cached_kernel).
void scan_launch_split(hipStream_t s, const uint32_t* slotOf, uint32_t nFrames, const uint8_t* table, uint64_t fs, uint64_t total, uint64_t first, uint32_t n,
                       uint64_t* frameOff, uint64_t* outOff, uint32_t* expect, uint32_t* copies, uint32_t* counts);
void upd_launch_stage_cached(hipStream_t s, const uint32_t* copies, uint32_t n, uint32_t s0, uint64_t fs, const uint8_t* arena, uint8_t* stage);
void search_launch_scan(hipStream_t s, const uint32_t* counts, uint32_t nItems, uint64_t* bases, const uint64_t* cntIn, uint64_t* cntOut);
void search_launch_carry(hipStream_t s, uint8_t* win, uint64_t L, uint32_t n);
// The diff's steps that do not depend on how a grain became dirty (zra_compare.hip; the signature diff shares them): the three-column
// scan of zra_diff_scan_kernel over tab[3 * (nItems + 1)], and the tail copy of zra_diff_tail_kernel.
void diff_launch_scan(hipStream_t s, uint64_t* tab, uint32_t nItems, const uint64_t* totIn, uint64_t* totOut);
void diff_launch_tail(hipStream_t s, const uint8_t* src, uint64_t n, const uint64_t* dirtyBytes, uint64_t tailOff, uint8_t* dData, uint64_t dataCap);

}  // namespace zra_eng
