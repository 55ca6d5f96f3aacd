// zra_amd — host engine: owns one HIP device, one stream and a grow-only scratch pool, and drives the
// decode / encode kernels. Internal C++ interface used by the C ABI (zra_capi.cpp) and zra_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "zra_kernels.h"

namespace zra_eng {

struct Status { int zra; int zstd; };   // mirrors ZraStatus (kept free of the public header here)
enum : int { kSuccess = 0, kZStdError = 1, kVersionLow = 2, kHeaderInvalid = 3, kHeaderIncomplete = 4, kOutOfBounds = 5,
             kOutputTooSmall = 6, kCompressedTooLarge = 7, kFrameSizeMismatch = 8 };
inline Status ok() { return {kSuccess, 0}; }
inline Status zerr(int code) { return {kZStdError, (int)(int8_t)code}; }   // i8 narrowing like zra.cpp:440

// grow-only device allocation
struct DevBuf {
  void* p = nullptr; size_t cap = 0;
  bool reserve(size_t n);
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
  // pieces of the batch, shared with the archive handle (zra_archive.hip): the header read + checks, the walk over the host query
  // arrays (bounds, tuples uploaded to the device), the planner of the decode jobs, and the batch behind an already checked header
  Status ra_header(const uint8_t* dArc, size_t arcSize, HeaderInfo* h);
  Status ra_walk_queries(const HeaderInfo& h, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, uint64_t* maxPieces);
  Status ra_plan_fill(uint32_t* plan, size_t nq, uint32_t nFrames, const uint8_t* table, uint64_t bodyBase, uint64_t fs, uint64_t U,
                      uint32_t passSlots, bool fullFrames, const uint32_t* victim, uint32_t totals[2]);
  Status ra_batch_body(const uint8_t* dArc, const HeaderInfo& h, const uint8_t* dBody, uint64_t bodyBytes, uint64_t bodyBase, uint8_t* dOut,
                       const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq);
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
                             uint64_t tableWords, uint64_t seqStride, uint64_t litStride, uint64_t slotStride);
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
  void verify_stats(uint64_t out[8]) const { for (int i = 0; i < 8; i++) out[i] = vstats_[i]; }

  // ---- search (zra_search.hip): every content offset p of [offset, offset + size) (size ~0: to the end) at which the patternSize host
  // bytes at hPattern occur whole inside the range, ascending. Only the frames of the range are decoded, whole, a staging window at a
  // time; the window's plaintext is scanned on the device. Statuses and their order: zra_hip.h, ZraHipSearchArchive.
  Status search_archive(const uint8_t* dArc, size_t arcSize, const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size,
                        size_t stagingBytes, uint64_t* hMatches, size_t matchCap, uint64_t* nMatches);
  // the last search_archive: {frames, decoded, content bytes regenerated, matches, matches listed, passes, 0, 0}; all zero unless it succeeded
  void search_stats(uint64_t out[8]) const { for (int i = 0; i < 8; i++) out[i] = sstats_[i]; }
  // bring-up: HIP-event time of the last search's scan launches (count, scan, fill, carry), summed over its passes
  double search_scan_ms() const { return searchScanMs_; }

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
  void free_scratch();                       // every DevBuf of the engine handed back: release_scratch() and the destructor
  hipEvent_t evR_[17] = {nullptr};   // per-round events of one encode batch: e[2r] before mf, e[2r+1] between, e[2r+2] after entropy
  // decode scratch
  DevBuf decFrames_, decTables_, decLists_, decCounters_, decLits_, decSeqs_, roundN_;
  DevBuf decBlkRecs_, decBlkTables_, decBlkLists_;   // block-parallel pass (frames of several blocks): per-block records, tables, job lists
  DevBuf raPlan_, raLimit_, raPieceBase_, raPieces_;
  uint8_t* pinSmall_ = nullptr;             // page-locked staging of small host-pointer decodes (decode_host: job arrays + compressed span in, answer out)
  uint64_t* pinQ_ = nullptr; size_t pinQCap_ = 0;   // page-locked query tuples of the running batch (host side of an asynchronous copy)
  int decOccParse_ = 0, decOccExec_ = 0, decOccHuf_ = 0; // resident workgroups per CU of the parse / execute kernels
  bool raVerifyWholeFrames_ = false;     // batched random access decodes every touched frame in full and checks its checksum
  DevBuf status_, produced_, frameMeta_, frameOff_, outOff_, expect_, result_, temp_, qmeta_;
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
  // update scratch (zra_update.hip): per-frame plan words, plaintext staging of one pass, the packed newly encoded frames, their sizes,
  // the per-frame sizes / offsets / source displacements, the new seek table, the frames staged from a handle's cache (4 words each)
  struct UpdScratch { DevBuf plan, stage, packed, encSizes, frames, table, copies; };
  UpdScratch upd_;
  uint64_t ustats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t evUpd_[2] = {nullptr, nullptr};   // around a pass's stage-from-cache kernel (created by the first update through a handle)
  double updStageMs_ = 0;
  // verify scratch (zra_verify.hip): per-frame structure codes and job numbers + totals, the staging window of one decode pass, the fault list
  struct VerifyScratch { DevBuf plan, stage, faults; };
  VerifyScratch vfy_;
  uint64_t vstats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // search scratch (zra_search.hip): the carry area + staging window of one decode pass, the pattern + match count + per-tile tables,
  // the match list
  struct SearchScratch { DevBuf stage, tables, list; };
  SearchScratch srch_;
  uint64_t sstats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t evSearch_[2] = {nullptr, nullptr};   // around a pass's scan launches (created by the first search)
  double searchScanMs_ = 0;
  friend struct EncodeImpl;
  friend struct UpdateImpl;        // the update drives the walk's pinned tuples, the decoder's job arrays and the encoder (zra_update.hip)
  friend struct VerifyImpl;        // the verifier drives the decoder's job arrays and reads its per-job status words (zra_verify.hip)
  friend struct SearchImpl;        // the search drives the decoder's job arrays as the verifier does (zra_search.hip)
  friend class ArchiveCache;       // the archive handle drives the random-access scratch and the decoder of its engine (zra_archive.hip)
};

}  // namespace zra_eng
