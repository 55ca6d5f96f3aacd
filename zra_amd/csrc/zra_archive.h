// zra_amd — archive handle: a device-resident archive opened once (header parsed a single time) with a cache of whole decoded frames
// in an HBM arena of its own (zra_hip.h: ZraHipArchive*). The engine's streams and decoder do the work; zra_archive.hip.
#pragma once
#include "zra_engine.h"

namespace zra_eng {

class ArchiveCache {
 public:
  // the archive checks of ZraHipDecompressRABatch; slots = min(cacheBytes / frameSize, frames); memory_allocation (64) when the arena
  // or the tables cannot be had (nothing is kept then)
  static Status open(Engine* e, const uint8_t* dArc, size_t arcSize, size_t cacheBytes, ArchiveCache** out);
  ~ArchiveCache();
  // query i: bytes [hOff[i], hOff[i] + hSize[i]) of the content at dOut + hOutOff[i]; wholeFramesOpt: the process-wide
  // ZRA_HIP_OPT_RA_WHOLE_FRAMES (what a handle without slots follows, like the batch call)
  // endInclusive (internal, the record read alone): a query may end AT the content's end; *jobsOut (optional): the frames the read decoded
  Status read(uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool wholeFramesOpt, bool endInclusive = false,
              uint32_t* jobsOut = nullptr);
  // forget every resident frame (the cumulative counters stay)
  Status drop();
  // {slots, resident, reads, hits, misses, evictions, uncompressed size, frame size}
  void stats(uint64_t out[8]) const;
  // Engine::update_archive of the archive the handle is bound to, old plaintext taken from the arena where it is resident; on Success
  // the handle serves the archive at dOut and every resident frame holds its new content (zra_hip.h: ZraHipArchiveUpdate). On any other
  // status nothing has changed.
  Status update(const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hDataOff, size_t nw, const uint8_t* dAppend,
                size_t appendSize, uint8_t* dOut, size_t outCap, size_t* outSize, int level, bool checksum);
  // {updates accepted, frames now, archive size now, staged from the cache (last update), resident frames refreshed (last), staged
  // (cumulative), refreshed (cumulative), 0}
  void update_stats(uint64_t out[8]) const;
  // The range scans of the engine (zra_scan.h) on the archive the handle is bound to: a pass copies its resident frames out of the
  // arena and decodes the others (zra_hip.h: ZraHipArchiveSearch .. ZraHipArchiveExtractRecords). A scan is not a read: it changes
  // nothing of the cache and none of stats()' words, on any status.
  Status search(const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hMatches, size_t matchCap, uint64_t* nMatches);
  Status search_multi(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint64_t offset, uint64_t size, size_t stagingBytes, void* hMatches,
                      size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern);
  // Engine::record_scan of c with the handle's archive in place of c.dArc / c.arcSize: the five record scans
  Status record_scan(RecordCall c);
  // {scans accepted, frames staged from the cache (last accepted scan), frames decoded (last), passes (last), staged (cumulative),
  // decoded (cumulative), 0, 0}
  void scan_stats(uint64_t out[8]) const;
  // bring-up: HIP-event time of the last accepted scan's job-split and stage-from-cache launches, summed over its passes (0: none ran)
  double scan_stage_ms() const { return scanStageMs_; }
  // bring-up: where the arena lies, [*base, *base + *bytes); nullptr and 0 for a handle without a cache
  void arena_range(const void** base, size_t* bytes) const { *base = arena_; *bytes = arena_ ? (size_t)slots_ * h_.frameSize : 0; }
  // the composite calls (ZraHipArchiveTallyFields): the engine the handle runs on, and where the archive it serves lies
  Engine* engine() const { return e_; }
  void archive_range(const void** base, size_t* bytes) const { *base = dArc_; *bytes = arcSize_; }
  // The record calls of the engine (zra_records.hip) on the archive the handle is bound to (zra_hip.h: ZraHipArchiveIndexRecords,
  // ZraHipArchiveLocateRecords, ZraHipArchiveReadRecords): a whole-frame sweep copies the resident frames it needs out of the arena and
  // decodes the others. Index and locate are not reads: they change nothing of the cache and none of stats()' words, on any status. The
  // read's byte fetch is one: read() of the located ranges, with the inclusive end bound.
  Status index_records(uint32_t delimiter, uint64_t first, uint64_t count, size_t stagingBytes, uint64_t* dIndex, size_t indexCapWords, uint64_t info6[6]);
  Status locate_records(const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n, size_t stagingBytes, uint64_t* hRanges);
  Status read_records(const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n, size_t stagingBytes, uint64_t* hRanges,
                      uint8_t* dData, size_t dataCap, uint64_t* dataSize);
  // {record calls accepted, frames staged from the cache by the last accepted call's whole-frame sweep, frames decoded by it, its passes,
  // staged (cumulative), decoded (cumulative), 0, 0}
  void record_stats(uint64_t out[8]) const;
  // bring-up: HIP-event time of the last accepted record call's job-split and stage-from-cache launches, summed over its passes (0: none ran)
  double record_stage_ms() const { return recStageMs_; }

 private:
  ArchiveCache() = default;
  static const uint32_t* update_table(void* ctx, uint32_t frames);   // UpdCacheView::table
  ArchiveView view() const { return ArchiveView::over(h_, dArc_, arcSize_); }   // the archive the handle serves now, its header checked at open / by the update
  ScanCacheView scan_view() const;                  // what a scan borrows: header, arena, table, the pinned count words
  Status scanned(Status st, const ScanCacheView& v); // the scan counters, kept when the scan was accepted
  Status recorded(Status st, const ScanCacheView& v); // the record counters, kept when the call was accepted
  Status read_cached(uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool endInclusive, uint32_t* jobsOut);
  Engine* e_ = nullptr;
  const uint8_t* dArc_ = nullptr;
  size_t arcSize_ = 0;
  HeaderInfo h_{};
  uint32_t nFrames_ = 0, slots_ = 0, maxPass_ = 0;
  // device state, one allocation: frameOf[slots] | victim[maxPass] (u32) | ref[slots] (u8) | hand (u32) + counters (u64)
  void* state_ = nullptr;
  uint8_t* arena_ = nullptr;            // slots x frameSize
  // frame -> slot, kNone when not resident. An allocation of its own: it grows with the archive (update), slotCap_ entries, those
  // behind nFrames_ always kNone
  uint32_t* slotOf_ = nullptr;
  size_t slotCap_ = 0;
  uint32_t* grown_ = nullptr;           // a larger table made for the running update, not yet swapped in
  size_t grownCap_ = 0;
  uint32_t* frameOf_ = nullptr;         // slot -> frame, kEmpty when free
  uint32_t* victim_ = nullptr;          // the slots the current read decodes into
  uint8_t* ref_ = nullptr;              // CLOCK reference bit (2: claimed by the running read)
  uint32_t* hand_ = nullptr;
  unsigned long long* dctr_ = nullptr;  // {evictions, resident}
  uint64_t* pin_ = nullptr;             // page-locked read-back words
  uint64_t reads_ = 0, hits_ = 0, misses_ = 0, evictions_ = 0, resident_ = 0;
  uint64_t scans_ = 0, scanLast_[3] = {0, 0, 0}, scanStagedTotal_ = 0, scanDecodedTotal_ = 0;
  double scanStageMs_ = 0;
  uint64_t recCalls_ = 0, recLast_[3] = {0, 0, 0}, recStagedTotal_ = 0, recDecodedTotal_ = 0;
  double recStageMs_ = 0;
  uint64_t updates_ = 0, stagedLast_ = 0, refreshedLast_ = 0, stagedTotal_ = 0, refreshedTotal_ = 0;
};

}  // namespace zra_eng
