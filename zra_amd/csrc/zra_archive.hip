// zra_amd — archive handle with a cache of decoded frames (zra_archive.h, zra_hip.h: ZraHipArchive*).
//
// A read whose frames are all resident costs the query upload, ONE launch (zra_cache_lookup_kernel: every slice of a resident frame
// is copied out of the arena, every other frame is counted as a miss) and one 8-byte read-back. Misses go through the batch's own
// planner and decoder, whole frames, into arena slots chosen by CLOCK (zra_cache_victims_kernel), and are published by
// zra_cache_commit_kernel once they have decoded cleanly.
//
// Ordering conditions of a read (all on the engine's stream):
//  (a) hit or miss is decided ONCE per frame, by the lookup kernel, before anything in the read changes slotOf. The planner and the
//      fill kernel go by that snapshot (RaPlan::cnt != 0), never by slotOf: a frame hit earlier in the read and evicted as a victim
//      afterwards has no job, and must get no piece.
//  (b) the lookup kernel (every hit copy) runs before the victims kernel and the decoder: no hit can read a slot that is being
//      overwritten.
//  (c) a frame is mapped (slotOf / frameOf) only by the commit kernel, after its decode pass: no lookup can find a half-decoded slot.
#include "zra_archive.h"
#include "zra_scan.h"
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include "zra_kernels.h"
#include <algorithm>
#include <cstring>
#include <vector>

using namespace zra_dev;

namespace {
constexpr u32 kNone = 0xFFFFFFFFu;    // slotOf: the frame is not resident
constexpr u32 kEmpty = 0xFFFFFFFFu;   // frameOf: the slot holds no frame
constexpr u8 kClaimed = 2;            // ref: the slot is being decoded into by the running read (neither a victim again nor skipped)
constexpr u32 kMaxPass = 1u << 16;    // frames of one decode pass: well inside one internal pass of Engine::decode_jobs (>= 128 Ki frames)

}  // namespace

// Wave per slice (slice = the part of a query inside one frame; q[4i + 3] = the first slice of query i, as the batch's direct kernel
// reads it). Resident frame: the slice is copied from the arena to out and the slot's reference bit set; the frame counts as a hit
// once (seen[]). Otherwise the slice is counted into cnt[f] (the planner's piece count) and the frame as a miss once.
// words[0] = distinct missed frames, words[1] = distinct hit frames.
extern "C" __global__ void __launch_bounds__(256) zra_cache_lookup_kernel(const u64* q, u32 nq, u64 nSlices, u64 fs, const u32* slotOf, u8* ref,
                                                                        const u8* arena, u8* out, u32* cnt, u32* seen, u32* words) {
  const int lane = (int)(threadIdx.x & 63);
  for (u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); s < nSlices; s += (u64)gridDim.x * 4) {
    const Slice c = slice_of(q, nq, s, fs);
    const u64 f = c.frame;
    const u32 v = slotOf[f];
    if (v != kNone) {
      copy_slice(out + c.user, arena + (u64)v * fs + c.inFrame, c.len, lane);
      if (lane == 0) {
        if (!ref[v]) ref[v] = 1;
        if (atomicExch(&seen[f], 1u) == 0) atomicAdd(&words[1], 1u);
      }
    } else if (lane == 0) {
      if (atomicAdd(&cnt[f], 1u) == 0) atomicAdd(&words[0], 1u);
    }
  }
}

// One workgroup. reuse == 0: CLOCK from *hand — a slot whose reference bit is set has it cleared and is passed over, an empty slot or one
// with a clear bit becomes the next victim, until V are chosen; the hand stops behind the last. reuse != 0: the V slots in victim[]
// again (a later decode pass of the same read). Either way every victim's frame is unmapped (counted as an eviction) and the slot
// claimed. ctr = {evictions, resident}.
extern "C" __global__ void __launch_bounds__(1024) zra_cache_victims_kernel(u32* slotOf, u32* frameOf, u8* ref, u32* hand, unsigned long long* ctr,
                                                                         u32 slots, u32 V, u32* victim, u32 reuse) {
  __shared__ u32 sWave[16], sCut, sEvict;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) sEvict = 0;
  __syncthreads();
  auto claim = [&](u32 v) {
    const u32 old = frameOf[v];
    if (old != kEmpty) { slotOf[old] = kNone; frameOf[v] = kEmpty; atomicAdd(&sEvict, 1u); }
    ref[v] = kClaimed;
  };
  if (reuse) {
    for (u32 i = tid; i < V; i += 1024) claim(victim[i]);
  } else {
    const u32 C = min(slots, 1024u);                         // a chunk never holds one slot twice
    u32 pos = *hand, taken = 0;
    // (terminates: V <= slots, a claimed slot is never a candidate again, and one turn of the hand clears every reference bit)
    while (taken < V) {
      const bool in = tid < C;
      const u32 p = in ? (pos + tid < slots ? pos + tid : pos + tid - slots) : 0u;
      const u8 r = in ? ref[p] : kClaimed;
      const bool cand = in && r != kClaimed && (r == 0 || frameOf[p] == kEmpty);
      const u64 m = __ballot(cand);
      const u32 rank = (u32)__popcll(m & ((1ull << lane) - 1));
      if (lane == 0) sWave[wave] = (u32)__popcll(m);
      __syncthreads();
      u32 before = 0, total = 0;
      for (u32 w = 0; w < 16; w++) { const u32 c = sWave[w]; before += w < wave ? c : 0u; total += c; }
      const u32 need = V - taken, r2 = before + rank;
      if (cand && total >= need && r2 == need - 1) sCut = tid;          // the hand stops behind the last victim it needs
      __syncthreads();
      const u32 cut = total >= need ? sCut : C - 1;
      if (in && tid <= cut) {
        if (cand) { victim[taken + r2] = p; claim(p); }
        else if (r == 1) ref[p] = 0;                                  // second chance
      }
      taken += min(total, need);
      pos = pos + cut + 1 < slots ? pos + cut + 1 : pos + cut + 1 - slots;
      __syncthreads();                                                // (sWave, sCut of the next chunk)
    }
    if (tid == 0) *hand = pos;
  }
  __syncthreads();
  if (tid == 0 && sEvict) { ctr[0] += sEvict; ctr[1] -= sEvict; }
}

// After decode pass [s0, s0 + n) of the planned jobs (jobOf = RaPlan::slot, job numbers in frame order): a frame of the pass that decoded
// with status 0 and exactly its size is published in its slot (reference bit clear); any other leaves its slot empty, and so does every
// slot of a pass that failed (passOk == 0). Claimed slots the pass did not need (its last, short pass) are released empty.
extern "C" __global__ void __launch_bounds__(256) zra_cache_commit_kernel(const u32* cnt, const u32* jobOf, u32 nFrames, u32 s0, u32 n, const u32* victim,
                                                                        u32 V, const u32* status, const u32* produced, u32 passOk, u64 fs, u64 total,
                                                                        u32* slotOf, u32* frameOf, u8* ref, unsigned long long* ctr) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nFrames && cnt[t]) {
    const u32 st = jobOf[t];
    if (st >= s0 && st - s0 < n) {
      const u32 j = st - s0, v = victim[j];
      const u32 expect = (u32)frame_expect(t, fs, total);
      if (passOk && status[j] == 0 && produced[j] == expect) { slotOf[t] = v; frameOf[v] = t; atomicAdd(&ctr[1], 1ull); }
      ref[v] = 0;
    }
  }
  if (t >= n && t < V) ref[victim[t]] = 0;
}

// A pass of a range scan through the handle (zra_scan.h): the frames [first, first + n) of the pass, split by residency into decode
// jobs and copy entries (zra_joblist.h, split_by_residency: entry k is frame first + k).
extern "C" __global__ void __launch_bounds__(1024) zra_scan_split_kernel(const u32* slotOf, u32 nFrames, const u8* table, u64 fs, u64 total, u64 first, u32 n,
                                                                      u64* frameOff, u64* outOff, u32* expect, u32* copies, u32* counts) {
  split_by_residency(n, [=](u32 k) { return first + k; }, slotOf, nFrames, table, fs, total, frameOff, outOff, expect, copies, counts);
}

// =================================================================================================
namespace zra_eng {

void scan_launch_split(hipStream_t s, const uint32_t* slotOf, uint32_t nFrames, const uint8_t* table, uint64_t fs, uint64_t total, uint64_t first, uint32_t n,
                       uint64_t* frameOff, uint64_t* outOff, uint32_t* expect, uint32_t* copies, uint32_t* counts) {
  hipLaunchKernelGGL(zra_scan_split_kernel, dim3(1), dim3(1024), 0, s, slotOf, nFrames, table, (u64)fs, (u64)total, (u64)first, n, frameOff, outOff, expect, copies,
                     counts);
}

Status ArchiveCache::open(Engine* e, const uint8_t* dArc, size_t arcSize, size_t cacheBytes, ArchiveCache** out) {
  HIPCHK_CLR(hipSetDevice(e->device_));
  HeaderInfo h;
  { Status st = e->ra_header(dArc, arcSize, &h); if (st.zra) return st; }
  ArchiveCache* c = new ArchiveCache();
  c->e_ = e; c->dArc_ = dArc; c->arcSize_ = arcSize; c->h_ = h;
  c->nFrames_ = h.frames();
  const uint64_t fs = h.frameSize;
  c->slots_ = fs ? (uint32_t)std::min<uint64_t>(cacheBytes / fs, c->nFrames_) : 0u;
  c->maxPass_ = std::min(c->slots_, kMaxPass);
  const size_t S = c->slots_, F = c->nFrames_;
  const size_t u32Bytes = (S + c->maxPass_) * 4, stateBytes = ((u32Bytes + S + 7) & ~(size_t)7) + 8 + 16;
  auto fail = [&]() { (void)hipGetLastError(); delete c; return zerr(64); };
  if (hipHostMalloc((void**)&c->pin_, 64, hipHostMallocDefault) != hipSuccess) { c->pin_ = nullptr; return fail(); }
  if (S) {
    if (hipMalloc((void**)&c->arena_, S * fs) != hipSuccess) { c->arena_ = nullptr; return fail(); }
    if (hipMalloc(&c->state_, stateBytes) != hipSuccess) { c->state_ = nullptr; return fail(); }
    if (hipMalloc((void**)&c->slotOf_, F * 4) != hipSuccess) { c->slotOf_ = nullptr; return fail(); }
    c->slotCap_ = F;
    uint8_t* b = (uint8_t*)c->state_;
    c->frameOf_ = (uint32_t*)b; c->victim_ = c->frameOf_ + S;
    c->ref_ = b + u32Bytes;
    c->hand_ = (uint32_t*)(b + ((u32Bytes + S + 7) & ~(size_t)7));
    c->dctr_ = (unsigned long long*)((uint8_t*)c->hand_ + 8);
    if (hipMemsetAsync(c->slotOf_, 0xFF, F * 4, e->stream_) != hipSuccess || hipMemsetAsync(b, 0xFF, u32Bytes, e->stream_) != hipSuccess ||
        hipMemsetAsync(c->ref_, 0, stateBytes - u32Bytes, e->stream_) != hipSuccess || hipStreamSynchronize(e->stream_) != hipSuccess) {
      (void)hipGetLastError(); delete c; return zerr(1);
    }
  }
  *out = c;
  return ok();
}

ArchiveCache::~ArchiveCache() {
  if (e_) { (void)hipSetDevice(e_->device_); (void)hipStreamSynchronize(e_->stream_); }
  if (arena_) (void)hipFree(arena_);
  if (state_) (void)hipFree(state_);
  if (slotOf_) (void)hipFree(slotOf_);
  if (pin_) (void)hipHostFree(pin_);
}

void ArchiveCache::stats(uint64_t out[8]) const {
  const uint64_t v[8] = {slots_, resident_, reads_, hits_, misses_, evictions_, h_.uncompressedSize, h_.frameSize};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

Status ArchiveCache::drop() {
  HIPCHK_CLR(hipSetDevice(e_->device_));
  if (!slots_) return ok();
  HIPCHK_CLR(hipMemsetAsync(slotOf_, 0xFF, (size_t)nFrames_ * 4, e_->stream_));
  HIPCHK_CLR(hipMemsetAsync(frameOf_, 0xFF, (size_t)slots_ * 4, e_->stream_));
  HIPCHK_CLR(hipMemsetAsync(ref_, 0, slots_, e_->stream_));
  HIPCHK_CLR(hipMemsetAsync(dctr_ + 1, 0, 8, e_->stream_));
  HIPCHK_CLR(hipStreamSynchronize(e_->stream_));
  resident_ = 0;
  return ok();
}

void ArchiveCache::update_stats(uint64_t out[8]) const {
  const uint64_t v[8] = {updates_, nFrames_, arcSize_, stagedLast_, refreshedLast_, stagedTotal_, refreshedTotal_, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

// The update is not a read: it maps and unmaps no frame, sets no reference bit and leaves the hand where it is. What it changes of the
// cache are the BYTES of the touched resident frames (Engine::update_archive lays the new bytes over their slots, behind its last
// check) and the length of slotOf, which must cover the frames of the result before the update's planner reads it. The update asks
// for that table behind its host-side checks (UpdCacheView::table): a grown one is a copy with the new entries kNone, swapped in
// after the update's last synchronisation, or freed again.
const uint32_t* ArchiveCache::update_table(void* ctx, uint32_t frames) {
  ArchiveCache* c = (ArchiveCache*)ctx;
  if (frames <= c->slotCap_) return c->slotOf_;
  // headroom of a quarter and 1,024 frames: a stream of appends does not allocate each time
  const size_t cap = (size_t)std::min<uint64_t>((uint64_t)frames + frames / 4 + 1024, 0xFFFFFFF0ull);
  hipStream_t s = c->e_->stream_;
  if (hipMalloc((void**)&c->grown_, cap * 4) != hipSuccess) { (void)hipGetLastError(); c->grown_ = nullptr; return nullptr; }
  if (hipMemsetAsync(c->grown_, 0xFF, cap * 4, s) != hipSuccess ||
      hipMemcpyAsync(c->grown_, c->slotOf_, (size_t)c->nFrames_ * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    (void)hipGetLastError(); (void)hipStreamSynchronize(s); (void)hipFree(c->grown_); c->grown_ = nullptr; return nullptr;
  }
  c->grownCap_ = cap;
  return c->grown_;
}

Status ArchiveCache::update(const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hDataOff, size_t nw,
                            const uint8_t* dAppend, size_t appendSize, uint8_t* dOut, size_t outCap, size_t* outSize, int level, bool checksum) {
  Engine& E = *e_;
  UpdCacheView v;
  v.h = h_; v.arena = arena_; v.slots = slots_; v.table = &ArchiveCache::update_table; v.ctx = this;
  const Status st = E.update_archive(dArc_, arcSize_, dData, hOff, hSize, hDataOff, nw, dAppend, appendSize, dOut, outCap, outSize, level, checksum, &v);
  if (st.zra) {
    if (grown_) { (void)hipStreamSynchronize(E.stream_); (void)hipFree(grown_); grown_ = nullptr; }
    return st;
  }
  if (grown_) { (void)hipFree(slotOf_); slotOf_ = grown_; slotCap_ = grownCap_; grown_ = nullptr; }
  dArc_ = dOut; arcSize_ = *outSize; h_ = v.newHeader; nFrames_ = h_.frames();
  updates_++;
  stagedLast_ = v.staged; refreshedLast_ = v.refreshed; stagedTotal_ += v.staged; refreshedTotal_ += v.refreshed;
  return ok();
}

// ---- the range scans through the handle. A scan is not a read: it inserts, evicts and refreshes nothing, sets no reference bit and
// moves no hand; the driver reads the arena and slotOf and writes neither, so reads / hits / misses / evictions / resident stay, on
// success and on failure. The call is one of its kind on the handle's engine: it overwrites that kind's counters and timer.
ScanCacheView ArchiveCache::scan_view() const {
  ScanCacheView v;
  v.h = h_; v.arena = arena_; v.slotOf = slotOf_; v.slots = slots_; v.frames = nFrames_; v.pin = (uint32_t*)(pin_ + 4);
  return v;
}

Status ArchiveCache::scanned(Status st, const ScanCacheView& v) {
  if (st.zra) return st;
  scans_++;
  scanLast_[0] = v.staged; scanLast_[1] = v.decoded; scanLast_[2] = v.passes;
  scanStagedTotal_ += v.staged; scanDecodedTotal_ += v.decoded;
  scanStageMs_ = v.stageMs;
  return st;
}

void ArchiveCache::scan_stats(uint64_t out[8]) const {
  const uint64_t v[8] = {scans_, scanLast_[0], scanLast_[1], scanLast_[2], scanStagedTotal_, scanDecodedTotal_, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

Status ArchiveCache::search(const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hMatches, size_t matchCap,
                            uint64_t* nMatches) {
  Engine& E = *e_;
  ScanCacheView v = scan_view();
  return scanned(ScanImpl::call(E, kScanSearch, nMatches, nullptr, [&] {
    return ScanImpl::search(E, dArc_, arcSize_, (const uint8_t*)hPattern, patternSize, offset, size, stagingBytes, hMatches, matchCap, nMatches, &v);
  }), v);
}

Status ArchiveCache::search_multi(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint64_t offset, uint64_t size, size_t stagingBytes,
                                  void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern) {
  Engine& E = *e_;
  ScanCacheView v = scan_view();
  return scanned(ScanImpl::call(E, kScanMulti, nMatches, nullptr, [&] {
    return ScanImpl::msearch(E, dArc_, arcSize_, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, offset, size, stagingBytes, hMatches, matchCap, nMatches,
                             hPerPattern, &v);
  }), v);
}

Status ArchiveCache::record_scan(RecordCall c) {
  ScanCacheView v = scan_view();
  c.dArc = dArc_; c.arcSize = arcSize_;
  return scanned(e_->record_scan(c, &v), v);
}

// ---- the record calls through the handle. Index and locate are not reads, like the scans above: their sweeps read the arena and slotOf
// and write neither. The read's byte fetch is a read of the handle, through read() itself: reads / hits / misses / evictions / resident
// move exactly as for ZraHipArchiveRead of the located ranges. The call is one of its kind on the handle's engine.
Status ArchiveCache::recorded(Status st, const ScanCacheView& v) {
  if (st.zra) return st;
  recCalls_++;
  recLast_[0] = v.staged; recLast_[1] = v.decoded; recLast_[2] = v.passes;
  recStagedTotal_ += v.staged; recDecodedTotal_ += v.decoded;
  recStageMs_ = v.stageMs;
  return st;
}

void ArchiveCache::record_stats(uint64_t out[8]) const {
  const uint64_t v[8] = {recCalls_, recLast_[0], recLast_[1], recLast_[2], recStagedTotal_, recDecodedTotal_, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

Status ArchiveCache::index_records(uint32_t delimiter, uint64_t first, uint64_t count, size_t stagingBytes, uint64_t* dIndex, size_t indexCapWords, uint64_t info6[6]) {
  ScanCacheView v = scan_view();
  return recorded(e_->index_records(dArc_, arcSize_, delimiter, first, count, stagingBytes, dIndex, indexCapWords, info6, &v), v);
}

Status ArchiveCache::locate_records(const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n, size_t stagingBytes,
                                    uint64_t* hRanges) {
  ScanCacheView v = scan_view();
  return recorded(e_->locate_records(dArc_, arcSize_, info6, dIndex, indexWords, hNumbers, n, stagingBytes, hRanges, &v), v);
}

Status ArchiveCache::read_records(const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n, size_t stagingBytes,
                                  uint64_t* hRanges, uint8_t* dData, size_t dataCap, uint64_t* dataSize) {
  ScanCacheView v = scan_view();
  RecordFetch fetch;
  fetch.ctx = this;
  // (the read sweep decodes up to the last byte a record needs whatever the process option says, as the plain call's: what a handle
  // without slots follows; with slots a miss is decoded whole either way)
  fetch.fn = [](void* ctx, uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, uint32_t* jobs) {
    return ((ArchiveCache*)ctx)->read(dOut, hOff, hSize, hOutOff, nq, false, true, jobs);
  };
  return recorded(e_->read_records(dArc_, arcSize_, info6, dIndex, indexWords, hNumbers, n, stagingBytes, hRanges, dData, dataCap, dataSize, &v, &fetch), v);
}

Status ArchiveCache::read(uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool wholeFramesOpt, bool endInclusive,
                          uint32_t* jobsOut) {
  Engine& E = *e_;
  if (jobsOut) *jobsOut = 0;
  HIPCHK_CLR(hipSetDevice(E.device_));
  if (!slots_) {
    // no cache: the batch call itself, header read and checked at open
    E.set_ra_verify_whole_frames(wholeFramesOpt);
    Status st = E.ra_batch_body(view(), dOut, hOff, hSize, hOutOff, nq, endInclusive, jobsOut);
    // (a read refused for its bounds or for lack of scratch decoded nothing and wrote nothing: it is not counted)
    if (st.zra == kOutOfBounds || (st.zra == kZStdError && st.zstd == 64)) return st;
    reads_++;
    const uint64_t fs = h_.frameSize;
    if (fs && nFrames_) {
      std::vector<uint8_t> seen(nFrames_, 0);
      for (size_t i = 0; i < nq; i++) {
        if (!hSize[i]) continue;
        for (uint64_t f = hOff[i] / fs, f1 = (hOff[i] + hSize[i] - 1) / fs; f <= f1; f++) {
          if (!seen[f]) misses_++;
          seen[f] = 1;
        }
      }
    }
    return st;
  }
  E.reset_decode_stats();
  return read_cached(dOut, hOff, hSize, hOutOff, nq, endInclusive, jobsOut);
}

Status ArchiveCache::read_cached(uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool endInclusive, uint32_t* jobsOut) {
  Engine& E = *e_;
  hipStream_t s = E.stream_;
  const ArchiveView a = view();
  const uint64_t fs = a.fs, U = a.U;
  const uint32_t nF = a.frames;
  if (nq == 0) { reads_++; return ok(); }
  uint64_t nSlices = 0;
  { Status st = E.ra_walk_queries(a, hOff, hSize, hOutOff, nq, &nSlices, endInclusive); if (st.zra) return st; }
  // the batch's planner scratch (the lookup's two result words inside its totals), then seen[nFrames]: one memset; and the job arrays a
  // miss will need, a few bytes per frame and per slice: all of it in front of the lookup, which copies the hits to dOut and is counted,
  // so that a read refused for lack of these tables ({ZStdError, 64}) has written and counted nothing
  const size_t planWords = RaPlan::words(nF);
  if (nSlices && (!E.raPlan_.reserve((planWords + nF) * 4) || !E.frameOff_.reserve(((size_t)nF + 1) * 16) || !E.outOff_.reserve((size_t)nF * 8) ||
                  !E.expect_.reserve((size_t)nF * 4) || !E.raLimit_.reserve((size_t)nF * 4) || !E.raPieceBase_.reserve(((size_t)nF + 1) * 4) ||
                  !E.raPieces_.reserve((size_t)nSlices * sizeof(ZraRaPiece) + 64))) {
    (void)hipStreamSynchronize(s);                    // (the tuples' copy)
    return zerr(64);
  }
  reads_++;
  if (nSlices == 0) { HIPCHK_CLR(hipStreamSynchronize(s)); return ok(); }
  uint32_t* plan = E.raPlan_.as<uint32_t>();
  const RaPlan P = RaPlan::over(plan, nF);
  uint32_t* const seen = plan + planWords, * const words = P.lookup_words();
  HIPCHK_CLR(hipMemsetAsync(plan, 0, (planWords + nF) * 4, s));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((nSlices + 3) / 4, 1u << 20);
  hipLaunchKernelGGL(zra_cache_lookup_kernel, dim3(grid), dim3(256), 0, s, E.qmeta_.as<uint64_t>(), (u32)nq, (u64)nSlices, (u64)fs, slotOf_, ref_,
                     arena_, dOut, P.cnt, seen, words);
  HIPCHK_CLR(hipMemcpyAsync(pin_, words, 8, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  const uint32_t missed = ((const uint32_t*)pin_)[0], hit = ((const uint32_t*)pin_)[1];
  hits_ += hit; misses_ += missed;
  if (!missed) return ok();

  // ---- misses: whole frames into CLOCK victims, passes of at most maxPass_ frames through the batch's planner and decoder (their job
  // arrays: reserved above)
  const uint32_t V = std::min(missed, maxPass_);
  hipLaunchKernelGGL(zra_cache_victims_kernel, dim3(1), dim3(1024), 0, s, slotOf_, frameOf_, ref_, hand_, dctr_, slots_, V, victim_, 0u);
  uint32_t totals[2];
  Status fail = E.ra_plan_fill(plan, nq, a, V, true, victim_, totals);
  const uint32_t jobs = fail.zra ? 0u : totals[0];
  if (jobsOut) *jobsOut = jobs;
  ZraDecodeArgs ra{};
  ra.pieces = E.raPieces_.as<ZraRaPiece>(); ra.raOut = dOut;
  const uint32_t commitGrid = (std::max(nF, V) + 255) / 256;
  for (uint32_t s0 = 0; s0 < jobs && !fail.zra; s0 += V) {
    const uint32_t n = std::min(V, jobs - s0);
    if (s0) hipLaunchKernelGGL(zra_cache_victims_kernel, dim3(1), dim3(1024), 0, s, slotOf_, frameOf_, ref_, hand_, dctr_, slots_, V, victim_, 1u);
    ra.limit = E.raLimit_.as<uint32_t>() + s0; ra.pieceBase = E.raPieceBase_.as<uint32_t>() + s0;
    fail = E.decode_jobs(a.body, a.bodyBytes, E.frameOff_.as<uint64_t>() + 2 * (size_t)s0, arena_, E.outOff_.as<uint64_t>() + s0,
                         E.expect_.as<uint32_t>() + s0, n, (uint32_t)std::min<uint64_t>(fs, 0xFFFFFFFFu), 2, 0, &ra);
    hipLaunchKernelGGL(zra_cache_commit_kernel, dim3(commitGrid), dim3(256), 0, s, P.cnt, P.slot, nF, s0, n, victim_, V,
                       E.status_.as<uint32_t>(), E.produced_.as<uint32_t>(), fail.zra ? 0u : 1u, (u64)fs, (u64)U, slotOf_, frameOf_, ref_, dctr_);
  }
  if (!jobs)   // (the planner failed: the claimed slots are released all the same)
    hipLaunchKernelGGL(zra_cache_commit_kernel, dim3(commitGrid), dim3(256), 0, s, P.cnt, P.slot, 0u, 0u, 0u, victim_, V,
                       E.status_.as<uint32_t>(), E.produced_.as<uint32_t>(), 0u, (u64)fs, (u64)U, slotOf_, frameOf_, ref_, dctr_);
  HIPCHK_CLR(hipMemcpyAsync(pin_ + 2, dctr_, 16, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  evictions_ = pin_[2]; resident_ = pin_[3];
  if (fail.zra == kZStdError) {
    // Damage: the status is the batch call's under ZRA_HIP_OPT_RA_WHOLE_FRAMES. Which of several failing frames that call reports
    // depends on how it lays out its jobs (one per slice for small batches, one per frame otherwise), so on this cold path the batch
    // itself is asked; the frames it decodes are the same, whole.
    const bool was = E.ra_verify_whole_frames();
    E.set_ra_verify_whole_frames(true);
    const Status st2 = E.ra_batch_body(a, dOut, hOff, hSize, hOutOff, nq, endInclusive);
    E.set_ra_verify_whole_frames(was);
    if (st2.zra) return st2;
  }
  return fail;
}

}  // namespace zra_eng
