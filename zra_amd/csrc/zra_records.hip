// zra_amd — the record index of a device-resident archive (zra_hip.h: ZraHipIndexRecords, ZraHipLocateRecords, ZraHipReadRecords).
// A record is the bytes between two delimiter bytes, as ZraHipGrepArchive cuts the range [0, U). The index is one 64-bit word per
// frame: bits 0..62 the delimiter bytes of the frame's content, bit 63 set iff its last content byte is not the delimiter. A word
// depends on its own frame only, so an update refreshes the words of the touched frames and appends those of the new ones.
//
// Index, per pass of at most passSlots consecutive frames of the range:
//   1. the frames become decode jobs, slot = frame - first frame of the pass                                      search_launch_jobs
//   2. the pass is decoded whole, checksums verified, into the staging window                                     Engine::staged_pass
//   3. the delimiters of every 8 KiB tile of every slot are counted                                               zra_rec_count_kernel
//   4. a wave per slot: the tile counts become their exclusive prefix and the frame's word                        zra_rec_frames_kernel
// then one reduction over all F words as they lie in dIndex: D, R and the delimiters of the range                 zra_rec_totals_kernel
// (plain passes of the one frame-pass driver, zra_framepass.h: steps 1 and 2, the timed span and the failing frame's code are its)
// Locate:
//   1. the counts of the F words (32 bits each) and their exclusive prefix, D behind it                zra_rec_counts_kernel, search_launch_scan
//   2. a lane per request: up to two boundaries, delimiter r - 1 and delimiter r; each one is searched in the prefix,
//      becomes (frame, ordinal in the frame) and flags its frame                                                  zra_rec_bounds_kernel
//   3. the flagged frames, ascending, get dense job numbers and decode jobs                                       zra_rec_jobs_kernel
//   4. per pass of at most passSlots NEEDED frames: decode (staged_pass), count (3. above), prefix and compare with the index
//      word (4. above, a differing word raises the stale flag), then a wave per boundary whose frame is in the pass finds the
//      tile in the frame's tile prefix and the delimiter inside that one tile                                     zra_rec_select_kernel
//   5. the positions come to the host, once, behind the last pass.
// Read: the locate sweep, then one batched read of the located ranges through Engine::ra_batch_body (a record k < D is read with its
// delimiter, so a read may end at U: the walk's inclusive bound); the delimiter behind an open last record is stored on its own.
// Through an archive handle with a cache (ScanCacheView, zra_hip.h: ZraHipArchiveIndexRecords .. ZraHipArchiveReadRecords) the header is
// the handle's, and a resident frame that a whole-frame sweep needs is copied out of the arena, not decoded. The index: the frame-pass
// driver's steps 2a .. 2c. The locate sweep, per pass, in front of step 4's launches:
//   4a. the needed frames of the pass, slotFrame[j0 .. j0 + nj), are split by residency, one launch: a missing one becomes a decode job,
//       compacted in frame order from job 0 of the pass, into its slot of the pass; a resident one a copy entry      zra_rec_split_kernel
//   4b. the pass's four count words come to the host through the handle's pinned words (the pass's one read-back)
//   4c. the resident frames are copied from their arena slots into their window slots, when there are any             zra_upd_stage_cached_kernel
//   4d. the missing frames are decoded whole, checksums verified, when there are any                                  Engine::staged_pass
// The count, frame-word and select launches run over the same window and are the plain call's: a stale word in a staged frame is found
// like any other. Index and locate only read the arena and the handle's table: they are not reads. The read's byte fetch IS one: it
// goes through the handle's own read path (RecordFetch), hits copied out of the arena, misses decoded whole into CLOCK victims.
//
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
//  (slots) job k of a locate is the k-th needed frame, ascending; pass p holds the jobs [p * passSlots, ...), job k in slot
//      k - p * passSlots at (k - p * passSlots) * frameSize of the window. slotOf[frame] = k, slotFrame[k] = frame.
//  (counts) every count is an integer sum: tile counts by a wave reduction, frame counts by a wave scan, the totals by a tree in LDS.
//      No position depends on an atomic; the stale and out-of-range flags are plain stores of the value 1.
//  (stale) a boundary is resolved only inside a frame that was decoded in this call, and its ordinal is checked against the decoded
//      frame's own count before a byte is read. A frame whose count or bit 63 differs from its word raises the flag, and the call
//      ends with {ZStdError, 20} before a range leaves the device.
//  (split) through a handle the jobs of pass p are rebuilt by 4a over frameOff_ / outOff_ / expect_ [0, nj): what the jobs launch left
//      there is not read again (slotFrame / slotOf, which the passes do read, lie in the call's tables). Positions are prefix counts in
//      frame order, so the first failing job is the lowest failing needed frame of the pass, by construction a missing one.
//  (d) an index call writes the words of its range only; locate and read write nothing but engine scratch and, the read, dData in
//      front of dataCapacity.
#include "zra_framepass.h"
#include "zra_scan.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include <algorithm>
#include <vector>

using namespace zra_dev;

namespace {
constexpr u32 kTile = zra_eng::kScanTile;
// the header words of the tables scratch (bytes): D (the scan's total) | the scan's zero | totals {D, R, delimiters of the range} |
// decode jobs (u32) | stale (u32) | out of range (u32)
constexpr u32 kHdrBytes = 128, kOffD = 0, kOffZero = 8, kOffTot = 16, kOffJobs = 40, kOffStale = 44, kOffOob = 48;
constexpr u64 kCountMask = ~(1ull << 63);
constexpr u64 kDirect = ~0ull;               // a boundary that needs no lookup: its position is written by the bounds launch

// bit 7 of every byte of w that equals the delimiter (d4: the delimiter in all four bytes); exact, no carry between bytes
__device__ __forceinline__ u32 eq_bytes(u32 w, u32 d4) {
  const u32 x = w ^ d4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// bit k set iff byte k of the n <= 16 bytes at p equals the delimiter: one 16-byte load for a whole piece, byte loads for a short one
__device__ __forceinline__ u32 piece_mask(const u8* p, u32 n, u32 d4) {
  if (n >= 16) {
    const u128_u v = *(const u128_u*)p;
    const u32 a = eq_bytes(v.a, d4), b = eq_bytes(v.b, d4), c = eq_bytes(v.c, d4), d = eq_bytes(v.d, d4);
    auto nib = [](u32 m) { return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u); };
    return nib(a) | (nib(b) << 4) | (nib(c) << 8) | (nib(d) << 12);
  }
  u32 m = 0;
  for (u32 k = 0; k < n; k++) m |= (u32)(p[k] == (u8)d4) << k;
  return m;
}
}  // namespace

// Workgroup b: tile b % tpf of slot b / tpf of a pass, the bytes [t * kTile, min((t + 1) * kTile, the frame's content)) of the slot.
// tc[s * (tpf + 1) + t] = its delimiter bytes (0 for a tile behind the frame's content). A lane takes 16 bytes per trip (the slots are
// not 16-byte aligned when the frame size is not: the loads are the hardware's unaligned ones, and only bytes of the frame are read).
// slotFrame == nullptr: slot s holds frame first + s (index); otherwise frame slotFrame[s] (locate).
extern "C" __global__ void __launch_bounds__(256) zra_rec_count_kernel(const u8* win, u64 fs, u64 U, const u32* slotFrame, u64 first, u32 tpf, u32 d4, u32* tc) {
  __shared__ u32 sCnt[4];
  const u32 s = blockIdx.x / tpf, t = blockIdx.x % tpf;
  const u64 f = slotFrame ? (u64)slotFrame[s] : first + s;
  const u32 len = (u32)frame_expect(f, fs, U);
  const u32 t0 = t * kTile;
  const u32 n = t0 < len ? min(kTile, len - t0) : 0u;
  const u8* const p = win + (u64)s * fs + t0;
  u32 c = 0;
  for (u32 x = threadIdx.x * 16; x < n; x += 256 * 16) {
    if (n - x >= 16) {
      const u128_u v = *(const u128_u*)(p + x);
      c += (u32)__popc(eq_bytes(v.a, d4)) + (u32)__popc(eq_bytes(v.b, d4)) + (u32)__popc(eq_bytes(v.c, d4)) + (u32)__popc(eq_bytes(v.d, d4));
    } else {
      c += (u32)__popc(piece_mask(p + x, n - x, d4));
    }
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tc[(u64)s * (tpf + 1) + t] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
}

// A wave per slot of a pass: the slot's tile counts become their exclusive prefix in place, entry tpf the frame's count; the frame's
// word = count | bit 63 when the frame's last content byte is not the delimiter.
// check == 0 (index): words[frame] = the word. check != 0 (locate): *stale = 1 when words[frame] differs from it.
extern "C" __global__ void __launch_bounds__(256) zra_rec_frames_kernel(const u8* win, u64 fs, u64 U, const u32* slotFrame, u64 first, u32 nSlots, u32 tpf, u32 delim,
                                                                        u32* tc, u64* words, u32 check, u32* stale) {
  const u32 s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nSlots) return;                                                    // (uniform in the wave)
  const u64 f = slotFrame ? (u64)slotFrame[s] : first + s;
  const u32 len = (u32)frame_expect(f, fs, U);
  u32* const e = tc + (u64)s * (tpf + 1);
  u32 run = 0;
  for (u32 t0 = 0; t0 < tpf; t0 += 64) {
    const u32 t = t0 + lane;
    const u32 c = t < tpf ? e[t] : 0u;
    const u32 inc = wave_incl_scan(c);
    if (t < tpf) e[t] = run + inc - c;
    run += __shfl(inc, 63, 64);
  }
  if (lane != 0) return;
  e[tpf] = run;
  const u64 w = (u64)run | (len && win[(u64)s * fs + len - 1] != (u8)delim ? 1ull << 63 : 0ull);
  if (!check) words[f] = w;
  else if (words[f] != w) *stale = 1u;
}

// One workgroup: out3 = {D = the counts of all F words, R = D + bit 63 of word F - 1, the counts of the words [lo, hi)}.
extern "C" __global__ void __launch_bounds__(1024) zra_rec_totals_kernel(const u64* words, u64 F, u64 lo, u64 hi, u64* out3) {
  __shared__ u64 sA[1024], sB[1024];
  const u32 tid = threadIdx.x;
  u64 a = 0, b = 0;
  for (u64 f = tid; f < F; f += 1024) {
    const u64 c = words[f] & kCountMask;
    a += c;
    if (f >= lo && f < hi) b += c;
  }
  sA[tid] = a; sB[tid] = b;
  __syncthreads();
  for (u32 d = 512; d > 0; d >>= 1) {
    if (tid < d) { sA[tid] += sA[tid + d]; sB[tid] += sB[tid + d]; }
    __syncthreads();
  }
  if (tid == 0) { out3[0] = sA[0]; out3[1] = sA[0] + (F ? words[F - 1] >> 63 : 0ull); out3[2] = sB[0]; }
}

// Lane per frame: the count of its word in 32 bits, what the prefix scan takes (a frame holds fewer than 2^32 bytes; a word that says
// more is a wrong word, and the frame's check finds it when a boundary falls there).
extern "C" __global__ void __launch_bounds__(256) zra_rec_counts_kernel(const u64* words, u32 F, u32* cnt) {
  const u32 f = blockIdx.x * 256 + threadIdx.x;
  if (f < F) cnt[f] = (u32)(words[f] & kCountMask);
}

// Lane per request i, record r = numbers[i]: boundary 2 i is the record's start (behind delimiter r - 1; 0 for record 0), boundary
// 2 i + 1 its end (delimiter r; U for an open record D). A delimiter k lies in the last frame f with pre[f] <= k, as ordinal
// k - pre[f]: bnd = f << 32 | ordinal, and the frame is flagged. r >= R raises *oob. (pre: the exclusive prefix of the counts, D at *totD.)
extern "C" __global__ void __launch_bounds__(256) zra_rec_bounds_kernel(const u64* numbers, u32 n, const u64* pre, const u64* words, u32 F, const u64* totD, u64 U,
                                                                        u8* need, u64* bnd, u64* pos, u32* oob) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 D = *totD, R = D + (F ? words[F - 1] >> 63 : 0ull);
  const u64 r = numbers[i];
  if (r >= R) { *oob = 1u; bnd[2 * (u64)i] = bnd[2 * (u64)i + 1] = kDirect; pos[2 * (u64)i] = pos[2 * (u64)i + 1] = 0; return; }
  for (u32 side = 0; side < 2; side++) {
    const u64 x = 2 * (u64)i + side;
    if (side == 0 && r == 0) { bnd[x] = kDirect; pos[x] = 0; continue; }
    if (side == 1 && r == D) { bnd[x] = kDirect; pos[x] = U; continue; }
    const u64 k = side ? r : r - 1;                                           // (k < D: F > 0)
    u32 lo = 0, hi = F - 1;
    while (lo < hi) {
      const u32 mid = lo + (hi - lo + 1) / 2;
      if (pre[mid] <= k) lo = mid; else hi = mid - 1;
    }
    need[lo] = 1;
    bnd[x] = (u64)lo << 32 | (u64)(u32)(k - pre[lo]);
    pos[x] = 0;
  }
}

// One workgroup walks the frames, 1024 at a time: the flagged ones, ascending, become jobs 0 .. nJobs - 1 (zra_joblist.h: block_rank,
// emit_job). slotFrame[k] = the frame of job k, slotOf[frame] = k; outOff[j] = j * fs for the slots of one pass (the same every pass).
extern "C" __global__ void __launch_bounds__(1024) zra_rec_jobs_kernel(const u8* need, u32 F, const u8* table, u64 U, u64 fs, u32 passSlots, u64* frameOff, u64* outOff,
                                                                       u32* expect, u32* slotFrame, u32* slotOf, u32* nJobs) {
  u32 jobBase = 0;
  for (u64 base = 0; base < F; base += 1024) {                        // (64 bits: F may lie within 1024 of 2^32)
    const u64 f = base + threadIdx.x;
    const bool p[1] = {f < F && need[f] != 0};
    u32 rank[1], total[1];
    block_rank<1>(p, rank, total);
    if (p[0]) {
      const u32 k = jobBase + rank[0];
      emit_job(table, f, fs, U, k, k, frameOff, k < passSlots ? outOff : nullptr, expect);
      slotFrame[k] = (u32)f; slotOf[f] = k;
    }
    jobBase += total[0];
  }
  if (threadIdx.x == 0) *nJobs = jobBase;
}

// A pass of the locate sweep through a handle: the frame LIST slotFrame[0 .. n) of the pass (ascending; the caller passes
// slotFrame + j0), split by residency into decode jobs and copy entries (zra_joblist.h, split_by_residency: entry k is frame
// slotFrame[k] in slot k of the window).
extern "C" __global__ void __launch_bounds__(1024) zra_rec_split_kernel(const u32* slotFrame, u32 n, const u32* cacheSlotOf, u32 nFrames, const u8* table, u64 fs, u64 U,
                                                                        u64* frameOff, u64* outOff, u32* expect, u32* copies, u32* counts) {
  split_by_residency(n, [=](u32 k) { return slotFrame[k]; }, cacheSlotOf, nFrames, table, fs, U, frameOff, outOff, expect, copies, counts);
}

// A wave per boundary x whose frame is one of the jobs [j0, j0 + nj) of this pass: ordinal j of the frame. A binary search over the
// frame's tile prefix finds the tile, then the wave reads that one tile, 1 KiB per trip: per-lane masks, their popcounts, a wave
// prefix, and the lane that holds the delimiter writes its content position (+ 1 for a start boundary). It leaves with the trip
// that holds it. An ordinal at or behind the decoded frame's own count belongs to a stale word and is not resolved.
extern "C" __global__ void __launch_bounds__(256) zra_rec_select_kernel(const u8* win, u64 fs, u64 U, const u64* bnd, u64 nb, const u32* slotOf,
                                                                        u32 j0, u32 nj, u32 tpf, const u32* tc, u32 d4, u64* pos) {
  const u64 x = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  if (x >= nb) return;                                                        // (everything up to the trips is uniform in the wave)
  const u64 b = bnd[x];
  if (b == kDirect) return;
  const u32 f = (u32)(b >> 32), j = (u32)b;
  const u32 k = slotOf[f];
  if (k < j0 || k - j0 >= nj) return;
  const u32 s = k - j0;
  const u32* const e = tc + (u64)s * (tpf + 1);
  if (j >= e[tpf]) return;
  u32 lo = 0, hi = tpf - 1;
  while (lo < hi) {                                                           // the last tile whose prefix is <= j
    const u32 mid = lo + (hi - lo + 1) / 2;
    if (e[mid] <= j) lo = mid; else hi = mid - 1;
  }
  u32 rem = j - e[lo];
  const u32 len = (u32)frame_expect(f, fs, U);
  const u32 t0 = lo * kTile;
  const u32 n = t0 < len ? min(kTile, len - t0) : 0u;
  const u8* const p = win + (u64)s * fs + t0;
  for (u32 x0 = 0; x0 < n; x0 += 1024) {
    const u32 off = x0 + lane * 16;
    u32 m = off < n ? piece_mask(p + off, min(16u, n - off), d4) : 0u;
    const u32 c = (u32)__popc(m);
    const u32 inc = wave_incl_scan(c);
    const u32 tot = __shfl(inc, 63, 64);
    if (rem < tot) {
      if (rem >= inc - c && rem < inc) {
        for (u32 q = rem - (inc - c); q; q--) m &= m - 1;
        pos[x] = (u64)f * fs + t0 + off + (u32)__builtin_ctz(m) + ((x & 1) ? 0u : 1u);
      }
      return;
    }
    rem -= tot;
  }
}

// Lane per entry: one delimiter byte at dData + at[i], the byte behind an open last record (the read).
extern "C" __global__ void __launch_bounds__(256) zra_rec_delim_kernel(const u64* at, u32 n, u32 delim, u8* dData, u64 dataCap) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && at[i] < dataCap) dData[at[i]] = (u8)delim;
}

// =================================================================================================
namespace zra_eng {

struct RecordsImpl {
  static Status index(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dArc, size_t arcSize, uint32_t delim, uint64_t first, uint64_t count,
                      size_t stagingBytes, uint64_t* dIndex, size_t cap, uint64_t info6[6], ScanCacheView* cv);
  // the locate sweep: hPos[2 i], hPos[2 i + 1] = start and end of record hNumbers[i]; st6 = {frames, boundaries looked up, frames
  // decoded, content bytes regenerated, passes, D}. *view: the archive's checked view, for the read that follows. *ms gains the
  // HIP-event time of the sweep's own launches. cv (every call below; a call through an archive handle): the header step is the
  // handle's; with slots a needed frame that is resident is staged from the arena, and st6[2], st6[3] count the decode jobs alone.
  static Status sweep(Engine& E, double* ms, const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers,
                      size_t n, size_t stagingBytes, const uint8_t* dData, size_t dataCap, std::vector<uint64_t>& hPos, uint64_t st6[6], ArchiveView* view, ScanCacheView* cv);
  static Status read(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n,
                     size_t stagingBytes, uint64_t* hRanges, uint8_t* dData, size_t dataCap, uint64_t* dataSize, ScanCacheView* cv, const RecordFetch* fetch);
};

namespace {
bool ranges_overlap(const void* p, uint64_t n, const void* q, uint64_t m) {
  return n && m && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}
// the arena check of the update through a handle: a buffer the call writes must not lie over the handle's decoded frames
bool overlaps_arena(const ScanCacheView* cv, const void* p, uint64_t n) {
  return cv && cv->slots && ranges_overlap(p, n, cv->arena, (uint64_t)cv->slots * cv->h.frameSize);
}
uint32_t tiles_per_frame(uint64_t fs) { return (uint32_t)((fs + kTile - 1) / kTile); }
uint32_t delim4(uint32_t d) { return d * 0x01010101u; }
}  // namespace

Status Engine::index_records(const uint8_t* dArc, size_t arcSize, uint32_t delim, uint64_t first, uint64_t count, size_t stagingBytes, uint64_t* dIndex,
                             size_t indexCapWords, uint64_t info6[6], ScanCacheView* cv) {
  // (rule 5, OutputTooSmall, leaves the first four words: they say how many words the index needs)
  return entry_call(callStats_[kCallIndex], &callMs_[kCallIndex], {{info6, 6}}, true, [&] {
    return RecordsImpl::index(*this, callStats_[kCallIndex], &callMs_[kCallIndex], dArc, arcSize, delim, first, count, stagingBytes, dIndex, indexCapWords, info6, cv);
  });
}

Status RecordsImpl::index(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dArc, size_t arcSize, uint32_t delim, uint64_t first, uint64_t count,
                          size_t stagingBytes, uint64_t* dIndex, size_t cap, uint64_t info6[6], ScanCacheView* cv) {
  // ---- 1. arguments, 2. overlap (with the archive, and with the arena of the handle the call goes through)
  if (!info6 || (!dArc && arcSize) || (!dIndex && cap) || delim > 255) return zerr(42);
  if (cap > (~(size_t)0) / 8 || ranges_overlap(dIndex, 8 * (uint64_t)cap, dArc, arcSize) || overlaps_arena(cv, dIndex, 8 * (uint64_t)cap)) return zerr(42);
  FramePasses F(E, ms);
  STCHK(F.start());
  // ---- 3. header: the statuses of ZraHipArchiveOpen, or the header a handle checked when it was opened
  ArchiveView arc;
  STCHK(ScanImpl::view(E, dArc, arcSize, cv, &arc));
  if (arc.fs == 0) return {kHeaderInvalid, 0};
  const uint64_t fs = arc.fs, U = arc.U;
  const uint64_t Fr = (U + fs - 1) / fs;
  // ---- 4. the range, as the verifier's
  uint64_t n;
  if (!frame_range(Fr, first, count, &n)) return {kOutOfBounds, 0};
  const uint64_t head[4] = {U, fs, delim, Fr};
  for (int i = 0; i < 4; i++) info6[i] = head[i];
  // ---- 5. capacity: header arithmetic alone. (An empty range over words the caller holds still gives their totals.)
  if (n && cap < Fr) return {kOutputTooSmall, 0};
  if (!Fr || cap < Fr) { stats[0] = Fr; return ok(); }
  // ---- 6. scratch: the call's tables are the record index's own; an empty range has no pass and reserves nothing of the decoder's
  const PassPlan P = pass_plan(first, n, pass_slots(fs, stagingBytes));
  const uint32_t tpf = tiles_per_frame(fs);
  if (!E.rec_.tables.reserve(kHdrBytes + ((size_t)P.nSlots * (tpf + 1) + 16) * 4)) return zerr(64);
  STCHK(F.open({n ? (size_t)((uint64_t)P.nSlots * fs) + 64 : 0, 0, 0, 0, 0, P.nSlots, P.nSlots, cv && cv->slots ? (size_t)P.nSlots : 0}));
  uint8_t* const hdr = E.rec_.tables.as<uint8_t>();
  uint32_t* const tc = (uint32_t*)(hdr + kHdrBytes);
  // ---- passes: plain, one side (zra_framepass.h); through a handle the resident frames of a pass are staged, steps 2a .. 2c there
  STCHK(F.begin(nullptr, 0));
  STCHK(F.run(P, FramePasses::Side{&arc, 0, F.win, cv}, nullptr, nullptr, nullptr, nullptr, [&](const FramePass& ps, uint32_t) {
      hipLaunchKernelGGL(zra_rec_count_kernel, dim3(ps.nj * tpf), dim3(256), 0, F.s, F.win, (u64)fs, (u64)U, (const u32*)nullptr, (u64)ps.first, tpf, delim4(delim), tc);
      hipLaunchKernelGGL(zra_rec_frames_kernel, dim3((ps.nj + 3) / 4), dim3(256), 0, F.s, F.win, (u64)fs, (u64)U, (const u32*)nullptr, (u64)ps.first, ps.nj, tpf, delim, tc,
                         (u64*)dIndex, 0u, (u32*)nullptr);
      return ok();
    }));
  uint64_t tot[3] = {0, 0, 0};
  hipLaunchKernelGGL(zra_rec_totals_kernel, dim3(1), dim3(1024), 0, F.s, (const u64*)dIndex, (u64)Fr, (u64)first, (u64)(first + n), (u64*)(hdr + kOffTot));
  STCHK(F.finish(tot, hdr + kOffTot, 24));
  info6[4] = tot[0]; info6[5] = tot[1];
  const uint64_t st8[8] = {Fr, n, content_bytes(U, fs, first, n), tot[2], P.passes, 0, 0, 0};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  return ok();
}

Status RecordsImpl::sweep(Engine& E, double* ms, const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers,
                          size_t n, size_t stagingBytes, const uint8_t* dData, size_t dataCap, std::vector<uint64_t>& hPos, uint64_t st6[6], ArchiveView* view,
                          ScanCacheView* cv) {
  // ---- 1. arguments and the info's own consistency, the read's overlap
  if (!info6 || (!dArc && arcSize) || (!dIndex && indexWords) || (n && !hNumbers)) return zerr(42);
  const uint64_t iU = info6[0], ifs = info6[1], delim = info6[2], iF = info6[3];
  if (ifs == 0 || ifs > 0xFFFFFFFFull || delim > 255 || iF != iU / ifs + (iU % ifs != 0) || indexWords < iF || indexWords > (~(size_t)0) / 8) return zerr(42);
  if (n > 0xFFFFFFF0ull) return zerr(64);
  if (ranges_overlap(dData, dataCap, dArc, arcSize) || ranges_overlap(dData, dataCap, dIndex, 8 * (uint64_t)indexWords) || overlaps_arena(cv, dData, dataCap))
    return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header (a handle's: the one it checked), 3. the archive the index was made of
  ArchiveView arc;
  STCHK(ScanImpl::view(E, dArc, arcSize, cv, &arc));
  if (arc.fs == 0) return {kHeaderInvalid, 0};
  const uint64_t fs = arc.fs, U = arc.U;
  const uint64_t F64 = (U + fs - 1) / fs;
  if (U != iU || fs != ifs || F64 != iF) return zerr(40);
  *view = arc;
  const uint32_t F = (uint32_t)F64;
  for (int i = 0; i < 6; i++) st6[i] = 0;
  st6[0] = F;
  hPos.clear();
  if (!F) return n ? Status{kOutOfBounds, 0} : ok();                          // (no content: R = 0)
  // ---- 5. scratch (the record numbers are checked on the device, in front of the first decode)
  const uint32_t passSlots = pass_slots(fs, stagingBytes), tpf = tiles_per_frame(fs);
  const size_t jobsMax = (size_t)std::min<uint64_t>(F, 2 * (uint64_t)n);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, jobsMax);
  const bool cached = cv && cv->slots;
  // tables: header | cnt[F] (u32) | slotOf[F] (u32) | slotFrame[F] (u32) | tile prefixes | pre[F + 1] (u64) | need[F] (u8)
  const size_t offCnt = kHdrBytes, offSlotOf = offCnt + (size_t)F * 4, offSlotFrame = offSlotOf + (size_t)F * 4, offTc = offSlotFrame + (size_t)F * 4;
  const size_t offPre = (offTc + ((size_t)nSlots * (tpf + 1) + 1) * 4 + 15) & ~(size_t)15, offNeed = offPre + ((size_t)F + 1) * 8;
  // ranges: numbers[n] | bnd[2 n] | pos[2 n]
  if (!E.rec_.tables.reserve(offNeed + F + 64) || !E.rec_.ranges.reserve(((size_t)n * 5 + 8) * 8) || !E.frameOff_.reserve((jobsMax + 1) * 16) ||
      !E.outOff_.reserve(((size_t)nSlots + 1) * 8) || !E.expect_.reserve((jobsMax + 1) * 4) || (cached && !E.upd_.copies.reserve(((size_t)nSlots + 1) * 16)))
    return zerr(64);
  if (nSlots && !E.stage_.reserve((size_t)((uint64_t)nSlots * fs) + 64)) return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>();
  uint8_t* const hdr = E.rec_.tables.as<uint8_t>();
  uint32_t* const cnt = (uint32_t*)(hdr + offCnt);
  uint32_t* const slotOf = (uint32_t*)(hdr + offSlotOf);
  uint32_t* const slotFrame = (uint32_t*)(hdr + offSlotFrame);
  uint32_t* const tc = (uint32_t*)(hdr + offTc);
  uint64_t* const pre = (uint64_t*)(hdr + offPre);
  uint8_t* const need = hdr + offNeed;
  uint64_t* const numbers = E.rec_.ranges.as<uint64_t>();
  uint64_t* const bnd = numbers + n;
  uint64_t* const pos = bnd + 2 * n;
  // (through a handle's cache) the pass's count words, then its copy entries, 4 words each
  uint32_t* const counts = cached ? E.upd_.copies.as<uint32_t>() : nullptr, * const copies = cached ? counts + 4 : nullptr;
  bool stageTimed = false;
  // (behind a synchronisation of the stream)
  auto take_time = [&]() {
    *ms += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
    if (stageTimed) cv->stageMs += Engine::elapsed_ms(E.evCall_[4], E.evCall_[5]);
    stageTimed = false;
  };
  // ---- the prefix, the boundaries, the jobs
  HIPCHK_CLR(hipMemsetAsync(hdr, 0, kHdrBytes, s));
  HIPCHK_CLR(hipMemsetAsync(need, 0, F, s));
  HIPCHK_CLR(hipMemsetAsync(slotOf, 0xFF, (size_t)F * 4, s));
  if (n) HIPCHK_CLR(hipMemcpyAsync(numbers, hNumbers, n * 8, hipMemcpyHostToDevice, s));
  HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
  hipLaunchKernelGGL(zra_rec_counts_kernel, dim3((F + 255) / 256), dim3(256), 0, s, (const u64*)dIndex, F, cnt);
  search_launch_scan(s, cnt, F, pre, (const uint64_t*)(hdr + kOffZero), (uint64_t*)(hdr + kOffD));
  if (n)
    hipLaunchKernelGGL(zra_rec_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const u64*)numbers, (u32)n, (const u64*)pre, (const u64*)dIndex, F,
                       (const u64*)(hdr + kOffD), (u64)U, need, bnd, pos, (u32*)(hdr + kOffOob));
  hipLaunchKernelGGL(zra_rec_jobs_kernel, dim3(1), dim3(1024), 0, s, (const u8*)need, F, arc.table, (u64)U, (u64)fs, passSlots, E.frameOff_.as<uint64_t>(),
                     E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>(), slotFrame, slotOf, (u32*)(hdr + kOffJobs));
  HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
  uint64_t h16[kHdrBytes / 8] = {0};
  HIPCHK_CLR(hipMemcpyAsync(h16, hdr, kHdrBytes, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const uint8_t* const hb = (const uint8_t*)h16;
  const uint64_t D = h16[kOffD / 8];
  const uint32_t nJobs = *(const uint32_t*)(hb + kOffJobs);
  // ---- 4. a record number at or behind R
  if (*(const uint32_t*)(hb + kOffOob)) return {kOutOfBounds, 0};
  if (nJobs > jobsMax) return zerr(1);                                        // (cannot happen)
  // ---- passes over the needed frames. Not the frame-pass driver's (zra_framepass.h): the jobs of all passes were built once, above, so
  // a pass has no job launch and decodes at job base j0; its span closes BEHIND its own launches (the first span is the prefix's, taken
  // above, hence `if (p)`); and the frames are not consecutive. Each of the three would be a special case there. A fourth through a
  // handle's cache: the driver splits a RANGE of frames by residency (scan_launch_split), this sweep a LIST (slotFrame), with its own
  // kernel, and a pass's jobs are rebuilt from job 0, (split), where the driver's plain pass had none to rebuild. The previous pass's
  // span is read behind the first synchronisation of the pass: the read-back's of 4b through a cache, staged_pass's without.
  const uint64_t passes = ((uint64_t)nJobs + passSlots - 1) / passSlots;
  uint64_t decJobs = 0, decBytes = 0;
  for (uint64_t p = 0; p < passes; p++) {
    const uint32_t j0 = (uint32_t)(p * passSlots), nj = std::min<uint32_t>(passSlots, nJobs - j0);
    uint32_t nDec = nj;
    bool taken = false;
    if (cached) {                                                             // 4a .. 4c
      HIPCHK_CLR(hipEventRecord(E.evCall_[2], s));
      hipLaunchKernelGGL(zra_rec_split_kernel, dim3(1), dim3(1024), 0, s, (const u32*)(slotFrame + j0), nj, (const u32*)cv->slotOf, cv->frames, arc.table, (u64)fs, (u64)U,
                         E.frameOff_.as<u64>(), E.outOff_.as<u64>(), E.expect_.as<u32>(), copies, counts);
      HIPCHK_CLR(hipEventRecord(E.evCall_[3], s));
      HIPCHK_CLR(hipMemcpyAsync(cv->pin, counts, 16, hipMemcpyDeviceToHost, s));
      HIPCHK_CLR(hipStreamSynchronize(s));
      HIPCHK_CLR(hipGetLastError());
      if (p) take_time();
      taken = true;
      cv->stageMs += Engine::elapsed_ms(E.evCall_[2], E.evCall_[3]);
      nDec = cv->pin[0];
      const uint32_t nCopy = cv->pin[1];
      if (nDec > nj || nCopy != nj - nDec) return zerr(1);                    // (cannot happen)
      decBytes += (uint64_t)cv->pin[2] | (uint64_t)cv->pin[3] << 32;
      if (nCopy) {
        HIPCHK_CLR(hipEventRecord(E.evCall_[4], s));
        upd_launch_stage_cached(s, copies, nCopy, 0, fs, cv->arena, win);
        HIPCHK_CLR(hipEventRecord(E.evCall_[5], s));
        stageTimed = true;
        cv->staged += nCopy;
      }
    }
    if (nDec) {                                                               // (always, without a handle's cache: a pass has a frame)
      unsigned long long firstError;
      STCHK(E.staged_pass(arc, cached ? 0 : j0, nDec, win, &firstError));
      if (p && !taken) take_time();
      if (firstError != ~0ull) return zerr(reported_code(firstError));        // 6. the lowest failing frame of the first failing pass
    }
    decJobs += nDec;
    if (cv) { cv->decoded += nDec; cv->passes++; }
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    hipLaunchKernelGGL(zra_rec_count_kernel, dim3(nj * tpf), dim3(256), 0, s, (const u8*)win, (u64)fs, (u64)U, (const u32*)(slotFrame + j0), (u64)0, tpf,
                       delim4((uint32_t)delim), tc);
    hipLaunchKernelGGL(zra_rec_frames_kernel, dim3((nj + 3) / 4), dim3(256), 0, s, (const u8*)win, (u64)fs, (u64)U, (const u32*)(slotFrame + j0), (u64)0, nj, tpf,
                       (u32)delim, tc, (u64*)dIndex, 1u, (u32*)(hdr + kOffStale));
    hipLaunchKernelGGL(zra_rec_select_kernel, dim3((unsigned)((2 * (uint64_t)n + 3) / 4)), dim3(256), 0, s, (const u8*)win, (u64)fs, (u64)U, (const u64*)bnd,
                       (u64)(2 * (uint64_t)n), (const u32*)slotOf, j0, nj, tpf, (const u32*)tc, delim4((uint32_t)delim), pos);
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
  }
  // ---- the stale flag and the positions, once
  uint32_t stale = 0;
  hPos.resize(2 * n);
  HIPCHK_CLR(hipMemcpyAsync(&stale, hdr + kOffStale, 4, hipMemcpyDeviceToHost, s));
  if (n) HIPCHK_CLR(hipMemcpyAsync(hPos.data(), pos, 2 * n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  if (passes) take_time();
  if (stale) return zerr(20);                                                 // 7. a decoded frame contradicts its word
  uint64_t lookups = 0, bytes = 0;
  for (size_t i = 0; i < n; i++) lookups += (hNumbers[i] != 0) + (hNumbers[i] != D);
  if (cached) bytes = decBytes;
  else if (nJobs) {
    std::vector<uint32_t> ex(nJobs);
    HIPCHK_CLR(hipMemcpyAsync(ex.data(), E.expect_.p, (size_t)nJobs * 4, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    for (uint32_t e : ex) bytes += e;
  }
  if (cv) cv->decodedBytes += bytes;
  st6[1] = lookups; st6[2] = decJobs; st6[3] = bytes; st6[4] = passes; st6[5] = D;
  return ok();
}

Status Engine::locate_records(const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n,
                              size_t stagingBytes, uint64_t* hRanges, ScanCacheView* cv) {
  uint64_t (&stats)[8] = callStats_[kCallLocate];
  // (the locate has no output words, and no status that keeps any)
  return entry_call(stats, &callMs_[kCallLocate], {}, false, [&]() -> Status {
    if (n && !hRanges) return zerr(42);
    std::vector<uint64_t> hPos;
    uint64_t st6[6];
    ArchiveView arc;
    const Status st = RecordsImpl::sweep(*this, &callMs_[kCallLocate], dArc, arcSize, info6, dIndex, indexWords, hNumbers, n, stagingBytes, nullptr, 0, hPos, st6, &arc, cv);
    if (st.zra) return st;
    for (size_t i = 0; i < n && hPos.size() == 2 * n; i++) { hRanges[2 * i] = hPos[2 * i]; hRanges[2 * i + 1] = hPos[2 * i + 1] - hPos[2 * i]; }
    const uint64_t st8[8] = {st6[0], n, st6[1], st6[2], st6[3], st6[4], 0, 0};
    for (int i = 0; i < 8; i++) stats[i] = st8[i];
    return ok();
  });
}

Status Engine::read_records(const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords, const uint64_t* hNumbers, size_t n,
                            size_t stagingBytes, uint64_t* hRanges, uint8_t* dData, size_t dataCap, uint64_t* dataSize, ScanCacheView* cv, const RecordFetch* fetch) {
  // (rule OutputTooSmall leaves the packed size the read needs)
  return entry_call(callStats_[kCallRead], &callMs_[kCallRead], {{dataSize, 1}}, true, [&]() -> Status {
    if (!dataSize || (!dData && dataCap)) return zerr(42);
    return RecordsImpl::read(*this, callStats_[kCallRead], &callMs_[kCallRead], dArc, arcSize, info6, dIndex, indexWords, hNumbers, n, stagingBytes, hRanges, dData, dataCap,
                             dataSize, cv, fetch);
  });
}

Status RecordsImpl::read(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dArc, size_t arcSize, const uint64_t info6[6], const uint64_t* dIndex, size_t indexWords,
                         const uint64_t* hNumbers, size_t n, size_t stagingBytes, uint64_t* hRanges, uint8_t* dData, size_t dataCap, uint64_t* dataSize, ScanCacheView* cv,
                         const RecordFetch* fetch) {
  // the locate sweep runs under a timer of its own (the read's, once it has succeeded) and leaves the locate's counters and time alone
  double sweepMs = 0;
  std::vector<uint64_t> hPos;
  uint64_t st6[6];
  ArchiveView arc;
  const Status st = sweep(E, &sweepMs, dArc, arcSize, info6, dIndex, indexWords, hNumbers, n, stagingBytes, dData, dataCap, hPos, st6, &arc, cv);
  if (st.zra) return st;
  if (!n || hPos.size() != 2 * n) return ok();
  // ---- the located ranges as one batch: record k < D with its delimiter, an open record D without (its byte is stored below)
  const uint64_t D = st6[5], delim = info6[2];
  std::vector<uint64_t> q(3 * n), open;
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    const uint64_t len = hPos[2 * i + 1] - hPos[2 * i], isOpen = hNumbers[i] == D;
    q[i] = hPos[2 * i]; q[n + i] = isOpen ? len : len + 1; q[2 * n + i] = at;
    if (isOpen) open.push_back(at + len);
    at += len + 1;
  }
  *dataSize = at;
  if (at > dataCap) return {kOutputTooSmall, 0};
  HIPCHK_CLR(hipSetDevice(E.device_));
  if (!open.empty()) {
    if (!E.rec_.ranges.reserve(open.size() * 8 + 64)) return zerr(64);
    HIPCHK_CLR(hipMemcpyAsync(E.rec_.ranges.p, open.data(), open.size() * 8, hipMemcpyHostToDevice, E.stream_));
    hipLaunchKernelGGL(zra_rec_delim_kernel, dim3((unsigned)((open.size() + 255) / 256)), dim3(256), 0, E.stream_, E.rec_.ranges.as<u64>(), (u32)open.size(), (u32)delim,
                       dData, (u64)dataCap);
    HIPCHK_CLR(hipStreamSynchronize(E.stream_));
  }
  // the second sweep: up to the last byte a record needs, whatever the process option says (the locate sweep decoded the boundary
  // frames whole, checksums verified)
  const bool whole = E.raVerifyWholeFrames_;
  E.raVerifyWholeFrames_ = false;
  uint32_t readJobs = 0;
  // (through a handle the fetch is a read of the handle: hits out of the arena, misses decoded whole into CLOCK victims)
  const Status rs = fetch ? fetch->fn(fetch->ctx, dData, q.data(), q.data() + n, q.data() + 2 * n, n, &readJobs)
                          : E.ra_batch_body(arc, dData, q.data(), q.data() + n, q.data() + 2 * n, n, true, &readJobs);
  E.raVerifyWholeFrames_ = whole;
  if (rs.zra) return rs;
  if (hRanges) for (size_t i = 0; i < n; i++) { hRanges[2 * i] = hPos[2 * i]; hRanges[2 * i + 1] = hPos[2 * i + 1] - hPos[2 * i]; }
  const uint64_t st8[8] = {st6[0], n, at, st6[2], readJobs, st6[4], 0, 0};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  *ms = sweepMs;
  return ok();
}

}  // namespace zra_eng
