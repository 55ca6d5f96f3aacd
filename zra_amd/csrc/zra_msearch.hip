// zra_amd — search of a device-resident archive for several patterns in one decode pass (zra_hip.h: ZraHipSearchArchiveMulti): every
// (content offset, pattern index) at which one of up to 64 byte patterns occurs inside a content range, ascending, without an output
// buffer for the content. What `grep -F -f patterns` is to `grep`: the frames are decoded once, whatever the number of patterns.
//
// The passes, the staging window and the conditions (contiguity), (carry), (ownership) with trim = 0, (c) and (d) are those of the range
// scans' one driver (zra_scan.h); the prefix scan chained by the ping-pong count is zra_search.hip's, used as it is. This call's own:
//  (filter) the 65,536-bit first-two-bytes table in LDS and the bucketed compare of a survivor: zra_patterns.h.
//  (order) count gives per tile the sum of popcount(mask), and beside it the four sums of the tile's waves; the scan turns the tile
//      sums into list bases; the fill redoes a tile that holds a listed match and writes (offset, pattern) pairs, positions ascending
//      and inside a position the set bits of the mask from the lowest: a place in the list is the tile's base, plus the waves in front,
//      plus the wave's earlier trips, plus a wave prefix sum of popcounts, plus the bits below. Never the result of an atomic.
//  (totals) matches per pattern and survivors are order-independent sums: LDS counters, then one global atomic add per non-zero
//      pattern and workgroup. They come to the host once, with the count.
// A workgroup takes kGroup consecutive tiles, so that the 13 KiB pattern table is staged once per 64 KiB of positions.
#include "zra_patterns.h"   // the pattern table, its staging and the test of one position: shared with zra_grep.hip

namespace {
// The words the launches of a call add up, zeroed with the table's upload: the ping-pong match count (c), matches per pattern, survivors.
struct Totals { u64 cnt[2], pad0[6], per[kMaxPatterns], survivors, pad1[7]; };
struct __attribute__((aligned(16))) Match { u64 offset; u32 pattern, reserved; };   // ZraHipPatternMatch
}  // namespace

// The run of a pass: win = slot 0, position x is the byte win[x]; the start positions of the pass are xLo + [0, nPos), xHi is the
// position of the range's end (hi - passBase), M the longest pattern. Workgroup g takes the tiles [g * kGroup, (g + 1) * kGroup): per
// tile the matches -> counts[tile], those of its four waves -> waveCnt[4 * tile + wave]; per call the totals.
template <class TB>
__device__ __forceinline__ void msearch_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 nPat,
                                                                           u32* counts, u32* waveCnt, Totals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ u32 sPer[kMaxPatterns], sCnt[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  stage_table(tbl, &sT);
  if (tid < kMaxPatterns) sPer[tid] = 0;
  u32 survivors = 0;
  for (u32 b = blockIdx.x * kGroup, bEnd = min(tiles, b + kGroup); b < bEnd; b++) {
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();                                                         // (the tile in front is done with)
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u32 c = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u32 j = w0 + t * 64 + lane;
      if (j >= n) continue;
      bool surv;
      u64 mask = position_mask(&sT, sTile, d + j, (u32)min(toHi - (long long)j, (long long)kMaxPattern), &surv);
      survivors += surv;
      c += (u32)__popcll(mask);
      for (; mask; mask &= mask - 1) atomicAdd(&sPer[__builtin_ctzll(mask)], 1u);
    }
    c = wave_sum(c);
    if (lane == 0) { waveCnt[4 * (size_t)b + wave] = c; sCnt[wave] = c; }
    __syncthreads();
    if (tid == 0) counts[b] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
  }
  survivors = wave_sum(survivors);
  if (lane == 0 && survivors) atomicAdd((unsigned long long*)&tot->survivors, (unsigned long long)survivors);
  __syncthreads();
  if (tid < nPat && sPer[tid]) atomicAdd((unsigned long long*)&tot->per[tid], (unsigned long long)sPer[tid]);
}
extern "C" __global__ void __launch_bounds__(256) zra_msearch_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 nPat,
                                                                           u32* counts, u32* waveCnt, Totals* tot) {
  msearch_count<Table>(win, xLo, xHi, nPos, M, tbl, nPat, counts, waveCnt, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_msearch_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 nPat,
                                                                           u32* counts, u32* waveCnt, Totals* tot) {
  msearch_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, nPat, counts, waveCnt, tot);
}

// The same workgroups redo the tiles that hold a listed match (a tile without matches, or behind the list's capacity, is skipped; a
// workgroup without such a tile leaves at once) and write the pairs, (order). p0 = the content offset of position xLo.
template <class TB>
__device__ __forceinline__ void msearch_fill(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl,
                                                                          const u32* counts, const u32* waveCnt, const u64* bases, u64 p0, Match* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  bool any = false;                                                          // (uniform in the workgroup, like `listed` below)
  for (u32 b = bBegin; b < bEnd; b++) any |= counts[b] != 0 && bases[b] < cap;
  if (!any) return;
  stage_table(tbl, &sT);
  for (u32 b = bBegin; b < bEnd; b++) {
    const bool listed = counts[b] != 0 && bases[b] < cap;
    if (!listed) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u64 at = bases[b];
    for (u32 w = 0; w < wave; w++) at += waveCnt[4 * (size_t)b + w];
    if (waveCnt[4 * (size_t)b + wave] == 0 || at >= cap) continue;           // (uniform in the wave; the barriers are at the loop's head)
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u32 j = w0 + t * 64 + lane;
      bool surv;
      u64 mask = j < n ? position_mask(&sT, sTile, d + j, (u32)min(toHi - (long long)j, (long long)kMaxPattern), &surv) : 0;
      const u32 c = (u32)__popcll(mask);
      if (__ballot(c != 0) == 0) continue;
      const u32 incl = wave_incl_scan(c);
      u64 idx = at + incl - c;
      for (; mask; mask &= mask - 1, idx++)
        if (idx < cap) { Match e; e.offset = p0 + t0 + j; e.pattern = (u32)__builtin_ctzll(mask); e.reserved = 0; list[idx] = e; }
      at += __shfl(incl, 63, 64);
    }
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_msearch_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl,
                                                                          const u32* counts, const u32* waveCnt, const u64* bases, u64 p0, Match* list, u64 cap) {
  msearch_fill<Table>(win, xLo, xHi, nPos, M, tbl, counts, waveCnt, bases, p0, list, cap);
}
extern "C" __global__ void __launch_bounds__(256) zra_msearch_fill_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                          const u32* counts, const u32* waveCnt, const u64* bases, u64 p0, Match* list, u64 cap) {
  msearch_fill<ClassTable>(win, xLo, xHi, nPos, M, tbl, counts, waveCnt, bases, p0, list, cap);
}

// =================================================================================================
namespace zra_eng {

Status Engine::search_archive_multi(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint64_t offset,
                                    uint64_t size, size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern) {
  return ScanImpl::call(*this, kScanMulti, nMatches, nullptr, [&] {
    return ScanImpl::msearch(*this, dArc, arcSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, offset, size, stagingBytes, hMatches, matchCap,
                             nMatches, hPerPattern);
  });
}

Status ScanImpl::msearch(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, uint64_t offset,
                         uint64_t size, size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern, ScanCacheView* cv) {
  // ---- 1. arguments
  if (!nMatches || !hPat || !hSizes || (!dArc && arcSize) || (!hMatches && matchCap)) return zerr(42);
  PatternSet pset;
  if (!patterns_ok(hPat, hSizes, nPat, syntax, -1, &pset)) return zerr(42);
  const uint32_t M = pset.M, mMin = pset.mMin;
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen, as the search
  ArchiveView arc;
  { Status st = view(E, dArc, arcSize, cv, &arc); if (st.zra) return st; }
  // ---- 3. the range [lo, hi)
  uint64_t lo, hi;
  if (!scan_range(arc.U, offset, size, &lo, &hi)) return {kOutOfBounds, 0};
  uint64_t* const stats = E.callStats_[kScanMulti];
  if (hi - lo < mMin) {
    if (hPerPattern) std::fill(hPerPattern, hPerPattern + nPat, 0ull);
    stats[0] = arc.frames; stats[6] = nPat;
    return ok();
  }
  if (arc.fs == 0 || arc.frames == 0) return {kHeaderInvalid, 0};
  // ---- 4. the passes. tables: Table | Totals | bases[tiles] | counts[tiles] | waveCnt[4 * tiles]
  const ScanPlan P = scan_plan(arc.U, arc.fs, lo, hi, M, 0, stagingBytes);
  uint64_t possible = 0;                                                     // no list is longer: a start per pattern that fits the range
  for (size_t i = 0; i < nPat && possible < matchCap; i++) possible += hi - lo >= pset.len[i] ? hi - lo - pset.len[i] + 1 : 0;
  const size_t listCap = (size_t)std::min<uint64_t>(matchCap, possible);
  const size_t kTotals = pset.table_bytes() + 64, kHead = kTotals + sizeof(Totals);
  std::vector<uint8_t> head(kHead, 0);                                       // (the totals go up as zeros)
  build_pattern_table(head.data(), pset, hPat, hSizes, nPat);
  uint32_t launches = 0;                                                     // (the driver counts the callbacks in place: inside one, those in front of it)
  Status st = ScanImpl::passes(E, arc, P, &E.callMs_[kScanMulti], head.data(), kHead, kTotals, sizeof(Totals), kHead + P.tilesMax * 28 + 64, listCap * sizeof(Match) + 64, true,
                               [&](const ScanPass& ps) {
    uint8_t* const win = window(E), * const tb = E.scan_.tables.as<uint8_t>();
    const Table* const tbl = (const Table*)tb;
    const ClassTable* const ctbl = (const ClassTable*)tb;                    // (one of the two, by the syntax word)
    Totals* const tot = (Totals*)(tb + kTotals);
    uint64_t* const bases = (uint64_t*)(tb + kHead);
    uint32_t* const counts = (uint32_t*)(bases + P.tilesMax);
    uint32_t* const waveCnt = counts + P.tilesMax;
    const uint32_t tiles = (uint32_t)((ps.nPos + kTile - 1) / kTile), groups = (tiles + kGroup - 1) / kGroup;
    if (pset.classes)
      hipLaunchKernelGGL(zra_msearch_count_class_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, (u32)nPat, counts, waveCnt, tot);
    else
      hipLaunchKernelGGL(zra_msearch_count_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, (u32)nPat, counts, waveCnt, tot);
    search_launch_scan(s, counts, tiles, bases, tot->cnt + (launches & 1), tot->cnt + ((launches + 1) & 1));
    if (listCap && pset.classes)
      hipLaunchKernelGGL(zra_msearch_fill_class_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, counts, waveCnt, bases, (u64)ps.p0,
                         E.scan_.list.as<Match>(), (u64)listCap);
    else if (listCap)
      hipLaunchKernelGGL(zra_msearch_fill_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, counts, waveCnt, bases, (u64)ps.p0,
                         E.scan_.list.as<Match>(), (u64)listCap);
  }, &launches, cv);
  if (st.zra) return st;
  // ---- 5. the totals (they came back with the last synchronisation), then the list, once
  const Totals& h = *(const Totals*)(head.data() + kTotals);
  const uint64_t total = h.cnt[launches & 1];
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hMatches, E.scan_.list.p, nOut * sizeof(Match), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  if (hPerPattern) std::copy(h.per, h.per + nPat, hPerPattern);
  *nMatches = total;
  const uint64_t st8[8] = {arc.frames, decoded_frames(P, cv), decoded_bytes(P, cv), total, nOut, P.passes, nPat, h.survivors};
  std::copy(st8, st8 + 8, stats);
  return ok();
}

}  // namespace zra_eng
