// zra_amd — search of a device-resident archive for several patterns in one decode pass (zra_hip.h: ZraHipSearchArchiveMulti): every
// (content offset, pattern index) at which one of up to 64 byte patterns occurs inside a content range, ascending, without an output
// buffer for the content. What `grep -F -f patterns` is to `grep`: the frames are decoded once, whatever the number of patterns.
//
// The passes are those of zra_search.hip (header, jobs per pass, Engine::staged_pass, the staging window [ carry area | slot 0 | ... ],
// the prefix scan chained by a ping-pong count, the carry move; its launch wrappers are used as they are), and so are its conditions
// (contiguity), (carry) with m = M, the longest pattern, (c) and (d). What differs:
//  (ownership) a start position p belongs to the pass that holds content byte min(p + M - 1, hi - 1): one rule for all patterns,
//      monotone in p, so every position of [lo, hi) has one owner and the list ascends across passes whatever the pattern lengths
//      are. A pass that is not the range's last owns only p with p + M - 1 < passEnd < hi: every byte any pattern needs is there. The
//      last pass owns every remaining start up to hi - 1 and tests pattern i only where p + m_i <= hi.
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
extern "C" __global__ void __launch_bounds__(256) zra_msearch_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 nPat,
                                                                           u32* counts, u32* waveCnt, Totals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ Table sT;
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

// The same workgroups redo the tiles that hold a listed match (a tile without matches, or behind the list's capacity, is skipped; a
// workgroup without such a tile leaves at once) and write the pairs, (order). p0 = the content offset of position xLo.
extern "C" __global__ void __launch_bounds__(256) zra_msearch_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl,
                                                                          const u32* counts, const u32* waveCnt, const u64* bases, u64 p0, Match* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ Table sT;
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

// =================================================================================================
namespace zra_eng {

struct MSearchImpl {
  static Status run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint64_t offset, uint64_t size,
                    size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern);
};

Status Engine::search_archive_multi(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint64_t offset,
                                    uint64_t size, size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern) {
  for (auto& v : mstats_) v = 0;
  msearchScanMs_ = 0;
  if (nMatches) *nMatches = 0;
  return MSearchImpl::run(*this, dArc, arcSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, offset, size, stagingBytes, hMatches, matchCap, nMatches,
                          hPerPattern);
}

Status MSearchImpl::run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint64_t offset, uint64_t size,
                        size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern) {
  // ---- 1. arguments
  if (!nMatches || !hPat || !hSizes || (!dArc && arcSize) || (!hMatches && matchCap)) return zerr(42);
  uint32_t M = 0, mMin = kMaxPattern;
  if (!pattern_sizes_ok(hSizes, nPat, &M, &mMin)) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen, as the search
  ArchiveView arc;
  { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  const uint32_t F = arc.frames;
  const uint64_t fs = arc.fs, U = arc.U;
  // ---- 3. the range [lo, hi), inclusive bound
  if (offset > U || (size != ~0ull && (offset + size < offset || offset + size > U))) return {kOutOfBounds, 0};
  const uint64_t lo = offset, hi = size == ~0ull ? U : offset + size;
  if (hi - lo < mMin) {
    if (hPerPattern) std::fill(hPerPattern, hPerPattern + nPat, 0ull);
    E.mstats_[0] = F; E.mstats_[6] = nPat;
    return ok();
  }
  if (fs == 0 || F == 0) return {kHeaderInvalid, 0};
  const uint64_t f0 = lo / fs, f1 = (hi - 1) / fs, n = f1 - f0 + 1;
  // ---- 4. scratch
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, n);
  const uint64_t passes = (n + passSlots - 1) / passSlots;
  const uint64_t window = (uint64_t)nSlots * fs;
  // (the last pass owns up to M - 1 starts inside the carry area on top of a window's worth)
  const size_t tilesMax = (size_t)((window + kMaxPattern + kTile - 1) / kTile);
  uint64_t possible = 0;                                                     // no list is longer: a start per pattern that fits the range
  for (size_t i = 0; i < nPat && possible < matchCap; i++) possible += hi - lo >= hSizes[i] ? hi - lo - hSizes[i] + 1 : 0;
  const size_t listCap = (size_t)std::min<uint64_t>(matchCap, possible);
  // tables: Table | Totals | bases[tiles] | counts[tiles] | waveCnt[4 * tiles]
  constexpr size_t kHead = sizeof(Table) + 64 + sizeof(Totals);
  if (!E.stage_.reserve(kMaxPattern + (size_t)window + 64) || !E.msrch_.tables.reserve(kHead + tilesMax * 28 + 64) ||
      !E.msrch_.list.reserve(listCap * sizeof(Match) + 64) || !E.frameOff_.reserve(((size_t)nSlots + 1) * 16) ||
      !E.outOff_.reserve(((size_t)nSlots + 1) * 8) || !E.expect_.reserve(((size_t)nSlots + 1) * 4))
    return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>() + kMaxPattern;                // slot 0; the carry area lies in front of it
  uint8_t* const tb = E.msrch_.tables.as<uint8_t>();
  const Table* const tbl = (const Table*)tb;
  Totals* const tot = (Totals*)(tb + sizeof(Table) + 64);
  uint64_t* const bases = (uint64_t*)(tb + kHead);
  uint32_t* const counts = (uint32_t*)(bases + tilesMax);
  uint32_t* const waveCnt = counts + tilesMax;
  Match* const list = E.msrch_.list.as<Match>();
  {
    std::vector<uint8_t> head(kHead, 0);                                     // (the totals go up as zeros)
    build_table(*(Table*)head.data(), hPat, hSizes, nPat);
    HIPCHK_CLR(hipMemcpyAsync(tb, head.data(), kHead, hipMemcpyHostToDevice, s));
    HIPCHK_CLR(hipStreamSynchronize(s));                                    // (`head` goes out of scope)
  }
  // ---- passes
  uint32_t launches = 0, carry = 0;
  bool timed = false;
  // (behind a synchronisation of the stream)
  auto take_time = [&]() { if (timed) E.msearchScanMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]); timed = false; };
  for (uint64_t p = 0; p < passes; p++) {
    const uint64_t first = f0 + p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, n - p * passSlots);
    search_launch_jobs(s, arc.table, fs, U, first, nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
    unsigned long long firstError;
    Status st = E.staged_pass(arc, 0, nj, win, &firstError);
    take_time();
    if (st.zra) { E.msearchScanMs_ = 0; return st; }
    if (firstError != ~0ull) {                                              // the lowest failing frame of the first failing pass
      E.msearchScanMs_ = 0;
      return zerr(reported_code(firstError));
    }
    // (contiguity) the run of this pass, and (ownership) the start positions it owns, relative to slot 0
    const uint64_t passBase = first * fs, passEnd = std::min<uint64_t>(U, (first + nj) * fs), L = passEnd - passBase;
    const long long xLo = lo > passBase ? (long long)(lo - passBase) : -(long long)std::min<uint64_t>(M - 1, passBase - lo);
    const long long xHi = (long long)(hi - passBase);
    const long long xEnd = p + 1 == passes ? xHi : (long long)L - (long long)M + 1;
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    if (xEnd > xLo) {
      const uint64_t nPos = (uint64_t)(xEnd - xLo);
      const uint32_t tiles = (uint32_t)((nPos + kTile - 1) / kTile), groups = (tiles + kGroup - 1) / kGroup;
      hipLaunchKernelGGL(zra_msearch_count_kernel, dim3(groups), dim3(256), 0, s, win, xLo, xHi, (u64)nPos, M, tbl, (u32)nPat, counts, waveCnt, tot);
      search_launch_scan(s, counts, tiles, bases, tot->cnt + (launches & 1), tot->cnt + ((launches + 1) & 1));
      launches++;
      if (listCap)
        hipLaunchKernelGGL(zra_msearch_fill_kernel, dim3(groups), dim3(256), 0, s, win, xLo, xHi, (u64)nPos, M, tbl, counts, waveCnt, bases,
                           (u64)(passBase + xLo), list, (u64)listCap);
    }
    if (p + 1 < passes && M > 1) {
      carry = (uint32_t)std::min<uint64_t>(M - 1, carry + L);
      search_launch_carry(s, win, L, carry);
    }
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    timed = true;
  }
  // ---- the totals, then the list, once
  Totals h;
  std::memset(&h, 0, sizeof(h));
  if (launches) HIPCHK_CLR(hipMemcpyAsync(&h, tot, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const uint64_t total = h.cnt[launches & 1];
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hMatches, list, nOut * sizeof(Match), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  if (hPerPattern) std::copy(h.per, h.per + nPat, hPerPattern);
  *nMatches = total;
  const uint64_t st8[8] = {F, n, std::min<uint64_t>(U, (f1 + 1) * fs) - f0 * fs, total, nOut, passes, nPat, h.survivors};
  for (int i = 0; i < 8; i++) E.mstats_[i] = st8[i];
  return ok();
}

}  // namespace zra_eng
