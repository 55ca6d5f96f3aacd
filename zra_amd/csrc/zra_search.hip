// zra_amd — search of a device-resident archive (zra_hip.h: ZraHipSearchArchive): every content offset at which a byte pattern
// occurs inside a content range, in ascending order, without an output buffer for the content.
//
// The passes, the staging window [ carry area | slot 0 | slot 1 | ... ] and the ordering conditions (contiguity), (carry), (ownership),
// (c) and (d) are those of the range scans' one driver: zra_scan.h. This file holds the three launches that driver makes for every
// call of the family (zra_search_jobs_kernel, zra_search_carry_kernel, and the prefix scan the multi-pattern search shares) and what
// is the single search's own:
//  (ownership) with one pattern of m bytes M = m and trim = m - 1: an occurrence belongs to the pass that holds its LAST byte, pass k
//      tests the starts p with p + m - 1 in [passBase, passEnd), p >= lo, p + m <= hi.
//  (launches) per pass that owns a start: the window's plaintext is scanned a tile per workgroup, matches per tile (zra_search_count_kernel);
//      the tile counts become list positions behind the matches of the earlier passes (zra_search_scan_kernel); tiles that hold a listed
//      match redo their compare and write the offsets (zra_search_fill_kernel). The match count and the first matchCapacity offsets
//      come to the host, once.
#include "zra_scan.h"
#include "zra_scan_tile.h"
#include "zra_joblist.h"
#include <algorithm>

namespace {
// One tile of a pass's run. win = slot 0; position x of the run is the byte win[x], x in [-carry, L); the tile's start positions are
// x0 + j, j in [0, n). Stages the pattern and the bytes [x0, x0 + n + m - 1) into LDS (stage_tile), then every wave tests its kWavePos
// consecutive positions, lanes interleaved (lane l of trip t: j = wave * kWavePos + 64 t + l, so neighbouring lanes read neighbouring
// LDS bytes). A lane compares the first min(m, 4) bytes as one word; only a survivor goes on, a word at a time.
// Returns the wave's matches; masks != nullptr receives the ballot of every trip (kWaveIters words of this wave).
__device__ __forceinline__ u32 scan_tile(const u8* win, long long x0, u32 n, const u32* pat, u32 m, u32* sTile, u32* sPat, u64* masks) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 d = stage_tile(win + x0, n + m - 1, sTile);
  if (tid < kMaxPattern / 4) sPat[tid] = pat[tid];
  __syncthreads();
  const u32 head = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1;
  const u32 p0 = sPat[0] & head;
  u32 count = 0;
  const u32 w0 = wave * kWavePos;
  for (u32 t = 0; t < kWaveIters; t++) {
    const u32 j = w0 + t * 64 + lane;
    if (w0 + t * 64 >= n) { if (masks && lane == 0) masks[t] = 0; continue; }   // (uniform in the wave)
    bool hit = j < n && (lds_word(sTile, d + j) & head) == p0;
    if (hit) {
      for (u32 k = 4; k < m; k += 4) {
        const u32 mask = m - k >= 4 ? 0xFFFFFFFFu : (1u << (8 * (m - k))) - 1;
        if ((lds_word(sTile, d + j + k) ^ sPat[k >> 2]) & mask) { hit = false; break; }
      }
    }
    const u64 b = __ballot(hit);
    if (masks && lane == 0) masks[t] = b;
    count += (u32)__popcll(b);
  }
  return count;
}
}  // namespace

// Lane per frame of a pass: job j decodes frame first + j into slot j (zra_joblist.h, emit_job).
extern "C" __global__ void __launch_bounds__(256) zra_search_jobs_kernel(const u8* table, u64 fs, u64 total, u64 first, u32 n, u64* frameOff, u64* outOff,
                                                                         u32* expect) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) emit_job(table, first + j, fs, total, j, j, frameOff, outOff, expect);
}

// Workgroup b: the matches among the start positions xLo + [b * kTile, min(nPos, (b + 1) * kTile)) of the run -> counts[b].
extern "C" __global__ void __launch_bounds__(256) zra_search_count_kernel(const u8* win, long long xLo, u64 nPos, const u32* pat, u32 m, u32* counts) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ u32 sPat[kMaxPattern / 4], sCnt[4];
  const u64 t0 = (u64)blockIdx.x * kTile;
  const u32 n = (u32)min((u64)kTile, nPos - t0);
  const u32 c = scan_tile(win, xLo + (long long)t0, n, pat, m, sTile, sPat, nullptr);
  if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
}

// One workgroup: bases[t] = *cntIn + the matches of the tiles in front of tile t; *cntOut = *cntIn + all of them (condition (c)).
// Every lane sums a run of consecutive tiles, the 1024 sums are scanned in LDS, then the lane walks its run again. (Not zra_joblist.h's
// block_excl_scan like the other additive scans: tests/test_pattern_expr.py pins this kernel's registers where this body has them.)
extern "C" __global__ void __launch_bounds__(1024) zra_search_scan_kernel(const u32* counts, u32 nTiles, u64* bases, const u64* cntIn, u64* cntOut) {
  __shared__ u64 sS[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  u64 own = 0;
  for (u32 t = b0; t < b1; t++) own += counts[t];
  sS[tid] = own;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {                     // Hillis-Steele inclusive scan of the 1024 partials
    const u64 x = tid >= d ? sS[tid - d] : 0;
    __syncthreads();
    sS[tid] += x;
    __syncthreads();
  }
  const u64 in = *cntIn;
  u64 at = in + sS[tid] - own;
  for (u32 t = b0; t < b1; t++) { bases[t] = at; at += counts[t]; }
  if (tid == 1023) *cntOut = in + sS[1023];
}

// Workgroup b redoes tile b's compare when one of its matches has a place in the list (a tile without matches, or behind the list's
// capacity, leaves at once) and writes the offsets: a match's place is the tile's base, plus the matches of the waves in front of its
// own, plus those of its wave's earlier trips, plus the prefix count of its trip's ballot. p0 = the content offset of position xLo.
extern "C" __global__ void __launch_bounds__(256) zra_search_fill_kernel(const u8* win, long long xLo, u64 nPos, const u32* pat, u32 m, const u32* counts,
                                                                         const u64* bases, u64 p0, u64* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ u32 sPat[kMaxPattern / 4], sCnt[4];
  __shared__ u64 sMask[4][kWaveIters];
  if (counts[blockIdx.x] == 0 || bases[blockIdx.x] >= cap) return;   // (uniform in the workgroup)
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const u32 n = (u32)min((u64)kTile, nPos - t0);
  const u32 c = scan_tile(win, xLo + (long long)t0, n, pat, m, sTile, sPat, sMask[wave]);
  if (lane == 0) sCnt[wave] = c;
  __syncthreads();
  u64 at = bases[blockIdx.x];
  for (u32 w = 0; w < wave; w++) at += sCnt[w];
  for (u32 t = 0; t < kWaveIters; t++) {
    const u64 b = sMask[wave][t];
    const u64 idx = at + (u32)__popcll(b & ((1ull << lane) - 1));
    if (((b >> lane) & 1) && idx < cap) list[idx] = p0 + t0 + wave * kWavePos + t * 64 + lane;
    at += (u32)__popcll(b);
  }
}

// One workgroup. The run of the pass is win[-c, L); its last n = min(m - 1, c + L) bytes move to win[-n, 0). Read, synchronise, write:
// the two spans overlap when L < n.
extern "C" __global__ void __launch_bounds__(256) zra_search_carry_kernel(u8* win, u64 L, u32 n) {
  const u32 tid = threadIdx.x;
  const u8 v = tid < n ? win[(long long)L - (long long)n + tid] : (u8)0;
  __syncthreads();
  if (tid < n) win[(long long)tid - (long long)n] = v;
}

// =================================================================================================
namespace zra_eng {

// the steps every range scan shares (zra_engine.h)
void search_launch_jobs(hipStream_t s, const uint8_t* table, uint64_t fs, uint64_t total, uint64_t first, uint32_t n, uint64_t* frameOff, uint64_t* outOff,
                        uint32_t* expect) {
  hipLaunchKernelGGL(zra_search_jobs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, table, (u64)fs, (u64)total, (u64)first, n, frameOff, outOff, expect);
}
void search_launch_scan(hipStream_t s, const uint32_t* counts, uint32_t nItems, uint64_t* bases, const uint64_t* cntIn, uint64_t* cntOut) {
  hipLaunchKernelGGL(zra_search_scan_kernel, dim3(1), dim3(1024), 0, s, counts, nItems, bases, cntIn, cntOut);
}
void search_launch_carry(hipStream_t s, uint8_t* win, uint64_t L, uint32_t n) {
  hipLaunchKernelGGL(zra_search_carry_kernel, dim3(1), dim3(256), 0, s, win, (u64)L, n);
}

Status Engine::search_archive(const uint8_t* dArc, size_t arcSize, const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size,
                              size_t stagingBytes, uint64_t* hMatches, size_t matchCap, uint64_t* nMatches) {
  return ScanImpl::call(*this, kScanSearch, nMatches, nullptr, [&] {
    return ScanImpl::search(*this, dArc, arcSize, (const uint8_t*)hPattern, patternSize, offset, size, stagingBytes, hMatches, matchCap, nMatches);
  });
}

Status ScanImpl::search(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, size_t m, uint64_t offset, uint64_t size, size_t stagingBytes,
                        uint64_t* hMatches, size_t matchCap, uint64_t* nMatches, ScanCacheView* cv) {
  // ---- 1. arguments
  if (!nMatches || !hPat || (!dArc && arcSize) || (!hMatches && matchCap) || m == 0 || m > kMaxPattern) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen; a handle's was checked at open. (The header's CRC-32 is not looked at: that is the verifier's job.)
  ArchiveView arc;
  { Status st = view(E, dArc, arcSize, cv, &arc); if (st.zra) return st; }
  // ---- 3. the range [lo, hi)
  uint64_t lo, hi;
  if (!scan_range(arc.U, offset, size, &lo, &hi)) return {kOutOfBounds, 0};
  uint64_t* const stats = E.callStats_[kScanSearch];
  if (hi - lo < m) { stats[0] = arc.frames; return ok(); }
  if (arc.fs == 0 || arc.frames == 0) return {kHeaderInvalid, 0};            // (content without frames: ra_header lets a frame size of 0 through)
  // ---- 4. the passes. tables: pattern (kMaxPattern bytes) | the ping-pong match count (2 words of 8 bytes, padded to 64) | bases[tiles] | counts[tiles]
  const ScanPlan P = scan_plan(arc.U, arc.fs, lo, hi, (uint32_t)m, (uint32_t)m - 1, stagingBytes);
  const size_t listCap = (size_t)std::min<uint64_t>(matchCap, hi - lo - m + 1);
  alignas(8) uint8_t padded[kMaxPattern + 64] = {0};                         // (the pattern's words behind its end read as zero, and so does the count)
  std::copy(hPat, hPat + m, padded);
  uint32_t launches = 0;                                                     // (the driver counts the callbacks in place: inside one, those in front of it)
  Status st = ScanImpl::passes(E, arc, P, &E.callMs_[kScanSearch], padded, sizeof(padded), kMaxPattern, 16, sizeof(padded) + P.tilesMax * 12 + 64, listCap * 8 + 64, true,
                               [&](const ScanPass& ps) {
    uint8_t* const win = window(E), * const tb = E.scan_.tables.as<uint8_t>();
    const uint32_t* const pat = (const uint32_t*)tb;
    uint64_t* const cnt = (uint64_t*)(tb + kMaxPattern);
    uint64_t* const bases = (uint64_t*)(tb + sizeof(padded));
    uint32_t* const counts = (uint32_t*)(bases + P.tilesMax);
    const uint32_t tiles = (uint32_t)((ps.nPos + kTile - 1) / kTile);
    hipLaunchKernelGGL(zra_search_count_kernel, dim3(tiles), dim3(256), 0, s, win, ps.xLo, (u64)ps.nPos, pat, (u32)m, counts);
    search_launch_scan(s, counts, tiles, bases, cnt + (launches & 1), cnt + ((launches + 1) & 1));
    if (listCap)
      hipLaunchKernelGGL(zra_search_fill_kernel, dim3(tiles), dim3(256), 0, s, win, ps.xLo, (u64)ps.nPos, pat, (u32)m, counts, bases, (u64)ps.p0,
                         E.scan_.list.as<uint64_t>(), (u64)listCap);
  }, &launches, cv);
  if (st.zra) return st;
  // ---- 5. the count (it came back with the last synchronisation), then the list, once
  const uint64_t total = ((const uint64_t*)(padded + kMaxPattern))[launches & 1];
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hMatches, E.scan_.list.p, nOut * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  *nMatches = total;
  const uint64_t st8[8] = {arc.frames, decoded_frames(P, cv), decoded_bytes(P, cv), total, nOut, P.passes, 0, 0};
  std::copy(st8, st8 + 8, stats);
  return ok();
}

}  // namespace zra_eng
