// zra_amd — search of a device-resident archive (zra_hip.h: ZraHipSearchArchive): every content offset at which a byte pattern
// occurs inside a content range, in ascending order, without an output buffer for the content.
//
//   1. the fixed header comes to the host (Engine::archive_view); the range becomes frames [f0, f1]
//   2. per pass of at most passSlots consecutive frames: the frames become decode jobs                   zra_search_jobs_kernel
//   3. the pass is decoded whole, checksums verified, into the staging window                            Engine::staged_pass
//   4. the window's plaintext is scanned a tile per workgroup: matches per tile                          zra_search_count_kernel
//   5. the tile counts become list positions behind the matches of the earlier passes                    zra_search_scan_kernel
//   6. tiles that hold a listed match redo their compare and write the offsets                           zra_search_fill_kernel
//   7. the last m - 1 bytes seen so far move in front of slot 0 for the next pass                         zra_search_carry_kernel
//   8. the match count and the first matchCapacity offsets come to the host, once
// The staging window (Engine::stage_, reserved kMaxPattern bytes larger) is  [ carry area | slot 0 | slot 1 | ... ]: slot s lies at s * frameSize behind the carry area.
//
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
//  (contiguity) the frames of a pass are consecutive and all but the archive's last regenerate frameSize bytes (anything else is a
//      failing frame and ends the call), so the slots hold the content [passBase, passEnd) as one run, passEnd = min(U, (last frame of
//      the pass + 1) * frameSize). The scan's bounds come from that arithmetic alone: what lies behind a short last frame, and in slots a
//      smaller last pass does not fill, is plaintext of earlier passes and is never compared.
//  (carry) after pass k the carry area holds, right-aligned against slot 0, the last min(m - 1, bytes decoded so far) bytes of the
//      content decoded so far. A pass can be shorter than m - 1 bytes, so source and destination of the move overlap: one workgroup
//      reads all of its bytes, synchronises, then writes.
//  (ownership) an occurrence belongs to the pass that holds its LAST byte: pass k tests the starts p with p + m - 1 in [passBase,
//      passEnd), p >= lo, p + m <= hi; they begin up to m - 1 bytes inside the carry. p + m - 1 is monotone in p: every occurrence has
//      one owner and the list is ascending across passes.
//  (c) the scan launches are chained by a 64-bit match count that ping-pongs between two words: launch k reads word k & 1 and writes
//      word (k + 1) & 1. A list position is a prefix count, never the result of an atomic, and no workgroup waits for another one.
//  (d) nothing goes to the caller's array before the last pass is done: a call that fails midway writes nothing.
#include "zra_host.h"
#include "zra_dev.h"
#include <algorithm>

using namespace zra_dev;

namespace {
constexpr u32 kMaxPattern = 256;          // ZRA_HIP_SEARCH_MAX_PATTERN
// Start positions of one workgroup. 8 KiB: the halo of up to 255 bytes a tile stages beyond its own positions is then 3 % of its global
// reads, tile + halo take 8.5 KiB of LDS (a CU holds its 8 workgroups of 256 lanes with room to spare), 1 GiB of plaintext is 131,072
// workgroups, and the per-tile tables (4-byte count, 8-byte base) cost 0.15 % of the window.
constexpr u32 kTile = 8192;
constexpr u32 kWavePos = kTile / 4;       // consecutive start positions of one wave
constexpr u32 kWaveIters = kWavePos / 64;
// staged bytes: up to 15 in front (the 16-byte alignment of the first global load), the tile, m - 1 halo bytes, rounded up to 16; the
// compare reads whole words and may look up to 7 bytes beyond its pattern's end (masked off)
constexpr u32 kLdsWords = (kTile + kMaxPattern + 64) / 4;

// the four bytes at byte index i of an LDS word array
__device__ __forceinline__ u32 lds_word(const u32* s, u32 i) {
  const u64 pair = ((u64)s[(i >> 2) + 1] << 32) | s[i >> 2];
  return (u32)(pair >> ((i & 3) * 8));
}

// One tile of a pass's run. win = slot 0; position x of the run is the byte win[x], x in [-carry, L); the tile's start positions are
// x0 + j, j in [0, n). Stages the pattern and the bytes [x0, x0 + n + m - 1) into LDS (16-byte global loads from the aligned address
// at or below win + x0: at most 15 bytes in front, inside the carry area, and at most 15 behind, inside the buffer's slack), then every
// wave tests its kWavePos consecutive positions, lanes interleaved (lane l of trip t: j = wave * kWavePos + 64 t + l, so neighbouring
// lanes read neighbouring LDS bytes). A lane compares the first min(m, 4) bytes as one word; only a survivor goes on, a word at a time.
// Returns the wave's matches; masks != nullptr receives the ballot of every trip (kWaveIters words of this wave).
__device__ __forceinline__ u32 scan_tile(const u8* win, long long x0, u32 n, const u32* pat, u32 m, u32* sTile, u32* sPat, u64* masks) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u8* const src = win + x0;
  const u32 d = (u32)((size_t)src & 15);
  const uint4* const g = (const uint4*)(src - d);
  const u32 chunks = (d + n + m - 1 + 15) >> 4;
  for (u32 c = tid; c < chunks; c += 256) lds_st128((u8*)sTile + 16 * (size_t)c, g[c]);
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

// Lane per frame of a pass: job j decodes frame first + j (its seek-table span, whatever it says: the decoder refuses a span that runs
// backwards or leaves the body) into slot j, and has to regenerate that frame's share of the content.
extern "C" __global__ void __launch_bounds__(256) zra_search_jobs_kernel(const u8* table, u64 fs, u64 total, u64 first, u32 n, u64* frameOff, u64* outOff,
                                                                         u32* expect) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const u64 f = first + j;
  frameOff[2 * (size_t)j] = seek_entry(table, f); frameOff[2 * (size_t)j + 1] = seek_entry(table, f + 1);
  outOff[j] = (u64)j * fs;
  expect[j] = (u32)frame_expect(f, fs, total);
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
// Every lane sums a run of consecutive tiles, the 1024 sums are scanned in LDS, then the lane walks its run again.
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

// the steps ZraHipSearchArchiveMulti shares (zra_engine.h)
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

struct SearchImpl {
  static Status run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, size_t m, uint64_t offset, uint64_t size, size_t stagingBytes,
                    uint64_t* hMatches, size_t matchCap, uint64_t* nMatches);
};

Status Engine::search_archive(const uint8_t* dArc, size_t arcSize, const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size,
                              size_t stagingBytes, uint64_t* hMatches, size_t matchCap, uint64_t* nMatches) {
  for (auto& v : sstats_) v = 0;
  searchScanMs_ = 0;
  if (nMatches) *nMatches = 0;
  return SearchImpl::run(*this, dArc, arcSize, (const uint8_t*)hPattern, patternSize, offset, size, stagingBytes, hMatches, matchCap, nMatches);
}

Status SearchImpl::run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, size_t m, uint64_t offset, uint64_t size, size_t stagingBytes,
                       uint64_t* hMatches, size_t matchCap, uint64_t* nMatches) {
  // ---- 1. arguments
  if (!nMatches || !hPat || (!dArc && arcSize) || (!hMatches && matchCap) || m == 0 || m > kMaxPattern) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen. (The header's CRC-32 is not looked at: that is the verifier's job.)
  ArchiveView arc;
  { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  const uint32_t F = arc.frames;
  const uint64_t fs = arc.fs, U = arc.U;
  // ---- 3. the range [lo, hi), inclusive bound: a search reaches the last byte
  if (offset > U || (size != ~0ull && (offset + size < offset || offset + size > U))) return {kOutOfBounds, 0};
  const uint64_t lo = offset, hi = size == ~0ull ? U : offset + size;
  if (hi - lo < m) { E.sstats_[0] = F; return ok(); }
  if (fs == 0 || F == 0) return {kHeaderInvalid, 0};                       // (content without frames: ra_header lets a frame size of 0 through)
  const uint64_t f0 = lo / fs, f1 = (hi - 1) / fs, n = f1 - f0 + 1;
  // ---- 4. scratch
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, n);
  const uint64_t passes = (n + passSlots - 1) / passSlots;
  const uint64_t window = (uint64_t)nSlots * fs;
  const size_t tilesMax = (size_t)((window + kTile - 1) / kTile);
  const size_t listCap = (size_t)std::min<uint64_t>(matchCap, hi - lo - m + 1);
  // tables: pattern (kMaxPattern bytes) | the ping-pong match count (2 words of 8 bytes, padded to 64) | bases[tiles] | counts[tiles]
  if (!E.stage_.reserve(kMaxPattern + (size_t)window + 64) || !E.srch_.tables.reserve(kMaxPattern + 64 + tilesMax * 12 + 64) ||
      !E.srch_.list.reserve(listCap * 8 + 64) || !E.frameOff_.reserve(((size_t)nSlots + 1) * 16) || !E.outOff_.reserve(((size_t)nSlots + 1) * 8) ||
      !E.expect_.reserve(((size_t)nSlots + 1) * 4))
    return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>() + kMaxPattern;                // slot 0; the carry area lies in front of it
  uint8_t* const tb = E.srch_.tables.as<uint8_t>();
  const uint32_t* const pat = (const uint32_t*)tb;
  uint64_t* const cnt = (uint64_t*)(tb + kMaxPattern);
  uint64_t* const bases = (uint64_t*)(tb + kMaxPattern + 64);
  uint32_t* const counts = (uint32_t*)(bases + tilesMax);
  uint64_t* const list = E.srch_.list.as<uint64_t>();
  {
    uint8_t padded[kMaxPattern + 64] = {0};                                 // (the pattern's words behind its end read as zero)
    std::copy(hPat, hPat + m, padded);
    HIPCHK_CLR(hipMemcpyAsync(tb, padded, sizeof(padded), hipMemcpyHostToDevice, s));
    HIPCHK_CLR(hipStreamSynchronize(s));                                    // (`padded` goes out of scope)
  }
  // ---- passes
  uint32_t launches = 0, carry = 0;
  bool timed = false;
  // (behind a synchronisation of the stream)
  auto take_time = [&]() { if (timed) E.searchScanMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]); timed = false; };
  for (uint64_t p = 0; p < passes; p++) {
    const uint64_t first = f0 + p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, n - p * passSlots);
    search_launch_jobs(s, arc.table, fs, U, first, nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
    unsigned long long firstError;
    Status st = E.staged_pass(arc, 0, nj, win, &firstError);
    take_time();
    if (st.zra) { E.searchScanMs_ = 0; return st; }
    if (firstError != ~0ull) {                                              // the lowest failing frame of the first failing pass
      E.searchScanMs_ = 0;
      return zerr(reported_code(firstError));
    }
    // (contiguity) the run of this pass, and (ownership) the start positions it owns, relative to slot 0
    const uint64_t passBase = first * fs, passEnd = std::min<uint64_t>(U, (first + nj) * fs), L = passEnd - passBase;
    const long long xLo = lo > passBase ? (long long)(lo - passBase) : -(long long)std::min<uint64_t>(m - 1, passBase - lo);
    const long long xEnd = (long long)(std::min<uint64_t>(passEnd, hi) - passBase) - (long long)m + 1;
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    if (xEnd > xLo) {
      const uint64_t nPos = (uint64_t)(xEnd - xLo);
      const uint32_t tiles = (uint32_t)((nPos + kTile - 1) / kTile);
      hipLaunchKernelGGL(zra_search_count_kernel, dim3(tiles), dim3(256), 0, s, win, xLo, (u64)nPos, pat, (u32)m, counts);
      search_launch_scan(s, counts, tiles, bases, cnt + (launches & 1), cnt + ((launches + 1) & 1));
      launches++;
      if (listCap)
        hipLaunchKernelGGL(zra_search_fill_kernel, dim3(tiles), dim3(256), 0, s, win, xLo, (u64)nPos, pat, (u32)m, counts, bases,
                           (u64)(passBase + xLo), list, (u64)listCap);
    }
    if (p + 1 < passes && m > 1) {
      carry = (uint32_t)std::min<uint64_t>(m - 1, carry + L);
      search_launch_carry(s, win, L, carry);
    }
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    timed = true;
  }
  // ---- the count, then the list, once
  uint64_t total = 0;
  if (launches) HIPCHK_CLR(hipMemcpyAsync(&total, cnt + (launches & 1), 8, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hMatches, list, nOut * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  *nMatches = total;
  const uint64_t st8[8] = {F, n, std::min<uint64_t>(U, (f1 + 1) * fs) - f0 * fs, total, nOut, passes, 0, 0};
  for (int i = 0; i < 8; i++) E.sstats_[i] = st8[i];
  return ok();
}

}  // namespace zra_eng
