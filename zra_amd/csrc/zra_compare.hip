// zra_amd — compare of two device-resident archives (zra_hip.h: ZraHipCompareArchives): the maximal runs of content positions inside a
// content range at which the two archives differ, in ascending order, without an output buffer for either content.
//
//   1. both fixed headers come to the host (Engine::archive_view, A then B); the range becomes frames [f0, f1] of both archives
//   2. per pass of at most passSlots consecutive frames: the two seek-table spans of every frame are compared as they
//      lie, a wave per frame: one flag per slot, equal or decode                                          zra_cmp_spans_kernel
//   3. the decode-flagged frames of the pass, in frame order, become decode jobs of both archives          zra_cmp_jobs_kernel
//   4. the jobs are decoded whole, checksums verified, A into the first half of the window, B into the
//      second; none flagged: the decoder is not launched                                                   Engine::staged_pass, twice
//   5. the two halves are compared a tile per workgroup: run starts and run ends per tile                  zra_cmp_count_kernel
//   6. the tile counts become list positions behind the starts and ends of the earlier passes             zra_cmp_scan_kernel
//   7. tiles that hold a listed start or end redo their compare and write the positions                    zra_cmp_fill_kernel
//   8. the counts and the first rangeCapacity starts and ends come to the host, once; the host writes {start, end - start}
// The staging window (Engine::stage_) is [ half A | half B ], a half = the pass's slots rounded up to 16 bytes: slot s of either half
// lies at s * frameSize of it, so the two plaintexts of a frame share their alignment modulo 16.
//
// The passes run through the one frame-pass driver, flagged and with two sides: their order on the stream, the timed span and which
// failing frame ends the call are stated there (zra_framepass.h). What the kernels of this file rely on:
//  (slots) slot = frame - first frame of the pass, on both sides, whether the frame is decoded or not. A decoded frame that is not the
//      last of the range regenerates frameSize bytes on both sides (anything else is a failing frame and ends the call), so the byte in
//      front of a decoded frame's first byte is the last byte of the slot in front: the window is addressed by arithmetic alone. The
//      slot of an equal-flagged frame, and what lies behind a short last frame, is plaintext of earlier passes and is never read: a
//      tile's positions are clipped to [lo, hi) and hi <= min(UA, UB), the bytes both sides regenerate.
//  (look-behind) with d(p) = "A and B differ at p", a start is d(p) && !(p > lo && d(p - 1)), an end (exclusive) is
//      !d(p) && p > lo && d(p - 1), found by the tile that holds p. Three ends lie at positions no tile holds, and belong to the tile
//      that holds p - 1 (they are the last end of that tile): the end at hi; the end at the first byte of an equal-flagged frame behind
//      a decoded one of the same pass (the flags of a pass are complete before its tiles run); and, when the decoded frame was the last
//      of its pass, the carry: the count launch leaves d(p - 1) in a word, and the next pass reads it: as d(p - 1) of its first tile if
//      its first frame is decoded, else in its item 0, which owns the end at the pass's first byte.
//  (order) the items of a pass are item 0, then the tiles of the decoded frames in content order; starts and ends are counted per item,
//      scanned, and filled independently. Every run has one start and one end, so start i and end i belong together, and a range cut by
//      the capacity never appears. The scan launches are chained by two 64-bit totals that ping-pong between two word pairs, the carry
//      between two words (pass k reads word k & 1 and writes word (k + 1) & 1, which the host zeroed in front of the count launch). A
//      list position is a sum of counts and lane prefixes, never the result of an atomic, and no workgroup waits for another one.
//  (d) nothing goes to the caller's array before the last pass is done: a call that fails midway writes nothing.
// The diff of two archives (zra_hip.h: ZraHipDiffArchives) is the second half of this file: the same passes with the plaintext kept.
#include "zra_framepass.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include <algorithm>

using namespace zra_dev;

namespace {
constexpr u32 kTile = 8192;                  // content positions of one workgroup: the search's tile (zra_search.hip)
constexpr u32 kChunks = kTile / 16 + 1;      // 16-byte loads of a tile that starts behind a 16-byte boundary
constexpr u32 kOwn = 3;                      // consecutive chunks a lane owns when the boundaries are taken: 171 lanes x 3 = 513
constexpr u32 kOwners = kChunks / kOwn;
static_assert(kOwners * kOwn == kChunks && kOwners <= 256, "every chunk has one owner");
// the table words in front of the per-item entries (bytes): totals {starts, ends} x 2 | differing bytes | content bytes compared |
// carry x 2 (u32) | decode jobs of the pass (u32)
constexpr u32 kHdrBytes = 64, kOffDiff = 32, kOffBytes = 40, kOffCarry = 48, kOffJobs = 56;

// bit j = byte j of the 16 is not zero
__device__ __forceinline__ u32 nonzero_bytes(uint4 x) {
  auto four = [](u32 w) {
    const u32 b = ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;
    return (b | (b >> 7) | (b >> 14) | (b >> 21)) & 0xFu;
  };
  return four(x.x) | (four(x.y) << 4) | (four(x.z) << 8) | (four(x.w) << 12);
}
// bits j of a chunk whose byte 0 is tile position r0 with a <= r0 + j < b
__device__ __forceinline__ u32 valid_bits(int r0, int a, int b) {
  const int l = min(16, max(0, a - r0)), h = min(16, max(0, b - r0));
  return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}

struct TileArgs {
  const u8* winA; const u8* winB;            // slot 0 of the two halves
  const u64* outOff; const u8* flags;        // job -> slot * frameSize; slot -> 1 decode, 0 equal
  u64 fs, first, lo, hi;
  u32 nj, tpf;                               // slots of the pass, tiles per frame
  const u32* carryIn;
};
// What one tile found: the run starts and ends among the positions its lane owns (st / en: bit j of word q = byte j of chunk
// kOwn * tid + q), their counts over the workgroup (per wave: sRed[w] starts, sRed[4 + w] ends), the differing bytes, the end no
// position of the tile holds (look-behind), the carry.
struct TileOut {
  u32 st[kOwn], en[kOwn];
  u32 nS, nE;                                // this lane's
  u32 totS, totE, totDiff;                   // the workgroup's
  bool extraEnd, carryOut;
  u64 extraAt, pos0;                         // content position of the extra end; of byte 0 of chunk 0
};

// Item `item` (>= 0: job item / tpf, tile item % tpf of its frame) of a pass. The tile's positions are [a, b) of its frame, clipped to
// [lo, hi) and the frame size by arithmetic. Both halves are loaded with 16-byte loads from the aligned address at or below the tile's
// first byte (the halves share their alignment), only chunks that hold a position of [a, b): at most 15 bytes in front of it (inside
// the window: slot 0 is aligned) and 15 behind (inside the window's slack). sM: kChunks + 3 words.
// The tile's place (item -> slot s of the pass, tile t0 of its frame, positions [a64, b64) of the frame) ...
#define ZRA_TILE_GEOMETRY(T, item)                                                                   \
  const u32 k = (item) / (T).tpf, t = (item) % (T).tpf;                                              \
  const u64 off = (T).outOff[k];                                                                     \
  const u32 s = (u32)(off / (T).fs);                                                                 \
  const u64 fBase = ((T).first + s) * (T).fs, t0 = (u64)t * kTile;                                   \
  const u64 iLo = (T).lo > fBase ? (T).lo - fBase : 0, iHi = min((T).fs, (T).hi - fBase);            \
  const u64 a64 = max(t0, iLo), b64 = min(t0 + kTile, iHi)
// ... and its difference bits in ADDRESS space: bit j of sM[c + 1] = byte j of chunk c of the two halves differs and is position
// 16 c + j - d of the tile, inside [a, b); chunk c = the 16 bytes at gA + c / gB + c. sM[1 .. kChunks + 2] are written.
__device__ __forceinline__ void tile_bits(const uint4* gA, const uint4* gB, u32 d, int a, int b, u32* sM) {
  for (u32 c = threadIdx.x; c < kChunks + 2; c += 256) {
    const int r0 = (int)(16 * c) - (int)d;
    u32 m = 0;
    if (c < kChunks && r0 < b && r0 + 16 > a) {
      const uint4 x = gA[c], y = gB[c];
      m = nonzero_bytes(make_uint4(x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w)) & valid_bits(r0, a, b);
    }
    sM[c + 1] = m;                                                            // bit j of word c + 1 = position 16 (c + 1) + j - 16 - d of the tile
  }
}

__device__ __forceinline__ void diff_tile(const TileArgs& T, u32 item, u32* sM, u32* sRed, TileOut& o) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ZRA_TILE_GEOMETRY(T, item);
  for (u32 q = 0; q < kOwn; q++) o.st[q] = o.en[q] = 0;
  o.nS = o.nE = o.totS = o.totE = o.totDiff = 0; o.extraEnd = o.carryOut = false; o.extraAt = 0; o.pos0 = 0;
  if (a64 >= b64) return;                                                     // (uniform in the workgroup)
  const int a = (int)(a64 - t0), b = (int)(b64 - t0);
  const u8* const pA = T.winA + off + t0; const u8* const pB = T.winB + off + t0;
  const u32 d = (u32)((size_t)pA & 15);
  const uint4* const gA = (const uint4*)(pA - d); const uint4* const gB = (const uint4*)(pB - d);
  o.pos0 = fBase + t0 - d;
  // d(p - 1) of the tile's first position (look-behind)
  bool prev = false;
  if (tid == 0 && fBase + a64 != T.lo) {
    if (a64 > 0) prev = pA[a - 1] != pB[a - 1];                               // the same frame, or the tile in front
    else if (s > 0) prev = T.flags[s - 1] && pA[-1] != pB[-1];                // the frame in front: decoded in this pass, or equal
    else prev = *T.carryIn != 0;                                              // the last frame of the pass in front
  }
  tile_bits(gA, gB, d, a, b, sM);
  if (tid == 0) sM[0] = 0;
  __syncthreads();
  if (tid == 0 && prev) { const u32 e = (u32)a + d + 15; sM[e >> 4] |= 1u << (e & 15); }   // position a - 1: outside the valid bits, seen as a predecessor
  __syncthreads();
  u32 diff = 0;
  if (tid < kOwners) {
#pragma unroll
    for (u32 q = 0; q < kOwn; q++) {
      const u32 c = kOwn * tid + q;
      const u32 m = sM[c + 1], before = ((m << 1) | (sM[c] >> 15)) & 0xFFFFu, v = valid_bits((int)(16 * c) - (int)d, a, b);
      o.st[q] = m & ~before & v;
      o.en[q] = ~m & before & v;
      o.nS += (u32)__popc(o.st[q]); o.nE += (u32)__popc(o.en[q]); diff += (u32)__popc(m & v);
    }
  }
  const u32 wS = wave_sum(o.nS), wE = wave_sum(o.nE), wD = wave_sum(diff);
  if (lane == 0) { sRed[wave] = wS; sRed[4 + wave] = wE; sRed[8 + wave] = wD; }
  __syncthreads();
  for (u32 w = 0; w < 4; w++) { o.totS += sRed[w]; o.totE += sRed[4 + w]; o.totDiff += sRed[8 + w]; }
  // the end behind the frame's last position of the range, when no tile holds it
  const u32 eL = (u32)b - 1 + d + 16;
  if (b64 == iHi && ((sM[eL >> 4] >> (eL & 15)) & 1)) {
    o.extraAt = fBase + b64;
    if (o.extraAt == T.hi) o.extraEnd = true;
    else if (s + 1 < T.nj) o.extraEnd = T.flags[s + 1] == 0;
    else o.carryOut = true;
  }
}
}  // namespace

// Wave per frame of a pass: flags[j] = 0 when the two seek-table spans of frame first + j are well formed (the decoder's convention:
// a <= b <= body size), equally long and hold the same bytes; 1 otherwise: the frame is decoded. Only bytes of the two spans are read.
// The spans start at unrelated alignments: up to 15 head bytes bring side A to a 16-byte boundary, then 16-byte vectors (A aligned,
// B as it lies), four per lane and trip, then up to 15 tail bytes. The wave leaves on the first trip with a differing vector.
// The compare is exact for every length, 0 included: two identical spans too short to be a frame (fewer than 9 bytes) are equal on
// purpose, like any other pair of identical damaged frames (zra_hip.h: compare is not verify).
extern "C" __global__ void __launch_bounds__(256) zra_cmp_spans_kernel(const u8* tableA, const u8* bodyA, u64 bodyBytesA, const u8* tableB, const u8* bodyB,
                                                                       u64 bodyBytesB, u64 first, u32 nj, u8* flags) {
  const u32 j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= nj) return;                                                        // (uniform in the wave)
  const u64 f = first + j;
  const u64 a0 = seek_entry(tableA, f), a1 = seek_entry(tableA, f + 1), b0 = seek_entry(tableB, f), b1 = seek_entry(tableB, f + 1);
  bool decode = !(a0 <= a1 && a1 <= bodyBytesA && b0 <= b1 && b1 <= bodyBytesB && a1 - a0 == b1 - b0);
  if (!decode) {
    const u64 n = a1 - a0;
    const u8* pa = bodyA + a0; const u8* pb = bodyB + b0;
    const u32 head = (u32)min<u64>(n, (16u - (u32)((size_t)pa & 15)) & 15u);
    bool differ = lane < head && pa[lane] != pb[lane];
    pa += head; pb += head;
    const u64 nv = (n - head) >> 4;
    const u32 tail = (u32)((n - head) & 15);
    if (lane < tail) differ |= pa[16 * nv + lane] != pb[16 * nv + lane];
    const uint4* const va = (const uint4*)pa;
    const u128_u* const vb = (const u128_u*)pb;
    for (u64 i0 = 0; i0 < nv && !__any(differ); i0 += 256) {
      uint4 x[4]; u128_u y[4];
#pragma unroll
      for (u32 q = 0; q < 4; q++) {
        const u64 i = i0 + 64 * q + lane;
        if (i < nv) { x[q] = va[i]; y[q] = vb[i]; } else { x[q] = make_uint4(0, 0, 0, 0); y[q].a = y[q].b = y[q].c = y[q].d = 0; }
      }
#pragma unroll
      for (u32 q = 0; q < 4; q++) differ |= ((x[q].x ^ y[q].a) | (x[q].y ^ y[q].b) | (x[q].z ^ y[q].c) | (x[q].w ^ y[q].d)) != 0;
    }
    decode = __any(differ);
  }
  if (lane == 0) flags[j] = decode ? 1 : 0;
}

// One workgroup walks the slots of the pass, 1024 at a time: the decode-flagged ones, in order, become jobs 0 .. nDec - 1 of archive A
// (zra_joblist.h: block_rank, emit_job at job k) and of archive B (at job jobsB + k); outOff[k] = the slot's place in its half, the
// same for both. A job has to regenerate its frame's share of its own archive's content. hdr: the job count for the host, and the
// content bytes of [lo, hi) inside the decoded frames, summed.
extern "C" __global__ void __launch_bounds__(1024) zra_cmp_jobs_kernel(const u8* flags, u32 nj, const u8* tableA, u64 UA, const u8* tableB, u64 UB, u64 fs,
                                                                       u64 first, u64 lo, u64 hi, u64* frameOff, u64* outOff, u32* expect, u32 jobsB, u8* hdr) {
  u32 jobBase = 0;
  u64 bytes[1] = {0}, allBytes[1];
  for (u32 base = 0; base < nj; base += 1024) {
    const u32 s = base + threadIdx.x;
    const bool p[1] = {s < nj && flags[s] != 0};
    u32 rank[1], total[1];
    block_rank<1>(p, rank, total);
    if (p[0]) {
      const u64 f = first + s;
      const size_t k = jobBase + rank[0];
      emit_job(tableA, f, fs, UA, k, s, frameOff, outOff, expect);
      emit_job(tableB, f, fs, UB, (size_t)jobsB + k, s, frameOff, nullptr, expect);
      bytes[0] += min(hi, (f + 1) * fs) - max(lo, f * fs);
    }
    jobBase += total[0];
  }
  block_excl_scan<1>(bytes, allBytes);
  if (threadIdx.x == 0) { *(u32*)(hdr + kOffJobs) = jobBase; *(u64*)(hdr + kOffBytes) += allBytes[0]; }
}

// Workgroup 0 is item 0 of the pass (the end at the pass's first byte, when the pass in front left a run open and the first frame is
// equal); workgroup i > 0: tile i - 1 of the decoded frames. tab[2 i] = the item's starts, tab[2 i + 1] = its ends. The differing
// bytes are summed into one word (a sum, not a position); the tile behind which the pass ends leaves the carry.
extern "C" __global__ void __launch_bounds__(256) zra_cmp_count_kernel(TileArgs T, u64* tab, u64* diffBytes, u32* carryOut) {
  __shared__ u32 sM[kChunks + 3], sRed[12];
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) { tab[0] = 0; tab[1] = (*T.carryIn != 0 && T.flags[0] == 0) ? 1 : 0; }
    return;
  }
  TileOut o;
  diff_tile(T, blockIdx.x - 1, sM, sRed, o);
  if (threadIdx.x == 0) {
    tab[2 * (size_t)blockIdx.x] = o.totS; tab[2 * (size_t)blockIdx.x + 1] = o.totE + (o.extraEnd ? 1 : 0);
    if (o.totDiff) atomicAdd((unsigned long long*)diffBytes, (unsigned long long)o.totDiff);
    if (o.carryOut) *carryOut = 1;
  }
}

// One workgroup, in place: tab[2 i] / tab[2 i + 1] = totIn + the starts / ends of the items in front of item i, for i = 0 .. nItems
// (entry nItems: behind all of them; an item's own counts are the difference to the next entry); totOut = that last entry
// (zra_joblist.h, scan_in_place).
extern "C" __global__ void __launch_bounds__(1024) zra_cmp_scan_kernel(u64* tab, u32 nItems, const u64* totIn, u64* totOut) {
  scan_in_place<2>(tab, nItems, totIn, totOut);
}

// Workgroup i redoes item i's compare when one of its starts or ends has a place in the lists (an item without any, or behind the
// capacity, leaves at once). A start's place is the item's base, plus the starts of the waves in front of its own, plus those of the
// lanes in front of its own (a prefix sum over the wave), plus those in front of it in its lane; an end's likewise.
extern "C" __global__ void __launch_bounds__(256) zra_cmp_fill_kernel(TileArgs T, const u64* tab, u64* starts, u64* ends, u64 cap) {
  __shared__ u32 sM[kChunks + 3], sRed[12];
  const u64 baseS = tab[2 * (size_t)blockIdx.x], baseE = tab[2 * (size_t)blockIdx.x + 1];
  const u64 cntS = tab[2 * (size_t)blockIdx.x + 2] - baseS, cntE = tab[2 * (size_t)blockIdx.x + 3] - baseE;
  if ((cntS == 0 || baseS >= cap) && (cntE == 0 || baseE >= cap)) return;   // (uniform in the workgroup)
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) ends[baseE] = T.first * T.fs;                       // (cntE == 1 and baseE < cap)
    return;
  }
  TileOut o;
  diff_tile(T, blockIdx.x - 1, sM, sRed, o);
  const u32 tid = threadIdx.x, wave = tid >> 6;
  u64 atS = baseS + wave_incl_scan(o.nS) - o.nS, atE = baseE + wave_incl_scan(o.nE) - o.nE;
  for (u32 w = 0; w < wave; w++) { atS += sRed[w]; atE += sRed[4 + w]; }
#pragma unroll
  for (u32 q = 0; q < kOwn; q++) {
    const u64 p = o.pos0 + 16 * (u64)(kOwn * tid + q);
    for (u32 m = o.st[q]; m; m &= m - 1, atS++) if (atS < cap) starts[atS] = p + (u32)__builtin_ctz(m);
    for (u32 m = o.en[q]; m; m &= m - 1, atE++) if (atE < cap) ends[atE] = p + (u32)__builtin_ctz(m);
  }
  if (tid == 0 && o.extraEnd && baseE + o.totE < cap) ends[baseE + o.totE] = o.extraAt;
}

// =================================================================================================
// Diff (zra_hip.h: ZraHipDiffArchives): the compare over [0, C) with the plaintext kept. The passes, the span compare, the job build
// and the two staged_pass calls are the compare's. A tile's difference bits become a DIRTY-GRAIN mask, the runs of that mask are the
// writes, and the fill copies B's bytes of the dirty grains, packed, to the caller's buffer; B's content behind C follows in passes
// of its own. The four ordering conditions above hold with "dirty grain" in place of d(p):
//  (slots) unchanged. Frame f's grains are counted from the frame's first byte and grain divides kTile, so a grain lies inside one
//      tile of one decoded frame: its bits come from bytes the pass regenerated, clipped to the frame and to C by arithmetic.
//  (look-behind) D(p) = "the grain that holds p is dirty". D(p - 1) of a tile's first position is the grain in front: the last one of
//      the tile in front, or the (possibly short) last one of the frame in front when that frame was decoded in this pass, whose bytes
//      the workgroup compares itself; 0 in front of position 0 and behind an equal-flagged frame; the carry word behind the last frame
//      of the pass in front. The three tile-less ends (at C, in front of an equal-flagged frame, the pass carry) are the compare's.
//  (order) three columns per item: starts, ends, dirty bytes; three 64-bit totals ping-pong between passes. A list position and a
//      byte's place in the packed data are sums of counts and prefixes, never the result of an atomic.
//  (d) the lists stay on the device until the last pass is done; dData alone is written while the passes run, never at or behind
//      dataCapacity.
namespace {
constexpr u32 kWords = kTile / 16;           // 16-bit words of a tile's mask in tile-position space: a lane owns words 2 tid and 2 tid + 1
// the diff's table words in front of the per-item entries (bytes): dirty grains at kOffDiff | kOffBytes, kOffCarry, kOffJobs as above (the
// job build writes them) | totals {starts, ends, dirty bytes} x 2
constexpr u32 kDiffHdrBytes = 128, kOffTot3 = 64;

struct GrainOut {
  u32 st[2], en[2], dm[2];                   // starts, ends and dirty positions of the lane's two words (bit j = tile position 16 w + j)
  u32 nS, nE, nB;                            // this lane's
  u32 totS, totE, totB, totG;                // the workgroup's; totG: dirty grains
  bool extraEnd, carryOut;
  u64 extraAt, pos0;                         // content position of the extra end; of tile position 0
  const u8* pB;                              // B's byte at tile position 0
};

// Item `item` of a pass as diff_tile takes it, lo = 0: the tile's positions are [0, b). sM: kChunks + 3 words, sD: kWords + 1,
// sRed: 20. The difference bits are built in address space (tile_bits: chunk c starts d bytes in front of the tile when the slot is
// not 16-byte aligned), re-indexed to tile positions, smeared over their grains (inside a word for grain <= 16, over grain / 16
// words above), and clipped to [0, b) again: the last grain of a frame, or the one that holds C, is short.
__device__ __forceinline__ void grain_tile(const TileArgs& T, u32 item, u32 grain, u32* sM, u32* sD, u32* sRed, GrainOut& o) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ZRA_TILE_GEOMETRY(T, item);
  for (u32 q = 0; q < 2; q++) o.st[q] = o.en[q] = o.dm[q] = 0;
  o.nS = o.nE = o.nB = o.totS = o.totE = o.totB = o.totG = 0; o.extraEnd = o.carryOut = false; o.extraAt = 0; o.pos0 = fBase + t0; o.pB = nullptr;
  if (a64 >= b64) return;                                                     // (uniform in the workgroup)
  const int b = (int)(b64 - t0);                                              // (a64 == t0: lo is 0)
  const u8* const pA = T.winA + off + t0; const u8* const pB = T.winB + off + t0;
  const u32 d = (u32)((size_t)pA & 15);
  o.pB = pB;
  tile_bits((const uint4*)(pA - d), (const uint4*)(pB - d), d, 0, b, sM);
  // (look-behind) the grain in front of position 0: n bytes that end at pA / pB, compared by the whole workgroup; or the carry
  u32 n = 0;
  if (t0 > 0) n = grain;                                                      // the last grain of the tile in front
  else if (s > 0) n = T.flags[s - 1] ? (u32)(T.fs - ((T.fs - 1) / grain) * grain) : 0;   // the last grain of the frame in front: decoded in this pass, or equal
  int behind = tid == 0 && t0 == 0 && s == 0 && fBase != 0 && *T.carryIn != 0;           // the last frame of the pass in front
  if (n) {
    const u8* const qA = pA - n;
    const u32 d0 = (u32)((size_t)qA & 15);                                    // (the halves share their alignment; qA - d0 is inside the window: slot 0 is aligned)
    const uint4* const hA = (const uint4*)(qA - d0); const uint4* const hB = (const uint4*)(pB - n - d0);
    for (u32 c = tid; c < (d0 + n + 15) / 16; c += 256) {
      const uint4 x = hA[c], y = hB[c];
      behind |= (nonzero_bytes(make_uint4(x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w)) & valid_bits((int)(16 * c) - (int)d0, 0, (int)n)) != 0;
    }
  }
  const bool prev = __syncthreads_or(behind) != 0;                            // (and sM is complete)
  // address space -> tile positions: position 16 w + i is bit 16 w + i + d of the address-space mask
  u32 g[2], grains = 0;
  bool any = false;
#pragma unroll
  for (u32 q = 0; q < 2; q++) {
    const u32 w = 2 * tid + q;
    g[q] = ((sM[w + 1] >> d) | (sM[w + 2] << (16 - d))) & 0xFFFFu;
    if (grain <= 16) {                                                        // bit i of x = a difference in positions i .. i + grain - 1; a grain starts at every multiple of `grain`
      u32 x = g[q];
      for (u32 sh = 1; sh < grain; sh <<= 1) x |= x >> sh;
      x &= 0xFFFFu / ((1u << grain) - 1u);                                    // (0x5555 for 2, 0x1111 for 4, 0x0101 for 8, 1 for 16)
      grains += (u32)__popc(x);
      g[q] = x * ((1u << grain) - 1u);
    }
    any |= g[q] != 0;
  }
  // grain > 16: the grain's grain / 16 words belong to H = grain / 32 consecutive lanes (a lane's two words lie in one grain)
  const unsigned long long lanes = __ballot(any);
  if (lane == 0) sRed[16 + wave] = lanes != 0;
  __syncthreads();
  if (grain > 16) {
    const u32 H = grain / 32;
    bool dirty;
    if (H <= 64) dirty = ((lanes >> (lane & ~(H - 1))) & (H == 64 ? ~0ull : (1ull << H) - 1)) != 0;
    else { dirty = false; for (u32 w = wave & ~(H / 64 - 1), e = w + H / 64; w < e; w++) dirty |= sRed[16 + w] != 0; }
    g[0] = g[1] = dirty ? 0xFFFFu : 0u;
    grains = dirty && (tid & (H - 1)) == 0;
  }
#pragma unroll
  for (u32 q = 0; q < 2; q++) { o.dm[q] = g[q] & valid_bits((int)(16 * (2 * tid + q)), 0, b); sD[2 * tid + q + 1] = o.dm[q]; }
  if (tid == 0) sD[0] = prev ? 0x8000u : 0u;
  __syncthreads();
#pragma unroll
  for (u32 q = 0; q < 2; q++) {
    const u32 w = 2 * tid + q, m = o.dm[q], before = ((m << 1) | (sD[w] >> 15)) & 0xFFFFu, v = valid_bits((int)(16 * w), 0, b);
    o.st[q] = m & ~before & v;
    o.en[q] = ~m & before & v;
    o.nS += (u32)__popc(o.st[q]); o.nE += (u32)__popc(o.en[q]); o.nB += (u32)__popc(m);
  }
  const u32 wS = wave_sum(o.nS), wE = wave_sum(o.nE), wB = wave_sum(o.nB), wG = wave_sum(grains);
  if (lane == 0) { sRed[wave] = wS; sRed[4 + wave] = wE; sRed[8 + wave] = wB; sRed[12 + wave] = wG; }
  __syncthreads();
  for (u32 w = 0; w < 4; w++) { o.totS += sRed[w]; o.totE += sRed[4 + w]; o.totB += sRed[8 + w]; o.totG += sRed[12 + w]; }
  // the end behind the frame's last position of [0, C), when no tile holds it
  const u32 eL = (u32)b - 1;
  if (b64 == iHi && ((sD[(eL >> 4) + 1] >> (eL & 15)) & 1)) {
    o.extraAt = fBase + b64;
    if (o.extraAt == T.hi) o.extraEnd = true;
    else if (s + 1 < T.nj) o.extraEnd = T.flags[s + 1] == 0;
    else o.carryOut = true;
  }
}
}  // namespace

// zra_cmp_count_kernel for grains: tab[3 i] = the item's starts, tab[3 i + 1] = its ends, tab[3 i + 2] = its dirty bytes. The dirty
// grains are summed into one word (a sum, not a position).
extern "C" __global__ void __launch_bounds__(256) zra_diff_count_kernel(TileArgs T, u32 grain, u64* tab, u64* grains, u32* carryOut) {
  __shared__ u32 sM[kChunks + 3], sD[kWords + 1], sRed[20];
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) { tab[0] = 0; tab[1] = (*T.carryIn != 0 && T.flags[0] == 0) ? 1 : 0; tab[2] = 0; }
    return;
  }
  GrainOut o;
  grain_tile(T, blockIdx.x - 1, grain, sM, sD, sRed, o);
  if (threadIdx.x == 0) {
    u64* const e = tab + 3 * (size_t)blockIdx.x;
    e[0] = o.totS; e[1] = o.totE + (o.extraEnd ? 1 : 0); e[2] = o.totB;
    if (o.totG) atomicAdd((unsigned long long*)grains, (unsigned long long)o.totG);
    if (o.carryOut) *carryOut = 1;
  }
}

// zra_cmp_scan_kernel's table with three columns: tab[3 i + c] = totIn[c] + column c of the items in front of item i, for
// i = 0 .. nItems; totOut = the last entry.
extern "C" __global__ void __launch_bounds__(1024) zra_diff_scan_kernel(u64* tab, u32 nItems, const u64* totIn, u64* totOut) {
  scan_in_place<3>(tab, nItems, totIn, totOut);
}

// Workgroup i redoes item i's mask when it holds a listed start or end, or a dirty byte with a place in front of dataCap (an item
// without any leaves at once). Starts and ends as zra_cmp_fill_kernel. A dirty byte's place in dData is the item's base, plus the
// dirty bytes of the waves, lanes and words in front. A whole dirty word (16 positions: every word of a grain >= 16 but a clipped
// one) whose place is 16-byte aligned leaves as one 16-byte store; anything else byte by byte, each byte checked against dataCap.
extern "C" __global__ void __launch_bounds__(256) zra_diff_fill_kernel(TileArgs T, u32 grain, const u64* tab, u64* starts, u64* ends, u64 cap, u8* dData,
                                                                       u64 dataCap) {
  __shared__ u32 sM[kChunks + 3], sD[kWords + 1], sRed[20];
  const u64* const e = tab + 3 * (size_t)blockIdx.x;
  const u64 baseS = e[0], baseE = e[1], baseB = e[2];
  const u64 cntS = e[3] - baseS, cntE = e[4] - baseE, cntB = e[5] - baseB;
  if ((cntS == 0 || baseS >= cap) && (cntE == 0 || baseE >= cap) && (cntB == 0 || baseB >= dataCap)) return;   // (uniform in the workgroup)
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) ends[baseE] = T.first * T.fs;                       // (cntE == 1 and baseE < cap)
    return;
  }
  GrainOut o;
  grain_tile(T, blockIdx.x - 1, grain, sM, sD, sRed, o);
  const u32 tid = threadIdx.x, wave = tid >> 6;
  u64 atS = baseS + wave_incl_scan(o.nS) - o.nS, atE = baseE + wave_incl_scan(o.nE) - o.nE, atB = baseB + wave_incl_scan(o.nB) - o.nB;
  for (u32 w = 0; w < wave; w++) { atS += sRed[w]; atE += sRed[4 + w]; atB += sRed[8 + w]; }
#pragma unroll
  for (u32 q = 0; q < 2; q++) {
    const u32 r = 16 * (2 * tid + q);
    const u64 p = o.pos0 + r;
    for (u32 m = o.st[q]; m; m &= m - 1, atS++) if (atS < cap) starts[atS] = p + (u32)__builtin_ctz(m);
    for (u32 m = o.en[q]; m; m &= m - 1, atE++) if (atE < cap) ends[atE] = p + (u32)__builtin_ctz(m);
    const u8* const src = o.pB + r;
    if (o.dm[q] == 0xFFFFu && atB + 16 <= dataCap && (((size_t)dData + atB) & 15) == 0) {
      const u128_u v = *(const u128_u*)src;
      *(uint4*)(dData + atB) = make_uint4(v.a, v.b, v.c, v.d);
      atB += 16;
    } else {
      for (u32 m = o.dm[q]; m; m &= m - 1, atB++) if (atB < dataCap) dData[atB] = src[__builtin_ctz(m)];
    }
  }
  if (tid == 0 && o.extraEnd && baseE + o.totE < cap) ends[baseE + o.totE] = o.extraAt;
}

// B's content behind C: the n bytes at src (one pass's run of the window) go to dData + *dirtyBytes + tailOff, 16 per lane, clipped
// byte-exactly at dataCap. The base is read on the device: the dirty-bytes total of the last pair pass.
extern "C" __global__ void __launch_bounds__(256) zra_diff_tail_kernel(const u8* src, u64 n, const u64* dirtyBytes, u64 tailOff, u8* dData, u64 dataCap) {
  const u64 i = ((u64)blockIdx.x * 256 + threadIdx.x) * 16;
  if (i >= n) return;
  const u64 at = *dirtyBytes + tailOff + i;
  if (i + 16 <= n && at + 16 <= dataCap && (((size_t)dData + at) & 15) == 0) {
    const u128_u v = *(const u128_u*)(src + i);
    *(uint4*)(dData + at) = make_uint4(v.a, v.b, v.c, v.d);
  } else {
    for (u32 j = 0; j < 16 && i + j < n; j++) if (at + j < dataCap) dData[at + j] = src[i + j];
  }
}

// =================================================================================================
namespace zra_eng {

void diff_launch_scan(hipStream_t s, uint64_t* tab, uint32_t nItems, const uint64_t* totIn, uint64_t* totOut) {
  hipLaunchKernelGGL(zra_diff_scan_kernel, dim3(1), dim3(1024), 0, s, (u64*)tab, nItems, (const u64*)totIn, (u64*)totOut);
}
void diff_launch_tail(hipStream_t s, const uint8_t* src, uint64_t n, const uint64_t* dirtyBytes, uint64_t tailOff, uint8_t* dData, uint64_t dataCap) {
  hipLaunchKernelGGL(zra_diff_tail_kernel, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, s, src, (u64)n, (const u64*)dirtyBytes, (u64)tailOff, dData, (u64)dataCap);
}

namespace {
constexpr uint32_t kDecodeAll = 1u;                                           // ZRA_HIP_COMPARE_DECODE_ALL, ZRA_HIP_DIFF_DECODE_ALL

// The pair passes of compare and diff over the frames of [lo, hi): the passes run through the one driver (zra_framepass.h), flagged,
// two sides. `before` is the same for both calls (steps 2 and 3 of the file head), `after` the call's own tile launches.
struct PairPasses {
  FramePasses& F;
  const ArchiveView& A; const ArchiveView& B;
  uint64_t fs, lo, hi;
  PassPlan P;
  uint64_t half;
  uint32_t tpf;
  uint8_t* winB() const { return F.win + half; }
  uint32_t* carry() const { return (uint32_t*)(F.tables + kOffCarry); }
  const uint32_t* job_count() const { return (const uint32_t*)(F.tables + kOffJobs); }
  size_t items_max() const { return 1 + (size_t)P.nSlots * tpf; }

  Status before(uint32_t mode, const FramePass& ps) const {
    if (mode & kDecodeAll) HIPCHK_CLR(hipMemsetAsync(F.flags, 1, ps.nj, F.s));
    else
      hipLaunchKernelGGL(zra_cmp_spans_kernel, dim3((ps.nj + 3) / 4), dim3(256), 0, F.s, A.table, A.body, (u64)A.bodyBytes, B.table, B.body, (u64)B.bodyBytes,
                         (u64)ps.first, ps.nj, F.flags);
    hipLaunchKernelGGL(zra_cmp_jobs_kernel, dim3(1), dim3(1024), 0, F.s, F.flags, ps.nj, A.table, (u64)A.U, B.table, (u64)B.U, (u64)fs, (u64)ps.first, (u64)lo, (u64)hi,
                       F.frameOff, F.outOff, F.expect, P.nSlots, F.tables);
    return ok();
  }
  // (look-behind) the tiles of a pass: item 0 and tpf tiles per decoded frame; the carry word the pass writes is zeroed first
  Status tiles(const FramePass& ps, TileArgs* T) const {
    T->winA = F.win; T->winB = winB(); T->outOff = F.outOff; T->flags = F.flags; T->fs = fs; T->first = ps.first; T->lo = lo; T->hi = hi; T->nj = ps.nj; T->tpf = tpf;
    T->carryIn = carry() + ps.parity;
    HIPCHK_CLR(hipMemsetAsync(carry() + (ps.parity ^ 1), 0, 4, F.s));
    return ok();
  }
  template <class After>
  Status run(uint32_t mode, uint64_t* decoded, After&& after) {
    const FramePasses::Side a{&A, 0, F.win}, b{&B, P.nSlots, winB()};
    return F.run(P, a, &b, job_count(), decoded, [&](const FramePass& ps) { return before(mode, ps); }, after);
  }
};
PairPasses pair_passes(FramePasses& F, const ArchiveView& A, const ArchiveView& B, uint64_t lo, uint64_t hi, size_t stagingBytes) {
  const uint64_t fs = A.fs, f0 = lo / fs, n = hi > lo ? (hi - 1) / fs - f0 + 1 : 0;   // (frames of both archives: hi <= C, and ra_header ties frames to U)
  const PassPlan P = pass_plan(f0, n, pair_pass_slots(fs, stagingBytes));
  return PairPasses{F, A, B, fs, lo, hi, P, pair_half(P.nSlots, fs), (uint32_t)((fs + kTile - 1) / kTile)};
}
// 2. headers, A then B: the statuses of ZraHipArchiveOpen. (The headers' CRC-32 is not looked at: that is the verifier's job.) 3. one frame size
Status pair_views(Engine& E, const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, ArchiveView* A, ArchiveView* B) {
  STCHK(E.archive_view(dA, sizeA, A));
  if (A->fs == 0) return {kHeaderInvalid, 0};
  STCHK(E.archive_view(dB, sizeB, B));
  if (B->fs == 0) return {kHeaderInvalid, 0};
  return A->fs != B->fs ? zerr(40) : ok();
}

Status compare_run(Engine& E, uint64_t (&stats)[8], double* ms, uint64_t sizes[2], const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode,
                   uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRanges, size_t rangeCap, uint64_t* nRanges, uint64_t* differingBytes) {
  // ---- 1. arguments
  if (!nRanges || (!dA && sizeA) || (!dB && sizeB) || (!hRanges && rangeCap) || (mode & ~kDecodeAll)) return zerr(42);
  FramePasses F(E, ms);
  STCHK(F.start());
  // ---- 2. headers, 3. one frame size
  ArchiveView A, B;
  STCHK(pair_views(E, dA, sizeA, dB, sizeB, &A, &B));
  // ---- 4. the range [lo, hi) of the common content, inclusive bound (the range rule of the scans)
  uint64_t lo, hi;
  if (!scan_range(std::min(A.U, B.U), offset, size, &lo, &hi)) return {kOutOfBounds, 0};
  if (hi == lo) { sizes[0] = A.U; sizes[1] = B.U; return ok(); }
  // ---- 5. scratch
  PairPasses X = pair_passes(F, A, B, lo, hi, stagingBytes);
  const PassPlan& P = X.P;
  const size_t listCap = (size_t)std::min<uint64_t>(rangeCap, (hi - lo + 1) / 2);   // (runs are at least one byte long and one byte apart)
  STCHK(F.open({(size_t)(2 * X.half) + 64, (size_t)P.nSlots + 64, 0, kHdrBytes + (X.items_max() + 1) * 16 + 64, listCap * 16 + 64, 2 * (size_t)P.nSlots, P.nSlots}));
  uint8_t* const hdr = F.tables;
  uint64_t* const tot = (uint64_t*)hdr;
  uint64_t* const tab = (uint64_t*)(hdr + kHdrBytes);
  uint64_t* const starts = F.list;
  uint64_t* const ends = starts + listCap;
  // ---- passes
  uint64_t decoded = 0;
  STCHK(F.begin(hdr, kHdrBytes));
  STCHK(X.run(mode, &decoded, [&](const FramePass& ps, uint32_t nDec) {
      const uint32_t items = 1 + nDec * X.tpf;
      TileArgs T;
      STCHK(X.tiles(ps, &T));
      hipLaunchKernelGGL(zra_cmp_count_kernel, dim3(items), dim3(256), 0, F.s, T, tab, (u64*)(hdr + kOffDiff), X.carry() + (ps.parity ^ 1));
      hipLaunchKernelGGL(zra_cmp_scan_kernel, dim3(1), dim3(1024), 0, F.s, tab, items, tot + 2 * ps.parity, tot + 2 * (ps.parity ^ 1));
      if (listCap) hipLaunchKernelGGL(zra_cmp_fill_kernel, dim3(items), dim3(256), 0, F.s, T, tab, starts, ends, (u64)listCap);
      return ok();
    }));
  // ---- the counts, then the lists, once
  uint64_t h8[8] = {0};
  STCHK(F.finish(h8, hdr, kHdrBytes));
  const uint64_t total = h8[2 * (P.passes & 1)];
  if (h8[2 * (P.passes & 1) + 1] != total) return zerr(1);                    // (cannot happen: every run has one start and one end)
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    std::vector<uint64_t> se(2 * nOut);
    HIPCHK_CLR(hipMemcpyAsync(se.data(), starts, nOut * 8, hipMemcpyDeviceToHost, F.s));
    HIPCHK_CLR(hipMemcpyAsync(se.data() + nOut, ends, nOut * 8, hipMemcpyDeviceToHost, F.s));
    HIPCHK_CLR(hipStreamSynchronize(F.s));
    for (size_t i = 0; i < nOut; i++) { hRanges[2 * i] = se[i]; hRanges[2 * i + 1] = se[nOut + i] - se[i]; }
  }
  *nRanges = total;
  if (differingBytes) *differingBytes = h8[kOffDiff / 8];
  const uint64_t st8[8] = {P.n, P.n - decoded, decoded, h8[kOffBytes / 8], total, nOut, P.passes, 0};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  sizes[0] = A.U; sizes[1] = B.U;
  return ok();
}

Status diff_run(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode, uint32_t grain,
                size_t stagingBytes, const PatchOut& out) {
  // ---- 1. arguments, 2. overlap
  if (!out.args_ok() || (!dA && sizeA) || (!dB && sizeB) || (mode & ~kDecodeAll) || grain == 0 || grain > kTile || (grain & (grain - 1))) return zerr(42);
  if (out.data_overlaps(dA, sizeA) || out.data_overlaps(dB, sizeB)) return zerr(42);
  FramePasses F(E, ms);
  STCHK(F.start());
  // ---- 3. headers, A then B, 4. one frame size, 5. an update cannot shorten content
  ArchiveView A, B;
  STCHK(pair_views(E, dA, sizeA, dB, sizeB, &A, &B));
  if (B.U < A.U) return zerr(40);
  const uint64_t fs = A.fs, C = A.U;
  const TailPlan tail = tail_plan(C, B.U, fs);                                 // B's frames that hold content behind C
  const uint64_t tailBytes = B.U - C;
  // ---- 6. scratch
  PairPasses X = pair_passes(F, A, B, 0, C, stagingBytes);
  const PassPlan& P = X.P;
  const PassPlan PT = pass_plan(tail.fT0, tail.nTail, pass_slots(fs, stagingBytes));
  const size_t listCap = (size_t)std::min<uint64_t>(out.writeCap, (C + 1) / 2);   // (writes are at least one byte long and one byte apart)
  STCHK(F.open({(size_t)std::max<uint64_t>(2 * X.half, (uint64_t)PT.nSlots * fs) + 64, (size_t)P.nSlots + 64, 0, kDiffHdrBytes + (X.items_max() + 1) * 24 + 64,
                        listCap * 16 + 64, std::max<size_t>(2 * (size_t)P.nSlots, PT.nSlots), std::max<size_t>(P.nSlots, PT.nSlots)}));
  uint8_t* const hdr = F.tables;
  uint64_t* const tot = (uint64_t*)(hdr + kOffTot3);
  uint64_t* const tab = (uint64_t*)(hdr + kDiffHdrBytes);
  uint64_t* const starts = F.list;
  uint64_t* const ends = starts + listCap;
  uint8_t* const dData = out.dData;
  const uint64_t dataCap = out.dataCap;
  // ---- pair passes: the compare's, with the grain kernels
  uint64_t decoded = 0;
  STCHK(F.begin(hdr, kDiffHdrBytes));
  STCHK(X.run(mode, &decoded, [&](const FramePass& ps, uint32_t nDec) {
      const uint32_t items = 1 + nDec * X.tpf;
      TileArgs T;
      STCHK(X.tiles(ps, &T));
      hipLaunchKernelGGL(zra_diff_count_kernel, dim3(items), dim3(256), 0, F.s, T, grain, tab, (u64*)(hdr + kOffDiff), X.carry() + (ps.parity ^ 1));
      hipLaunchKernelGGL(zra_diff_scan_kernel, dim3(1), dim3(1024), 0, F.s, tab, items, tot + 3 * ps.parity, tot + 3 * (ps.parity ^ 1));
      if (listCap || dataCap) hipLaunchKernelGGL(zra_diff_fill_kernel, dim3(items), dim3(256), 0, F.s, T, grain, tab, starts, ends, (u64)listCap, dData, (u64)dataCap);
      return ok();
    }));
  // ---- tail passes: B's frames from the one that holds C on, decoded on their own; their bytes behind C follow the dirty bytes
  const uint64_t* const totEnd = tot + 3 * (P.passes & 1);                     // {writes, ends, dirty bytes} behind the last pair pass
  STCHK(F.run(PT, FramePasses::Side{&B, 0, F.win}, nullptr, nullptr, nullptr, nullptr, [&](const FramePass& ps, uint32_t) {
      const TailRun r = tail_run(tail, ps);
      if (dataCap) diff_launch_tail(F.s, F.win + (r.pLo - ps.first * fs), r.len, totEnd + 2, r.pLo - C, dData, dataCap);
      return ok();
    }));
  // ---- the counts, then the lists, once
  uint64_t h16[kDiffHdrBytes / 8] = {0};
  STCHK(F.finish(h16, hdr, kDiffHdrBytes));
  const uint64_t* const t3 = h16 + kOffTot3 / 8 + 3 * (P.passes & 1);
  const uint64_t total = t3[0], dirty = t3[2];
  if (t3[1] != total) return zerr(1);                                         // (cannot happen: every write has one start and one end)
  STCHK(F.patch(out, starts, ends, total, total, C, dirty, tailBytes));
  const uint64_t st8[8] = {P.n, P.n - decoded, decoded, tail.nTail, total, dirty, P.passes + PT.passes, h16[kOffDiff / 8]};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  return ok();
}
}  // namespace

Status Engine::compare_archives(const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode, uint64_t offset, uint64_t size,
                                size_t stagingBytes, uint64_t* hRanges, size_t rangeCap, uint64_t* nRanges, uint64_t* differingBytes) {
  // (no status of the compare leaves a word behind: rangeCapacity cuts the list, it refuses nothing; the two sizes are words of the call too)
  return entry_call(callStats_[kCallCompare], &callMs_[kCallCompare], {{nRanges, 1}, {differingBytes, 1}, {cmpSizes_, 2}}, false, [&] {
    return compare_run(*this, callStats_[kCallCompare], &callMs_[kCallCompare], cmpSizes_, dA, sizeA, dB, sizeB, mode, offset, size, stagingBytes, hRanges, rangeCap,
                       nRanges, differingBytes);
  });
}

Status Engine::diff_archives(const uint8_t* dA, size_t sizeA, const uint8_t* dB, size_t sizeB, uint32_t mode, uint32_t grain, size_t stagingBytes,
                             uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap,
                             uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize) {
  const PatchOut out{hOff, hSize, hDataOff, writeCap, nWrites, dData, dataCap, dataSize, appendOffset, appendSize};
  // (rule 8, OutputTooSmall, alone leaves what is needed in the four words)
  return entry_call(callStats_[kCallDiff], &callMs_[kCallDiff], {{nWrites, 1}, {dataSize, 1}, {appendOffset, 1}, {appendSize, 1}}, true, [&] {
    return diff_run(*this, callStats_[kCallDiff], &callMs_[kCallDiff], dA, sizeA, dB, sizeB, mode, grain, stagingBytes, out);
  });
}

}  // namespace zra_eng
