// zra_amd — the tile of the two regex record scans (zra_grep_regex.hip: ZraHipGrepArchiveRegex; zra_extract_regex.hip:
// ZraHipExtractRecordsRegex): the automaton in LDS, a lane's walk over a record, a tile's delimiters and a wave's
// share of them, the composition of maps, and the two pieces the two calls run alike: the forward half of the one-workgroup scan
// (regex_scan_forward; kBytes: the extract's two summary fields {first, bytes} ride along) and phase 1 of the fill and the copy
// (regex_select). The two count kernels stay in their files: joined into one body they measured slower for the extract
// (profiles/record_scan_refactor.md). (state), (summary), (count) and (scan) are described in zra_grep_regex.hip, the two fields in
// zra_extract_regex.hip. Device code: included by those two translation units and by zra_grep_regex_context.hip.
#pragma once
#include "zra_scan_tile.h"
#include "zra_regex.h"

namespace {
using RxTable = zra_regex::Table;
static_assert(sizeof(RxTable) % 16 == 0 && offsetof(RxTable, next) == 256, "stage_dfa's chunks");
constexpr u32 kPosMask = 0x1FFFu;                          // a tile position is below 2^13; the copy keeps a flag above it in sPos

// the automaton in LDS: the class of every byte and the rows of the classes in use
struct Dfa { u8 classOf[256]; u8 next[256 * 64]; };

__device__ __forceinline__ void stage_dfa(const RxTable* tbl, Dfa* s, u32 classes) {
  const uint4* const g = (const uint4*)tbl;
  for (u32 c = threadIdx.x; c < 16 + classes * 4; c += 256) lds_st128((u8*)s + 16 * (size_t)c, g[c]);
}
__device__ __forceinline__ u32 tile_byte(const u32* sTile, u32 i) { return ((const u8*)sTile)[i]; }

// One lane's walk over the tile bytes [from, to) from state st. The table names the states that every byte leads back to (the dead
// state, the accepting sink), where a lane could leave: built and measured, the test on the dependent chain cost more than it saved
// on every expression but `^$`, so a lane walks to its record's end.
__device__ __forceinline__ u32 walk(const Dfa* D, const u32* sTile, u32 d, u32 from, u32 to, u32 st) {
#pragma unroll 2
  for (u32 j = from; j < to; j++) st = D->next[(u32)D->classOf[tile_byte(sTile, d + j)] * 64 + st];
  return st;
}

// The delimiter positions of a tile of n positions, in order, into sPos; returns their number (the same in every lane). sCnt[w]
// keeps wave w's number. A wave takes its 2,048 consecutive positions twice: to count, and behind the prefix over the waves to write.
__device__ __forceinline__ u32 compact_delims(const u32* sTile, u32 d, u32 n, u32 delim, u16* sPos, u32* sCnt) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  u32 mine = 0;
#pragma unroll 1
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    const u32 j = w0 + t * 64 + lane;
    mine += (u32)__popcll(__ballot(j < n && tile_byte(sTile, d + j) == delim));
  }
  if (lane == 0) sCnt[wave] = mine;
  __syncthreads();
  u32 at = 0, all = 0;
  for (u32 v = 0; v < 4; v++) { if (v < wave) at += sCnt[v]; all += sCnt[v]; }
#pragma unroll 1
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    const u32 j = w0 + t * 64 + lane;
    const bool isD = j < n && tile_byte(sTile, d + j) == delim;
    const u64 dm = __ballot(isD);
    if (isD) sPos[at + (u32)__popcll(dm & ((1ull << lane) - 1))] = (u16)j;
    at += (u32)__popcll(dm);
  }
  __syncthreads();
  return all;
}

// a wave's share of a tile's nD compacted delimiters: a quarter, in whole trips
__device__ __forceinline__ void wave_share(u32 nD, u32 wave, u32* k0, u32* k1) {
  const u32 quarter = ((nD + 255) / 256) * 64;
  *k0 = wave * quarter; *k1 = min(nD, *k0 + quarter);
}

// F := m o src, maps of 64 states as 16 words of four: F[s] = m[src[s]]. F lives in registers, indexed by constants only; src may be F.
__device__ __forceinline__ void compose(u32 (&F)[16], const u8* m, const u32* src) {
#pragma unroll
  for (u32 w = 0; w < 16; w++) {
    const u32 a = src[w];
    F[w] = (u32)m[a & 0xFF] | (u32)m[(a >> 8) & 0xFF] << 8 | (u32)m[(a >> 16) & 0xFF] << 16 | (u32)m[a >> 24] << 24;
  }
}

// What lies in front of a lane's run of tiles [b0, b1) in the one-workgroup scan, moved over the run: the open record's start and
// state, the list position, (kBytes) the packed offset; the matched records the lane saw end; look (kBytes): 2 the run has a
// delimiter, 1 the record its first one ends is selected.
struct RegexFront { u64 start, count, at; u32 state, matched, look, b0, b1; };

// The forward half of the one-workgroup scan of both calls, 1,024 lanes: every lane reduces a run of consecutive tiles, the 1,024
// summaries are scanned in LDS (Hillis-Steele over (summary)'s combine), then the lane walks its run again from the state in front
// of it: heads[t] = {base, open, state, (kBytes) at}, sums[t].sel becomes ALL the selected records that end in tile t, the first
// included, and (kBytes) sums[t].fsel says whether the first of them is one. A lane's map lives in 16 words of registers between the
// steps. in: the state carried into the pass. Returns what lies behind the lane's run; the last lane's is the pass's end.
template <bool kBytes, class Sum, class Head, class State>
__device__ __forceinline__ RegexFront regex_scan_forward(Sum* sums, const u8* maps, u32 nTiles, Head* heads, const State* in, u64 accept, u32 inv) {
  __shared__ __attribute__((aligned(16))) u32 sMap[1024 * 16];
  __shared__ u64 sFirst[kBytes ? 1024 : 1], sLast[1024], sSel[1024], sBytes[kBytes ? 1024 : 1];
  __shared__ u8 sHas[1024], sTl[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  const u8* const myMap = (const u8*)(sMap + tid * 16);
  // ---- the lane's run. F starts as the identity
  u32 F[16];
#pragma unroll
  for (u32 w = 0; w < 16; w++) F[w] = 0x03020100u + 0x04040404u * w;
  u64 first = 0, last = 0, sel = 0, bytes = 0;
  u32 has = 0, tail = 0;
  for (u32 t = b0; t < b1; t++) {
    const Sum s = sums[t];
    const u8* const m = maps + (size_t)t * 64;
    if (has) {
      if (!s.has) { tail = m[tail]; continue; }
      const u32 j = ((u32)(accept >> m[tail]) & 1) ^ inv;
      sel += s.sel + j;
      if constexpr (kBytes) bytes += s.bytes + (j ? s.first - last + 1 : 0);
      tail = s.tail; last = s.last;
      continue;
    }
    compose(F, m, F);
    if (s.has) {
      has = 1; sel = s.sel; tail = s.tail; last = s.last;
      if constexpr (kBytes) { bytes = s.bytes; first = s.first; }
    }
  }
  auto put = [&] {
#pragma unroll
    for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
    sLast[tid] = last; sSel[tid] = sel; sHas[tid] = (u8)has; sTl[tid] = (u8)tail;
    if constexpr (kBytes) { sFirst[tid] = first; sBytes[tid] = bytes; }
  };
  put();
  __syncthreads();
  // ---- the scan: A = the lanes in front (at tid - d), B = this lane
  for (u32 d = 1; d < 1024; d <<= 1) {
    const bool on = tid >= d;
    if (on) {
      const u32 a = tid - d;
      if (sHas[a]) {
        // A's map stands; B's acts on A's tail
        const u32 through = myMap[sTl[a]];
        if (has) {
          const u32 j = ((u32)(accept >> through) & 1) ^ inv;
          sel += sSel[a] + j;
          if constexpr (kBytes) bytes += sBytes[a] + (j ? first - sLast[a] + 1 : 0);
        } else {
          has = 1; sel = sSel[a]; last = sLast[a]; tail = through;
          if constexpr (kBytes) bytes = sBytes[a];
        }
        if constexpr (kBytes) first = sFirst[a];
#pragma unroll
        for (u32 w = 0; w < 16; w++) F[w] = sMap[a * 16 + w];
      } else compose(F, myMap, sMap + a * 16);
    }
    __syncthreads();
    if (on) put();
    __syncthreads();
  }
  // ---- the front of this lane's run: the carried one, moved over the lanes in front
  RegexFront e = {in->start, in->sel, 0, (u32)in->state, 0, 0, b0, b1};
  if constexpr (kBytes) e.at = in->bytes;
  if (tid) {
    const u32 a = tid - 1;
    const u32 through = ((const u8*)(sMap + a * 16))[e.state];
    if (sHas[a]) {
      const u32 j = ((u32)(accept >> through) & 1) ^ inv;
      e.count += sSel[a] + j;
      if constexpr (kBytes) e.at += sBytes[a] + (j ? sFirst[a] - e.start + 1 : 0);
      e.state = sTl[a]; e.start = sLast[a];
    } else e.state = through;
  }
  for (u32 t = b0; t < b1; t++) {
    const Sum s = sums[t];
    Head h = {};
    h.base = e.count; h.open = e.start; h.state = e.state;
    if constexpr (kBytes) h.at = e.at;
    heads[t] = h;
    const u32 through = maps[(size_t)t * 64 + e.state];
    if (s.has) {
      const u32 m = (u32)(accept >> through) & 1, j = m ^ inv;
      sums[t].sel = s.sel + j;
      if constexpr (kBytes) {
        sums[t].fsel = (u8)j;
        if (!e.look) e.look = 2 | j;
        e.at += s.bytes + (j ? s.first - e.start + 1 : 0);
      }
      e.matched += m; e.count += s.sel + j;
      e.state = s.tail; e.start = s.last;
    } else e.state = through;
  }
  return e;
}

// Phase 1 of the fill and the copy: the tile's delimiters into sPos (compact_delims), then the selection bit of the record that
// delimiter k ends, a lane's walk per record; record 0 goes on from the state in the tile's head entry. put(k, position of delimiter
// k, bit) keeps the bit; it may flag sPos[k] above kPosMask: lane k + 1 may read sPos[k] for its `from` while that store is under
// way, with no barrier between. It masks the word, the store is one 16-bit LDS write (ds_write_b16, never torn) and leaves the
// position's 13 bits as they are, so either value it sees gives the same `from`. The bits are read behind the barrier at the end.
// (The grep's fill keeps its bits in an array of their own and never flags sPos: for it the mask changes nothing.)
// Returns the number of delimiters.
template <class Put>
__device__ __forceinline__ u32 regex_select(const Dfa* D, const u32* sTile, u32 d, u32 n, u32 delim, u16* sPos, u32* sCnt, u32 start, u32 headState, u64 accept,
                                            u32 inv, Put put) {
  const u32 nD = compact_delims(sTile, d, n, delim, sPos, sCnt);
  for (u32 k = threadIdx.x; k < nD; k += 256) {
    const u32 from = k ? ((u32)sPos[k - 1] & kPosMask) + 1 : 0, to = (u32)sPos[k];
    const u32 st = walk(D, sTile, d, from, to, k ? start : headState);
    put(k, to, ((u32)(accept >> st) & 1) ^ inv);
  }
  __syncthreads();
  return nD;
}
}  // namespace
