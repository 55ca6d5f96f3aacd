// zra_amd — grep of a device-resident archive with regular expressions (zra_hip.h: ZraHipGrepArchiveRegex): the
// records of a content range that a POSIX extended regular expression over bytes matches, in one decode and one scan of the range.
//
// Records, range, passes, (stream), (forward), (launches), (order) and (d) are the plain grep's (zra_grep.hip), word for word; the
// driver is zra_scan.h's with M = 1: a position owns its own byte only, so no pass reads the carry area. The expressions become a
// DFA of at most 64 states on the host (zra_regex.h); the plain grep's and the predicate grep's kernels are not touched. What differs:
//  (state) where the plain grep carries one bit, this call carries the DFA state of the open record. A record that begins inside a
//      tile begins at the start state; only the bytes in front of a tile's first delimiter (its head) depend on what lies in front of
//      the tile, and for them the tile keeps a MAP: for every state s the state reached from s over the head.
//  (summary) a run of positions reduces to {has a delimiter, F, tail, last, sel}: F[s] the state reached from s over the bytes in
//      front of the run's first delimiter (without one: over the whole run), tail the state of the record open behind the last
//      delimiter (from the start state), last the position behind the last delimiter, sel the records selected among those that end
//      inside the run APART from the first. For A followed by B: B without a delimiter: A.tail = B.F[A.tail] if A has one, else
//      A.F = B.F o A.F; A without one: B with B.F o A.F; both: the record that B's first delimiter ends is selected iff
//      accept(B.F[A.tail]) ^ invert. A run with a delimiter acts on its successor as one byte; only delimiter-free runs compose maps.
//  (count) the tile's delimiter positions are compacted into LDS in order (ballots, one prefix over the four waves). Record k lies
//      between delimiters k - 1 and k; the 256 lanes take the records k >= 1 in turn and walk each from the start state, one lane
//      per record; the lane that takes the stretch behind the last delimiter gives tail. The head takes one lane per STATE: wave 0
//      steps all 64 states at once, 64 bytes per trip classified by one lane each and broadcast, and writes F. Per tile a 16-byte
//      summary and a 64-byte map; the matched records and the delimiters are added up as atomics.
//  (scan) one workgroup of 1,024 lanes as zra_grepw_scan_kernel; the maps of the 1,024 lane runs are 64 KiB of LDS.
//  (fill) only tiles that hold a listed record are redone: the head record is one lane's walk from the state in the tile's head
//      entry, the others are walked as in the count; the selection bits go to LDS by delimiter and a ballot walk writes
//      {start, delimiter - start} at prefix counts.
// Every loop is bounded by the tile's size, no workgroup waits for another one, and no tile byte beyond hi is read: a tile stages n
// bytes, n the positions it owns inside [lo, hi).
#include "zra_scan.h"
#include "zra_scan_tile.h"
#include "zra_regex.h"

namespace {
using zra_regex::Table;
constexpr u32 kGroup = 8;                                   // consecutive tiles of one workgroup, as the family's
struct __attribute__((aligned(16))) Range { u64 offset, size; };   // ZraHipContentRange

struct __attribute__((aligned(16))) SumX { u64 last; u32 sel; u8 has, tail; u16 pad; };
struct __attribute__((aligned(16))) HeadX { u64 base, open; u32 state, pad[3]; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi
struct StateX { u64 start, state, sel, tail; };
// The words the launches of a call add up, uploaded behind the table: the ping-pong state (c), then the atomics.
struct TotalsX { StateX st[2]; u64 matches, delims, pad[6]; };

// the automaton in LDS: the class of every byte and the rows of the classes in use
struct Dfa { u8 classOf[256]; u8 next[256 * 64]; };

__device__ __forceinline__ void stage_dfa(const Table* tbl, Dfa* s, u32 classes) {
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

// The delimiter positions of a tile of n positions, in order, into sPos; returns their number (the same in every lane). A wave
// takes its 2,048 consecutive positions twice: to count, and behind the prefix over the waves to write.
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
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grep.hip's grep_count. Per tile its summary -> sums[tile] and its map -> maps[tile].
extern "C" __global__ void __launch_bounds__(256) zra_grepx_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const Table* tbl, u32 delim, u32 inv,
                                                                         u64 p0, SumX* sums, u8* maps, TotalsX* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u32 sCnt[4], sSel[4], sTail;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 start = tbl->start;
  const u64 accept = tbl->accept;
  stage_dfa(tbl, &sD, tbl->classes);
  u32 matched = 0, delims = 0;
  for (u32 b = blockIdx.x * kGroup, bEnd = min(tiles, b + kGroup); b < bEnd; b++) {
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0;
    __syncthreads();                                                         // (the tile in front is done with)
    const u32 d = stage_tile(win + x0, n, sTile);
    __syncthreads();
    const u32 nD = compact_delims(sTile, d, n, delim, sPos, sCnt);
    if (tid == 0) delims += nD;
    // (count) records 1 .. nD - 1 end at a delimiter; "record" nD is the stretch behind the last one: the tile's tail
    u32 sel = 0;
    for (u32 k = 1 + tid; k <= nD; k += 256) {
      const u32 from = (u32)sPos[k - 1] + 1, to = k < nD ? (u32)sPos[k] : n;
      const u32 st = walk(&sD, sTile, d, from, to, start);
      if (k == nD) { sTail = st; continue; }
      const u32 m = (u32)(accept >> st) & 1;
      matched += m; sel += m ^ inv;
    }
    sel = wave_sum(sel);
    if (lane == 0) sSel[wave] = sel;
    // the head, one lane per state
    if (wave == 0) {
      const u32 first = nD ? (u32)sPos[0] : n;
      u32 st = lane;
      for (u32 i0 = 0; i0 < first; i0 += 64) {
        const u32 cnt = min(64u, first - i0);
        const u32 cls = lane < cnt ? (u32)sD.classOf[tile_byte(sTile, d + i0 + lane)] : 0;
#pragma unroll 4
        for (u32 q = 0; q < cnt; q++) st = sD.next[(u32)__builtin_amdgcn_readlane((int)cls, (int)q) * 64 + st];   // (q is uniform)
      }
      maps[(size_t)b * 64 + lane] = (u8)st;
    }
    __syncthreads();
    if (tid == 0) {
      SumX r; r.last = nD ? p0 + t0 + sPos[nD - 1] + 1 : 0; r.sel = sSel[0] + sSel[1] + sSel[2] + sSel[3]; r.has = nD ? 1 : 0; r.tail = (u8)(nD ? sTail : 0); r.pad = 0;
      sums[b] = r;
    }
  }
  matched = wave_sum(matched);
  if (lane == 0 && matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
  if (tid == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);
}

// One workgroup: zra_grepw_scan_kernel over the 16-byte summaries and the 64-byte maps. Every lane reduces a run of consecutive tiles,
// the 1,024 summaries are scanned in LDS (Hillis-Steele over (summary)'s combine), then the lane walks its run again from the state in
// front of it: heads[t], and sums[t].sel becomes ALL the selected records that end in tile t, the first included. A lane's map lives
// in 16 words of registers between the steps, indexed by constants only. lastPass: the record open at hi ends there.
extern "C" __global__ void __launch_bounds__(1024) zra_grepx_scan_kernel(SumX* sums, const u8* maps, u32 nTiles, HeadX* heads, const StateX* in, StateX* out,
                                                                         const Table* tbl, u32 inv, u32 lastPass, u64 hi, Range* list, u64 cap, TotalsX* tot) {
  __shared__ __attribute__((aligned(16))) u32 sMap[1024 * 16];
  __shared__ u64 sLast[1024], sSel[1024];
  __shared__ u8 sHas[1024], sTl[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  const u64 accept = tbl->accept;
  const u8* const myMap = (const u8*)(sMap + tid * 16);
  // ---- the lane's run. F starts as the identity
  u32 F[16];
#pragma unroll
  for (u32 w = 0; w < 16; w++) F[w] = 0x03020100u + 0x04040404u * w;
  u64 last = 0, sel = 0;
  u32 has = 0, tail = 0;
  for (u32 t = b0; t < b1; t++) {
    const SumX s = sums[t];
    const u8* const m = maps + (size_t)t * 64;
    if (has) {
      if (!s.has) { tail = m[tail]; continue; }
      sel += s.sel + (((u32)(accept >> m[tail]) & 1) ^ inv);
      tail = s.tail; last = s.last;
      continue;
    }
#pragma unroll
    for (u32 w = 0; w < 16; w++) {
      const u32 a = F[w];
      F[w] = (u32)m[a & 0xFF] | (u32)m[(a >> 8) & 0xFF] << 8 | (u32)m[(a >> 16) & 0xFF] << 16 | (u32)m[a >> 24] << 24;
    }
    if (s.has) { has = 1; sel = s.sel; tail = s.tail; last = s.last; }
  }
#pragma unroll
  for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
  sLast[tid] = last; sSel[tid] = sel; sHas[tid] = (u8)has; sTl[tid] = (u8)tail;
  __syncthreads();
  // ---- the scan: A = the lanes in front (at tid - d), B = this lane
  for (u32 d = 1; d < 1024; d <<= 1) {
    const bool on = tid >= d;
    u32 hasA = 0, tailA = 0;
    u64 selA = 0, lastA = 0;
    if (on) {
      const u32 a = tid - d;
      hasA = sHas[a]; tailA = sTl[a]; selA = sSel[a]; lastA = sLast[a];
      if (hasA) {
        // A's map stands; B's acts on A's tail
        const u32 through = myMap[tailA];
        if (has) { sel += selA + (((u32)(accept >> through) & 1) ^ inv); }
        else { has = 1; sel = selA; last = lastA; tail = through; }
#pragma unroll
        for (u32 w = 0; w < 16; w++) F[w] = sMap[a * 16 + w];
      } else {
#pragma unroll
        for (u32 w = 0; w < 16; w++) {
          const u32 x = sMap[a * 16 + w];
          F[w] = (u32)myMap[x & 0xFF] | (u32)myMap[(x >> 8) & 0xFF] << 8 | (u32)myMap[(x >> 16) & 0xFF] << 16 | (u32)myMap[x >> 24] << 24;
        }
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
      sLast[tid] = last; sSel[tid] = sel; sHas[tid] = (u8)has; sTl[tid] = (u8)tail;
    }
    __syncthreads();
  }
  // ---- the state in front of this lane's run: the carried one, then the lanes in front
  u64 start = in->start, count = in->sel;
  u32 state = (u32)in->state, matched = 0;
  if (tid) {
    const u32 through = ((const u8*)(sMap + (tid - 1) * 16))[state];
    if (sHas[tid - 1]) { count += sSel[tid - 1] + (((u32)(accept >> through) & 1) ^ inv); state = sTl[tid - 1]; start = sLast[tid - 1]; }
    else state = through;
  }
  for (u32 t = b0; t < b1; t++) {
    const SumX s = sums[t];
    HeadX h; h.base = count; h.open = start; h.state = state; h.pad[0] = h.pad[1] = h.pad[2] = 0;
    heads[t] = h;
    const u32 through = maps[(size_t)t * 64 + state];
    if (s.has) {
      const u32 m = (u32)(accept >> through) & 1;
      const u32 all = s.sel + (m ^ inv);
      sums[t].sel = all;
      matched += m; count += all; state = s.tail; start = s.last;
    } else state = through;
  }
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tl = 0;
    if (lastPass && start < hi) {
      tl = 1;
      const u32 m = (u32)(accept >> state) & 1;
      matched += m;
      if (m ^ inv) {
        if (count < cap) { Range r; r.offset = start; r.size = hi - start; list[count] = r; }
        count++;
      }
    }
    StateX o; o.start = start; o.state = state; o.sel = count; o.tail = tl;
    *out = o;
  }
  if (matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
}

// zra_grep.hip's grep_fill: the count's workgroups redo the tiles that hold a listed record.
extern "C" __global__ void __launch_bounds__(256) zra_grepx_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const Table* tbl, u32 delim, u32 inv,
                                                                        u64 p0, const SumX* sums, const HeadX* heads, Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u8 sBit[kTile];
  __shared__ u32 sCnt[4], sOn[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  bool any = false;                                                          // (uniform in the workgroup, like `listed` below)
  for (u32 b = bBegin; b < bEnd; b++) any |= sums[b].sel != 0 && heads[b].base < cap;
  if (!any) return;
  const u32 start = tbl->start;
  const u64 accept = tbl->accept;
  stage_dfa(tbl, &sD, tbl->classes);
  for (u32 b = bBegin; b < bEnd; b++) {
    const HeadX head = heads[b];
    const bool listed = sums[b].sel != 0 && head.base < cap;
    if (!listed) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, n, sTile);
    __syncthreads();
    const u32 nD = compact_delims(sTile, d, n, delim, sPos, sCnt);             // (not zero: a record ends here)
    // the selection bit of the record that delimiter k ends: record 0 goes on from the head's state
    for (u32 k = tid; k < nD; k += 256) {
      const u32 from = k ? (u32)sPos[k - 1] + 1 : 0;
      const u32 st = walk(&sD, sTile, d, from, (u32)sPos[k], k ? start : head.state);
      sBit[k] = (u8)(((u32)(accept >> st) & 1) ^ inv);
    }
    __syncthreads();
    // a wave takes a quarter of the delimiters (whole trips): its selected records, then the ballot walk
    const u32 quarter = ((nD + 255) / 256) * 64, k0 = wave * quarter, k1 = min(nD, k0 + quarter);
    u32 on = 0;
    for (u32 k = k0; k < k1; k += 64) on += (u32)__popcll(__ballot(k + lane < k1 && sBit[k + lane]));
    if (lane == 0) sOn[wave] = on;
    __syncthreads();
    u64 at = head.base;
    for (u32 v = 0; v < wave; v++) at += sOn[v];
    for (u32 k = k0; k < k1 && at < cap; k += 64) {
      const u32 mine = k + lane;
      const bool s = mine < k1 && sBit[mine];
      const u64 sm = __ballot(s);
      const u64 idx = at + (u32)__popcll(sm & ((1ull << lane) - 1));
      if (s && idx < cap) {
        const u64 from = mine ? p0 + t0 + sPos[mine - 1] + 1 : head.open;
        Range r; r.offset = from; r.size = p0 + t0 + sPos[mine] - from;
        list[idx] = r;
      }
      at += (u32)__popcll(sm);
    }
  }
}

// =================================================================================================
namespace zra_eng {

Status Engine::grep_archive_regex(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
                                  uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap,
                                  uint64_t* nRecords) {
  return ScanImpl::call(*this, kScanGrep, nRecords, nullptr, [&] {
    return ScanImpl::grep_regex(*this, dArc, arcSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes, hRecords,
                                recordCap, nRecords);
  });
}

// ScanImpl::grep_where step by step; the differences are the compiler in step 1, no shortcut in step 3, and the entries.
Status ScanImpl::grep_regex(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, uint8_t delimiter,
                            uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap, uint64_t* nRecords,
                            ScanCacheView* cv) {
  // ---- 1. arguments
  if (!nRecords || !hPat || !hSizes || (!dArc && arcSize) || (!hRecords && recordCap) || (mode & ~1u)) return zerr(42);
  const size_t kTotals = sizeof(Table), kHead = kTotals + sizeof(TotalsX);
  static_assert(sizeof(Table) % 16 == 0 && sizeof(TotalsX) == 128 && sizeof(SumX) == 16 && sizeof(HeadX) == 32 && sizeof(Range) == 16 && offsetof(Table, next) == 256,
                "16-byte entries behind a 16-byte head; stage_dfa's chunks");
  std::vector<uint8_t> head;
  {
    zra_regex::Compiled C;
    if (!zra_regex::compile(hPat, hSizes, nPat, syntax, delimiter, &C)) return zerr(42);
    head.assign(kHead, 0);                                                   // (the totals go up as zeros, the state as "a record opens at lo" in the start state)
    std::memcpy(head.data(), &C.table, sizeof(Table));
    ((TotalsX*)(head.data() + kTotals))->st[0].state = C.table.start;
  }
  const u32 inv = mode & 1u;
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen, as the search
  ArchiveView arc;
  { Status st = view(E, dArc, arcSize, cv, &arc); if (st.zra) return st; }
  // ---- 3. the range [lo, hi)
  uint64_t lo, hi;
  if (!scan_range(arc.U, offset, size, &lo, &hi)) return {kOutOfBounds, 0};
  uint64_t* const stats = E.callStats_[kScanGrep];
  if (hi == lo) { stats[0] = arc.frames; return ok(); }
  if (arc.fs == 0 || arc.frames == 0) return {kHeaderInvalid, 0};
  // ---- 4. the passes. tables: Table | Totals | sums[tiles] | heads[tiles] | maps[tiles]
  const ScanPlan P = scan_plan(arc.U, arc.fs, lo, hi, 1, 0, stagingBytes);
  const size_t listCap = (size_t)std::min<uint64_t>(recordCap, hi - lo);
  ((TotalsX*)(head.data() + kTotals))->st[0].start = lo;
  uint32_t launches = 0;
  Status st = ScanImpl::passes(E, arc, P, &E.callMs_[kScanGrep], head.data(), kHead, kTotals, sizeof(TotalsX),
                               kHead + P.tilesMax * (sizeof(SumX) + sizeof(HeadX) + 64) + 64, listCap * sizeof(Range) + 64, true, [&](const ScanPass& ps) {
    uint8_t* const win = window(E), * const tb = E.scan_.tables.as<uint8_t>();
    const Table* const tbl = (const Table*)tb;
    TotalsX* const tot = (TotalsX*)(tb + kTotals);
    SumX* const sums = (SumX*)(tb + kHead);
    HeadX* const heads = (HeadX*)(sums + P.tilesMax);
    u8* const maps = (u8*)(heads + P.tilesMax);
    Range* const list = E.scan_.list.as<Range>();
    const uint32_t tiles = (uint32_t)((ps.nPos + kTile - 1) / kTile), groups = (tiles + kGroup - 1) / kGroup;
    hipLaunchKernelGGL(zra_grepx_count_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, (u32)delimiter, inv, (u64)ps.p0, sums, maps, tot);
    hipLaunchKernelGGL(zra_grepx_scan_kernel, dim3(1), dim3(1024), 0, s, sums, maps, tiles, heads, tot->st + (launches & 1), tot->st + ((launches + 1) & 1), tbl, inv,
                       (u32)ps.lastPass, (u64)hi, list, (u64)listCap, tot);
    if (listCap)
      hipLaunchKernelGGL(zra_grepx_fill_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, (u32)delimiter, inv, (u64)ps.p0, sums, heads, list,
                         (u64)listCap);
  }, &launches, cv);
  if (st.zra) return st;
  // ---- 5. the totals (they came back with the last synchronisation), then the list, once
  const TotalsX& h = *(const TotalsX*)(head.data() + kTotals);
  const StateX& fin = h.st[launches & 1];
  const uint64_t total = fin.sel;
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hRecords, E.scan_.list.p, nOut * sizeof(Range), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  *nRecords = total;
  const uint64_t st8[8] = {arc.frames, decoded_frames(P, cv), decoded_bytes(P, cv), h.delims + fin.tail, total, nOut, P.passes, h.matches};
  std::copy(st8, st8 + 8, stats);
  return ok();
}

}  // namespace zra_eng
