// zra_amd — grep of a device-resident archive with regular expressions (zra_hip.h: ZraHipGrepArchiveRegex): the
// records of a content range that a POSIX extended regular expression over bytes matches, in one decode and one scan of the range.
//
// Records, range, passes, (stream), (forward), (launches), (order) and (d) are the plain grep's (zra_grep.hip), word for word; the
// driver is zra_scan.h's with M = 1: a position owns its own byte only, so no pass reads the carry area. The expressions become a
// DFA of at most 64 states on the host (zra_regex.h); the host path is zra_record_scan.h's (the regex selector, the kernel set at the
// end of this file). What this call runs as the regex extract does (zra_extract_regex.hip) lies in zra_regex_tile.h: the automaton
// in LDS, the walks, the forward half of the scan and phase 1 of the fill; this file keeps its count, the end of the scan's pass and
// the fill's ballot walk. What differs from the plain grep:
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
#include "zra_record_scan.h"
#include "zra_regex_tile.h"

namespace {
struct __attribute__((aligned(16))) SumX { u64 last; u32 sel; u8 has, tail; u16 pad; };
struct __attribute__((aligned(16))) HeadX { u64 base, open; u32 state, pad[3]; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi
struct StateX { u64 start, state, sel, tail; };
// The words the launches of a call add up, uploaded behind the table: the ping-pong state (c), then the atomics.
struct TotalsX { StateX st[2]; u64 matches, delims, pad[6]; };
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grep.hip's grep_count. Per tile its summary -> sums[tile] and its map -> maps[tile].
extern "C" __global__ void __launch_bounds__(256) zra_grepx_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
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

// One workgroup, (scan): zra_regex_tile.h's forward scan over the 16-byte summaries and the 64-byte maps, then the last lane ends the
// pass. lastPass: the record open at hi ends there.
extern "C" __global__ void __launch_bounds__(1024) zra_grepx_scan_kernel(SumX* sums, const u8* maps, u32 nTiles, HeadX* heads, const StateX* in, StateX* out,
                                                                         const RxTable* tbl, u32 inv, u32 lastPass, u64 hi, Range* list, u64 cap, TotalsX* tot) {
  const u64 accept = tbl->accept;
  RegexFront e = regex_scan_forward<false>(sums, maps, nTiles, heads, in, accept, inv);
  if (threadIdx.x == 1023) {                                                 // (its run is the last one, or empty behind the last one)
    u64 tl = 0;
    if (lastPass && e.start < hi) {
      tl = 1;
      const u32 m = (u32)(accept >> e.state) & 1;
      e.matched += m;
      if (m ^ inv) {
        if (e.count < cap) { Range r; r.offset = e.start; r.size = hi - e.start; list[e.count] = r; }
        e.count++;
      }
    }
    StateX o; o.start = e.start; o.state = e.state; o.sel = e.count; o.tail = tl;
    *out = o;
  }
  if (e.matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)e.matched);
}

// zra_grep.hip's grep_fill: the count's workgroups redo the tiles that hold a listed record.
extern "C" __global__ void __launch_bounds__(256) zra_grepx_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
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
    // the selection bit of the record that delimiter k ends (nD is not zero: a record ends here)
    const u32 nD = regex_select(&sD, sTile, d, n, delim, sPos, sCnt, start, head.state, accept, inv, [&](u32 k, u32, u32 bit) { sBit[k] = (u8)bit; });
    // a wave takes its share of the delimiters: its selected records, then the ballot walk
    u32 k0, k1;
    wave_share(nD, wave, &k0, &k1);
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
// The kernel set of the regex grep for zra_record_scan.h's call path. tables: Table | Totals | sums[tiles] | heads[tiles] | maps[tiles]
namespace {
struct GrepRegexKernels {
  using Sum = SumX; using Head = HeadX; using Totals = TotalsX;
  static constexpr size_t kMapBytes = 64;
  static constexpr bool kData = false;
  static void launch(hipStream_t s, const RegexSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<GrepRegexKernels>& p, u32 parity) {
    const RxTable* const tbl = (const RxTable*)p.table;
    const u32 delim = c.delimiter, inv = sel.inv;
    hipLaunchKernelGGL(zra_grepx_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, (u64)ps.p0, p.sums, p.maps, p.tot);
    hipLaunchKernelGGL(zra_grepx_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.maps, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), tbl, inv,
                       (u32)ps.lastPass, (u64)p.hi, p.list, (u64)p.listCap, p.tot);
    if (p.listCap)
      hipLaunchKernelGGL(zra_grepx_fill_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, (u64)ps.p0, p.sums, p.heads, p.list,
                         (u64)p.listCap);
  }
};
static_assert(sizeof(TotalsX) == 128 && sizeof(SumX) == 16 && sizeof(HeadX) == 32, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::grep_regex(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<RegexSelect, GrepRegexKernels>(E, c, cv); }
}  // namespace zra_eng
