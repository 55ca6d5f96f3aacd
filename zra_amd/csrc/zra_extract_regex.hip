// zra_amd — extract of a device-resident archive with regular expressions (zra_hip.h: ZraHipExtractRecordsRegex): the
// records the regex grep selects (zra_grep_regex.hip) WITH their bytes, packed as the extract packs them (zra_extract.hip): the text
// `grep -E` (and `-v`) prints, from the one decode pass that selects the records.
//
// Selection, (state), (count) and the driver with M = 1 are the regex grep's, word for word; (compaction), (look-ahead), (provisional
// tail) and (stores) are the extract's. What it runs as the regex grep does lies in zra_regex_tile.h (the automaton in LDS, the walks,
// the forward half of the scan with this call's two fields switched on, phase 1 of the copy), what it runs as the
// extract does behind the forward scan in zra_extract_tail.h; the host path is zra_record_scan.h's (the regex selector, the kernel
// set at the end of this file). This file keeps its count, the end of the scan and phases 2 and 3 of the copy. What this call joins:
//  (summary) the regex grep's {has, F[64], tail, last, sel} plus {first, bytes}: the position of the run's first delimiter, and the
//      packed bytes (n + 1 each) of the selected records that end inside the run APART from the one its first delimiter ends. For A
//      followed by B, both with a delimiter, s = accept(B.F[A.tail]) ^ invert: bytes = A.bytes + B.bytes + s * (B.first - A.last + 1),
//      first is A's, last is B's; the rest is the regex grep's. The joined record's length needs only A.last and B.first, which the
//      combination keeps from its outer ends, so combine stays associative. Moving a front {start, state, list position, packed
//      offset} over a run is the same operation with the open record's start in place of A.last.
//  (count) the regex grep's; a record lane also adds its record's n + 1 when it is selected.
//  (scan) one workgroup of 1,024 lanes: forward as the regex grep's, carrying the packed offset D beside the list position; then the
//      extract's reverse pass, which gives every tile the bit "the record open at my tail is copied".
//  (copy) only tiles that hold a copied byte or a listed record inside the capacities. Phase 1 is the regex grep's fill: delimiters
//      compacted, a lane's walk per record for its selection bit. Phase 2: an exclusive prefix over the tile's delimiters of
//      {selected, selected * size}, the record that the first delimiter ends left out of the sizes, so both sums stay below 2^14
//      and share a 32-bit LDS word. Phase 3 is position-parallel: the lane of position q counts the delimiters in front of q
//      (ballots, a running count) and stores q's byte at its record's base + (q - the record's start).
// Every store to dData is clamped to [0, dataCapacity); no atomic decides an address; no workgroup waits for another one; every loop
// is bounded by the tile's size; a tile stages n bytes, n the positions it owns inside [lo, hi).
#include "zra_record_scan.h"
#include "zra_regex_tile.h"
#include "zra_extract_tail.h"

namespace {
// (summary) without the map. sel: after the scan ALL the selected records that end in the tile; fsel (set by the scan): the record
// the first delimiter ends is selected
struct __attribute__((aligned(16))) SumR { u64 first, last; u32 bytes, sel; u8 has, tail, fsel, pad[5]; };
// what the scan makes of it for the copy: the list position of the tile's first record, the start of the record open at its head, the
// packed bytes in front of that record, that record's state at the tile's first byte, and (look-ahead)'s bit
struct __attribute__((aligned(16))) HeadR { u64 base, open, at; u32 state, look; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi; bytes: packed so far, (provisional tail)'s D
struct StateR { u64 start, state, sel, tail, bytes, pad[3]; };
struct TotalsR { StateR st[2]; u64 matches, delims, pad[6]; };
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grepx_count_kernel with (summary)'s two fields. Per tile its summary -> sums[tile]
// and its map -> maps[tile]. (Kept beside the regex grep's count, not joined with it: one body for both, with the two fields switched
// on, cost this kernel 0.06 ms per GiB, profiles/record_scan_refactor.md.)
extern "C" __global__ void __launch_bounds__(256) zra_extractx_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
                                                                            u64 p0, SumR* sums, u8* maps, TotalsR* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u32 sCnt[4], sSel[4], sBytes[4], sTail;
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
    u32 sel = 0, bytes = 0;
    for (u32 k = 1 + tid; k <= nD; k += 256) {
      const u32 from = (u32)sPos[k - 1] + 1, to = k < nD ? (u32)sPos[k] : n;
      const u32 st = walk(&sD, sTile, d, from, to, start);
      if (k == nD) { sTail = st; continue; }
      const u32 m = (u32)(accept >> st) & 1, s = m ^ inv;
      matched += m; sel += s; bytes += s ? to - from + 1 : 0;
    }
    sel = wave_sum(sel); bytes = wave_sum(bytes);
    if (lane == 0) { sSel[wave] = sel; sBytes[wave] = bytes; }
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
      SumR r;
      r.first = nD ? p0 + t0 + sPos[0] : 0; r.last = nD ? p0 + t0 + sPos[nD - 1] + 1 : 0;
      r.bytes = sBytes[0] + sBytes[1] + sBytes[2] + sBytes[3]; r.sel = sSel[0] + sSel[1] + sSel[2] + sSel[3];
      r.has = nD ? 1 : 0; r.tail = (u8)(nD ? sTail : 0); r.fsel = 0;
      for (u32 i = 0; i < 5; i++) r.pad[i] = 0;
      sums[b] = r;
    }
  }
  matched = wave_sum(matched);
  if (lane == 0 && matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
  if (tid == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);
}

// One workgroup, (scan). Forward, zra_regex_tile.h's with (summary)'s two fields. The last lane ends the pass: in the last pass the
// record open at hi ends there (its list entry and its delimiter byte). Backward, the extracts' (look-ahead): the bit of the nearest
// following tile with a delimiter, or of the pass's end, reaches every tile's head.
extern "C" __global__ void __launch_bounds__(1024) zra_extractx_scan_kernel(SumR* sums, const u8* maps, u32 nTiles, HeadR* heads, const StateR* in, StateR* out,
                                                                            const RxTable* tbl, u32 inv, u32 lastPass, u64 hi, u64 p0, u64 nPos, Range* list, u64 cap,
                                                                            u8* dData, u64 dataCap, u32 delim, TotalsR* tot) {
  const u64 accept = tbl->accept;
  RegexFront e = regex_scan_forward<true>(sums, maps, nTiles, heads, in, accept, inv);
  u32 tailSel = 0;
  if (threadIdx.x == 1023) {                                                 // (its run is the last one, or empty behind the last one)
    const u32 m = (u32)(accept >> e.state) & 1;
    if (lastPass && e.start < hi) e.matched += m;
    u64 tl;
    tailSel = extract_pass_end(lastPass, (m ^ inv) != 0, e.start, hi, e.count, e.at, tl, list, cap, dData, dataCap, delim);
    StateR o; o.start = e.start; o.state = e.state; o.sel = e.count; o.tail = tl; o.bytes = e.at; o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *out = o;
  }
  if (e.matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)e.matched);
  look_ahead(e.look, tailSel, e.b0, e.b1, p0, nPos, heads, [&](u32 t) { const SumR s = sums[t]; return LookTile{s.has != 0, s.fsel, s.last}; });
}

// The count's workgroups redo the tiles that hold a byte of a selected record or a listed record in front of the capacities (the
// others are skipped; a workgroup without such a tile leaves at once).
extern "C" __global__ void __launch_bounds__(256) zra_extractx_copy_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
                                                                           u64 p0, const SumR* sums, const HeadR* heads, Range* list, u64 cap, u8* dData, u64 dataCap) {
  constexpr u32 kSelBit = 0x8000u;                                           // in sPos: the record this delimiter ends is selected (above kPosMask)
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u32 sPre[kTile + 1];                                            // in front of delimiter k: selected records << 16 | their packed bytes, the first record's left out
  __shared__ u32 sCnt[4], sW[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  // a tile's bytes go to head.at and behind, its list entries to head.base and behind (uniform in the workgroup)
  auto wanted = [&](u32 b) {
    const u32 sel = sums[b].sel;
    const HeadR h = heads[b];
    return ((sel != 0 || h.look != 0) && h.at < dataCap) || (sel != 0 && h.base < cap);
  };
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) any |= wanted(b);
  if (!any) return;
  const u32 start = tbl->start;
  const u64 accept = tbl->accept;
  stage_dfa(tbl, &sD, tbl->classes);
  const u64 below = (1ull << lane) - 1;
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!wanted(b)) continue;
    const HeadR head = heads[b];
    const u64 t0 = (u64)b * kTile, pos0 = p0 + t0;                           // pos0: the content offset of the tile's position 0
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, n, sTile);
    __syncthreads();
    // ---- phase 1: the delimiters, and in sPos[k] the selection bit of the record that delimiter k ends
    const u32 nD = regex_select(&sD, sTile, d, n, delim, sPos, sCnt, start, head.state, accept, inv, [&](u32 k, u32 to, u32 bit) { if (bit) sPos[k] = (u16)(to | kSelBit); });
    // ---- phase 2: the exclusive prefix. A lane takes `chunk` consecutive delimiters; the 256 lane sums are scanned by wave
    const u32 chunk = (nD + 255) / 256, k0 = min(nD, tid * chunk), k1 = min(nD, k0 + chunk);
    u32 mine = 0;
    for (u32 k = k0; k < k1; k++) {
      const u32 e = sPos[k];
      if (e & kSelBit) mine += 0x10000u + (k ? (e & kPosMask) - ((u32)sPos[k - 1] & kPosMask) : 0);
    }
    const u32 incl = wave_incl_scan(mine);
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    u32 run = incl - mine;
    for (u32 v = 0; v < wave; v++) run += sW[v];
    for (u32 k = k0; k < k1; k++) {
      sPre[k] = run;
      const u32 e = sPos[k];
      if (e & kSelBit) run += 0x10000u + (k ? (e & kPosMask) - ((u32)sPos[k - 1] & kPosMask) : 0);
    }
    if (tid == 255) sPre[nD] = sW[0] + sW[1] + sW[2] + sW[3];                // (lane 255's chunk is the last one, or empty)
    __syncthreads();
    // ---- phase 3: a lane per position. k = the delimiters in front of q = the record q lies in; q's record ends at delimiter k
    if (w0 >= n) continue;                                                   // (uniform in the wave; the barriers are at the loop's head)
    // the packed bytes of record 0, which began at head.open, when it is selected
    const u64 firstAdd = nD && (sPos[0] & kSelBit) ? pos0 + ((u32)sPos[0] & kPosMask) - head.open + 1 : 0;
    u32 kw = 0;
    for (u32 v = 0; v < wave; v++) kw += sCnt[v];
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u32 q = w0 + t * 64 + lane;
      const bool inside = q < n;
      const u32 byte = inside ? tile_byte(sTile, d + q) : 0;
      const bool isD = inside && byte == delim;
      const u64 dm = __ballot(isD);
      const u32 k = kw + (u32)__popcll(dm & below);
      kw += (u32)__popcll(dm);
      bool sel = false;
      u64 to = 0;                                                            // where q's byte goes
      if (inside) {
        sel = k < nD ? (sPos[k] & kSelBit) != 0 : head.look != 0;
        if (k == 0) to = head.at + (pos0 + q - head.open);                   // the record open at the tile's head
        else to = head.at + firstAdd + (sPre[k] & 0xFFFFu) + (q - (((u32)sPos[k - 1] & kPosMask) + 1));
      }
      if (sel && to < dataCap) dData[to] = (u8)byte;
      if (sel && isD) {
        const u64 idx = head.base + (sPre[k] >> 16);
        if (idx < cap) {
          const u64 from = k ? pos0 + ((u32)sPos[k - 1] & kPosMask) + 1 : head.open;
          Range r; r.offset = from; r.size = pos0 + q - from;
          list[idx] = r;
        }
      }
    }
  }
}

// =================================================================================================
// The kernel set of the regex extract for zra_record_scan.h's call path. tables: Table | Totals | sums[tiles] | heads[tiles] | maps[tiles]
namespace {
struct ExtractRegexKernels {
  using Sum = SumR; using Head = HeadR; using Totals = TotalsR;
  static constexpr size_t kMapBytes = 64;
  static constexpr bool kData = true;
  static void launch(hipStream_t s, const RegexSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<ExtractRegexKernels>& p, u32 parity) {
    const RxTable* const tbl = (const RxTable*)p.table;
    const u32 delim = c.delimiter, inv = sel.inv;
    hipLaunchKernelGGL(zra_extractx_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, (u64)ps.p0, p.sums, p.maps, p.tot);
    hipLaunchKernelGGL(zra_extractx_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.maps, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), tbl, inv,
                       (u32)ps.lastPass, (u64)p.hi, (u64)ps.p0, (u64)ps.nPos, p.list, (u64)p.listCap, c.dData, (u64)c.dataCap, delim, p.tot);
    if (p.listCap || c.dataCap)
      hipLaunchKernelGGL(zra_extractx_copy_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, (u64)ps.p0, p.sums, p.heads, p.list,
                         (u64)p.listCap, c.dData, (u64)c.dataCap);
  }
};
static_assert(sizeof(TotalsR) == 192 && sizeof(SumR) == 32 && sizeof(HeadR) == 32, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::extract_regex(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<RegexSelect, ExtractRegexKernels>(E, c, cv); }
}  // namespace zra_eng
