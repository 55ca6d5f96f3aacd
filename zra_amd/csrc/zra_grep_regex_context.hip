// zra_amd — regex grep with context records (zra_hip.h: ZraHipGrepArchiveRegexContext): the records of a content range
// that the regex grep selects (zra_grep_regex.hip), and the `before` records in front and the `after` records behind each of them, as
// ascending {offset, size} pairs with ZRA_HIP_CONTEXT_SELECTED in the size of the selected ones; |S| and the number of groups beside
// |O|. What `grep -E -e expr... -b -A after -B before` prints, `--` lines counted.
//
// The passes, the window, (stream), (launches) and (order) are zra_grep.hip's; the selector is the regex grep's (RegexSelect), the
// automaton in LDS, the walks and the delimiter compaction are zra_regex_tile.h's, the algebra over records whose selection is known,
// (pending) included, is zra_context.h's, what joins the two, (summary), (combine) and (front), is zra_regex_context.h's, and the
// carried state, the head, the end of the scan kernel and the fill's writing trip, which the literal set runs alike, are
// zra_context_tile.h's. This file's own:
//  (count) zra_grepxc_count_kernel: the tile's delimiters compacted into LDS, one lane per record from the start state, as the regex
//      grep's count; the selection bits stay in LDS by delimiter, and the waves reduce a quarter of them each to a Ctx, in trips of
//      64 COMPACTED delimiters: dm is the mask of the trip's valid lanes, sm the bits, record 0 left out. Per tile a 16-byte summary
//      and the 64-byte head map.
//  (scan) zra_grepxc_scan_kernel, ONE workgroup of 1,024 lanes. Forwards: every lane reduces a run of tiles with (combine), the 1,024
//      Runs and maps are scanned in LDS (64 KiB of maps, 48 KiB of Runs), then the lane walks its run from the (front) in front of it:
//      per tile the DFA state and the Ctx in front, and, its first record now resolved, the tile's own look. Backwards, the end of
//      the pass and the carried state: context_scan_tail. Neither direction depends on before or after beyond the arithmetic of Ctx.
//  (fill) zra_grepxc_fill_kernel: the tiles with a listed or a pending record are redone. regex_select gives every delimiter's bit,
//      the head record's from the state in the tile's head entry, so a wave's quarter reduces to a Ctx with nothing left open; the
//      (forward) in front of a wave is the head's and the waves' in front, the (look) behind it the waves' behind and the head's. Then
//      the three walks over the trips of compacted delimiters: looks, looks backwards, and the writes at prefix counts, the pending
//      records behind the capacity.
// Every loop is bounded by the tile's size, no workgroup waits for another one, and no tile byte beyond hi is read.
#include "zra_record_scan.h"
#include "zra_regex_tile.h"
#include "zra_regex_context.h"
#include "zra_context_tile.h"

namespace {
using zra_rxc::Run;
using zra_rxc::Front;

// a tile's Run in device memory, 16 bytes, its map apart: w = has (1 bit) | tail state << 1 (6) | zra_context.h's ctx_pack above them
struct __attribute__((aligned(16))) XCSum { u64 last, w; };
__device__ __forceinline__ XCSum pack(const Run& r) { return XCSum{r.last, zra_ctx::ctx_pack((u64)r.has | (u64)r.tail << 1, r.c, 7)}; }
__device__ __forceinline__ Run unpack(const XCSum& s) { return Run{s.last, (u32)s.w & 1, (u32)(s.w >> 1) & 63, zra_ctx::ctx_unpack(s.w, 7)}; }
// per tile for the fill: CHead and the DFA state of the record open at the tile's first position
struct __attribute__((aligned(16))) XCHead : CHead { u32 state, pad[3]; };

// One trip of compacted delimiters [k, k + 64) below k1: the mask of the valid lanes and their selection bits; skip0: record 0 is
// not the tile's to decide.
__device__ __forceinline__ void trip_bits(const u8* sBit, u32 k, u32 k1, u32 lane, bool skip0, u64* dm, u64* sm) {
  const u32 mine = k + lane;
  const bool valid = mine < k1 && !(skip0 && mine == 0);
  *dm = __ballot(valid);
  *sm = __ballot(valid && sBit[mine] != 0);
}
// A wave's share reduced to its Ctx (uniform in the wave).
__device__ __forceinline__ Ctx share_ctx(const u8* sBit, u32 k0, u32 k1, u32 lane, bool skip0, u32 before, u32 after) {
  zra_ctx::CtxWalk cw = {false, 0, 0, 0, 0};
  for (u32 k = k0; k < k1; k += 64) {
    u64 dm, sm;
    trip_bits(sBit, k, k1, lane, skip0, &dm, &sm);
    zra_ctx::ctx_trip(cw, dm, sm, lane, before, after);
  }
  return zra_ctx::ctx_close(cw, before, after);
}
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grep.hip's grep_count. Per tile its summary -> sums[tile] and its map -> maps[tile].
extern "C" __global__ void __launch_bounds__(256) zra_grepxc_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
                                                                          u32 before, u32 after, u64 p0, XCSum* sums, u8* maps, CtxTotals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u8 sBit[kTile];
  __shared__ Ctx sW[4];
  __shared__ u32 sCnt[4], sTail;
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
    // records 1 .. nD - 1 end at a delimiter; "record" nD is the stretch behind the last one: the tile's tail
    for (u32 k = 1 + tid; k <= nD; k += 256) {
      const u32 from = (u32)sPos[k - 1] + 1, to = k < nD ? (u32)sPos[k] : n;
      const u32 st = walk(&sD, sTile, d, from, to, start);
      if (k == nD) { sTail = st; continue; }
      const u32 m = zra_rxc::accepts(accept, st);
      matched += m; sBit[k] = (u8)(m ^ inv);
    }
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
    __syncthreads();                                                         // (the bits are in LDS)
    u32 k0, k1;
    wave_share(nD, wave, &k0, &k1);
    const Ctx c = share_ctx(sBit, k0, k1, lane, true, before, after);
    if (lane == 0) sW[wave] = c;
    __syncthreads();
    if (tid == 0) {
      Run r; r.last = nD ? p0 + t0 + sPos[nD - 1] + 1 : 0; r.has = nD ? 1 : 0; r.tail = nD ? sTail : 0;
      r.c = sW[0];
      for (u32 w = 1; w < 4; w++) zra_ctx::append(r.c, sW[w], before, after);
      sums[b] = pack(r);
    }
  }
  matched = wave_sum(matched);
  if (lane == 0 && matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
  if (tid == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);
}

// One workgroup: (scan). pend = list + cap.
extern "C" __global__ void __launch_bounds__(1024) zra_grepxc_scan_kernel(const XCSum* sums, const u8* maps, u32 nTiles, XCHead* heads, const CtxState* in, CtxState* out,
                                                                          const RxTable* tbl, u32 inv, u32 before, u32 after, u32 lastPass, u64 hi, Range* list, u64 cap,
                                                                          CtxTotals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sMap[1024 * 16];
  __shared__ Run sR[1024];
  const u64 accept = tbl->accept;
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  const u8* const myMap = (const u8*)(sMap + tid * 16);
  // ---- the lane's run of tiles. F starts as the identity
  u32 F[16];
#pragma unroll
  for (u32 w = 0; w < 16; w++) F[w] = 0x03020100u + 0x04040404u * w;
  Run r; r.last = 0; r.has = 0; r.tail = 0; r.c = Ctx{0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) {
    const u8* const m = maps + (size_t)t * 64;
    if (zra_rxc::combine(r, unpack(sums[t]), m[r.tail], accept, inv, before, after)) compose(F, m, F);
  }
  auto put = [&] {
#pragma unroll
    for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
    sR[tid] = r;
  };
  put();
  __syncthreads();
  // ---- the scan: A = the lanes in front (at tid - d), B = this lane
  for (u32 d = 1; d < 1024; d <<= 1) {
    const bool on = tid >= d;
    if (on) {
      const u32 a = tid - d;
      Run A = sR[a];
      if (zra_rxc::combine(A, r, myMap[A.tail], accept, inv, before, after)) compose(F, myMap, sMap + a * 16);
      else {
#pragma unroll
        for (u32 w = 0; w < 16; w++) F[w] = sMap[a * 16 + w];                 // (A's map stands)
      }
      r = A;
    }
    __syncthreads();
    if (on) put();
    __syncthreads();
  }
  // ---- forwards: the front of this lane's run is the carried one, moved over the lanes in front
  Front f; f.start = in->start; f.state = (u32)in->state; f.c = in->c;
  if (tid) zra_rxc::advance(f, sR[tid - 1], ((const u8*)(sMap + (tid - 1) * 16))[f.state], accept, inv, before, after);
  u32 matched = 0;
  u32 runLook = zra_ctx::look(false, 0);
  for (u32 t = b0; t < b1; t++) {
    const Run s = unpack(sums[t]);
    const u32 through = maps[(size_t)t * 64 + f.state];
    XCHead h;
    h.base = f.c.out; h.open = f.start; h.state = f.state; h.pad[0] = h.pad[1] = h.pad[2] = 0;
    h.fwd = (f.c.sel ? zra_ctx::kLookHas : 0u) | f.c.tail;
    h.la = zra_ctx::look(false, 0); h.cnt = 0;
    h.pend = zra_ctx::uncovered(f.c, after);                                  // (until the walk backwards knows how many of them count)
    if (s.has) h.la = zra_rxc::resolved_look(zra_rxc::selected(accept, through, inv), s.c);
    matched += zra_rxc::advance(f, s, through, accept, inv, before, after);
    runLook = zra_ctx::look_cat(runLook, h.la);
    heads[t] = h;
  }
  // the record open at hi
  const bool tailRec = lastPass && f.start < hi, tailSel = zra_rxc::selected(accept, f.state, inv) != 0;
  if (tid == 1023 && tailRec) matched += zra_rxc::accepts(accept, f.state);
  if (matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
  context_scan_tail(f.c, f.start, f.state, runLook, tailRec, tailSel, b0, b1, heads, in, out, list, cap, hi, lastPass, before, after);
}

// The count's workgroups redo the tiles that hold a record of O in front of the capacity, or a pending one: (fill).
extern "C" __global__ void __launch_bounds__(256) zra_grepxc_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const RxTable* tbl, u32 delim, u32 inv,
                                                                         u32 before, u32 after, u64 p0, const XCSum* sums, const XCHead* heads, const CtxState* st,
                                                                         Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ __attribute__((aligned(16))) Dfa sD;
  __shared__ u16 sPos[kTile];
  __shared__ u8 sBit[kTile];
  __shared__ Ctx sW[4];
  __shared__ u32 sCnt[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  const u32 pendBase = st->pendBase, npThis = st->npThis;
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) any |= context_wanted(heads, sums, b, npThis, cap);
  if (!any) return;
  const u32 start = tbl->start;
  const u64 accept = tbl->accept;
  stage_dfa(tbl, &sD, tbl->classes);
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!context_wanted(heads, sums, b, npThis, cap)) continue;
    const XCHead head = heads[b];
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, n, sTile);
    __syncthreads();
    // the selection bit of the record that delimiter k ends, record 0 from the head's state: nothing of the tile is left open
    const u32 nD = regex_select(&sD, sTile, d, n, delim, sPos, sCnt, start, head.state, accept, inv, [&](u32 k, u32, u32 bit) { sBit[k] = (u8)bit; });
    u32 k0, k1;
    wave_share(nD, wave, &k0, &k1);
    const Ctx mine = share_ctx(sBit, k0, k1, lane, false, before, after);
    if (lane == 0) sW[wave] = mine;
    __syncthreads();
    if (k0 >= k1) continue;                                                  // (uniform in the wave; the barriers are in front)
    // (forward) in front of this wave and the (look) behind it, from the head and the four shares
    Ctx C = context_front(head);
#pragma unroll 1
    for (u32 w = 0; w < wave; w++) zra_ctx::append(C, sW[w], before, after);
    u32 behind = zra_ctx::look(false, 0);
#pragma unroll 1
    for (u32 w = wave + 1; w < 4; w++) behind = zra_ctx::look_cat(behind, zra_rxc::ctx_look(sW[w]));
    u32 la = zra_ctx::look_cat(behind, head.la);
    // forwards: every trip's look into lane t; backwards: the look at every trip's end into lane t
    const u32 trips = (k1 - k0 + 63) / 64;                                    // (at most 32)
    u32 keep = zra_ctx::look(false, 0);
#pragma unroll 1
    for (u32 t = 0; t < trips; t++) {
      u64 dm, sm;
      trip_bits(sBit, k0 + t * 64, k1, lane, false, &dm, &sm);
      const u32 tl = zra_ctx::ctx_trip_look(dm, sm);
      if (lane == t) keep = tl;
    }
    la = context_looks_back(keep, la, trips, lane);
    // la is now the look at the share's head: the (true count) in front of it
    u64 at = C.out + zra_ctx::confirmed(zra_ctx::uncovered(C, after), la, before);
    bool fAny = C.sel != 0;
    u32 fTail = C.tail;
#pragma unroll 1
    for (u32 t = 0; t < trips; t++) {
      u64 dm, sm;
      trip_bits(sBit, k0 + t * 64, k1, lane, false, &dm, &sm);
      const u32 k = k0 + t * 64 + lane;
      Range q; q.offset = 0; q.size = 0;
      if ((dm >> lane) & 1) {
        q.offset = k ? p0 + t0 + sPos[k - 1] + 1 : head.open;
        q.size = p0 + t0 + sPos[k] - q.offset;
      }
      context_write_trip(dm, sm, lane, q, (u32)__shfl((int)keep, (int)t, 64), at, fAny, fTail, list, cap, pendBase, npThis, before, after);
    }
  }
}

// =================================================================================================
// The kernel set of the regex grep with context for zra_record_scan.h's call path. tables: Table | Totals | sums[tiles] | heads[tiles]
// | maps[tiles]; the list scratch holds `before` pending entries behind the capacity.
namespace {
struct RegexContextKernels {
  using Sum = XCSum; using Head = XCHead; using Totals = CtxTotals;
  static constexpr size_t kMapBytes = 64;
  static constexpr bool kData = false;
  static void launch(hipStream_t s, const RegexSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<RegexContextKernels>& p, u32 parity) {
    const RxTable* const tbl = (const RxTable*)p.table;
    const u32 delim = c.delimiter, inv = sel.inv, before = c.before, after = c.after;
    hipLaunchKernelGGL(zra_grepxc_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, before, after, (u64)ps.p0, p.sums,
                       p.maps, p.tot);
    hipLaunchKernelGGL(zra_grepxc_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.maps, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), tbl, inv, before,
                       after, (u32)ps.lastPass, (u64)p.hi, p.list, (u64)p.listCap, p.tot);
    if (p.listCap)
      hipLaunchKernelGGL(zra_grepxc_fill_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, delim, inv, before, after, (u64)ps.p0, p.sums,
                         p.heads, p.tot->st + (parity ^ 1), p.list, (u64)p.listCap);
  }
};
static_assert(sizeof(CtxTotals) == 176 && sizeof(XCSum) == 16 && sizeof(XCHead) == 48 && sizeof(Run) == 48, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::grep_regex_context(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<RegexSelect, RegexContextKernels>(E, c, cv); }
}  // namespace zra_eng
