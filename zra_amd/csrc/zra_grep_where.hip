// zra_amd — grep of a device-resident archive with a record predicate (zra_hip.h: ZraHipGrepArchiveWhere): the records
// of a content range whose HIT SET satisfies a boolean combination of up to 64 patterns, in one decode and one scan of the range.
// What `grep A | grep B | grep -v C` is to one grep per term.
//
// Records, matches, range, passes, ownership, (stream), (forward), (launches), (order) and (d) are the plain grep's (zra_grep.hip), word
// for word; the pattern table, the staging and the test of one position are zra_patterns.h's, the driver is zra_scan.h's, the host
// path in front of it zra_record_scan.h's (the literal selector's patterns under clauses, the kernel set at the end of this file). The
// kernels are the plain grep's twins, in a translation unit of their own. What differs:
//  (set) where the plain grep carries one bit (has the open record matched yet), this call carries a 64-bit word: the patterns that
//      have hit in the open record so far. Sets are ORed where the grep ORs bits, and a record is selected by where_selected(set)
//      (zra_where.h) where the grep tests bit ^ invert.
//  (summary) a run of positions reduces to {has a delimiter, front: the patterns hit in front of the first one, behind: those hit
//      behind the last one, the position behind the last one, sel: records selected among those that end inside it APART from the
//      first}: 32 bytes. Without a delimiter front == behind == the patterns hit anywhere. combine() below has the grep's three cases;
//      the record that B's first delimiter ends is selected by where_selected(A.behind | B.front). The fill's head is 32 bytes as
//      well: list base, start of the record open at the tile's head, its set.
//  (trip) a delimiter lane needs the OR of the masks of the lanes between the previous delimiter and itself. A trip in which few
//      lanes hit (below kScanFrom) ORs their masks into a wave-uniform union U, one read of a lane per hitting lane; per pattern i
//      of U one ballot of bit i gives the lanes where it hit, and the plain grep's `seg` expression on that ballot is bit i of the
//      lane's set: the cost follows the hits, typically one or two patterns. A trip in which many lanes hit takes a six-step
//      segmented OR scan over the lanes instead, whose cost does not depend on the hits. A trip without a hit does neither: it
//      leaves as early as the plain grep's. Every loop is bounded by 64 and every branch depends on ballots only, so they are
//      uniform in the wave and no barrier lies under them.
//  (second walk) only the FIRST delimiter of a trip depends on what lies in front of the trip. The fill keeps four words per trip in
//      LDS: the delimiter ballot, the selection ballot of the other delimiters, front and behind. Its second walk selects the first
//      delimiter by one uniform test and never looks at a lane's set again.
#include "zra_record_scan.h"
#include "zra_where_tile.h"

namespace {
struct __attribute__((aligned(16))) SumW { u64 front, behind, last; u32 sel, has; };
struct __attribute__((aligned(16))) HeadW { u64 base, open, set, pad; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi
struct StateW { u64 start, set, sel, tail; };
// The words the launches of a call add up, uploaded with the table: the ping-pong state (c), then the atomics.
struct TotalsW { StateW st[2]; u64 matches, delims, pad[6]; };

// a summary while it is being combined: sel is kept wide by the scan
struct Acc { u64 front, behind, last, sel; u32 has; };

// A := the summary of run A followed by run B
__device__ __forceinline__ void combine(Acc& A, u32 hasB, u64 frontB, u64 behindB, u64 lastB, u64 selB, const Block& w) {
  if (!hasB) {
    if (A.has) A.behind |= frontB; else { A.front |= frontB; A.behind = A.front; }
    return;
  }
  if (!A.has) { A.front |= frontB; A.behind = behindB; A.sel = selB; A.last = lastB; A.has = 1; return; }
  A.sel += selB + (where_selected(w, A.behind | frontB) ? 1u : 0u);
  A.behind = behindB; A.last = lastB;
}

// A wave's first walk over its trips: the record that the wave's first delimiter ends is left to whoever combines the summaries
// (front says what hit in it inside the wave). set: the patterns hit in the record open behind the trips so far.
struct WalkW { bool seen; u32 sel; u64 set, front, start; };

// One trip of the first walk: dm / hm = the ballots of the two flags, m = the lane's mask, pos = the content offset of lane 0's
// position. kStore: the trip's four words of (second walk) go to out4.
template <bool kStore>
__device__ __forceinline__ void walk_trip_sets(WalkW& s, u64 dm, u64 hm, u64 m, u32 lane, const Block& w, u64 pos, u64* out4) {
  if (dm == 0) {                                                             // (uniform in the wave, as every branch on a ballot below)
    const u64 U = hm ? trip_union(m, hm, lane) : 0;
    s.set |= U;
    if (kStore && lane == 0) { out4[0] = 0; out4[1] = 0; out4[2] = U; out4[3] = U; }
    return;
  }
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;           // the delimiter in front of this lane, inside the trip
  const u64 seg = dBelow ? below & ~((2ull << prev) - 1) : below;            // the lanes between it (or the trip's head) and this lane
  u64 H = 0, front = 0, behind = 0;
  if (hm) trip_sets(m, hm, dm, lane, first, last, seg, &H, &front, &behind);
  const bool sel = ((dm >> lane) & 1) && lane != first && where_selected(w, H);
  const u64 sb = __ballot(sel);
  s.sel += (u32)__popcll(sb);
  if (!s.seen) { s.front = s.set | front; s.seen = true; }
  else s.sel += where_selected(w, s.set | front) ? 1u : 0u;
  s.set = behind;
  s.start = pos + last + 1;
  if (kStore && lane == 0) { out4[0] = dm; out4[1] = sb; out4[2] = front; out4[3] = behind; }
}

__device__ __forceinline__ SumW walk_sum(const WalkW& s) {
  SumW r;
  r.front = s.seen ? s.front : s.set; r.behind = s.set; r.last = s.start; r.sel = s.sel; r.has = s.seen ? 1u : 0u;
  return r;
}

// One trip of the (second walk): set / start are the open record's in front of the trip; the selected records that end in the trip go
// to list[at + ...] while there is room; at moves on.
__device__ __forceinline__ void emit_trip(u64& set, u64& start, u64 dm, u64 sb, u64 front, u64 behind, u32 lane, const Block& w, u64 pos, u64& at, Range* list,
                                          u64 cap) {
  if (dm == 0) { set |= front; return; }
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;
  const u64 sm = sb | (where_selected(w, set | front) ? 1ull << first : 0);
  const u64 idx = at + (u32)__popcll(sm & below);
  if (((sm >> lane) & 1) && idx < cap) {
    const u64 from = dBelow ? pos + prev + 1 : start;
    Range r; r.offset = from; r.size = pos + lane - from;
    list[idx] = r;
  }
  at += (u32)__popcll(sm);
  set = behind;
  start = pos + last + 1;
}
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grep.hip's grep_count. Per tile its summary -> sums[tile]; per call the totals.
template <class TB>
__device__ __forceinline__ void grepw_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, const Block& w, u64 p0, SumW* sums,
                                            TotalsW* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ SumW sW[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  stage_table(tbl, &sT);
  u32 pairs = 0, delims = 0;
  for (u32 b = blockIdx.x * kGroup, bEnd = min(tiles, b + kGroup); b < bEnd; b++) {
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();                                                         // (the tile in front is done with)
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    WalkW s = {false, 0, 0, 0, p0 + t0 + w0};
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      const u64 m = trip_masks(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      delims += (u32)__popcll(dm);
      walk_trip_sets<false>(s, dm, hm, m, lane, w, p0 + t0 + w0 + t * 64, nullptr);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (tid == 0) {
      Acc a = {sW[0].front, sW[0].behind, sW[0].last, sW[0].sel, sW[0].has};
      for (u32 v = 1; v < 4; v++) combine(a, sW[v].has, sW[v].front, sW[v].behind, sW[v].last, sW[v].sel, w);
      SumW r; r.front = a.front; r.behind = a.behind; r.last = a.last; r.sel = (u32)a.sel; r.has = a.has;
      sums[b] = r;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
extern "C" __global__ void __launch_bounds__(256) zra_grepw_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                         Block w, u64 p0, SumW* sums, TotalsW* tot) {
  grepw_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_grepw_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                               u32 delim, Block w, u64 p0, SumW* sums, TotalsW* tot) {
  grepw_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, tot);
}

// One workgroup: zra_grep_scan_kernel over the 32-byte summaries. Every lane reduces a run of consecutive tiles, the 1024 summaries are
// scanned in LDS (Hillis-Steele over combine()), then the lane walks its run again from the state in front of it: heads[t], and
// sums[t].sel becomes ALL the selected records that end in tile t, the first included. lastPass: the record open at hi ends there.
extern "C" __global__ void __launch_bounds__(1024) zra_grepw_scan_kernel(SumW* sums, u32 nTiles, HeadW* heads, const StateW* in, StateW* out, Block w, u32 lastPass,
                                                                         u64 hi, Range* list, u64 cap) {
  __shared__ u64 sFront[1024], sBehind[1024], sLast[1024], sSel[1024];
  __shared__ u32 sHas[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  Acc a = {0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) { const SumW s = sums[t]; combine(a, s.has, s.front, s.behind, s.last, s.sel, w); }
  sFront[tid] = a.front; sBehind[tid] = a.behind; sLast[tid] = a.last; sSel[tid] = a.sel; sHas[tid] = a.has;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    Acc p = {0, 0, 0, 0, 0};
    if (tid >= d) { p.front = sFront[tid - d]; p.behind = sBehind[tid - d]; p.last = sLast[tid - d]; p.sel = sSel[tid - d]; p.has = sHas[tid - d]; }
    __syncthreads();
    if (tid >= d) {
      combine(p, a.has, a.front, a.behind, a.last, a.sel, w);
      a = p;
      sFront[tid] = a.front; sBehind[tid] = a.behind; sLast[tid] = a.last; sSel[tid] = a.sel; sHas[tid] = a.has;
    }
    __syncthreads();
  }
  // the state in front of this lane's run: the carried one, then the lanes in front
  u64 start = in->start, count = in->sel, set = in->set;
  if (tid) {
    if (sHas[tid - 1]) { count += sSel[tid - 1] + (where_selected(w, set | sFront[tid - 1]) ? 1u : 0u); set = sBehind[tid - 1]; start = sLast[tid - 1]; }
    else set |= sFront[tid - 1];
  }
  for (u32 t = b0; t < b1; t++) {
    const SumW s = sums[t];
    HeadW h; h.base = count; h.open = start; h.set = set; h.pad = 0;
    heads[t] = h;
    if (s.has) {
      const u32 all = s.sel + (where_selected(w, set | s.front) ? 1u : 0u);
      sums[t].sel = all;
      count += all; set = s.behind; start = s.last;
    } else set |= s.front;
  }
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tail = 0;
    if (lastPass && start < hi) {
      tail = 1;
      if (where_selected(w, set)) {
        if (count < cap) { Range r; r.offset = start; r.size = hi - start; list[count] = r; }
        count++;
      }
    }
    StateW o; o.start = start; o.set = set; o.sel = count; o.tail = tail;
    *out = o;
  }
}

// zra_grep.hip's grep_fill: the count's workgroups redo the tiles that hold a listed record. The first walk leaves every trip's four
// words in LDS with the waves' summaries; a wave takes what lies in front of it from the tile's head and the waves in front, and its
// second walk writes.
template <class TB>
__device__ __forceinline__ void grepw_fill(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, const Block& w, u64 p0,
                                           const SumW* sums, const HeadW* heads, Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ SumW sW[4];
  __shared__ u64 sTrip[4][kWaveIters][4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  bool any = false;                                                          // (uniform in the workgroup, like `listed` below)
  for (u32 b = bBegin; b < bEnd; b++) any |= sums[b].sel != 0 && heads[b].base < cap;
  if (!any) return;
  stage_table(tbl, &sT);
  for (u32 b = bBegin; b < bEnd; b++) {
    const HeadW head = heads[b];
    const bool listed = sums[b].sel != 0 && head.base < cap;
    if (!listed) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    WalkW s = {false, 0, 0, 0, p0 + t0 + w0};
    u32 pairs = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      const u64 m = trip_masks(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      walk_trip_sets<true>(s, dm, hm, m, lane, w, p0 + t0 + w0 + t * 64, sTrip[wave][t]);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (!sW[wave].has) continue;                                             // (uniform in the wave; the barriers are at the loop's head)
    u64 set = head.set, start = head.open, at = head.base;
    for (u32 v = 0; v < wave; v++) {
      const SumW f = sW[v];
      if (f.has) { at += f.sel + (where_selected(w, set | f.front) ? 1u : 0u); set = f.behind; start = f.last; }
      else set |= f.front;
    }
    if (at >= cap) continue;
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u64* const q = sTrip[wave][t];
      emit_trip(set, start, q[0], q[1], q[2], q[3], lane, w, p0 + t0 + w0 + t * 64, at, list, cap);
    }
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_grepw_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                        Block w, u64 p0, const SumW* sums, const HeadW* heads, Range* list, u64 cap) {
  grepw_fill<Table>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, heads, list, cap);
}
extern "C" __global__ void __launch_bounds__(256) zra_grepw_fill_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                              u32 delim, Block w, u64 p0, const SumW* sums, const HeadW* heads, Range* list, u64 cap) {
  grepw_fill<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, heads, list, cap);
}

// =================================================================================================
// The kernel set of the grep with a record predicate for zra_record_scan.h's call path. tables: Table | Totals | sums[tiles] | heads[tiles]
namespace {
struct WhereKernels {
  using Sum = SumW; using Head = HeadW; using Totals = TotalsW;
  static constexpr size_t kMapBytes = 0;
  static constexpr bool kData = false;
  static void launch(hipStream_t s, const WhereSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<WhereKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, M = sel.M;
    const Block& w = sel.w;
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_grepw_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, w, (u64)ps.p0, p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_grepw_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, w, (u64)ps.p0, p.sums, p.tot);
    hipLaunchKernelGGL(zra_grepw_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), w, (u32)ps.lastPass,
                       (u64)p.hi, p.list, (u64)p.listCap);
    if (p.listCap && sel.pset.classes)
      hipLaunchKernelGGL(zra_grepw_fill_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, w, (u64)ps.p0, p.sums, p.heads,
                         p.list, (u64)p.listCap);
    else if (p.listCap)
      hipLaunchKernelGGL(zra_grepw_fill_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, w, (u64)ps.p0, p.sums, p.heads, p.list,
                         (u64)p.listCap);
  }
};
}  // namespace

namespace zra_eng {
Status ScanImpl::grep_where(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<WhereSelect, WhereKernels>(E, c, cv); }
}  // namespace zra_eng
