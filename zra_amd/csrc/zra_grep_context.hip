// zra_amd — grep with context records (zra_hip.h: ZraHipGrepArchiveContext): the records of a content range that the
// plain grep selects (zra_grep.hip), and the `before` records in front and the `after` records behind each of them, as ascending
// {offset, size} pairs with ZRA_HIP_CONTEXT_SELECTED in the size of the selected ones; |S| and the number of groups beside |O|.
// What `grep -F -f patterns -b -A after -B before` prints, `--` lines counted.
//
// The passes, the window, (stream), (launches) and (order) are zra_grep.hip's; the selector is the plain grep's (LiteralSelect); the
// algebra over records whose selection is known, (pending) included, is zra_context.h's; the carried state, the head, the end of the
// scan kernel and the fill's writing trip, which the regex set runs alike, are zra_context_tile.h's. This file's own:
//  (summary) a run of positions reduces to Run = {flags, last: as the grep's Sum; c: zra_context.h's Ctx of the records that end inside
//      the run APART from the first}, and combine() resolves the record that the second run's first delimiter ends, as the grep's does,
//      and appends it: A.c + single(selected) + B.c.
//  (launches) zra_grepc_count_kernel: per tile its Run; the totals as atomics. zra_grepc_scan_kernel, ONE workgroup: forwards, the
//      tiles' Runs become per tile the Ctx of everything in front (the carried one included) and the tile's own look; the walk
//      backwards, the end of the pass and the carried state are context_scan_tail's. zra_grepc_fill_kernel: the workgroups redo the
//      tiles that hold a listed or a pending record. A wave takes (forward) from the head and the waves in front and (look) from the
//      head and the waves behind, walks its trips forwards (the selection, from the position masks kept in LDS), backwards (the look
//      at every trip's end) and forwards again, writing.
#include "zra_record_scan.h"
#include "zra_context_tile.h"

namespace {
struct __attribute__((aligned(16))) CRun { u64 last; u32 flags, pad; Ctx c; };
// a tile's Run in device memory, 16 bytes as the grep's Sum: w = flags (3 bits) | zra_context.h's ctx_pack above them
struct __attribute__((aligned(16))) CSum { u64 last, w; };
__device__ __forceinline__ CSum pack(const CRun& r) { return CSum{r.last, zra_ctx::ctx_pack((u64)r.flags, r.c, 3)}; }
__device__ __forceinline__ CRun unpack(const CSum& s) { return CRun{s.last, (u32)s.w & 7, 0, zra_ctx::ctx_unpack(s.w, 3)}; }

__device__ __forceinline__ void combine(CRun& A, const CRun& B, u32 inv, u32 before, u32 after) {
  if (!(B.flags & 1)) { if (B.flags & 2) A.flags |= (A.flags & 1) ? 4u : 6u; return; }
  if (!(A.flags & 1)) { A.flags = 1 | ((A.flags | B.flags) & 2) | (B.flags & 4); A.last = B.last; A.c = B.c; return; }
  zra_ctx::push(A.c, (((A.flags >> 2) | (B.flags >> 1)) & 1) ^ inv, before, after);
  zra_ctx::append(A.c, B.c, before, after);
  A.flags = 1 | (A.flags & 2) | (B.flags & 4); A.last = B.last;
}

// the grep's walk state; seen = false: the record that the wave's first delimiter ends is left to whoever combines
struct CWalk { bool seen, hit, hitFirst; u64 start; };

// One trip: the ballot of "the record this delimiter ends is selected" over the resolved delimiters *dmr of dm.
__device__ __forceinline__ u64 select_trip(CWalk& s, u64 dm, u64 hm, u32 lane, u32 inv, u64 pos, u64* dmr) {
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;
  const u64 seg = dBelow ? hm & below & ~((2ull << prev) - 1) : hm & below;
  const bool hit = seg != 0 || (!dBelow && s.hit);
  const bool sel = ((dm >> lane) & 1) && (hit != (bool)inv) && (s.seen || lane != first);
  const u64 sm = __ballot(sel);
  *dmr = s.seen ? dm : dm & ~(1ull << first);
  if (!s.seen) { s.hitFirst = s.hit || (hm & ((1ull << first) - 1)) != 0; s.seen = true; }
  s.hit = last < 63 && (hm >> (last + 1)) != 0;
  s.start = pos + last + 1;
  return sm;
}

// A wave's trips -> its Run; kKeep: the ballots go to mask[t] for the fill's walks.
template <class TB, bool kKeep>
__device__ __forceinline__ CRun wave_run(const TB* sT, const u32* sTile, u32 d, u32 w0, u32 n, long long toHi, u32 delim, u32 inv, u32 before, u32 after, u64 pos0,
                                         u32 lane, u32* pairs, u32* delims, u64 (*mask)[2]) {
  CWalk s = {false, false, false, pos0};
  zra_ctx::CtxWalk cw = {false, 0, 0, 0, 0};
  u32 np = 0, nd = 0;
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    u64 dm, hm;
    trip_flags(sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &np);
    if (kKeep && lane == 0) { mask[t][0] = dm; mask[t][1] = hm; }
    nd += (u32)__popcll(dm);
    if (dm == 0) s.hit |= hm != 0;
    else {
      u64 dmr;
      const u64 sm = select_trip(s, dm, hm, lane, inv, pos0 + t * 64, &dmr);
      zra_ctx::ctx_trip(cw, dmr, sm, lane, before, after);
    }
  }
  *pairs += np; *delims += nd;
  CRun r;
  r.last = s.start; r.pad = 0;
  r.flags = s.seen ? 1u | (s.hitFirst ? 2u : 0u) | (s.hit ? 4u : 0u) : (s.hit ? 6u : 0u);
  r.c = zra_ctx::ctx_close(cw, before, after);
  return r;
}
}  // namespace

template <class TB>
__device__ __forceinline__ void grepc_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, u32 inv, u32 before, u32 after,
                                            u64 p0, CSum* sums, CtxTotals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ CRun sW[4];
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
    const CRun r = wave_run<TB, false>(&sT, sTile, d, w0, n, toHi, delim, inv, before, after, p0 + t0 + w0, lane, &pairs, &delims, nullptr);
    if (lane == 0) sW[wave] = r;
    __syncthreads();
    if (tid == 0) {
      CRun a = sW[0];
      for (u32 w = 1; w < 4; w++) combine(a, sW[w], inv, before, after);
      sums[b] = pack(a);
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
extern "C" __global__ void __launch_bounds__(256) zra_grepc_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                         u32 inv, u32 before, u32 after, u64 p0, CSum* sums, CtxTotals* tot) {
  grepc_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, before, after, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_grepc_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                               u32 delim, u32 inv, u32 before, u32 after, u64 p0, CSum* sums, CtxTotals* tot) {
  grepc_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, before, after, p0, sums, tot);
}

// One workgroup: (launches). Every lane reduces a run of consecutive tiles, the 1,024 Runs are scanned in LDS (Hillis-Steele over
// combine()), the lane walks its run forwards from the state in front of it, and context_scan_tail does the rest.
extern "C" __global__ void __launch_bounds__(1024) zra_grepc_scan_kernel(const CSum* sums, u32 nTiles, CHead* heads, const CtxState* in, CtxState* out, u32 inv, u32 before,
                                                                         u32 after, u32 lastPass, u64 hi, Range* list, u64 cap) {
  __shared__ CRun sR[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  CRun r; r.last = 0; r.flags = 0; r.pad = 0; r.c = Ctx{0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) combine(r, unpack(sums[t]), inv, before, after);
  sR[tid] = r;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    CRun a;
    if (tid >= d) a = sR[tid - d];
    __syncthreads();
    if (tid >= d) { combine(a, r, inv, before, after); r = a; sR[tid] = r; }
    __syncthreads();
  }
  // forwards: the state in front of this lane's run is the carried one, then the lanes in front
  u64 start = in->start;
  bool hit = in->state != 0;
  Ctx C = in->c;
  if (tid) {
    const CRun e = sR[tid - 1];
    if (e.flags & 1) {
      zra_ctx::push(C, (u32)(hit || (e.flags & 2)) ^ inv, before, after);
      zra_ctx::append(C, e.c, before, after);
      hit = (e.flags & 4) != 0; start = e.last;
    } else hit |= (e.flags & 2) != 0;
  }
  u32 runLook = zra_ctx::look(false, 0);
  for (u32 t = b0; t < b1; t++) {
    const CRun s = unpack(sums[t]);
    CHead h;
    h.base = C.out; h.open = start | (hit ? kHitBit : 0);
    h.fwd = (C.sel ? zra_ctx::kLookHas : 0u) | C.tail;
    h.la = zra_ctx::look(false, 0); h.cnt = 0;
    h.pend = zra_ctx::uncovered(C, after);                                    // (until the walk backwards knows how many of them count)
    if (s.flags & 1) {
      const u32 sel1 = (u32)(hit || (s.flags & 2)) ^ inv;
      h.la = zra_ctx::resolved_look(sel1, s.c);
      zra_ctx::push(C, sel1, before, after);
      zra_ctx::append(C, s.c, before, after);
      hit = (s.flags & 4) != 0; start = s.last;
    } else hit |= (s.flags & 2) != 0;
    runLook = zra_ctx::look_cat(runLook, h.la);
    heads[t] = h;
  }
  const bool tailRec = lastPass && start < hi, tailSel = (u32)hit != inv;      // the record open at hi
  context_scan_tail(C, start, hit, runLook, tailRec, tailSel, b0, b1, heads, in, out, list, cap, hi, lastPass, before, after);
}

// The count's workgroups redo the tiles that hold a record of O in front of the capacity, or a pending one.
template <class TB>
__device__ __forceinline__ void grepc_fill(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, u32 inv, u32 before, u32 after,
                                           u64 p0, const CSum* sums, const CHead* heads, const CtxState* st, Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ CRun sW[4];
  __shared__ u64 sMask[4][kWaveIters][2];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  const u32 pendBase = st->pendBase, npThis = st->npThis;
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) any |= context_wanted(heads, sums, b, npThis, cap);
  if (!any) return;
  stage_table(tbl, &sT);
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!context_wanted(heads, sums, b, npThis, cap)) continue;
    const CHead head = heads[b];
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u32 pairs = 0, delims = 0;
    const CRun mine = wave_run<TB, true>(&sT, sTile, d, w0, n, toHi, delim, inv, before, after, p0 + t0 + w0, lane, &pairs, &delims, sMask[wave]);
    if (lane == 0) sW[wave] = mine;
    __syncthreads();
    if (!(mine.flags & 1)) continue;                                         // (uniform in the wave; the barriers are at the loop's head)
    // (forward) in front of this wave and the (look) behind it, from the head and the four Runs
    Ctx C = context_front(head);
    bool hit = (head.open & kHitBit) != 0;
    u64 start = head.open & ~kHitBit;
#pragma unroll 1
    for (u32 w = 0; w < wave; w++) {
      const CRun v = sW[w];
      if (!(v.flags & 1)) { hit |= (v.flags & 2) != 0; continue; }
      zra_ctx::push(C, (u32)(hit || (v.flags & 2)) ^ inv, before, after);
      zra_ctx::append(C, v.c, before, after);
      hit = (v.flags & 4) != 0; start = v.last;
    }
    const Ctx myC = C;
    const u64 myStart = start;
    const bool myHit = hit;
    u32 behind = zra_ctx::look(false, 0);                                     // the waves behind this one, resolved
    hit = (mine.flags & 4) != 0;
#pragma unroll 1
    for (u32 w = wave + 1; w < 4; w++) {
      const u32 f = sW[w].flags;
      if (!(f & 1)) { hit |= (f & 2) != 0; continue; }
      behind = zra_ctx::look_cat(behind, zra_ctx::resolved_look((u32)(hit || (f & 2)) ^ inv, sW[w].c));
      hit = (f & 4) != 0;
    }
    u32 la = zra_ctx::look_cat(behind, head.la);
    // forwards: the selection of every trip, its look into lane t; backwards: the look at every trip's end into lane t
    const u32 trips = min(kWaveIters, (n - w0 + 63) / 64);
    CWalk e = {true, myHit, false, myStart};
    u32 keep = zra_ctx::look(false, 0);
#pragma unroll 1
    for (u32 t = 0; t < trips; t++) {
      const u64 dm = sMask[wave][t][0], hm = sMask[wave][t][1];
      if (dm == 0) { e.hit |= hm != 0; continue; }
      u64 dmr;
      const u64 sm = select_trip(e, dm, hm, lane, inv, 0, &dmr);
      const u32 tl = zra_ctx::ctx_trip_look(dm, sm);
      if (lane == t) keep = tl;
    }
    la = context_looks_back(keep, la, trips, lane);
    // la is now the look at the wave's head: the (true count) in front of it
    u64 at = myC.out + zra_ctx::confirmed(zra_ctx::uncovered(myC, after), la, before);
    bool fAny = myC.sel != 0;
    u32 fTail = myC.tail;
    e = CWalk{true, myHit, false, myStart};
#pragma unroll 1
    for (u32 t = 0; t < trips; t++) {
      const u64 dm = sMask[wave][t][0], hm = sMask[wave][t][1];
      if (dm == 0) { e.hit |= hm != 0; continue; }
      const u64 pos = p0 + t0 + w0 + t * 64;
      const u64 recStart = e.start;
      u64 dmr;
      const u64 sm = select_trip(e, dm, hm, lane, inv, pos, &dmr);
      const u64 below = (1ull << lane) - 1, dBelow = dm & below;
      Range q;
      q.offset = dBelow ? pos + (63 - (u32)__builtin_clzll(dBelow)) + 1 : recStart;
      q.size = pos + lane - q.offset;
      context_write_trip(dm, sm, lane, q, (u32)__shfl((int)keep, (int)t, 64), at, fAny, fTail, list, cap, pendBase, npThis, before, after);
    }
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_grepc_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                        u32 inv, u32 before, u32 after, u64 p0, const CSum* sums, const CHead* heads, const CtxState* st,
                                                                        Range* list, u64 cap) {
  grepc_fill<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, before, after, p0, sums, heads, st, list, cap);
}
extern "C" __global__ void __launch_bounds__(256) zra_grepc_fill_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                              u32 delim, u32 inv, u32 before, u32 after, u64 p0, const CSum* sums, const CHead* heads,
                                                                              const CtxState* st, Range* list, u64 cap) {
  grepc_fill<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, before, after, p0, sums, heads, st, list, cap);
}

// =================================================================================================
// The kernel set of the grep with context for zra_record_scan.h's call path. tables: Table | CtxTotals | sums[tiles] | heads[tiles];
// the list scratch holds `before` pending entries behind the capacity.
namespace {
struct ContextKernels {
  using Sum = ::CSum; using Head = ::CHead; using Totals = ::CtxTotals;
  static constexpr size_t kMapBytes = 0;
  static constexpr bool kData = false;
  static void launch(hipStream_t s, const LiteralSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<ContextKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, inv = sel.inv, M = sel.M, before = c.before, after = c.after;
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_grepc_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, before, after, (u64)ps.p0,
                         p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_grepc_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, before, after, (u64)ps.p0, p.sums,
                         p.tot);
    hipLaunchKernelGGL(zra_grepc_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), inv, before, after,
                       (u32)ps.lastPass, (u64)p.hi, p.list, (u64)p.listCap);
    if (p.listCap && sel.pset.classes)
      hipLaunchKernelGGL(zra_grepc_fill_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, before, after, (u64)ps.p0,
                         p.sums, p.heads, p.tot->st + (parity ^ 1), p.list, (u64)p.listCap);
    else if (p.listCap)
      hipLaunchKernelGGL(zra_grepc_fill_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, before, after, (u64)ps.p0, p.sums,
                         p.heads, p.tot->st + (parity ^ 1), p.list, (u64)p.listCap);
  }
};
}  // namespace

namespace zra_eng {

Status ScanImpl::grep_context(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<LiteralSelect, ContextKernels>(E, c, cv); }

}  // namespace zra_eng
