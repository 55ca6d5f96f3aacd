// zra_amd — what the kernel sets of the two greps with context records run alike once a record's selection bit is known
// (zra_grep_context.hip: zra_grepc_*; zra_grep_regex_context.hip: zra_grepxc_*): the carried state and the per-tile
// head, the end of the one-workgroup scan kernel behind its forward walk (context_scan_tail), and the fill's pieces that do not depend
// on where a trip's ballots come from. The algebra, (look), (true count) and (pending) are described in zra_context.h; how a trip's
// dm / sm and a record's offset come about stays with each set. Device code: included by those two translation units only.
#pragma once
#include "zra_scan_tile.h"
#include "zra_context.h"

namespace {
using zra_ctx::Ctx;
constexpr u64 kSelectedBit = 1ull << 63;   // ZRA_HIP_CONTEXT_SELECTED

// per tile for the fill: base = the (true count) in front of the tile, pend of which are confirmed records of the uncovered tail in
// front; open = the start of the record open at the tile's first position (the literal set: its hit bit beside it); fwd = {bit 31: a
// selected record in front, tail}; la = the (look) at the tile's end; cnt = the tile's records in O
struct __attribute__((aligned(16))) CHead { u64 base, open; u32 fwd, la, cnt, pend; };
// the carried state: the plain call's four words (state = the selector's own datum of the open record, the hit bit or the DFA state;
// sel = |O| so far), the Ctx of the stream so far, the pending count, and for the fill of the pass that wrote it where its own
// pending records go
struct CtxState { u64 start, state, sel, tail; Ctx c; u32 np, pendBase, npThis, pad; };
struct CtxTotals { CtxState st[2]; u64 matches, delims; };
static_assert(sizeof(CHead) == 32 && sizeof(CtxTotals) == 176, "the entries as the kernels index them");

// The end of the scan kernel, 1,024 lanes, behind the lane's forward walk over its tiles [b0, b1), which left in heads[t] what lies
// in front of tile t and in la the tile's own look. C / start / state: the front behind the lane's run (the last lane's is the
// pass's end); runLook: the look of the run's records; tailRec / tailSel: a record is open at hi in the last pass, and selected. The
// lanes' looks are scanned backwards (Hillis-Steele over look_cat), the lane walks its run backwards: heads[t].la becomes the look at
// the tile's end, base the (true count) in front of it, pend and cnt. The last lane ends the record open at hi, decides (pending)
// and writes the carried state; a wave moves the pending ranges. pend = list + cap. The lane's own values come by reference and
// are used up (C and runLook are changed); the uniform ones by value. (By value the forward walk of the regex kernel in front of
// the call was compiled with eleven more register moves a trip, and measured 2 % slower: profiles/context_tile.md.)
template <class Head, class St>
__device__ __forceinline__ void context_scan_tail(Ctx& C, const u64& start, const St& state, u32& runLook, const bool& tailRec, const bool& tailSel, u32 b0, u32 b1,
                                                  Head* heads, const CtxState* in, CtxState* out, Range* list, u64 cap, u64 hi, u32 lastPass, u32 before, u32 after) {
  __shared__ u32 sLook[1024];
  __shared__ u32 sMove[4];                                                   // {source in pend, count, to the list?, 0}
  __shared__ u64 sMoveTo;
  const u32 tid = threadIdx.x;
  u32 tailLook = zra_ctx::look(false, 0);                                     // the look behind the last tile
  if (tid == 1023) {
    if (tailRec) tailLook = tailSel ? zra_ctx::look(true, 0) : zra_ctx::look(false, 1);
    runLook = zra_ctx::look_cat(runLook, tailLook);
  }
  sLook[tid] = runLook;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    u32 b = 0;
    const bool on = tid + d < 1024;
    if (on) b = sLook[tid + d];
    __syncthreads();
    if (on) { runLook = zra_ctx::look_cat(runLook, b); sLook[tid] = runLook; }
    __syncthreads();
  }
  // backwards: the look behind this lane's run, then tile by tile
  u32 la = tid < 1023 ? sLook[tid + 1] : tailLook;
  u64 nextBase = C.out + zra_ctx::confirmed(zra_ctx::uncovered(C, after), la, before);
  for (u32 t = b1; t-- > b0;) {
    Head h = heads[t];
    const u32 own = h.la;
    h.la = la;
    la = zra_ctx::look_cat(own, la);
    h.pend = zra_ctx::confirmed(h.pend, la, before);
    h.base += h.pend;
    h.cnt = (u32)(nextBase - h.base);
    nextBase = h.base;
    heads[t] = h;
  }
  if (tid == 1023) {
    const u32 passLook = sLook[0];                                           // the whole pass, the record open at hi included
    u64 tail = 0;
    if (tailRec) {
      tail = 1;
      const u64 at = C.out + (tailSel ? min(zra_ctx::uncovered(C, after), before) : 0u);
      if ((tailSel || (C.sel && C.tail < after)) && at < cap) { Range q; q.offset = start; q.size = (hi - start) | (tailSel ? kSelectedBit : 0); list[at] = q; }
      zra_ctx::push(C, tailSel, before, after);
    }
    const zra_ctx::PassEnd e = zra_ctx::pass_end(passLook, in->c.out, in->np, C, lastPass != 0, before, after);
    sMove[0] = e.src; sMove[1] = e.cnt; sMove[2] = e.toList; sMove[3] = 0;
    sMoveTo = e.to;
    CtxState o;
    o.start = start; o.state = state; o.sel = C.out; o.tail = tail; o.c = C;
    o.np = e.np; o.pendBase = e.pendBase; o.npThis = e.npThis; o.pad = 0;
    *out = o;
  }
  __syncthreads();
  // (pending) at most 64 entries, one wave's job; source and destination may overlap inside pend
  const u32 cnt = sMove[1];
  Range q; q.offset = 0; q.size = 0;
  Range* const pend = list + cap;
  if (tid < cnt && sMove[0] + tid < before) q = pend[sMove[0] + tid];
  __syncthreads();
  if (tid < cnt && sMove[0] + tid < before) {
    if (sMove[2]) { if (sMoveTo + tid < cap) list[sMoveTo + tid] = q; }
    else pend[tid] = q;
  }
}

// ---- the fill. Is tile b redone: it holds a record of O in front of the capacity, or a pending one (bit 0 of a summary's w: a record
// ends in the tile). Uniform in the workgroup; the second half's loads wait for the first half's answer.
template <class Head, class Sum>
__device__ __forceinline__ bool context_wanted(const Head* heads, const Sum* sums, u32 b, u32 npThis, u64 cap) {
  const Head h = heads[b];
  return (h.cnt != 0 && h.base < cap) || (npThis != 0 && (sums[b].w & 1) && !zra_ctx::look_has(h.la) && zra_ctx::look_d(h.la) < npThis);
}
// the (forward) Ctx in front of a tile, as far as the fill needs it: {a selected record in front, out, tail}
__device__ __forceinline__ Ctx context_front(const CHead& h) {
  return Ctx{(h.fwd & zra_ctx::kLookHas) ? 1u : 0u, h.base - h.pend, 0, 0, h.fwd & ~zra_ctx::kLookHas};
}
// Lane t of keep holds trip t's own look, la is the look behind the wave's last trip: backwards, lane t of keep becomes the look at
// trip t's end. Returns the look at the wave's head.
__device__ __forceinline__ u32 context_looks_back(u32& keep, u32 la, u32 trips, u32 lane) {
#pragma unroll 1
  for (u32 t = trips; t-- > 0;) {
    const u32 tl = (u32)__shfl((int)keep, (int)t, 64);
    if (lane == t) keep = la;
    la = zra_ctx::look_cat(tl, la);
  }
  return la;
}
// One writing trip: the lanes of dm hold a record each, q its range, sm the selected ones, lk the look at the trip's end; at = the
// (true count) and fAny / fTail = (forward) in front of the trip, moved behind it. A member of O goes to the list at the prefix
// count, never an atomic; a pending record to its slot, (pending).
__device__ __forceinline__ void context_write_trip(u64 dm, u64 sm, u32 lane, Range q, u32 lk, u64& at, bool& fAny, u32& fTail, Range* list, u64 cap, u32 pendBase,
                                                   u32 npThis, u32 before, u32 after) {
  bool inO = false, has = false;
  u32 dist = 0;
  const bool isD = (dm >> lane) & 1;
  if (isD) zra_ctx::ctx_member(dm, sm, lane, fAny, fTail, lk, before, after, &inO, &has, &dist);
  const u64 om = __ballot(inO);
  if ((sm >> lane) & 1) q.size |= kSelectedBit;
  if (inO) {
    const u64 idx = at + (u32)__popcll(om & ((1ull << lane) - 1));
    if (idx < cap) list[idx] = q;
  } else if (isD && !has && dist < npThis) {
    const u32 slot = pendBase + npThis - 1 - dist;
    if (slot < before) (list + cap)[slot] = q;
  }
  at += (u32)__popcll(om);
  if (sm) { fAny = true; const u32 ls = 63 - (u32)__builtin_clzll(sm); fTail = ls < 63 ? (u32)__popcll(dm >> (ls + 1)) : 0; }
  else fTail = zra_ctx::sat(fTail + (u32)__popcll(dm));
}
}  // namespace
