// zra_amd — context records (grep -A / -B / -C) over a stream of records whose selection bits are known: the algebra that does not
// depend on HOW a record got selected. A kernel set hands it, per trip of 64 positions, the delimiter ballot and the ballot of "the
// record this delimiter ends is selected"; zra_grep_context.hip is its first user, zra_grep_regex_context.hip (trips of compacted
// delimiters) its second; the where set can be the next. What the kernels of such a set run alike is zra_context_tile.h's.
//  (records) R_0 .. R_(n-1) with a selected set S; the output set is O = { k : some j in S has j - before <= k <= j + after }, a
//      group is a maximal run of consecutive indices of O. before, after <= kMaxContext.
//  (summary) Ctx describes a run of consecutive records AS IF no record outside the run were selected:
//      sel = |S|, out = |O|, groups; head = the unselected records in front of the first selected one, tail = those behind the last
//      one; without a selected record head == tail == the number of records. The two distances saturate at kSat = 2 * kMaxContext + 1:
//      a gap of g unselected records between two selected ones holds min(g, after + before) output records and fuses the two groups
//      iff g <= after + before, so a distance has to be exact up to after + before <= 128. (Saturating at kMaxContext + 1 is not
//      enough: tail 70 and head 30 with after == before == 64 make a gap of 100 <= 128, all of it output; 65 + 30 would say 95.)
//      append(A, B) is associative, the empty run {0, 0, 0, 0, 0} is its identity, single(s) is one record.
//  (forward) what a record needs from in front of it: Ctx of everything in front, of which {sel != 0, tail} decide whether it lies in
//      the after-context of the last selected record (tail < after).
//  (look) what a record needs from behind it, a Look word: bit 31 = a selected record follows, low bits = the unselected records in
//      front of it; without one, the records that follow at all (saturating). look_cat(A, B): run A in front of run B. A record is in
//      the before-context of the next selected one iff has && d < before. Without a selected record behind it the record is PENDING
//      when it is one of the stream's last `before` records outside every after-context: a later pass may still select a record.
//  (true count) the records of O in front of a point = out of the run in front + confirmed(run in front, look at the point): the
//      last min(uncovered tail, before - d) records of the run in front that only the next selected record brings in.
//  (pending) -B breaks "nothing is ever patched later": whether the stream's last records are output is known only when a later pass
//      selects a record, or never does. The carried state counts np <= before PENDING ranges, the stream's trailing records outside
//      every after-context, kept ascending in a scratch of `before` entries. pass_end(): a pass whose first selected record has d
//      unselected records of the pass in front keeps the last max(0, before - d) of them, moves those to the list behind the carried
//      out count and drops the rest; a pass without a selected record keeps the last max(0, before - its own uncovered records) and
//      moves them to the scratch's head; a pass that ends no record leaves them alone; the last pass drops what is pending. The pass's
//      own pending records go behind the kept ones, the one with dist records behind it to slot pendBase + npThis - 1 - dist:
//      np == min(uncovered tail of the stream, before) after every pass. tools/model/context_pass_check.cpp runs this on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZRA_CTX_FN __host__ __device__ __forceinline__
#else
#define ZRA_CTX_FN inline
#endif

namespace zra_ctx {
constexpr uint32_t kMaxContext = 64;               // ZRA_HIP_GREP_MAX_CONTEXT
constexpr uint32_t kSat = 2 * kMaxContext + 1;
constexpr uint32_t kLookHas = 1u << 31;

struct Ctx { uint64_t sel, out, groups; uint32_t head, tail; };

ZRA_CTX_FN uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
ZRA_CTX_FN uint32_t sat(uint32_t x) { return umin(x, kSat); }
ZRA_CTX_FN Ctx single(uint32_t selected) { return Ctx{selected, selected, selected, selected ^ 1u, selected ^ 1u}; }

// A followed by B
ZRA_CTX_FN void append(Ctx& A, const Ctx& B, uint32_t before, uint32_t after) {
  const uint32_t a = A.tail, b = B.head, g = a + b;
  if (B.sel == 0) {
    if (A.sel == 0) { A.head = A.tail = sat(g); return; }
    A.out += umin(g, after) - umin(a, after);
    A.tail = sat(g);
    return;
  }
  if (A.sel == 0) {
    A.sel = B.sel; A.groups = B.groups;
    A.out = B.out + umin(g, before) - umin(b, before);
    A.head = sat(g); A.tail = B.tail;
    return;
  }
  A.sel += B.sel;
  A.out += B.out + umin(g, after + before) - umin(a, after) - umin(b, before);
  A.groups += B.groups - (g <= after + before ? 1u : 0u);
  A.tail = B.tail;
}

// A followed by one record: append(A, single(selected)), written out
ZRA_CTX_FN void push(Ctx& A, uint32_t selected, uint32_t before, uint32_t after) {
  const uint32_t a = A.tail;
  if (!selected) {
    if (A.sel == 0) A.head = sat(a + 1); else A.out += a < after;
    A.tail = sat(a + 1);
    return;
  }
  if (A.sel == 0) { A.out = 1 + umin(a, before); A.groups = 1; }
  else { A.out += 1 + umin(a, after + before) - umin(a, after); A.groups += a > after + before; }
  A.sel += 1; A.tail = 0;
}

// the records at the run's tail that lie in no after-context
ZRA_CTX_FN uint32_t uncovered(bool any, uint32_t tail, uint32_t after) { return any ? tail - umin(tail, after) : tail; }
ZRA_CTX_FN uint32_t uncovered(const Ctx& c, uint32_t after) { return uncovered(c.sel != 0, c.tail, after); }

ZRA_CTX_FN uint32_t look(bool has, uint32_t d) { return (has ? kLookHas : 0u) | sat(d); }
ZRA_CTX_FN bool look_has(uint32_t l) { return (l & kLookHas) != 0; }
ZRA_CTX_FN uint32_t look_d(uint32_t l) { return l & ~kLookHas; }
ZRA_CTX_FN uint32_t look_cat(uint32_t a, uint32_t b) { return look_has(a) ? a : (b & kLookHas) | sat(look_d(a) + look_d(b)); }
// (true count) how many of the uncovered tail records in front the next selected record brings in
ZRA_CTX_FN uint32_t confirmed(uint32_t unc, uint32_t lk, uint32_t before) {
  return look_has(lk) && look_d(lk) < before ? umin(unc, before - look_d(lk)) : 0u;
}

// the (look) of a run of resolved records
ZRA_CTX_FN uint32_t ctx_look(const Ctx& c) { return look(c.sel != 0, c.head); }
// the (look) of a run with a delimiter whose first record is resolved: that record, then the run's others
ZRA_CTX_FN uint32_t resolved_look(uint32_t sel1, const Ctx& rest) { return sel1 ? look(true, 0) : look(rest.sel != 0, 1 + rest.head); }

// A Ctx in a per-tile summary word above the `low` bits the kernel set keeps for itself, `own`: a tile ends at most 8,192 records, so
// own | head << low (8 bits) | tail << low + 8 (8) | sel << low + 16 (14) | out << low + 30 (14) | groups << low + 44 (13)
ZRA_CTX_FN uint64_t ctx_pack(uint64_t own, const Ctx& c, uint32_t low) {
  return own | (uint64_t)c.head << low | (uint64_t)c.tail << (low + 8) | c.sel << (low + 16) | c.out << (low + 30) | c.groups << (low + 44);
}
ZRA_CTX_FN Ctx ctx_unpack(uint64_t w, uint32_t low) {
  Ctx c;
  c.head = (uint32_t)(w >> low) & 0xFF; c.tail = (uint32_t)(w >> (low + 8)) & 0xFF;
  c.sel = (w >> (low + 16)) & 0x3FFF; c.out = (w >> (low + 30)) & 0x3FFF; c.groups = w >> (low + 44);
  return c;
}

// (pending) the end of a pass. passLook: the look of the pass's records, the record open at hi included; outIn, npIn: the stream's
// out count and pending count carried into the pass; end: the Ctx at the pass's end. The old pending ranges [src, src + cnt) move to
// the list at `to` (toList) or to the scratch's head; the pass's own go behind pendBase, npThis of them; np is carried on.
struct PassEnd { uint32_t src, cnt, toList, pendBase, np, npThis; uint64_t to; };
ZRA_CTX_FN PassEnd pass_end(uint32_t passLook, uint64_t outIn, uint32_t npIn, const Ctx& end, bool lastPass, uint32_t before, uint32_t after) {
  const uint32_t d = look_d(passLook);
  const bool has = look_has(passLook);
  PassEnd e = {0, 0, has, npIn, 0, 0, outIn};
  // d unselected records of the pass lie in front of its first selected one (has), or are all it ended: in both cases they push
  // the older pending ranges out. (Without a selected record a carried after-context may cover some of the d, but then nothing is
  // pending: npIn != 0 says that the stream's tail has left every after-context.)
  if (has || d) { e.cnt = d < before ? umin(npIn, before - d) : 0; e.pendBase = has ? 0 : e.cnt; }
  e.src = npIn - e.cnt;
  e.np = lastPass ? 0 : umin(uncovered(end, after), before);
  if (!has && !d) e.np = npIn;                                  // (the pass ended no record)
  e.npThis = e.np > e.pendBase ? e.np - e.pendBase : 0;
  return e;
}

#if defined(__HIPCC__)
// ---- a trip of 64 positions. dm: the delimiters whose records are resolved, sm (a subset): the selected ones among them.
// What a wave carries through its trips to the (summary) of its resolved records: uniform words, and one per-lane sum, acc: every
// selected lane adds its own record and the gap in front of it (out | groups << 16), and ctx_close() adds the lanes up once. (A
// uniform loop over sm's bits for the trips with few selected records was measured and was slower: profiles/grep_context.md.)
struct CtxWalk { bool any; uint32_t run, head, sel, acc; };

__device__ __forceinline__ void ctx_trip(CtxWalk& w, uint64_t dm, uint64_t sm, uint32_t lane, uint32_t before, uint32_t after) {
  w.sel += (uint32_t)__popcll(sm);
  if (sm == 0) { w.run += (uint32_t)__popcll(dm); return; }
  const uint64_t below = (1ull << lane) - 1;
  const uint32_t fs = (uint32_t)__builtin_ctzll(sm), ls = 63 - (uint32_t)__builtin_clzll(sm), T = after + before;
  if ((sm >> lane) & 1) {
    const uint64_t sBelow = sm & below;
    if (sBelow) {
      const uint32_t g = (uint32_t)__popcll(dm & below & ~((2ull << (63 - (uint32_t)__builtin_clzll(sBelow))) - 1));
      w.acc += 1 + umin(g, T) + ((g > T) << 16);
    } else if (w.any) {
      const uint32_t g = w.run + (uint32_t)__popcll(dm & below);
      w.acc += 1 + umin(g, T) + ((g > T) << 16);
    } else w.acc += 1 + (1u << 16);
  }
  if (!w.any) { w.head = w.run + (uint32_t)__popcll(dm & ((1ull << fs) - 1)); w.any = true; }
  w.run = ls < 63 ? (uint32_t)__popcll(dm >> (ls + 1)) : 0;
}

__device__ __forceinline__ uint32_t ctx_wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// (a wave ends at most 2,048 records: out and groups fit 16 bits each)
__device__ __forceinline__ Ctx ctx_close(const CtxWalk& w, uint32_t before, uint32_t after) {
  const uint32_t acc = w.any ? ctx_wave_sum(w.acc) : 0;                       // (uniform)
  Ctx c;
  c.sel = w.sel; c.groups = acc >> 16;
  c.out = w.any ? (acc & 0xFFFF) + umin(w.head, before) + umin(w.run, after) : 0;
  c.head = sat(w.any ? w.head : w.run); c.tail = sat(w.run);
  return c;
}

// the look of a trip's records, for the walk backwards
__device__ __forceinline__ uint32_t ctx_trip_look(uint64_t dm, uint64_t sm) {
  return sm ? look(true, (uint32_t)__popcll(dm & ((1ull << __builtin_ctzll(sm)) - 1))) : look(false, (uint32_t)__popcll(dm));
}

// One lane's record (its bit of dm is set) among the trip's: any / tail = (forward) at the trip's head, lk = (look) at its end.
// *inO: the record is in O; *d: without a selected record behind it, the records behind it (for the pending test).
__device__ __forceinline__ void ctx_member(uint64_t dm, uint64_t sm, uint32_t lane, bool any, uint32_t tail, uint32_t lk, uint32_t before, uint32_t after,
                                           bool* inO, bool* has, uint32_t* d) {
  const uint64_t below = (1ull << lane) - 1, above = lane < 63 ? ~((2ull << lane) - 1) : 0;
  const uint64_t sBelow = sm & below, sAbove = sm & above;
  uint32_t a;
  if (sBelow) { any = true; a = (uint32_t)__popcll(dm & below & ~((2ull << (63 - (uint32_t)__builtin_clzll(sBelow))) - 1)); }
  else a = sat(tail + (uint32_t)__popcll(dm & below));
  uint32_t l;
  if (sAbove) l = look(true, (uint32_t)__popcll(dm & above & ((1ull << __builtin_ctzll(sAbove)) - 1)));
  else l = (lk & kLookHas) | sat(look_d(lk) + (uint32_t)__popcll(dm & above));
  *has = look_has(l); *d = look_d(l);
  *inO = ((sm >> lane) & 1) || (any && a < after) || (*has && *d < before);
}
#endif
}  // namespace zra_ctx
