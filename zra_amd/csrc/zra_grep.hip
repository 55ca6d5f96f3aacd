// zra_amd — grep of a device-resident archive (zra_hip.h: ZraHipGrepArchive): the records of a content range, cut at a delimiter byte,
// that hold a match of one of up to 64 byte patterns (or, inverted, none), as ascending {offset, size} pairs, without an output buffer
// for the content. What `grep -F -f patterns -b` (and `-v`, `-c`) is to `zstdgrep`: the lines, not the offsets of the hits.
//
// The passes, the staging window and the conditions (contiguity), (carry), (ownership) with trim = 0 and (d) are those of the range scans'
// one driver (zra_scan.h); (filter), the pattern table, the test of one position and a position's two flags are zra_patterns.h's, shared
// with zra_msearch.hip and zra_extract.hip. This call's own:
//  (stream) the positions of [lo, hi) form one ascending stream, a pass owns the positions the multi search gives it, and a position
//      carries two flags that are both evaluated by its owner: `delimiter` (its byte, read from the carry area as often as from a slot)
//      and `hit` (a match starts here: position_mask != 0). No pattern holds the delimiter, so the two exclude each other and an
//      occurrence lies inside one record.
//  (forward) a record belongs to the delimiter that ENDS it, the last one to hi. What a delimiter needs from in front of it is the
//      position behind the previous delimiter and the OR of the hit flags since then. Nothing is ever patched later: what crosses a
//      trip, a wave, a tile or a pass is the pair (start of the open record, has it matched yet).
//  (summary) a run of positions (a trip's 64, a wave's 2,048, a tile, a lane's run of tiles in the scan) reduces to
//      {has a delimiter, hit in front of the first one, hit behind the last one, position behind the last one, records selected among
//      those that end inside it APART from the first}. Without a delimiter the two hit bits are both "a hit anywhere". Two runs
//      combine associatively (combine() below): the record that the second run's first delimiter ends is selected by
//      (hit behind A's last | hit in front of B's first) ^ invert and joins the sum.
//  (launches) zra_grep_count_kernel: per tile its summary, per call the order-independent totals (matches, delimiters) as atomics.
//      zra_grep_scan_kernel, ONE workgroup: the summaries become per tile {list base, start of the record open at the tile's head, its
//      hit bit}, and the state carried between passes {open record's start, its hit bit, records selected so far} moves on from word
//      k & 1 to word (k + 1) & 1 of a ping-pong pair, the search's condition (c). The last pass's scan ends the open record at hi.
//      zra_grep_fill_kernel: the workgroups redo the tiles that hold a listed record and write the pairs.
//  (order) a list position is a prefix count (the state's count, plus the tiles in front, plus the waves in front, plus the wave's
//      earlier trips, plus the selected lanes below), never the result of an atomic. No workgroup waits for another one: no spin-wait,
//      no look-back; the dependency runs through the launches.
//  (d) nothing goes to the caller's array before the last pass is done: a call that fails midway writes nothing.
#include "zra_record_scan.h"

namespace {
// (summary). flags: 1 a delimiter, 2 a hit in front of the first delimiter, 4 a hit behind the last; last: the content offset behind
// the last delimiter
struct __attribute__((aligned(16))) Sum { u64 last; u32 sel, flags; };
// what the scan makes of it for the fill: the list position of the tile's first record, the start of the record open at its head with
// that record's hit bit in bit 63
struct __attribute__((aligned(16))) Head { u64 base, open; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi
struct State { u64 start, hit, sel, tail; };
// The words the launches of a call add up, uploaded with the table: the ping-pong state (c), then the atomics.
struct Totals { State st[2]; u64 matches, delims, pad[6]; };

// the summary of run A followed by run B. sel is kept wide by the scan: selA + selB + the record B's first delimiter ends
__device__ __forceinline__ void combine(u32& fA, u64& selA, u64& lastA, u32 fB, u64 selB, u64 lastB, u32 inv) {
  if (!(fB & 1)) { if (fB & 2) fA |= (fA & 1) ? 4u : 6u; return; }
  if (!(fA & 1)) { fA = 1 | ((fA | fB) & 2) | (fB & 4); selA = selB; lastA = lastB; return; }
  selA += selB + ((((fA >> 2) | (fB >> 1)) & 1) ^ inv);
  fA = 1 | (fA & 2) | (fB & 4); lastA = lastB;
}

// A wave's walk over its trips. Count: seen = false, and the record that the wave's first delimiter ends is left to whoever combines
// the summaries (hitFirst says whether it matched inside the wave). Fill: seen = true, hit and start come from in front of the wave.
struct Walk { bool seen, hit, hitFirst; u32 sel; u64 start; };

// One trip: dm / hm = the ballots of the two flags, pos = the content offset of lane 0's position. kEmit: the selected records that
// end in the trip go to list[at + ...] while there is room; at moves on.
template <bool kEmit>
__device__ __forceinline__ void walk_trip(Walk& s, u64 dm, u64 hm, u32 lane, u32 inv, u64 pos, u64& at, Range* list, u64 cap) {
  if (dm == 0) { s.hit |= hm != 0; return; }                                 // (uniform in the wave)
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;           // the delimiter in front of this lane, inside the trip
  const u64 seg = dBelow ? hm & below & ~((2ull << prev) - 1) : hm & below;  // the hits between it (or the trip's head) and this lane
  const bool hit = seg != 0 || (!dBelow && s.hit);
  const bool sel = ((dm >> lane) & 1) && (hit != (bool)inv) && (s.seen || lane != first);
  const u64 sm = __ballot(sel);
  if (kEmit) {
    const u64 idx = at + (u32)__popcll(sm & below);
    if (sel && idx < cap) {
      const u64 start = dBelow ? pos + prev + 1 : s.start;
      Range r; r.offset = start; r.size = pos + lane - start;
      list[idx] = r;
    }
    at += (u32)__popcll(sm);
  }
  s.sel += (u32)__popcll(sm);
  if (!s.seen) { s.hitFirst = s.hit || (hm & ((1ull << first) - 1)) != 0; s.seen = true; }
  s.hit = last < 63 && (hm >> (last + 1)) != 0;
  s.start = pos + last + 1;
}

__device__ __forceinline__ Sum walk_sum(const Walk& s) {
  Sum r;
  r.last = s.start; r.sel = s.sel;
  r.flags = s.seen ? 1u | (s.hitFirst ? 2u : 0u) | (s.hit ? 4u : 0u) : (s.hit ? 6u : 0u);
  return r;
}
}  // namespace

// The run of a pass as the multi search sees it: win = slot 0, position x is the byte win[x]; the positions of the pass are xLo + [0,
// nPos), xHi is the position of the range's end (hi - passBase), M the longest pattern, p0 the content offset of position xLo.
// Workgroup g takes the tiles [g * kGroup, (g + 1) * kGroup): per tile its summary -> sums[tile]; per call the totals.
template <class TB>
__device__ __forceinline__ void grep_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim,
                                                                        u32 inv, u64 p0, Sum* sums, Totals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ Sum sW[4];
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
    Walk s = {false, false, false, 0, p0 + t0 + w0};
    u64 at = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      trip_flags(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      delims += (u32)__popcll(dm);
      walk_trip<false>(s, dm, hm, lane, inv, p0 + t0 + w0 + t * 64, at, nullptr, 0);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (tid == 0) {
      u32 f = sW[0].flags; u64 sel = sW[0].sel, last = sW[0].last;
      for (u32 w = 1; w < 4; w++) combine(f, sel, last, sW[w].flags, sW[w].sel, sW[w].last, inv);
      Sum r; r.last = last; r.sel = (u32)sel; r.flags = f;
      sums[b] = r;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
extern "C" __global__ void __launch_bounds__(256) zra_grep_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                        u32 inv, u64 p0, Sum* sums, Totals* tot) {
  grep_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_grep_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                        u32 inv, u64 p0, Sum* sums, Totals* tot) {
  grep_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, tot);
}

// One workgroup: (launches). Every lane reduces a run of consecutive tiles, the 1024 summaries are scanned in LDS (Hillis-Steele over
// combine()), then the lane walks its run again from the state in front of it: heads[t], and sums[t].sel becomes ALL the selected
// records that end in tile t, the first included (what the fill skips a tile by). lastPass: the record open at hi ends there.
extern "C" __global__ void __launch_bounds__(1024) zra_grep_scan_kernel(Sum* sums, u32 nTiles, Head* heads, const State* in, State* out, u32 inv, u32 lastPass, u64 hi,
                                                                        Range* list, u64 cap) {
  __shared__ u64 sSel[1024], sLast[1024];
  __shared__ u32 sF[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  u32 f = 0; u64 sel = 0, last = 0;
  for (u32 t = b0; t < b1; t++) { const Sum s = sums[t]; combine(f, sel, last, s.flags, s.sel, s.last, inv); }
  sF[tid] = f; sSel[tid] = sel; sLast[tid] = last;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    u32 fa = 0; u64 sa = 0, la = 0;
    if (tid >= d) { fa = sF[tid - d]; sa = sSel[tid - d]; la = sLast[tid - d]; }
    __syncthreads();
    if (tid >= d) { combine(fa, sa, la, f, sel, last, inv); f = fa; sel = sa; last = la; sF[tid] = f; sSel[tid] = sel; sLast[tid] = last; }
    __syncthreads();
  }
  // the state in front of this lane's run: the carried one, then the lanes in front
  u64 start = in->start, count = in->sel;
  bool hit = in->hit != 0;
  if (tid) {
    const u32 fe = sF[tid - 1];
    if (fe & 1) { count += sSel[tid - 1] + ((u32)(hit || (fe & 2)) ^ inv); hit = (fe & 4) != 0; start = sLast[tid - 1]; }
    else hit |= (fe & 2) != 0;
  }
  for (u32 t = b0; t < b1; t++) {
    const Sum s = sums[t];
    Head h; h.base = count; h.open = start | (hit ? kHitBit : 0);
    heads[t] = h;
    if (s.flags & 1) {
      const u32 all = s.sel + ((u32)(hit || (s.flags & 2)) ^ inv);
      sums[t].sel = all;
      count += all; hit = (s.flags & 4) != 0; start = s.last;
    } else hit |= (s.flags & 2) != 0;
  }
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tail = 0;
    if (lastPass && start < hi) {
      tail = 1;
      if ((u32)hit != inv) {
        if (count < cap) { Range r; r.offset = start; r.size = hi - start; list[count] = r; }
        count++;
      }
    }
    State o; o.start = start; o.hit = hit; o.sel = count; o.tail = tail;
    *out = o;
  }
}

// The count's workgroups redo the tiles that hold a listed record (a tile without a selected record, or behind the list's capacity, is
// skipped; a workgroup without such a tile leaves at once): the ballots of every trip go to LDS with the waves' summaries, a wave takes
// what lies in front of it from the tile's head and the waves in front, and walks its trips again, writing.
template <class TB>
__device__ __forceinline__ void grep_fill(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim,
                                                                       u32 inv, u64 p0, const Sum* sums, const Head* heads, Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ Sum sW[4];
  __shared__ u64 sMask[4][kWaveIters][2];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  bool any = false;                                                          // (uniform in the workgroup, like `listed` below)
  for (u32 b = bBegin; b < bEnd; b++) any |= sums[b].sel != 0 && heads[b].base < cap;
  if (!any) return;
  stage_table(tbl, &sT);
  for (u32 b = bBegin; b < bEnd; b++) {
    const Head head = heads[b];
    const bool listed = sums[b].sel != 0 && head.base < cap;
    if (!listed) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    Walk s = {false, false, false, 0, p0 + t0 + w0};
    u64 at = 0;
    u32 pairs = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      trip_flags(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      if (lane == 0) { sMask[wave][t][0] = dm; sMask[wave][t][1] = hm; }
      walk_trip<false>(s, dm, hm, lane, inv, p0 + t0 + w0 + t * 64, at, nullptr, 0);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (!(sW[wave].flags & 1)) continue;                                     // (uniform in the wave; the barriers are at the loop's head)
    Walk e = {true, (head.open & kHitBit) != 0, false, 0, head.open & ~kHitBit};
    at = head.base;
    for (u32 w = 0; w < wave; w++) {
      const Sum v = sW[w];
      if (v.flags & 1) { at += v.sel + ((u32)(e.hit || (v.flags & 2)) ^ inv); e.hit = (v.flags & 4) != 0; e.start = v.last; }
      else e.hit |= (v.flags & 2) != 0;
    }
    if (at >= cap) continue;
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++)
      walk_trip<true>(e, sMask[wave][t][0], sMask[wave][t][1], lane, inv, p0 + t0 + w0 + t * 64, at, list, cap);
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_grep_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                       u32 inv, u64 p0, const Sum* sums, const Head* heads, Range* list, u64 cap) {
  grep_fill<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, heads, list, cap);
}
extern "C" __global__ void __launch_bounds__(256) zra_grep_fill_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                       u32 inv, u64 p0, const Sum* sums, const Head* heads, Range* list, u64 cap) {
  grep_fill<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, heads, list, cap);
}

// =================================================================================================
// The kernel set of the plain grep for zra_record_scan.h's call path. tables: Table | Totals | sums[tiles] | heads[tiles]
namespace {
struct GrepKernels {
  using Sum = ::Sum; using Head = ::Head; using Totals = ::Totals;
  static constexpr size_t kMapBytes = 0;
  static constexpr bool kData = false;
  static void launch(hipStream_t s, const LiteralSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<GrepKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, inv = sel.inv, M = sel.M;
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_grep_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, (u64)ps.p0, p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_grep_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, (u64)ps.p0, p.sums, p.tot);
    hipLaunchKernelGGL(zra_grep_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), inv, (u32)ps.lastPass,
                       (u64)p.hi, p.list, (u64)p.listCap);
    if (p.listCap && sel.pset.classes)
      hipLaunchKernelGGL(zra_grep_fill_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, (u64)ps.p0, p.sums, p.heads,
                         p.list, (u64)p.listCap);
    else if (p.listCap)
      hipLaunchKernelGGL(zra_grep_fill_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, (u64)ps.p0, p.sums, p.heads, p.list,
                         (u64)p.listCap);
  }
};
}  // namespace

namespace zra_eng {

Status ScanImpl::grep(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<LiteralSelect, GrepKernels>(E, c, cv); }

}  // namespace zra_eng
