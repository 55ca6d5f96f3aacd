// zra_amd — extract of a device-resident archive (zra_hip.h: ZraHipExtractRecords): the grep's selected records (zra_grep.hip) WITH
// their bytes, packed into a device buffer in ascending order, each followed by the delimiter: the text `grep -F -f patterns` (and `-v`)
// prints, from the one decode pass that selects the records.
//
// The passes, the staging window and the conditions (contiguity), (carry), (ownership) with trim = 0 and (d) are those of the range scans'
// one driver (zra_scan.h); the pattern table, the test of one position and a position's two flags are zra_patterns.h's; the records, the
// selection, (stream), (forward) and (order) are the grep's (zra_grep.hip), word for word. This call's own:
//  (compaction) a position q of [lo, hi) belongs to the record it lies in, a delimiter to the record it ends. The packed text is the
//      stream compaction of the positions whose record is selected: the byte of q goes to dData[d + (q - s)], s = its record's start,
//      d = the packed bytes of the selected records in front of that record, and the delimiter at t is the same formula with q = t. The
//      lane that evaluates q's two flags stores q's byte, from the tile it staged. No lane loops over a record's bytes and no atomic
//      decides an address: d is a prefix sum, carried exactly as the grep carries a list position.
//  (summary) the grep's, plus {position of the first delimiter, packed bytes of the selected records that end inside the run APART
//      from the first}. combine() stays associative: the joined record adds B.first - A.last + 1 bytes when it is selected.
//  (look-ahead) a position behind its tile's last delimiter is selected by a delimiter further on. Inside a tile the fill sees it (the
//      ballots of all trips lie in LDS before a byte moves). Across tiles the one-workgroup scan, which knows for every tile whether
//      the record its first delimiter ends is selected, hands that bit back to the tiles in front: a reverse "nearest following tile
//      with a delimiter" over its lanes and their runs. Per tile: one bit, "the record open at my tail is copied".
//  (provisional tail) the look-ahead cannot cross a pass. In every pass but the last the record open at the end of the pass's owned
//      positions is copied at the current packed offset D, which moves only when a selected record ends. If that record turns out
//      selected its earlier part is in place and the next pass appends at the same D; if not, the next selected record overwrites it
//      (a later launch on the same stream) or it lies behind *dataSize. Real bytes of a pass lie in front of D, provisional ones at and
//      behind it. The last pass is exact: its open record ends at hi, and the scan stores that record's delimiter.
//  (stores) every store to dData is clamped to [0, dataCapacity), so the sizing call and a short buffer run the same code.
//  (launches) zra_extract_count_kernel, zra_extract_scan_kernel (ONE workgroup), zra_extract_copy_kernel: the grep's three, the third
//      redoing the tiles that hold a copied byte or a listed record.
#include "zra_record_scan.h"
#include "zra_extract_tail.h"

namespace {
// (summary). flags: 1 a delimiter, 2 a hit in front of the first delimiter, 4 a hit behind the last, 8 (set by the scan) the record
// the first delimiter ends is selected; first: the content offset of the first delimiter, last: the one behind the last delimiter
struct __attribute__((aligned(16))) XSum { u64 first, last, bytes; u32 sel, flags; };
// what the scan makes of it for the copy: the list position of the tile's first record, the start of the record open at its head with
// that record's hit bit in bit 63, the packed bytes in front of that record, and (look-ahead)'s bit
struct __attribute__((aligned(16))) XHead { u64 base, open, at, look; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi; bytes: packed so far (provisional tail)'s D
struct XState { u64 start, hit, sel, tail, bytes, pad[3]; };
struct XTotals { XState st[2]; u64 matches, delims, pad[6]; };

// a summary in registers; sel and bytes are kept wide by the scan
struct Run { u32 f; u64 first, last, sel, bytes; };

// the summary of run A followed by run B
__device__ __forceinline__ void combine(Run& a, const Run& b, u32 inv) {
  if (!(b.f & 1)) { if (b.f & 2) a.f |= (a.f & 1) ? 4u : 6u; return; }
  if (!(a.f & 1)) { a.f = 1 | ((a.f | b.f) & 2) | (b.f & 4); a.first = b.first; a.last = b.last; a.sel = b.sel; a.bytes = b.bytes; return; }
  const u32 s = (((a.f >> 2) | (b.f >> 1)) & 1) ^ inv;                       // the record B's first delimiter ends began in A
  a.sel += b.sel + s;
  a.bytes += b.bytes + (s ? b.first - a.last + 1 : 0);
  a.f = 1 | (a.f & 2) | (b.f & 4); a.last = b.last;
}

// what lies in front of a run, moved over the run: the open record's start and hit bit, the list position, the packed offset
struct Front { u64 start, idx, at; bool hit; };
__device__ __forceinline__ void advance(Front& e, u32 f, u64 first, u64 last, u64 sel, u64 bytes, u32 inv) {
  if (!(f & 1)) { e.hit |= (f & 2) != 0; return; }
  const u32 s = (u32)(e.hit || (f & 2)) ^ inv;
  e.idx += sel + s;
  e.at += bytes + (s ? first - e.start + 1 : 0);
  e.hit = (f & 4) != 0; e.start = last;
}

// The summary of one trip from its ballots; pos = the content offset of lane 0's position. A delimiter lane other than the first looks
// at the hit bits between the delimiter in front of it and itself; its record is at most 63 bytes and its delimiter.
__device__ __forceinline__ Run trip_run(u64 dm, u64 hm, u32 lane, u32 inv, u64 pos) {
  Run r = {0, 0, 0, 0, 0};
  if (dm == 0) { r.f = hm ? 6u : 0u; return r; }                             // (uniform in the wave)
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  bool sel = false;
  u32 size = 0;
  if (((dm >> lane) & 1) && dBelow) {
    const u32 prev = 63 - (u32)__builtin_clzll(dBelow);
    sel = ((hm & below & ~((2ull << prev) - 1)) != 0) != (bool)inv;
    size = lane - prev;
  }
  const u64 sm = __ballot(sel);
  r.f = 1u | ((hm & ((1ull << first) - 1)) ? 2u : 0u) | ((last < 63 && (hm >> (last + 1))) ? 4u : 0u);
  r.first = pos + first; r.last = pos + last + 1;
  r.sel = (u32)__popcll(sm);
  if (sm) r.bytes = wave_sum(sel ? size : 0);
  return r;
}

// One tile's first walk, the same in the count and in the copy: per trip the two ballots (kept in sMask when kKeep), per wave its
// summary -> sW[wave]. Returns the delimiters the wave saw.
template <bool kKeep, class TB>
__device__ __forceinline__ u32 tile_runs(const TB* sT, const u32* sTile, u32 d, u32 n, long long toHi, u32 delim, u32 inv, u64 tilePos, Run* sW,
                                         u64 (*sMask)[kWaveIters][2], u32* pairs) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w0 = wave * kWavePos;
  Run w = {0, 0, 0, 0, 0};
  u32 delims = 0;
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    u64 dm, hm;
    trip_flags(sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, pairs);
    if (kKeep && lane == 0) { sMask[wave][t][0] = dm; sMask[wave][t][1] = hm; }
    delims += (u32)__popcll(dm);
    combine(w, trip_run(dm, hm, lane, inv, tilePos + w0 + t * 64), inv);
  }
  if (lane == 0) sW[wave] = w;
  return delims;
}
}  // namespace

// The run of a pass as the grep sees it: win = slot 0, position x is the byte win[x]; the positions of the pass are xLo + [0, nPos), xHi
// is the position of the range's end (hi - passBase), M the longest pattern, p0 the content offset of position xLo. Workgroup g takes
// the tiles [g * kGroup, (g + 1) * kGroup): per tile its summary -> sums[tile]; per call the totals.
template <class TB>
__device__ __forceinline__ void extract_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim,
                                                                           u32 inv, u64 p0, XSum* sums, XTotals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ Run sW[4];
  const u32 tid = threadIdx.x, lane = tid & 63;
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
    delims += tile_runs<false>(&sT, sTile, d, n, toHi, delim, inv, p0 + t0, sW, nullptr, &pairs);
    __syncthreads();
    if (tid == 0) {
      Run r = sW[0];
      for (u32 w = 1; w < 4; w++) combine(r, sW[w], inv);
      XSum o; o.first = r.first; o.last = r.last; o.bytes = r.bytes; o.sel = (u32)r.sel; o.flags = r.f;
      sums[b] = o;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
extern "C" __global__ void __launch_bounds__(256) zra_extract_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                           u32 inv, u64 p0, XSum* sums, XTotals* tot) {
  extract_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_extract_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                           u32 inv, u64 p0, XSum* sums, XTotals* tot) {
  extract_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, tot);
}

// One workgroup. Forward, as the grep's scan: every lane reduces a run of consecutive tiles, the 1,024 summaries are scanned in LDS
// (Hillis-Steele over combine()), then the lane walks its run again from what lies in front of it: heads[t], sums[t].sel becomes ALL
// the selected records that end in tile t, and flag 8 says whether the first of them is one. The last lane ends the pass: the state
// moves on, and in the last pass the record open at hi ends there (its list entry and its delimiter byte). Backward, (look-ahead):
// the bit of the nearest following tile with a delimiter, or of the pass's end, reaches every tile's head.
extern "C" __global__ void __launch_bounds__(1024) zra_extract_scan_kernel(XSum* sums, u32 nTiles, XHead* heads, const XState* in, XState* out, u32 inv, u32 lastPass,
                                                                           u64 hi, u64 p0, u64 nPos, Range* list, u64 cap, u8* dData, u64 dataCap, u32 delim) {
  __shared__ u64 sFirst[1024], sLast[1024], sSel[1024], sBytes[1024];
  __shared__ u32 sF[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  Run r = {0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) { const XSum s = sums[t]; const Run b = {s.flags, s.first, s.last, s.sel, s.bytes}; combine(r, b, inv); }
  sF[tid] = r.f; sFirst[tid] = r.first; sLast[tid] = r.last; sSel[tid] = r.sel; sBytes[tid] = r.bytes;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    Run a = {0, 0, 0, 0, 0};
    if (tid >= d) { a.f = sF[tid - d]; a.first = sFirst[tid - d]; a.last = sLast[tid - d]; a.sel = sSel[tid - d]; a.bytes = sBytes[tid - d]; }
    __syncthreads();
    if (tid >= d) { combine(a, r, inv); r = a; sF[tid] = r.f; sFirst[tid] = r.first; sLast[tid] = r.last; sSel[tid] = r.sel; sBytes[tid] = r.bytes; }
    __syncthreads();
  }
  // what lies in front of this lane's run: the carried state, then the lanes in front
  Front e = {in->start, in->sel, in->bytes, in->hit != 0};
  if (tid) advance(e, sF[tid - 1], sFirst[tid - 1], sLast[tid - 1], sSel[tid - 1], sBytes[tid - 1], inv);
  u32 look = 0;                                                              // 2: the run has a delimiter, 1: the record its first one ends is selected
  for (u32 t = b0; t < b1; t++) {
    const XSum s = sums[t];
    XHead h; h.base = e.idx; h.open = e.start | (e.hit ? kHitBit : 0); h.at = e.at; h.look = 0;
    heads[t] = h;
    if (s.flags & 1) {
      const u32 fs = (u32)(e.hit || (s.flags & 2)) ^ inv;
      sums[t].sel = s.sel + fs;
      sums[t].flags = s.flags | (fs ? 8u : 0u);
      if (!look) look = 2 | fs;
    }
    advance(e, s.flags, s.first, s.last, s.sel, s.bytes, inv);
  }
  u32 tailSel = 0;
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tail;
    tailSel = extract_pass_end(lastPass, (u32)e.hit != inv, e.start, hi, e.idx, e.at, tail, list, cap, dData, dataCap, delim);
    XState o; o.start = e.start; o.hit = e.hit; o.sel = e.idx; o.tail = tail; o.bytes = e.at; o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *out = o;
  }
  look_ahead(look, tailSel, b0, b1, p0, nPos, heads, [&](u32 t) { const XSum s = sums[t]; return LookTile{(s.flags & 1) != 0, (s.flags >> 3) & 1, s.last}; });
}

// The count's workgroups redo the tiles that hold a byte of a selected record or a listed record in front of the capacities (the
// others are skipped; a workgroup without such a tile leaves at once). First walk: the ballots of every trip go to LDS with the waves'
// summaries. Second walk: a wave takes what lies in front of it from the tile's head and the waves in front, what lies behind it from
// the waves behind and the head's look-ahead bit, and every lane stores its position's byte where (compaction) puts it.
template <class TB>
__device__ __forceinline__ void extract_copy(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim,
                                                                          u32 inv, u64 p0, const XSum* sums, const XHead* heads, Range* list, u64 cap, u8* dData,
                                                                          u64 dataCap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ Run sW[4];
  __shared__ u64 sMask[4][kWaveIters][2];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  // a tile's bytes go to head.at and behind, its list entries to head.base and behind (uniform in the workgroup)
  auto wanted = [&](u32 b) {
    const u32 sel = sums[b].sel;
    const XHead h = heads[b];
    return ((sel != 0 || h.look != 0) && h.at < dataCap) || (sel != 0 && h.base < cap);
  };
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) any |= wanted(b);
  if (!any) return;
  stage_table(tbl, &sT);
  const u64 below = (1ull << lane) - 1;
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!wanted(b)) continue;
    const XHead head = heads[b];
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u32 pairs = 0;
    tile_runs<true>(&sT, sTile, d, n, toHi, delim, inv, p0 + t0, sW, sMask, &pairs);
    __syncthreads();
    if (w0 >= n) continue;                                                   // (uniform in the wave; the barriers are at the loop's head)
    Front e = {head.open & ~kHitBit, head.base, head.at, (head.open & kHitBit) != 0};
    for (u32 w = 0; w < wave; w++) { const Run v = sW[w]; advance(e, v.f, v.first, v.last, v.sel, v.bytes, inv); }
    // behind the wave: is the record open at its tail ended inside the tile, and the hits up to that delimiter
    bool closedW = false, hitAfterW = false;
    for (u32 w = wave + 1; w < 4 && !closedW; w++) { const u32 f = sW[w].f; hitAfterW |= (f & 2) != 0; closedW = (f & 1) != 0; }
    // the wave's trips as two masks: trip t has a delimiter, trip t has a hit in front of its first delimiter (or anywhere)
    u64 DM, HF;
    {
      u64 tdm = 0, thm = 0;
      if (lane < kWaveIters && w0 + lane * 64 < n) { tdm = sMask[wave][lane][0]; thm = sMask[wave][lane][1]; }
      DM = __ballot(tdm != 0);
      HF = __ballot((tdm ? thm & ((1ull << __builtin_ctzll(tdm)) - 1) : thm) != 0);
    }
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u64 dm = sMask[wave][t][0], hm = sMask[wave][t][1];
      const u32 j = w0 + t * 64 + lane;
      const u64 pos = p0 + t0 + w0 + t * 64;
      // the record open at the trip's tail: ended by the first delimiter of a later trip, a later wave, or behind the tile
      bool closed = closedW, hitAfter;
      const u64 restD = DM >> (t + 1), restH = HF >> (t + 1);
      if (restD) { closed = true; hitAfter = (restH & ((2ull << __builtin_ctzll(restD)) - 1)) != 0; }
      else hitAfter = restH != 0 || hitAfterW;
      const u64 dBelow = dm & below, above = dm >> lane;
      const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;       // the delimiter in front of this lane, inside the trip
      const u64 start = dBelow ? pos + prev + 1 : e.start;                   // this position's record
      u64 seg = dBelow ? hm & ~((2ull << prev) - 1) : hm;                    // its hits inside the trip
      bool sel;
      if (above) {
        seg &= (1ull << (lane + (u32)__builtin_ctzll(above))) - 1;
        sel = (seg != 0 || (!dBelow && e.hit)) != (bool)inv;
      } else {
        const bool hit = seg != 0 || (!dBelow && e.hit);
        sel = closed ? (hit || hitAfter) != (bool)inv : head.look != 0;
      }
      const bool ends = (above & 1) && sel;                                  // a selected record's delimiter
      const u64 sm = __ballot(ends);
      // the packed bytes of the trip's selected records in front of this position's record: the first one is as long as it likes
      // (uniform), the others are at most 64 bytes each
      u64 firstAdd = 0;
      u32 px = 0, total = 0, first = 64;
      if (dm) first = (u32)__builtin_ctzll(dm);
      if (sm) {
        if ((sm >> first) & 1) firstAdd = pos + first - e.start + 1;
        const u32 v = ends && lane != first ? lane - prev : 0;
        const u32 incl = wave_incl_scan(v);
        px = incl - v;
        total = __shfl(incl, 63, 64);
      }
      if (sel && j < n) {
        const u64 at = e.at + (lane > first ? firstAdd : 0) + px + (pos + lane - start);
        if (at < dataCap) dData[at] = (u8)lds_word(sTile, d + j);
      }
      if (ends) {
        const u64 idx = e.idx + (u32)__popcll(sm & below);
        if (idx < cap) { Range q; q.offset = start; q.size = pos + lane - start; list[idx] = q; }
      }
      if (dm) {
        const u32 last = 63 - (u32)__builtin_clzll(dm);
        e.at += firstAdd + total; e.idx += (u32)__popcll(sm);
        e.hit = last < 63 && (hm >> (last + 1)) != 0;
        e.start = pos + last + 1;
      } else e.hit |= hm != 0;
    }
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_extract_copy_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                          u32 inv, u64 p0, const XSum* sums, const XHead* heads, Range* list, u64 cap, u8* dData,
                                                                          u64 dataCap) {
  extract_copy<Table>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, heads, list, cap, dData, dataCap);
}
extern "C" __global__ void __launch_bounds__(256) zra_extract_copy_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                          u32 inv, u64 p0, const XSum* sums, const XHead* heads, Range* list, u64 cap, u8* dData,
                                                                          u64 dataCap) {
  extract_copy<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, inv, p0, sums, heads, list, cap, dData, dataCap);
}

// =================================================================================================
// The kernel set of the extract for zra_record_scan.h's call path. tables: Table | XTotals | sums[tiles] | heads[tiles]
namespace {
struct ExtractKernels {
  using Sum = XSum; using Head = XHead; using Totals = XTotals;
  static constexpr size_t kMapBytes = 0;
  static constexpr bool kData = true;
  static void launch(hipStream_t s, const LiteralSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<ExtractKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, inv = sel.inv, M = sel.M;
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_extract_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, (u64)ps.p0, p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_extract_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, (u64)ps.p0, p.sums, p.tot);
    hipLaunchKernelGGL(zra_extract_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), inv, (u32)ps.lastPass,
                       (u64)p.hi, (u64)ps.p0, (u64)ps.nPos, p.list, (u64)p.listCap, c.dData, (u64)c.dataCap, delim);
    if ((p.listCap || c.dataCap) && sel.pset.classes)
      hipLaunchKernelGGL(zra_extract_copy_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, inv, (u64)ps.p0, p.sums,
                         p.heads, p.list, (u64)p.listCap, c.dData, (u64)c.dataCap);
    else if (p.listCap || c.dataCap)
      hipLaunchKernelGGL(zra_extract_copy_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, inv, (u64)ps.p0, p.sums, p.heads,
                         p.list, (u64)p.listCap, c.dData, (u64)c.dataCap);
  }
};
static_assert(sizeof(XState) == 64 && sizeof(XSum) == 32 && sizeof(XHead) == 32, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::extract(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<LiteralSelect, ExtractKernels>(E, c, cv); }
}  // namespace zra_eng
