// zra_amd — extract of a device-resident archive with a record predicate (zra_hip.h: ZraHipExtractRecordsWhere): the
// records ZraHipGrepArchiveWhere selects (zra_grep_where.hip) WITH their bytes, packed as ZraHipExtractRecords packs them
// (zra_extract.hip): the text `grep A | grep B | grep -v C` prints, from the one decode pass that selects the records.
//
// The passes, the window and the driver's conditions are zra_scan.h's, the host path in front of them zra_record_scan.h's (the
// selector of the grep with a predicate, the kernel set at the end of this file); (set) and (trip) are zra_grep_where.hip's and
// (compaction), (provisional tail), (stores) and (launches) zra_extract.hip's, word for word. This call's own:
//  (summary) the two summaries side by side: {has a delimiter, front, behind: the sets in front of the first and behind the last one,
//      first, last: the position of the first delimiter and the one behind the last, sel, bytes: the selected records that end inside
//      the run APART from the first, and their packed bytes}: 48 bytes. combine() has the three cases of both parents; the record
//      that B's first delimiter ends, [A.last, B.first), is selected by s = where_selected(A.behind | B.front) and adds s to sel and
//      s * (B.first - A.last + 1) to bytes. It stays associative: a set is only ever tested where the two halves of a record
//      meet, and what it is ORed from does not depend on the bracketing.
//  (not monotone) under a predicate a record's selection can change along the record: with the clauses {0, 0, C}, {A | C, 0, 0} it is
//      selected while its set is {}, not when C arrives, and again when A arrives. So no part of the call tests a set in front of the
//      delimiter that ends the record. The scan's forward half carries the open record's set over delimiter-free tiles and tests it
//      at a tile's first delimiter; that bit is the one (look-ahead) hands to the tiles in front. Inside a tile the copy ORs the sets
//      of the trips and waves behind a position up to the next delimiter, and tests there; behind the tile's last delimiter it takes
//      the head's look-ahead bit. Across passes (provisional tail) copies the open record whatever its set says so far.
//  (second walk) the copy's first walk leaves zra_grep_where.hip's four words per trip. A backward step, a six-step segmented OR
//      over the wave's trips and then the waves behind, gives every trip {the record open at its tail ends inside the tile, the set
//      it gains up to that delimiter}. The second walk selects per trip two records by uniform tests (the one its first delimiter
//      ends, the one open at its tail), the others by the stored ballot, and stores each position's byte at d + (q - s).
#include "zra_record_scan.h"
#include "zra_where_tile.h"
#include "zra_extract_tail.h"

namespace {
// (summary). flags: 1 a delimiter, 8 (set by the scan) the record the first delimiter ends is selected
struct __attribute__((aligned(16))) XWSum { u64 front, behind, first, last, bytes; u32 sel, flags; };
// what the scan makes of it for the copy: the list position of the tile's first record, the start of the record open at its head, the
// packed bytes in front of that record, (look-ahead)'s bit, and that record's set so far
struct __attribute__((aligned(16))) XWHead { u64 base, open, at, look, set, pad; };
// the state carried from pass to pass: zra_extract.hip's XState with the open record's set in `hit`
struct XWState { u64 start, hit, sel, tail, bytes, pad[3]; };
struct XWTotals { XWState st[2]; u64 matches, delims, pad[6]; };

// a summary in registers; sel and bytes are kept wide by the scan
struct RunW { u32 has; u64 front, behind, first, last, sel, bytes; };

// A := the summary of run A followed by run B
__device__ __forceinline__ void combine(RunW& A, const RunW& B, const Block& w) {
  if (!B.has) {
    if (A.has) A.behind |= B.front; else { A.front |= B.front; A.behind = A.front; }
    return;
  }
  if (!A.has) { A.front |= B.front; A.behind = B.behind; A.first = B.first; A.last = B.last; A.sel = B.sel; A.bytes = B.bytes; A.has = 1; return; }
  const bool s = where_selected(w, A.behind | B.front);                      // the record B's first delimiter ends began in A
  A.sel += B.sel + (s ? 1u : 0u);
  A.bytes += B.bytes + (s ? B.first - A.last + 1 : 0);
  A.behind = B.behind; A.last = B.last;
}

// what lies in front of a run, moved over the run: the open record's start and set, the list position, the packed offset
struct FrontW { u64 start, set, idx, at; };
__device__ __forceinline__ void advance(FrontW& e, const RunW& r, const Block& w) {
  if (!r.has) { e.set |= r.front; return; }
  const bool s = where_selected(w, e.set | r.front);
  e.idx += r.sel + (s ? 1u : 0u);
  e.at += r.bytes + (s ? r.first - e.start + 1 : 0);
  e.set = r.behind; e.start = r.last;
}

// One trip: zra_grep_where.hip's four words {the delimiter ballot, the selection ballot of the delimiters but the first, front,
// behind} and the packed bytes of the records that ballot selects (each at most 63 bytes and its delimiter)
struct TripW { u64 dm, sb, front, behind; u32 bytes; };
__device__ __forceinline__ TripW trip_words(u64 dm, u64 hm, u64 m, u32 lane, const Block& w) {
  TripW r = {dm, 0, 0, 0, 0};
  if (dm == 0) {                                                             // (uniform in the wave, as every branch on a ballot below)
    r.front = r.behind = hm ? trip_union(m, hm, lane) : 0;
    return r;
  }
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;           // the delimiter in front of this lane, inside the trip
  const u64 seg = dBelow ? below & ~((2ull << prev) - 1) : below;            // the lanes between it (or the trip's head) and this lane
  u64 H = 0;
  if (hm) trip_sets(m, hm, dm, lane, first, last, seg, &H, &r.front, &r.behind);
  const bool sel = ((dm >> lane) & 1) && lane != first && where_selected(w, H);
  r.sb = __ballot(sel);
  if (r.sb) r.bytes = wave_sum(sel ? lane - prev : 0);
  return r;
}

// A wave's first walk over its trips: the record that the wave's first delimiter ends is left to whoever combines the summaries.
// set: the patterns hit in the record open behind the trips so far, start: the position behind the last delimiter.
struct WalkX { bool seen; u32 sel; u64 bytes, set, front, first, start; };
__device__ __forceinline__ void walk_trip(WalkX& s, const TripW& t, const Block& w, u64 pos) {
  if (t.dm == 0) { s.set |= t.front; return; }
  const u32 first = (u32)__builtin_ctzll(t.dm), last = 63 - (u32)__builtin_clzll(t.dm);
  s.sel += (u32)__popcll(t.sb); s.bytes += t.bytes;
  if (!s.seen) { s.front = s.set | t.front; s.first = pos + first; s.seen = true; }
  else if (where_selected(w, s.set | t.front)) { s.sel++; s.bytes += pos + first - s.start + 1; }
  s.set = t.behind;
  s.start = pos + last + 1;
}
__device__ __forceinline__ RunW walk_run(const WalkX& s) {
  RunW r;
  r.has = s.seen ? 1u : 0u; r.front = s.seen ? s.front : s.set; r.behind = s.set; r.first = s.first; r.last = s.start; r.sel = s.sel; r.bytes = s.bytes;
  return r;
}

// One tile's first walk, the same in the count and in the copy: per trip its words (the four of (second walk) kept in sTrip when
// kKeep), per wave its summary -> sW[wave]. Returns the delimiters the wave saw.
template <bool kKeep, class TB>
__device__ __forceinline__ u32 tile_runs(const TB* sT, const u32* sTile, u32 d, u32 n, long long toHi, u32 delim, const Block& w, u64 tilePos, RunW* sW,
                                         u64 (*sTrip)[kWaveIters][4], u32* pairs) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w0 = wave * kWavePos;
  WalkX s = {false, 0, 0, 0, 0, 0, tilePos + w0};
  u32 delims = 0;
#pragma unroll 1
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    u64 dm, hm;
    const u64 m = trip_masks(sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, pairs);
    delims += (u32)__popcll(dm);
    const TripW q = trip_words(dm, hm, m, lane, w);
    if (kKeep && lane == 0) { sTrip[wave][t][0] = q.dm; sTrip[wave][t][1] = q.sb; sTrip[wave][t][2] = q.front; sTrip[wave][t][3] = q.behind; }
    walk_trip(s, q, w, tilePos + w0 + t * 64);
  }
  if (lane == 0) sW[wave] = walk_run(s);
  return delims;
}
}  // namespace

// The run of a pass, its tiles and workgroups: zra_extract.hip's extract_count. Per tile its summary -> sums[tile]; per call the totals.
template <class TB>
__device__ __forceinline__ void extractw_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, const Block& w, u64 p0,
                                               XWSum* sums, XWTotals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ RunW sW[4];
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
    delims += tile_runs<false>(&sT, sTile, d, n, toHi, delim, w, p0 + t0, sW, nullptr, &pairs);
    __syncthreads();
    if (tid == 0) {
      RunW r = sW[0];
      for (u32 v = 1; v < 4; v++) combine(r, sW[v], w);
      XWSum o; o.front = r.front; o.behind = r.behind; o.first = r.first; o.last = r.last; o.bytes = r.bytes; o.sel = (u32)r.sel; o.flags = r.has;
      sums[b] = o;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
extern "C" __global__ void __launch_bounds__(256) zra_extractw_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                            Block w, u64 p0, XWSum* sums, XWTotals* tot) {
  extractw_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_extractw_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                                  u32 delim, Block w, u64 p0, XWSum* sums, XWTotals* tot) {
  extractw_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, tot);
}

// One workgroup: zra_extract_scan_kernel over the 48-byte summaries. Forward: every lane reduces a run of consecutive tiles, the 1,024
// summaries are scanned in LDS (Hillis-Steele over combine()), then the lane walks its run again from what lies in front of it:
// heads[t], sums[t].sel becomes ALL the selected records that end in tile t, and flag 8 says whether the first of them is one: the
// predicate on the set the record has gathered from its start, wherever that lies, up to this delimiter (not monotone). The last
// lane ends the pass; backward, (look-ahead) hands flag 8 of the nearest following tile with a delimiter, or the pass's end, to
// every tile's head.
extern "C" __global__ void __launch_bounds__(1024) zra_extractw_scan_kernel(XWSum* sums, u32 nTiles, XWHead* heads, const XWState* in, XWState* out, Block w,
                                                                            u32 lastPass, u64 hi, u64 p0, u64 nPos, Range* list, u64 cap, u8* dData, u64 dataCap,
                                                                            u32 delim) {
  __shared__ u64 sFront[1024], sBehind[1024], sFirst[1024], sLast[1024], sSel[1024], sBytes[1024];
  __shared__ u32 sHas[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  auto load = [&](u32 i) { const RunW r = {sHas[i], sFront[i], sBehind[i], sFirst[i], sLast[i], sSel[i], sBytes[i]}; return r; };
  auto store = [&](const RunW& r) { sHas[tid] = r.has; sFront[tid] = r.front; sBehind[tid] = r.behind; sFirst[tid] = r.first; sLast[tid] = r.last; sSel[tid] = r.sel; sBytes[tid] = r.bytes; };
  auto tile = [&](u32 t) { const XWSum s = sums[t]; const RunW r = {s.flags & 1, s.front, s.behind, s.first, s.last, s.sel, s.bytes}; return r; };
  RunW r = {0, 0, 0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) combine(r, tile(t), w);
  store(r);
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    RunW a = {0, 0, 0, 0, 0, 0, 0};
    if (tid >= d) a = load(tid - d);
    __syncthreads();
    if (tid >= d) { combine(a, r, w); r = a; store(r); }
    __syncthreads();
  }
  // what lies in front of this lane's run: the carried state, then the lanes in front
  FrontW e = {in->start, in->hit, in->sel, in->bytes};
  if (tid) advance(e, load(tid - 1), w);
  u32 look = 0;                                                              // 2: the run has a delimiter, 1: the record its first one ends is selected
  for (u32 t = b0; t < b1; t++) {
    const RunW s = tile(t);
    XWHead h; h.base = e.idx; h.open = e.start; h.at = e.at; h.look = 0; h.set = e.set; h.pad = 0;
    heads[t] = h;
    if (s.has) {
      const u32 fs = where_selected(w, e.set | s.front) ? 1u : 0u;
      sums[t].sel = (u32)s.sel + fs;
      sums[t].flags = 1u | (fs ? 8u : 0u);
      if (!look) look = 2 | fs;
    }
    advance(e, s, w);
  }
  u32 tailSel = 0;
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tail;
    tailSel = extract_pass_end(lastPass, where_selected(w, e.set), e.start, hi, e.idx, e.at, tail, list, cap, dData, dataCap, delim);
    XWState o; o.start = e.start; o.hit = e.set; o.sel = e.idx; o.tail = tail; o.bytes = e.at; o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *out = o;
  }
  look_ahead(look, tailSel, b0, b1, p0, nPos, heads, [&](u32 t) { const XWSum s = sums[t]; return LookTile{(s.flags & 1) != 0, (s.flags >> 3) & 1, s.last}; });
}

// zra_extract.hip's extract_copy: the count's workgroups redo the tiles that hold a byte of a selected record or a listed record in
// front of the capacities. First walk: the four words of every trip go to LDS with the waves' summaries. Then, per wave: what lies in
// front of it from the tile's head and the waves in front; (second walk)'s backward step; and the second walk, in which every lane
// stores its position's byte where (compaction) puts it.
template <class TB>
__device__ __forceinline__ void extractw_copy(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, const Block& w, u64 p0,
                                              const XWSum* sums, const XWHead* heads, Range* list, u64 cap, u8* dData, u64 dataCap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ RunW sW[4];
  __shared__ u64 sTrip[4][kWaveIters][4];
  __shared__ FrontW sFront[4];
  __shared__ u64 sGain[4];
  __shared__ u32 sClosed[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  // a tile's bytes go to head.at and behind, its list entries to head.base and behind (uniform in the workgroup)
  auto wanted = [&](u32 b) {
    const u32 sel = sums[b].sel;
    const XWHead h = heads[b];
    return ((sel != 0 || h.look != 0) && h.at < dataCap) || (sel != 0 && h.base < cap);
  };
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) any |= wanted(b);
  if (!any) return;
  stage_table(tbl, &sT);
  const u64 below = (1ull << lane) - 1;
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!wanted(b)) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u32 pairs = 0;
    tile_runs<true>(&sT, sTile, d, n, toHi, delim, w, p0 + t0, sW, sTrip, &pairs);
    __syncthreads();
    // per wave, by one lane: what lies in front of it (from the tile's head and the waves in front), and behind it: is the record open
    // at its tail ended inside the tile, and the set it gains up to that delimiter
    if (tid == 0) {
      const XWHead h = heads[b];
      FrontW f = {h.open, h.set, h.base, h.at};
      for (u32 v = 0; v < 4; v++) { sFront[v] = f; advance(f, sW[v], w); }
      u64 gain = 0;
      u32 closed = 0;
      for (u32 v = 4; v-- > 0;) {
        sGain[v] = gain; sClosed[v] = closed;
        if (sW[v].has) { gain = sW[v].front; closed = 1; } else gain |= sW[v].front;
      }
    }
    __syncthreads();
    if (w0 >= n) continue;                                                   // (uniform in the wave; the barriers are at the loop's head)
    const bool look = heads[b].look != 0;
    const u64 wavePos = p0 + t0 + w0;
    FrontW e = sFront[wave];
    const bool closedW = sClosed[wave] != 0;
    const u64 gainW = sGain[wave];
    // (second walk)'s backward step. Lane t holds trip t as {c: it has a delimiter, a: its front}; a run of trips X followed by a run
    // Y is X when X has a delimiter and {Y.c, X.a | Y.a} otherwise. Six steps leave in lane t the trips t .. of the wave; the trips
    // BEHIND trip t are lane t + 1's, followed by the waves behind. Lanes from the wave's trip count on hold the neutral {0, 0}, lane
    // 63 among them; a shuffle from beyond the wave returns the lane's own pair, and a pair followed by itself is that pair.
    static_assert(kWaveIters < 64, "a neutral lane behind the trips");
    u32 oc;
    u64 oa;
    {
      u32 c = 0;
      u64 a = 0;
      if (lane < kWaveIters && w0 + lane * 64 < n) { c = sTrip[wave][lane][0] != 0; a = sTrip[wave][lane][2]; }
      for (u32 s = 1; s < 64; s <<= 1) {
        const u32 vc = __shfl_down(c, s);
        const u64 va = __shfl_down(a, s);
        if (!c) { a |= va; c = vc; }
      }
      oc = __shfl_down(c, 1); oa = __shfl_down(a, 1);
      if (!oc) { oa |= gainW; oc = closedW ? 1u : 0u; }
    }
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      const u64* const q = sTrip[wave][t];
      const u64 dm = q[0], sb = q[1], front = q[2], behind = q[3];
      const u32 j = w0 + t * 64 + lane;
      const u64 pos = wavePos + t * 64;
      // the record open at the trip's tail: its set is complete at the delimiter that ends it, and only there is it tested
      const u32 closed = (u32)__builtin_amdgcn_readlane((int)oc, (int)t);
      const u64 tailSet = (dm ? behind : e.set | front) | lane_word(oa, (int)t);
      const bool tailSel = closed ? where_selected(w, tailSet) : look;
      u32 first = 64, last = 0;
      u64 sm = 0;                                                            // the delimiters of the trip that end a selected record
      if (dm) {
        first = (u32)__builtin_ctzll(dm); last = 63 - (u32)__builtin_clzll(dm);
        sm = sb | (where_selected(w, e.set | front) ? 1ull << first : 0);
      }
      const u64 dBelow = dm & below, above = dm >> lane;
      const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;       // the delimiter in front of this lane, inside the trip
      const u64 start = dBelow ? pos + prev + 1 : e.start;                   // this position's record
      const bool sel = above ? ((sm >> (lane + (u32)__builtin_ctzll(above))) & 1) != 0 : tailSel;
      const bool ends = (above & 1) && sel;                                  // a selected record's delimiter
      // the packed bytes of the trip's selected records in front of this position's record: the first one is as long as it likes
      // (uniform), the others are at most 64 bytes each
      u64 firstAdd = 0;
      u32 px = 0, total = 0;
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
        if (idx < cap) { Range r; r.offset = start; r.size = pos + lane - start; list[idx] = r; }
      }
      if (dm) {
        e.at += firstAdd + total; e.idx += (u32)__popcll(sm);
        e.set = behind;
        e.start = pos + last + 1;
      } else e.set |= front;
    }
  }
}
extern "C" __global__ void __launch_bounds__(256) zra_extractw_copy_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                           Block w, u64 p0, const XWSum* sums, const XWHead* heads, Range* list, u64 cap, u8* dData,
                                                                           u64 dataCap) {
  extractw_copy<Table>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, heads, list, cap, dData, dataCap);
}
extern "C" __global__ void __launch_bounds__(256) zra_extractw_copy_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl,
                                                                                 u32 delim, Block w, u64 p0, const XWSum* sums, const XWHead* heads, Range* list, u64 cap,
                                                                                 u8* dData, u64 dataCap) {
  extractw_copy<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, w, p0, sums, heads, list, cap, dData, dataCap);
}

// =================================================================================================
// The kernel set of the extract with a record predicate for zra_record_scan.h's call path. tables: Table | XWTotals | sums[tiles] | heads[tiles]
namespace {
struct ExtractWhereKernels {
  using Sum = XWSum; using Head = XWHead; using Totals = XWTotals;
  static constexpr size_t kMapBytes = 0;
  static constexpr bool kData = true;
  static void launch(hipStream_t s, const WhereSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<ExtractWhereKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, M = sel.M;
    const Block& w = sel.w;
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_extractw_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, w, (u64)ps.p0, p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_extractw_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, w, (u64)ps.p0, p.sums, p.tot);
    hipLaunchKernelGGL(zra_extractw_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, p.tot->st + parity, p.tot->st + (parity ^ 1), w, (u32)ps.lastPass,
                       (u64)p.hi, (u64)ps.p0, (u64)ps.nPos, p.list, (u64)p.listCap, c.dData, (u64)c.dataCap, delim);
    if ((p.listCap || c.dataCap) && sel.pset.classes)
      hipLaunchKernelGGL(zra_extractw_copy_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, w, (u64)ps.p0, p.sums,
                         p.heads, p.list, (u64)p.listCap, c.dData, (u64)c.dataCap);
    else if (p.listCap || c.dataCap)
      hipLaunchKernelGGL(zra_extractw_copy_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, w, (u64)ps.p0, p.sums, p.heads,
                         p.list, (u64)p.listCap, c.dData, (u64)c.dataCap);
  }
};
static_assert(sizeof(XWState) == 64 && sizeof(XWSum) == 48 && sizeof(XWHead) == 48, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::extract_where(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<WhereSelect, ExtractWhereKernels>(E, c, cv); }
}  // namespace zra_eng
