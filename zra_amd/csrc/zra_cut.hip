// zra_amd — cut of a device-resident archive (zra_hip.h: ZraHipCutRecords): the extract's selected records (zra_extract.hip), of each
// only the chosen FIELDS, packed into a device buffer in ascending order, each record followed by the delimiter: the text
// `grep -F -f patterns | cut -d SEP -f LIST` prints, from the one decode pass that selects the records.
//
// The passes, the staging window, the records, the selection, (stream), (forward), (order), (look-ahead) and (stores) are the extract's,
// word for word. This call's own:
//  (fields) inside a record field 1 starts at the record's start and every separator byte starts the next field. A position's keep
//      flag is a function of c = the separators in front of it in its record, and of its byte: a content byte is kept iff bit
//      min(c, 63) of the field mask is set; a separator (it starts field c + 2) iff bit min(c, 63) of the SEPARATOR MASK, which the
//      host derives: field c + 2 is chosen and some field in front of it is; the delimiter of a selected record always. c saturates at
//      63: field 64 (c = 63) and every later one answer to bit 63, and the separator in front of field 64 (c = 62) is the last one
//      whose answer differs from its successors'.
//  (summary) the extract's without `bytes`, plus the field carry {separators in front of the first delimiter, separators behind the
//      last}, saturating at 63: min(a + b, 63) is associative, so combine() stays so. A record's packed size is not its length and
//      the kept bytes of the piece in front of a run's first delimiter depend on the field number that comes in, so no packed offset
//      is carried in the summary: the addresses come from a second scan, over scalars.
//  (compaction) once the first scan has given every tile its head (list position, the open record's start, hit bit and separator
//      count, the look-ahead bit), every position's keep flag is decidable inside its tile. The keep launch writes the flags, 64 to a
//      word, and per tile two scalars: the kept positions, and those behind its last delimiter. The place launch scans the first
//      scalar into tile bases; the copy launch is a plain stream compaction: address = tile base + the keep flags in front of the
//      position, by popcounts over the tile's 128 words. No atomic decides an address.
//  (provisional tail) the extract's idea with the record's kept bytes K beside the packed offset D: the record open at the end of a
//      pass that is not the last is copied at D, K = its kept bytes so far. The next pass starts its compaction at D + K when the
//      record its first delimiter ends is selected (or no delimiter comes), at D otherwise. D moves over a record only at its
//      delimiter. In the last pass the record open at hi ends there, and its delimiter goes behind its kept bytes.
//  (launches) zra_cut_count_kernel, zra_cut_scan_kernel (ONE workgroup), zra_cut_keep_kernel, zra_cut_place_kernel (ONE workgroup),
//      zra_cut_copy_kernel, the last one only when there is a data buffer.
#include "zra_record_scan.h"
#include "zra_extract_tail.h"
#include "zra_joblist.h"

namespace {
constexpr u32 kSepMax = 63;                                                  // (fields)
constexpr u32 kKeepWords = kTile / 64;
// (summary). flags: the extract's. sepF: the separators in front of the first delimiter, sepB: behind the last; a run without a
// delimiter has both equal to all of its separators
struct __attribute__((aligned(16))) CSum { u64 first, last; u32 sel, flags, sepF, sepB; };
// what the first scan makes of it: the list position of the tile's first record, the start of the record open at its head with that
// record's hit bit in bit 63, (look-ahead)'s bit, that record's separators in front of the tile
struct __attribute__((aligned(16))) CHead { u64 base, open, look; u32 seps, pad; };
// a tile's keep flags and its scalars; base: the packed offset of its first kept byte (the place launch)
struct __attribute__((aligned(16))) CMap { u64 keep[kKeepWords]; u64 base; u32 total, tail; };
// the state carried from pass to pass. bytes / kept: (provisional tail)'s D and K; seps: the open record's separators so far. The
// scan hands the place launch of its pass: base, where the pass's compaction starts; lastTile: 1 + the tile of the pass's last
// delimiter, 0 without one; tailSel: the last pass ended a selected record at hi
struct CState { u64 start, hit, sel, tail, bytes, kept, seps, base, lastTile, tailSel, pad[2]; };
struct CTotals { CState st[2]; u64 matches, delims; };

struct Run { u32 f, sepF, sepB; u64 first, last, sel; };

__device__ __forceinline__ u32 sat(u32 v) { return min(v, kSepMax); }

// the summary of run A followed by run B
__device__ __forceinline__ void combine(Run& a, const Run& b, u32 inv) {
  if (!(b.f & 1)) {
    if (b.f & 2) a.f |= (a.f & 1) ? 4u : 6u;
    a.sepB = sat(a.sepB + b.sepF);
    if (!(a.f & 1)) a.sepF = a.sepB;
    return;
  }
  if (!(a.f & 1)) {
    a.f = 1 | ((a.f | b.f) & 2) | (b.f & 4); a.first = b.first; a.last = b.last; a.sel = b.sel;
    a.sepF = sat(a.sepF + b.sepF); a.sepB = b.sepB;
    return;
  }
  const u32 s = (((a.f >> 2) | (b.f >> 1)) & 1) ^ inv;                       // the record B's first delimiter ends began in A
  a.sel += b.sel + s;
  a.f = 1 | (a.f & 2) | (b.f & 4); a.last = b.last; a.sepB = b.sepB;
}

// what lies in front of a run, moved over the run: the open record's start, hit bit and separators, the list position
struct Front { u64 start, idx; u32 seps; bool hit; };
__device__ __forceinline__ void advance(Front& e, const Run& r, u32 inv) {
  if (!(r.f & 1)) { e.hit |= (r.f & 2) != 0; e.seps = sat(e.seps + r.sepF); return; }
  const u32 s = (u32)(e.hit || (r.f & 2)) ^ inv;
  e.idx += r.sel + s;
  e.hit = (r.f & 4) != 0; e.start = r.last; e.seps = r.sepB;
}

// The summary of one trip from its three ballots; pos = the content offset of lane 0's position.
__device__ __forceinline__ Run trip_run(u64 dm, u64 hm, u64 sm, u32 lane, u32 inv, u64 pos) {
  Run r = {0, 0, 0, 0, 0, 0};
  if (dm == 0) { r.f = hm ? 6u : 0u; r.sepF = r.sepB = sat((u32)__popcll(sm)); return r; }   // (uniform in the wave)
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  bool sel = false;
  if (((dm >> lane) & 1) && dBelow) {
    const u32 prev = 63 - (u32)__builtin_clzll(dBelow);
    sel = ((hm & below & ~((2ull << prev) - 1)) != 0) != (bool)inv;
  }
  r.f = 1u | ((hm & ((1ull << first) - 1)) ? 2u : 0u) | ((last < 63 && (hm >> (last + 1))) ? 4u : 0u);
  r.first = pos + first; r.last = pos + last + 1;
  r.sel = (u32)__popcll(__ballot(sel));
  r.sepF = (u32)__popcll(sm & ((1ull << first) - 1));
  r.sepB = last < 63 ? (u32)__popcll(sm >> (last + 1)) : 0;
  return r;
}

// One tile's first walk, the same in the count and in the keep launch: per trip the three ballots (kept in sMask when kKeep), per wave
// its summary -> sW[wave]. Returns the delimiters the wave saw.
template <bool kKeep, class TB>
__device__ __forceinline__ u32 tile_runs(const TB* sT, const u32* sTile, u32 d, u32 n, long long toHi, u32 delim, u32 sep, u32 inv, u64 tilePos, Run* sW,
                                         u64 (*sMask)[kWaveIters][3], u32* pairs) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w0 = wave * kWavePos;
  Run w = {0, 0, 0, 0, 0, 0};
  u32 delims = 0;
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    u64 dm, hm;
    const u32 j = w0 + t * 64 + lane;
    trip_flags(sT, sTile, d, j, n, toHi, delim, &dm, &hm, pairs);
    const u64 sm = __ballot(j < n && (lds_word(sTile, d + j) & 0xFF) == sep);
    if (kKeep && lane == 0) { sMask[wave][t][0] = dm; sMask[wave][t][1] = hm; sMask[wave][t][2] = sm; }
    delims += (u32)__popcll(dm);
    combine(w, trip_run(dm, hm, sm, lane, inv, tilePos + w0 + t * 64), inv);
  }
  if (lane == 0) sW[wave] = w;
  return delims;
}

// The count: extract_count with the separator carry. Workgroup g takes the tiles [g * kGroup, (g + 1) * kGroup).
template <class TB>
__device__ __forceinline__ void cut_count(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, u32 sep, u32 inv, u64 p0,
                                          CSum* sums, CTotals* tot) {
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
    delims += tile_runs<false>(&sT, sTile, d, n, toHi, delim, sep, inv, p0 + t0, sW, nullptr, &pairs);
    __syncthreads();
    if (tid == 0) {
      Run r = sW[0];
      for (u32 w = 1; w < 4; w++) combine(r, sW[w], inv);
      CSum o; o.first = r.first; o.last = r.last; o.sel = (u32)r.sel; o.flags = r.f; o.sepF = r.sepF; o.sepB = r.sepB;
      sums[b] = o;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) zra_cut_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim, u32 sep,
                                                                       u32 inv, u64 p0, CSum* sums, CTotals* tot) {
  cut_count<Table>(win, xLo, xHi, nPos, M, tbl, delim, sep, inv, p0, sums, tot);
}
extern "C" __global__ void __launch_bounds__(256) zra_cut_count_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                             u32 sep, u32 inv, u64 p0, CSum* sums, CTotals* tot) {
  cut_count<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, sep, inv, p0, sums, tot);
}

// One workgroup. Forward, as the extract's scan without the packed offset: every lane reduces a run of consecutive tiles, the 1,024
// summaries are scanned in LDS (Hillis-Steele over combine()), then the lane walks its run again from what lies in front of it:
// heads[t], sums[t].sel becomes ALL the selected records that end in tile t, flag 8 says whether the first of them is one. The last
// lane ends the pass: the state moves on apart from D and K, which the place launch writes; in the last pass the record open at hi
// ends there (its list entry). Backward: (look-ahead), zra_extract_tail.h's.
extern "C" __global__ void __launch_bounds__(1024) zra_cut_scan_kernel(CSum* sums, u32 nTiles, CHead* heads, const CState* in, CState* out, u32 inv, u32 lastPass, u64 hi,
                                                                       u64 p0, u64 nPos, Range* list, u64 cap) {
  __shared__ u64 sFirst[1024], sLast[1024], sSel[1024];
  __shared__ u32 sF[1024];                                                   // flags | sepF << 8 | sepB << 16
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  auto load = [&](u32 i) { const u32 f = sF[i]; const Run v = {f & 0xFF, (f >> 8) & 0xFF, f >> 16, sFirst[i], sLast[i], sSel[i]}; return v; };
  auto store = [&](u32 i, const Run& v) { sF[i] = v.f | v.sepF << 8 | v.sepB << 16; sFirst[i] = v.first; sLast[i] = v.last; sSel[i] = v.sel; };
  auto tile = [&](u32 t) { const CSum s = sums[t]; const Run v = {s.flags, s.sepF, s.sepB, s.first, s.last, s.sel}; return v; };
  Run r = {0, 0, 0, 0, 0, 0};
  for (u32 t = b0; t < b1; t++) combine(r, tile(t), inv);
  store(tid, r);
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    Run a = {0, 0, 0, 0, 0, 0};
    if (tid >= d) a = load(tid - d);
    __syncthreads();
    if (tid >= d) { combine(a, r, inv); r = a; store(tid, r); }
    __syncthreads();
  }
  // what lies in front of this lane's run: the carried state, then the lanes in front
  Front e = {in->start, in->sel, (u32)in->seps, in->hit != 0};
  if (tid) advance(e, load(tid - 1), inv);
  u32 look = 0;                                                              // 2: the run has a delimiter, 1: the record its first one ends is selected
  for (u32 t = b0; t < b1; t++) {
    const Run s = tile(t);
    CHead h; h.base = e.idx; h.open = e.start | (e.hit ? kHitBit : 0); h.look = 0; h.seps = e.seps; h.pad = 0;
    heads[t] = h;
    if (s.f & 1) {
      const u32 fs = (u32)(e.hit || (s.f & 2)) ^ inv;
      sums[t].sel = (u32)s.sel + fs;
      sums[t].flags = s.f | (fs ? 8u : 0u);
      if (!look) look = 2 | fs;
    }
    advance(e, s, inv);
  }
  u32 tailSel = 0;
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one; r is the whole pass)
    u64 tail = 0;
    if (!lastPass) tailSel = 1;
    else if (e.start < hi) {
      tail = 1;
      if ((u32)e.hit != inv) {
        if (e.idx < cap) { Range q; q.offset = e.start; q.size = hi - e.start; list[e.idx] = q; }
        e.idx++; tailSel = 1;
      }
    }
    // (provisional tail) does the record open at the pass's head keep its earlier part: the look-ahead bit in front of tile 0
    const u32 frontSel = (r.f & 1) ? (u32)(in->hit != 0 || (r.f & 2)) ^ inv : tailSel;
    CState o;
    o.start = e.start; o.hit = e.hit; o.sel = e.idx; o.tail = tail; o.bytes = 0; o.kept = 0; o.seps = e.seps;
    o.base = in->bytes + (frontSel ? in->kept : 0);
    o.lastTile = (r.f & 1) ? (r.last - 1 - p0) / kTile + 1 : 0;
    o.tailSel = lastPass ? tailSel : 0;
    o.pad[0] = o.pad[1] = 0;
    *out = o;
  }
  look_ahead(look, tailSel, b0, b1, p0, nPos, heads, [&](u32 t) { const CSum s = sums[t]; return LookTile{(s.flags & 1) != 0, (s.flags >> 3) & 1, s.last}; });
}

namespace {
// The count's workgroups redo the tiles that hold a position of a selected record (the others keep nothing: two zeros). First walk:
// the ballots of every trip go to LDS with the waves' summaries. Second walk, the extract's copy as far as the selection and the list
// go: a wave takes what lies in front of it from the tile's head and the waves in front, what lies behind it from the waves behind and
// the head's look-ahead bit; a lane counts the separators in front of its position in its record, (fields) decides, and the wave's
// ballot of keep flags is the tile's word for the trip.
template <class TB>
__device__ __forceinline__ void cut_keep(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const TB* tbl, u32 delim, u32 sep, u32 inv, u64 p0,
                                         const CSum* sums, const CHead* heads, CMap* maps, Range* list, u64 cap, u64 fieldMask, u64 sepMask) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ TB sT;
  __shared__ Run sW[4];
  __shared__ u64 sMask[4][kWaveIters][3];
  __shared__ u32 sKept[4][3];                                                // per wave: kept positions, those behind its last delimiter, has one
  __shared__ u64 sField[2];                                                  // the two masks of (fields), read per trip: they need not live in scalar registers
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  auto wanted = [&](u32 b) { return sums[b].sel != 0 || heads[b].look != 0; };   // (uniform in the workgroup)
  bool any = false;
  for (u32 b = bBegin; b < bEnd; b++) {
    const bool w = wanted(b);
    if (!w && tid == 0) { maps[b].base = 0; maps[b].total = 0; maps[b].tail = 0; }
    any |= w;
  }
  if (!any) return;
  stage_table(tbl, &sT);
  if (tid == 0) { sField[0] = fieldMask; sField[1] = sepMask; }              // (the barriers at the loop's head come before any read)
  const u64 below = (1ull << lane) - 1;
  for (u32 b = bBegin; b < bEnd; b++) {
    if (!wanted(b)) continue;
    const CHead head = heads[b];
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    u32 pairs = 0;
    tile_runs<true>(&sT, sTile, d, n, toHi, delim, sep, inv, p0 + t0, sW, sMask, &pairs);
    __syncthreads();
    u32 wTotal = 0, wTail = 0, wHas = 0;
    if (w0 < n) {                                                            // (uniform in the wave; the barriers are outside)
      Front e = {head.open & ~kHitBit, head.base, head.seps, (head.open & kHitBit) != 0};
      for (u32 w = 0; w < wave; w++) advance(e, sW[w], inv);
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
        const u64 dm = sMask[wave][t][0], hm = sMask[wave][t][1], sm = sMask[wave][t][2];
        const u32 j = w0 + t * 64 + lane;
        const u64 pos = p0 + t0 + w0 + t * 64;
        // the record open at the trip's tail: ended by the first delimiter of a later trip, a later wave, or behind the tile
        bool closed = closedW, hitAfter;
        const u64 restD = DM >> (t + 1), restH = HF >> (t + 1);
        if (restD) { closed = true; hitAfter = (restH & ((2ull << __builtin_ctzll(restD)) - 1)) != 0; }
        else hitAfter = restH != 0 || hitAfterW;
        const u64 dBelow = dm & below, above = dm >> lane;
        const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;     // the delimiter in front of this lane, inside the trip
        const u64 inRec = dBelow ? ~((2ull << prev) - 1) : ~0ull;            // the lanes of this position's record
        const u64 start = dBelow ? pos + prev + 1 : e.start;
        u64 seg = hm & inRec;                                                // its hits inside the trip
        bool sel;
        if (above) {
          seg &= (1ull << (lane + (u32)__builtin_ctzll(above))) - 1;
          sel = (seg != 0 || (!dBelow && e.hit)) != (bool)inv;
        } else {
          const bool hit = seg != 0 || (!dBelow && e.hit);
          sel = closed ? (hit || hitAfter) != (bool)inv : head.look != 0;
        }
        const bool ends = (above & 1) && sel;                                // a selected record's delimiter
        const u64 em = __ballot(ends);
        // (fields)
        const u32 c = sat((dBelow ? 0 : e.seps) + (u32)__popcll(sm & below & inRec));
        const bool keep = sel && j < n && ((above & 1) || ((sField[(sm >> lane) & 1] >> c) & 1));
        const u64 km = __ballot(keep);
        if (lane == 0) maps[b].keep[wave * kWaveIters + t] = km;
        if (ends) {
          const u64 idx = e.idx + (u32)__popcll(em & below);
          if (idx < cap) { Range q; q.offset = start; q.size = pos + lane - start; list[idx] = q; }
        }
        wTotal += (u32)__popcll(km);
        if (dm) {
          const u32 last = 63 - (u32)__builtin_clzll(dm);
          const u64 behind = last < 63 ? ~0ull << (last + 1) : 0;
          e.idx += (u32)__popcll(em);
          e.hit = (hm & behind) != 0;
          e.seps = sat((u32)__popcll(sm & behind));
          e.start = pos + last + 1;
          wTail = (u32)__popcll(km & behind); wHas = 1;
        } else {
          e.hit |= hm != 0;
          e.seps = sat(e.seps + (u32)__popcll(sm));
          wTail += (u32)__popcll(km);
        }
      }
    }
    if (lane == 0) { sKept[wave][0] = wTotal; sKept[wave][1] = wTail; sKept[wave][2] = wHas; }
    __syncthreads();
    if (tid == 0) {
      u32 total = 0, tail = 0;
      for (u32 w = 0; w < 4; w++) total += sKept[w][0];
      for (u32 w = 4; w-- > 0;) { tail += sKept[w][1]; if (sKept[w][2]) break; }
      maps[b].base = 0; maps[b].total = total; maps[b].tail = tail;
    }
  }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) zra_cut_keep_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim, u32 sep,
                                                                      u32 inv, u64 p0, const CSum* sums, const CHead* heads, CMap* maps, Range* list, u64 cap,
                                                                      u64 fieldMask, u64 sepMask) {
  cut_keep<Table>(win, xLo, xHi, nPos, M, tbl, delim, sep, inv, p0, sums, heads, maps, list, cap, fieldMask, sepMask);
}
extern "C" __global__ void __launch_bounds__(256) zra_cut_keep_class_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const ClassTable* tbl, u32 delim,
                                                                            u32 sep, u32 inv, u64 p0, const CSum* sums, const CHead* heads, CMap* maps, Range* list,
                                                                            u64 cap, u64 fieldMask, u64 sepMask) {
  cut_keep<ClassTable>(win, xLo, xHi, nPos, M, tbl, delim, sep, inv, p0, sums, heads, maps, list, cap, fieldMask, sepMask);
}

// One workgroup. The tiles' kept positions become their packed offsets: an exclusive scan (zra_joblist.h's) behind the base the scan
// of this pass left in *out. Then (provisional tail): in a pass that is not the last, D stops in front of the record open at the
// pass's end, which begins behind the pass's last delimiter, and K is what lies behind D; in the last pass the record that ends at hi
// gets its delimiter and D is the packed size.
extern "C" __global__ void __launch_bounds__(1024) zra_cut_place_kernel(CMap* maps, u32 nTiles, const CState* in, CState* out, u32 lastPass, u8* dData, u64 dataCap,
                                                                        u32 delim) {
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  u64 v[1] = {0}, tot[1];
  for (u32 t = b0; t < b1; t++) v[0] += maps[t].total;
  block_excl_scan<1>(v, tot);
  const u64 base = out->base, end = base + tot[0];
  const u32 lastTile = (u32)out->lastTile;
  u64 at = base + v[0];
  for (u32 t = b0; t < b1; t++) {
    const u32 total = maps[t].total;
    maps[t].base = at;
    if (!lastPass && t + 1 == lastTile) { const u64 D = at + total - maps[t].tail; out->bytes = D; out->kept = end - D; }
    at += total;
  }
  if (tid == 0 && lastPass) {
    u64 D = end;
    if (out->tailSel) { if (D < dataCap) dData[D] = (u8)delim; D++; }
    out->bytes = D; out->kept = 0;
  }
  if (tid == 0 && !lastPass && lastTile == 0) { out->bytes = in->bytes; out->kept = end - in->bytes; }
}

// The compaction. A workgroup takes the count's tiles; a tile that keeps nothing or lies behind the capacity is skipped. The tile's
// own bytes (no halo) and its keep words go to LDS, two waves scan the 128 popcounts, and every lane stores the kept bytes of its
// positions at base + the keep flags in front of them, clamped to the capacity.
extern "C" __global__ void __launch_bounds__(256) zra_cut_copy_kernel(const u8* win, long long xLo, u64 nPos, const CMap* maps, u8* dData, u64 dataCap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ u64 sKeep[kKeepWords];
  __shared__ u32 sPre[kKeepWords], sHalf;
  const u32 tid = threadIdx.x;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  for (u32 b = blockIdx.x * kGroup, bEnd = min(tiles, b + kGroup); b < bEnd; b++) {
    const u64 base = maps[b].base;
    if (maps[b].total == 0 || base >= dataCap) continue;                     // (uniform in the workgroup)
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    __syncthreads();                                                         // (the tile in front is done with)
    const u32 d = stage_tile(win + xLo + (long long)t0, n, sTile);
    if (tid < kKeepWords) {                                                  // (waves 0 and 1, whole)
      const u64 w = tid * 64 < n ? maps[b].keep[tid] : 0;
      const u32 c = (u32)__popcll(w), incl = wave_incl_scan(c);
      sKeep[tid] = w; sPre[tid] = incl - c;
      if (tid == 63) sHalf = incl;
    }
    __syncthreads();
    for (u32 j = tid; j < n; j += 256) {
      const u64 w = sKeep[j >> 6];
      if (!((w >> (j & 63)) & 1)) continue;
      const u64 at = base + sPre[j >> 6] + (j >= kTile / 2 ? sHalf : 0) + (u32)__popcll(w & ((1ull << (j & 63)) - 1));
      if (at < dataCap) dData[at] = (u8)lds_word(sTile, d + j);
    }
  }
}

// =================================================================================================
// The kernel set of the cut for zra_record_scan.h's call path. tables: Table | CTotals | sums[tiles] | heads[tiles] | maps[tiles]
namespace {
// the extract's selector; no pattern at all selects every record (plain cut): no position hits, and the selection is the inverted one
struct CutSelect : LiteralSelect {
  bool compile(const RecordCall& c) {
    if (c.separator == c.delimiter || c.fieldMask == 0) return false;
    if (c.nPat) return LiteralSelect::compile(c);
    if ((c.mode & 1u) || (c.syntax & ~(zra_expr::kFoldCase | zra_expr::kClasses))) return false;
    inv = 1; M = pset.M = pset.mMin = 1;
    return true;
  }
  void build(uint8_t* dst, const RecordCall& c) const { if (c.nPat) LiteralSelect::build(dst, c); }   // (zeros: a table nothing matches)
};

// (fields) bit c: a separator with c separators in front of it in its record is kept: field c + 2 is chosen, and so is one in front
inline uint64_t separator_mask(uint64_t fieldMask) {
  uint64_t m = 0;
  for (uint32_t c = 0; c < 64; c++) {
    const uint32_t bit = std::min(c + 1, 63u);                               // field c + 2, the fields from 64 on sharing bit 63
    const uint64_t front = c >= 63 ? ~0ull : (1ull << (c + 1)) - 1;          // the fields 1 .. c + 1
    if (((fieldMask >> bit) & 1) && (fieldMask & front)) m |= 1ull << c;
  }
  return m;
}

struct CutKernels {
  using Sum = CSum; using Head = CHead; using Totals = CTotals;
  static constexpr size_t kMapBytes = sizeof(CMap);
  static constexpr bool kData = true;
  static void launch(hipStream_t s, const CutSelect& sel, const RecordCall& c, const zra_eng::ScanPass& ps, const RecordPass<CutKernels>& p, u32 parity) {
    const Table* const tbl = (const Table*)p.table;
    const ClassTable* const ctbl = (const ClassTable*)p.table;                // (one of the two, by the syntax word)
    const u32 delim = c.delimiter, sep = c.separator, inv = sel.inv, M = sel.M;
    const u64 fieldMask = c.fieldMask, sepMask = separator_mask(c.fieldMask);
    CMap* const maps = (CMap*)p.maps;
    const CState* const in = p.tot->st + parity;
    CState* const out = p.tot->st + (parity ^ 1);
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_cut_count_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, sep, inv, (u64)ps.p0, p.sums, p.tot);
    else
      hipLaunchKernelGGL(zra_cut_count_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, sep, inv, (u64)ps.p0, p.sums, p.tot);
    hipLaunchKernelGGL(zra_cut_scan_kernel, dim3(1), dim3(1024), 0, s, p.sums, p.tiles, p.heads, in, out, inv, (u32)ps.lastPass, (u64)p.hi, (u64)ps.p0, (u64)ps.nPos, p.list,
                       (u64)p.listCap);
    if (sel.pset.classes)
      hipLaunchKernelGGL(zra_cut_keep_class_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, ctbl, delim, sep, inv, (u64)ps.p0, p.sums, p.heads,
                         maps, p.list, (u64)p.listCap, fieldMask, sepMask);
    else
      hipLaunchKernelGGL(zra_cut_keep_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, ps.xHi, (u64)ps.nPos, M, tbl, delim, sep, inv, (u64)ps.p0, p.sums, p.heads, maps,
                         p.list, (u64)p.listCap, fieldMask, sepMask);
    hipLaunchKernelGGL(zra_cut_place_kernel, dim3(1), dim3(1024), 0, s, maps, p.tiles, in, out, (u32)ps.lastPass, c.dData, (u64)c.dataCap, delim);
    if (c.dataCap) hipLaunchKernelGGL(zra_cut_copy_kernel, dim3(p.groups), dim3(256), 0, s, p.win, ps.xLo, (u64)ps.nPos, maps, c.dData, (u64)c.dataCap);
  }
};
static_assert(sizeof(CState) == 96 && sizeof(CSum) == 32 && sizeof(CHead) == 32 && sizeof(CMap) == 1040, "the entries as the kernels index them");
}  // namespace

namespace zra_eng {
Status ScanImpl::cut(Engine& E, const RecordCall& c, ScanCacheView* cv) { return record_scan<CutSelect, CutKernels>(E, c, cv); }
}  // namespace zra_eng
