// zra_amd — extract of a device-resident archive with regular expressions (zra_hip.h: ZraHipExtractRecordsRegex): the
// records the regex grep selects (zra_grep_regex.hip) WITH their bytes, packed as the extract packs them (zra_extract.hip): the text
// `grep -E` (and `-v`) prints, from the one decode pass that selects the records.
//
// Selection, (state), (count) and the driver with M = 1 are the regex grep's, word for word; (compaction), (look-ahead), (provisional
// tail) and (stores) are the extract's. Neither file is touched: the regex grep's helpers live in its anonymous namespace and are
// repeated here. What this call joins:
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
#include "zra_scan.h"
#include "zra_scan_tile.h"
#include "zra_regex.h"

namespace {
using zra_regex::Table;
constexpr u32 kGroup = 8;                                   // consecutive tiles of one workgroup, as the family's
struct __attribute__((aligned(16))) Range { u64 offset, size; };   // ZraHipContentRange

// (summary) without the map. sel: after the scan ALL the selected records that end in the tile; fsel (set by the scan): the record
// the first delimiter ends is selected
struct __attribute__((aligned(16))) SumR { u64 first, last; u32 bytes, sel; u8 has, tail, fsel, pad[5]; };
// what the scan makes of it for the copy: the list position of the tile's first record, the start of the record open at its head, the
// packed bytes in front of that record, that record's state at the tile's first byte, and (look-ahead)'s bit
struct __attribute__((aligned(16))) HeadR { u64 base, open, at; u32 state, look; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi; bytes: packed so far, (provisional tail)'s D
struct StateR { u64 start, state, sel, tail, bytes, pad[3]; };
struct TotalsR { StateR st[2]; u64 matches, delims, pad[6]; };

// the automaton in LDS: the class of every byte and the rows of the classes in use
struct Dfa { u8 classOf[256]; u8 next[256 * 64]; };

__device__ __forceinline__ void stage_dfa(const Table* tbl, Dfa* s, u32 classes) {
  const uint4* const g = (const uint4*)tbl;
  for (u32 c = threadIdx.x; c < 16 + classes * 4; c += 256) lds_st128((u8*)s + 16 * (size_t)c, g[c]);
}
__device__ __forceinline__ u32 tile_byte(const u32* sTile, u32 i) { return ((const u8*)sTile)[i]; }

// one lane's walk over the tile bytes [from, to) from state st
__device__ __forceinline__ u32 walk(const Dfa* D, const u32* sTile, u32 d, u32 from, u32 to, u32 st) {
#pragma unroll 2
  for (u32 j = from; j < to; j++) st = D->next[(u32)D->classOf[tile_byte(sTile, d + j)] * 64 + st];
  return st;
}

// The delimiter positions of a tile of n positions, in order, into sPos; returns their number (the same in every lane). sCnt[w]
// keeps wave w's number. A wave takes its 2,048 consecutive positions twice: to count, and behind the prefix over the waves to write.
__device__ __forceinline__ u32 compact_delims(const u32* sTile, u32 d, u32 n, u32 delim, u16* sPos, u32* sCnt) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  u32 mine = 0;
#pragma unroll 1
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    const u32 j = w0 + t * 64 + lane;
    mine += (u32)__popcll(__ballot(j < n && tile_byte(sTile, d + j) == delim));
  }
  if (lane == 0) sCnt[wave] = mine;
  __syncthreads();
  u32 at = 0, all = 0;
  for (u32 v = 0; v < 4; v++) { if (v < wave) at += sCnt[v]; all += sCnt[v]; }
#pragma unroll 1
  for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
    const u32 j = w0 + t * 64 + lane;
    const bool isD = j < n && tile_byte(sTile, d + j) == delim;
    const u64 dm = __ballot(isD);
    if (isD) sPos[at + (u32)__popcll(dm & ((1ull << lane) - 1))] = (u16)j;
    at += (u32)__popcll(dm);
  }
  __syncthreads();
  return all;
}
}  // namespace

// The run of a pass, its tiles and workgroups: zra_grepx_count_kernel. Per tile its summary -> sums[tile] and its map -> maps[tile].
extern "C" __global__ void __launch_bounds__(256) zra_extractx_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const Table* tbl, u32 delim, u32 inv,
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

// One workgroup. Forward, zra_grepx_scan_kernel with (summary)'s two fields: every lane reduces a run of consecutive tiles, the 1,024
// summaries are scanned in LDS, then the lane walks its run again from the front state: heads[t], sums[t].sel becomes ALL the
// selected records that end in tile t and sums[t].fsel says whether the first of them is one. The last lane ends the pass: in the
// last pass the record open at hi ends there (its list entry and its delimiter byte). Backward, zra_extract_scan_kernel's
// (look-ahead): the bit of the nearest following tile with a delimiter, or of the pass's end, reaches every tile's head.
extern "C" __global__ void __launch_bounds__(1024) zra_extractx_scan_kernel(SumR* sums, const u8* maps, u32 nTiles, HeadR* heads, const StateR* in, StateR* out,
                                                                            const Table* tbl, u32 inv, u32 lastPass, u64 hi, u64 p0, u64 nPos, Range* list, u64 cap,
                                                                            u8* dData, u64 dataCap, u32 delim, TotalsR* tot) {
  __shared__ __attribute__((aligned(16))) u32 sMap[1024 * 16];
  __shared__ u64 sFirst[1024], sLast[1024], sSel[1024], sBytes[1024];
  __shared__ u32 sLook[1024];
  __shared__ u8 sHas[1024], sTl[1024];
  __shared__ u32 sTailSel;
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  const u64 accept = tbl->accept;
  const u8* const myMap = (const u8*)(sMap + tid * 16);
  // ---- the lane's run. F starts as the identity
  u32 F[16];
#pragma unroll
  for (u32 w = 0; w < 16; w++) F[w] = 0x03020100u + 0x04040404u * w;
  u64 first = 0, last = 0, sel = 0, bytes = 0;
  u32 has = 0, tail = 0;
  for (u32 t = b0; t < b1; t++) {
    const SumR s = sums[t];
    const u8* const m = maps + (size_t)t * 64;
    if (has) {
      if (!s.has) { tail = m[tail]; continue; }
      const u32 j = ((u32)(accept >> m[tail]) & 1) ^ inv;
      sel += s.sel + j; bytes += s.bytes + (j ? s.first - last + 1 : 0);
      tail = s.tail; last = s.last;
      continue;
    }
#pragma unroll
    for (u32 w = 0; w < 16; w++) {
      const u32 a = F[w];
      F[w] = (u32)m[a & 0xFF] | (u32)m[(a >> 8) & 0xFF] << 8 | (u32)m[(a >> 16) & 0xFF] << 16 | (u32)m[a >> 24] << 24;
    }
    if (s.has) { has = 1; sel = s.sel; bytes = s.bytes; tail = s.tail; first = s.first; last = s.last; }
  }
#pragma unroll
  for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
  sFirst[tid] = first; sLast[tid] = last; sSel[tid] = sel; sBytes[tid] = bytes; sHas[tid] = (u8)has; sTl[tid] = (u8)tail;
  __syncthreads();
  // ---- the scan: A = the lanes in front (at tid - d), B = this lane
  for (u32 d = 1; d < 1024; d <<= 1) {
    const bool on = tid >= d;
    if (on) {
      const u32 a = tid - d;
      if (sHas[a]) {
        // A's map stands; B's acts on A's tail
        const u32 through = myMap[sTl[a]];
        if (has) {
          const u32 j = ((u32)(accept >> through) & 1) ^ inv;
          sel += sSel[a] + j; bytes += sBytes[a] + (j ? first - sLast[a] + 1 : 0);
        } else { has = 1; sel = sSel[a]; bytes = sBytes[a]; last = sLast[a]; tail = through; }
        first = sFirst[a];
#pragma unroll
        for (u32 w = 0; w < 16; w++) F[w] = sMap[a * 16 + w];
      } else {
#pragma unroll
        for (u32 w = 0; w < 16; w++) {
          const u32 x = sMap[a * 16 + w];
          F[w] = (u32)myMap[x & 0xFF] | (u32)myMap[(x >> 8) & 0xFF] << 8 | (u32)myMap[(x >> 16) & 0xFF] << 16 | (u32)myMap[x >> 24] << 24;
        }
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (u32 w = 0; w < 16; w++) sMap[tid * 16 + w] = F[w];
      sFirst[tid] = first; sLast[tid] = last; sSel[tid] = sel; sBytes[tid] = bytes; sHas[tid] = (u8)has; sTl[tid] = (u8)tail;
    }
    __syncthreads();
  }
  // ---- the front of this lane's run: the carried one, moved over the lanes in front
  u64 start = in->start, count = in->sel, at = in->bytes;
  u32 state = (u32)in->state, matched = 0;
  if (tid) {
    const u32 a = tid - 1;
    const u32 through = ((const u8*)(sMap + a * 16))[state];
    if (sHas[a]) {
      const u32 j = ((u32)(accept >> through) & 1) ^ inv;
      count += sSel[a] + j; at += sBytes[a] + (j ? sFirst[a] - start + 1 : 0);
      state = sTl[a]; start = sLast[a];
    } else state = through;
  }
  u32 look = 0;                                                              // 2: the run has a delimiter, 1: the record its first one ends is selected
  for (u32 t = b0; t < b1; t++) {
    const SumR s = sums[t];
    HeadR h; h.base = count; h.open = start; h.at = at; h.state = state; h.look = 0;
    heads[t] = h;
    const u32 through = maps[(size_t)t * 64 + state];
    if (s.has) {
      const u32 m = (u32)(accept >> through) & 1, j = m ^ inv;
      sums[t].sel = s.sel + j;
      sums[t].fsel = (u8)j;
      if (!look) look = 2 | j;
      matched += m; count += s.sel + j; at += s.bytes + (j ? s.first - start + 1 : 0);
      state = s.tail; start = s.last;
    } else state = through;
  }
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tl = 0;
    u32 tailSel = 1;                                                         // (provisional tail)
    if (lastPass) {
      tailSel = 0;
      if (start < hi) {
        tl = 1;
        const u32 m = (u32)(accept >> state) & 1;
        matched += m;
        if (m ^ inv) {
          tailSel = 1;
          if (count < cap) { Range r; r.offset = start; r.size = hi - start; list[count] = r; }
          const u64 end = at + (hi - start);
          if (end < dataCap) dData[end] = (u8)delim;
          count++; at = end + 1;
        }
      }
    }
    StateR o; o.start = start; o.state = state; o.sel = count; o.tail = tl; o.bytes = at; o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *out = o;
    sTailSel = tailSel;
  }
  if (matched) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)matched);
  // ---- (look-ahead)
  sLook[tid] = look;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {                                       // the nearest lane at or behind this one whose run has a delimiter
    const u32 o = tid + d < 1024 ? sLook[tid + d] : 0;
    __syncthreads();
    if (!(look & 2)) look = o;
    sLook[tid] = look;
    __syncthreads();
  }
  u32 carry = tid < 1023 ? sLook[tid + 1] : 0;
  carry = (carry & 2) ? carry & 1 : sTailSel;
  for (u32 t = b1; t-- > b0;) {
    const SumR s = sums[t];                                                  // (this lane's own stores above)
    const u64 tileEnd = p0 + min((u64)(t + 1) * kTile, nPos);
    heads[t].look = s.has && s.last == tileEnd ? 0 : carry;                  // (no position behind the tile's last delimiter)
    if (s.has) carry = s.fsel;
  }
}

// The count's workgroups redo the tiles that hold a byte of a selected record or a listed record in front of the capacities (the
// others are skipped; a workgroup without such a tile leaves at once).
extern "C" __global__ void __launch_bounds__(256) zra_extractx_copy_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, const Table* tbl, u32 delim, u32 inv,
                                                                           u64 p0, const SumR* sums, const HeadR* heads, Range* list, u64 cap, u8* dData, u64 dataCap) {
  constexpr u32 kSelBit = 0x8000u;                                           // in sPos: the record this delimiter ends is selected (a position is below 2^13)
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
    // ---- phase 1: the delimiters, and the selection bit of the record that delimiter k ends: record 0 goes on from the head's state
    const u32 nD = compact_delims(sTile, d, n, delim, sPos, sCnt);
    for (u32 k = tid; k < nD; k += 256) {
      const u32 from = k ? ((u32)sPos[k - 1] & 0x1FFFu) + 1 : 0, to = (u32)sPos[k];
      const u32 st = walk(&sD, sTile, d, from, to, k ? start : head.state);
      // Lane k + 1 may read sPos[k] for its `from` while this store is under way, with no barrier between: it masks the word with
      // 0x1FFF, the store is one 16-bit LDS write (ds_write_b16, never torn) and leaves those 13 bits as they are, so either value
      // it sees gives the same `from`. The bit itself is read behind the barrier below.
      if (((u32)(accept >> st) & 1) ^ inv) sPos[k] = (u16)(to | kSelBit);
    }
    __syncthreads();
    // ---- phase 2: the exclusive prefix. A lane takes `chunk` consecutive delimiters; the 256 lane sums are scanned by wave
    const u32 chunk = (nD + 255) / 256, k0 = min(nD, tid * chunk), k1 = min(nD, k0 + chunk);
    u32 mine = 0;
    for (u32 k = k0; k < k1; k++) {
      const u32 e = sPos[k];
      if (e & kSelBit) mine += 0x10000u + (k ? (e & 0x1FFFu) - ((u32)sPos[k - 1] & 0x1FFFu) : 0);
    }
    const u32 incl = wave_incl_scan(mine);
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    u32 run = incl - mine;
    for (u32 v = 0; v < wave; v++) run += sW[v];
    for (u32 k = k0; k < k1; k++) {
      sPre[k] = run;
      const u32 e = sPos[k];
      if (e & kSelBit) run += 0x10000u + (k ? (e & 0x1FFFu) - ((u32)sPos[k - 1] & 0x1FFFu) : 0);
    }
    if (tid == 255) sPre[nD] = sW[0] + sW[1] + sW[2] + sW[3];                // (lane 255's chunk is the last one, or empty)
    __syncthreads();
    // ---- phase 3: a lane per position. k = the delimiters in front of q = the record q lies in; q's record ends at delimiter k
    if (w0 >= n) continue;                                                   // (uniform in the wave; the barriers are at the loop's head)
    // the packed bytes of record 0, which began at head.open, when it is selected
    const u64 firstAdd = nD && (sPos[0] & kSelBit) ? pos0 + ((u32)sPos[0] & 0x1FFFu) - head.open + 1 : 0;
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
        else to = head.at + firstAdd + (sPre[k] & 0xFFFFu) + (q - (((u32)sPos[k - 1] & 0x1FFFu) + 1));
      }
      if (sel && to < dataCap) dData[to] = (u8)byte;
      if (sel && isD) {
        const u64 idx = head.base + (sPre[k] >> 16);
        if (idx < cap) {
          const u64 from = k ? pos0 + ((u32)sPos[k - 1] & 0x1FFFu) + 1 : head.open;
          Range r; r.offset = from; r.size = pos0 + q - from;
          list[idx] = r;
        }
      }
    }
  }
}

// =================================================================================================
namespace zra_eng {

Status Engine::extract_records_regex(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
                                     uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap,
                                     uint64_t* nRecords, uint8_t* dData, size_t dataCap, uint64_t* dataSize) {
  return ScanImpl::call(*this, kScanExtract, nRecords, dataSize, [&] {
    return ScanImpl::extract_regex(*this, dArc, arcSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                   hRecords, recordCap, nRecords, dData, dataCap, dataSize);
  });
}

// ScanImpl::grep_regex's steps with ScanImpl::extract's outputs: the statuses and their order are zra_hip.h's, ZraHipExtractRecordsRegex.
Status ScanImpl::extract_regex(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, uint8_t delimiter,
                               uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap, uint64_t* nRecords, uint8_t* dData,
                               size_t dataCap, uint64_t* dataSize, ScanCacheView* cv) {
  // ---- 1. arguments
  if (!nRecords || !dataSize || !hPat || !hSizes || (!dArc && arcSize) || (!hRecords && recordCap) || (!dData && dataCap) || (mode & ~1u)) return zerr(42);
  const size_t kTotals = sizeof(Table), kHead = kTotals + sizeof(TotalsR);
  static_assert(sizeof(Table) % 16 == 0 && sizeof(TotalsR) == 192 && sizeof(SumR) == 32 && sizeof(HeadR) == 32 && sizeof(Range) == 16 && offsetof(Table, next) == 256,
                "16-byte entries behind a 16-byte head; stage_dfa's chunks");
  std::vector<uint8_t> head;
  {
    zra_regex::Compiled C;
    if (!zra_regex::compile(hPat, hSizes, nPat, syntax, delimiter, &C)) return zerr(42);
    head.assign(kHead, 0);                                                   // (the totals go up as zeros, the state as "a record opens at lo" in the start state)
    std::memcpy(head.data(), &C.table, sizeof(Table));
    ((TotalsR*)(head.data() + kTotals))->st[0].state = C.table.start;
  }
  // ---- 2. overlap (with the archive, and with the arena of the handle the call goes through)
  if (dataCap && arcSize && (uintptr_t)dData < (uintptr_t)dArc + arcSize && (uintptr_t)dArc < (uintptr_t)dData + dataCap) return zerr(42);
  if (cv && cv->slots && dataCap && (uintptr_t)dData < (uintptr_t)cv->arena + (size_t)cv->slots * cv->h.frameSize && (uintptr_t)cv->arena < (uintptr_t)dData + dataCap)
    return zerr(42);
  const u32 inv = mode & 1u;
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 3. header: the statuses of ZraHipArchiveOpen, as the grep
  ArchiveView arc;
  { Status st = view(E, dArc, arcSize, cv, &arc); if (st.zra) return st; }
  // ---- 4. the range [lo, hi): every non-empty one is scanned
  uint64_t lo, hi;
  if (!scan_range(arc.U, offset, size, &lo, &hi)) return {kOutOfBounds, 0};
  uint64_t* const stats = E.callStats_[kScanExtract];
  if (hi == lo) { stats[0] = arc.frames; return ok(); }
  if (arc.fs == 0 || arc.frames == 0) return {kHeaderInvalid, 0};
  // ---- 5. the passes. tables: Table | Totals | sums[tiles] | heads[tiles] | maps[tiles]
  const ScanPlan P = scan_plan(arc.U, arc.fs, lo, hi, 1, 0, stagingBytes);
  const size_t listCap = (size_t)std::min<uint64_t>(recordCap, hi - lo);     // (no list is longer: a record per delimiter, or the one open at hi)
  ((TotalsR*)(head.data() + kTotals))->st[0].start = lo;
  uint32_t launches = 0;
  Status st = ScanImpl::passes(E, arc, P, &E.callMs_[kScanExtract], head.data(), kHead, kTotals, sizeof(TotalsR),
                               kHead + P.tilesMax * (sizeof(SumR) + sizeof(HeadR) + 64) + 64, listCap * sizeof(Range) + 64, true, [&](const ScanPass& ps) {
    uint8_t* const win = window(E), * const tb = E.scan_.tables.as<uint8_t>();
    const Table* const tbl = (const Table*)tb;
    TotalsR* const tot = (TotalsR*)(tb + kTotals);
    SumR* const sums = (SumR*)(tb + kHead);
    HeadR* const heads = (HeadR*)(sums + P.tilesMax);
    u8* const maps = (u8*)(heads + P.tilesMax);
    Range* const list = E.scan_.list.as<Range>();
    const uint32_t tiles = (uint32_t)((ps.nPos + kTile - 1) / kTile), groups = (tiles + kGroup - 1) / kGroup;
    hipLaunchKernelGGL(zra_extractx_count_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, (u32)delimiter, inv, (u64)ps.p0, sums, maps, tot);
    hipLaunchKernelGGL(zra_extractx_scan_kernel, dim3(1), dim3(1024), 0, s, sums, maps, tiles, heads, tot->st + (launches & 1), tot->st + ((launches + 1) & 1), tbl, inv,
                       (u32)ps.lastPass, (u64)hi, (u64)ps.p0, (u64)ps.nPos, list, (u64)listCap, dData, (u64)dataCap, (u32)delimiter, tot);
    if (listCap || dataCap)
      hipLaunchKernelGGL(zra_extractx_copy_kernel, dim3(groups), dim3(256), 0, s, win, ps.xLo, ps.xHi, (u64)ps.nPos, tbl, (u32)delimiter, inv, (u64)ps.p0, sums, heads, list,
                         (u64)listCap, dData, (u64)dataCap);
  }, &launches, cv);
  if (st.zra) return st;
  // ---- 6. the totals (they came back with the last synchronisation), then the list, once
  const TotalsR& h = *(const TotalsR*)(head.data() + kTotals);
  const StateR& fin = h.st[launches & 1];
  const uint64_t total = fin.sel, packed = fin.bytes;
  *nRecords = total;
  *dataSize = packed;
  if ((recordCap && total > recordCap) || packed > dataCap) return {kOutputTooSmall, 0};   // 7: the two words say what the call needs
  if (recordCap && total) {
    HIPCHK_CLR(hipMemcpyAsync(hRecords, E.scan_.list.p, (size_t)total * sizeof(Range), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  const uint64_t st8[8] = {arc.frames, decoded_frames(P, cv), decoded_bytes(P, cv), h.delims + fin.tail, total, packed, P.passes, h.matches};
  std::copy(st8, st8 + 8, stats);
  return ok();
}

}  // namespace zra_eng
