// zra_amd — the end of the two extracts' one-workgroup scan kernels (zra_extract.hip: zra_extract_scan_kernel; zra_extract_regex.hip:
// zra_extractx_scan_kernel), behind their forward halves: (provisional tail), the last lane's end of a pass, and (look-ahead), the
// reverse pass. Both conditions are described in zra_extract.hip. Device code, 1,024 lanes.
#pragma once
#include "zra_scan_tile.h"

namespace {
// (provisional tail) The end of a pass, by the last lane: start / idx / at = the open record's start, the list position and the packed
// offset behind the pass's tiles; selected: that record is, as far as it has come. In the last pass the record ends at hi: its list
// entry and its delimiter byte, *tail = 1 when there is such a record. Returns the bit of (look-ahead) for the pass's end: is the
// record open there copied (in every pass but the last: provisionally, always).
__device__ __forceinline__ u32 extract_pass_end(u32 lastPass, bool selected, u64 start, u64 hi, u64& idx, u64& at, u64& tail, Range* list, u64 cap, u8* dData,
                                                u64 dataCap, u32 delim) {
  tail = 0;
  if (!lastPass) return 1;
  if (start >= hi) return 0;
  tail = 1;
  if (!selected) return 0;
  if (idx < cap) { Range r; r.offset = start; r.size = hi - start; list[idx] = r; }
  const u64 end = at + (hi - start);
  if (end < dataCap) dData[end] = (u8)delim;
  idx++; at = end + 1;
  return 1;
}

// what (look-ahead) needs of tile t behind the forward half: has it a delimiter, is the record its first one ends selected, the
// content offset behind its last one
struct LookTile { bool has; u32 fsel; u64 last; };

// (look-ahead) look: 2 this lane's run of tiles [b0, b1) has a delimiter, 1 the record its first one ends is selected; tailSel:
// extract_pass_end's bit, the last lane's. heads[t].look becomes "the record open at tile t's tail is copied": the bit of the
// nearest following tile with a delimiter, or of the pass's end.
template <class Head, class Tile>
__device__ __forceinline__ void look_ahead(u32 look, u32 tailSel, u32 b0, u32 b1, u64 p0, u64 nPos, Head* heads, Tile tile) {
  __shared__ u32 sLook[1024];
  __shared__ u32 sTailSel;
  const u32 tid = threadIdx.x;
  if (tid == 1023) sTailSel = tailSel;
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
    const LookTile s = tile(t);                                              // (this lane's own stores in the forward half)
    const u64 tileEnd = p0 + min((u64)(t + 1) * kTile, nPos);
    heads[t].look = s.has && s.last == tileEnd ? 0 : carry;                  // (no position behind the tile's last delimiter)
    if (s.has) carry = s.fsel;
  }
}
}  // namespace
