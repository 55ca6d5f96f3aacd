// zra_amd — the trip of the two record scans with a predicate (zra_grep_where.hip: ZraHipGrepArchiveWhere; zra_extract_where.hip:
// ZraHipExtractRecordsWhere): a lane's hit mask beside the two ballots, and the sets of one trip of 64 positions, (trip) of
// zra_grep_where.hip. Device code: included by those two translation units.
#pragma once
#include "zra_patterns.h"
#include "zra_where.h"

namespace {
using zra_where::Block;
using zra_where::where_selected;

// The flags of trip t of a wave as zra_patterns.h's trip_flags gives them, and the lane's own hit mask.
template <class TB>
__device__ __forceinline__ u64 trip_masks(const TB* sT, const u32* sTile, u32 d, u32 j, u32 n, long long toHi, u32 delim, u64* dm, u64* hm, u32* pairs) {
  bool isD = false;
  u64 mask = 0;
  if (j < n) {
    isD = (lds_word(sTile, d + j) & 0xFF) == delim;
    bool surv;
    mask = position_mask(sT, sTile, d + j, (u32)min(toHi - (long long)j, (long long)kMaxPattern), &surv);
    *pairs += (u32)__popcll(mask);
  }
  *dm = __ballot(isD);
  *hm = __ballot(mask != 0);
  return mask;
}

__device__ __forceinline__ u64 lane_word(u64 v, int l) {   // l is uniform
  return (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, l) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l) << 32;
}

// (trip) The number of hitting lanes from which a trip takes the segmented scan; below it, the per-pattern ballots. Bring-up
// (-DZRA_GREPW_SCAN_FROM=n through ZRA_EXTRA_CFLAGS): 0 = the scan always, 65 = the ballots always, the two columns of
// profiles/grep_where.md.
#ifndef ZRA_GREPW_SCAN_FROM
#define ZRA_GREPW_SCAN_FROM 8
#endif
constexpr u32 kScanFrom = ZRA_GREPW_SCAN_FROM;

// A six-step segmented inclusive OR scan over the lanes: a lane takes the value d lanes below while no delimiter lies between the
// two. A delimiter lane's own mask is zero, so its scanned value is its set; the first delimiter's is front, lane 63's is behind.
__device__ __forceinline__ u64 seg_scan(u64 m, u64 dm, u32 lane) {
  const u64 dBelow = dm & ((1ull << lane) - 1);
  u64 acc = m;
  for (u32 d = 1; d < 64; d <<= 1) {
    const u64 v = __shfl_up(acc, d);
    if (lane >= d && !(dBelow >> (lane - d))) acc |= v;
  }
  return acc;
}

// the OR of the masks of the lanes of hm (not zero); a lane number from a ballot is uniform
__device__ __forceinline__ u64 trip_union(u64 m, u64 hm, u32 lane) {
  if ((u32)__popcll(hm) >= kScanFrom) return lane_word(seg_scan(m, 0, lane), 63);
  u64 U = 0;
  for (u64 r = hm; r; r &= r - 1) U |= lane_word(m, __builtin_ctzll(r));
  return U;
}

// A trip with a delimiter and a hit: H = the lane's set (what hit in the lanes of seg), front / behind = what hit in front of the
// first delimiter and behind the last one
__device__ __forceinline__ void trip_sets(u64 m, u64 hm, u64 dm, u32 lane, u32 first, u32 last, u64 seg, u64* H, u64* front, u64* behind) {
  if ((u32)__popcll(hm) >= kScanFrom) {
    const u64 acc = seg_scan(m, dm, lane);
    *H = acc; *front = lane_word(acc, (int)first); *behind = last < 63 ? lane_word(acc, 63) : 0;
    return;
  }
  const u64 frontLanes = (1ull << first) - 1, behindLanes = last < 63 ? ~0ull << (last + 1) : 0;
  for (u64 U = trip_union(m, hm, lane); U; U &= U - 1) {
    const u32 i = (u32)__builtin_ctzll(U);
    const u64 b = __ballot((m >> i) & 1);                                    // the lanes where pattern i hit
    if (b & seg) *H |= 1ull << i;
    if (b & frontLanes) *front |= 1ull << i;
    if (b & behindLanes) *behind |= 1ull << i;
  }
}
}  // namespace
