// zra_amd — the planning pieces of the device-archive calls (device only): a workgroup of 1024 lanes turns "some frames of a pass"
// into an ordered job list, and per-item counts into list positions.
//   block_rank<N>        a lane's rank among the lanes in front of it, for N predicates at once, and the workgroup's totals
//   emit_job             the job triple of one frame: compressed span, expected size, destination
//   block_excl_scan<N>   exclusive scan of N u64 columns over the workgroup; scan_in_place: a table of any length, in chunks of 2048
//                        behind a running total
//   split_by_residency   a pass through an archive handle: decode jobs for the frames that are not resident, copy entries for the rest
// No atomic decides a position anywhere: ranks and bases are prefix counts in thread order, so the lists are in item order.
// Every piece synchronises the workgroup: EVERY lane of a workgroup of exactly 1024 has to call it, from uniform control flow, a lane
// without an item with its predicates false / its values zero. Each keeps its own LDS table and ends with the barrier that frees it:
// a call may follow another at once, also in a loop. The caller keeps the running bases across chunks.
#pragma once
#include "zra_dev.h"

namespace zra_dev {

constexpr u32 kFrameNotResident = 0xFFFFFFFFu;   // a handle's frame -> arena slot table: the frame is not in the cache

// the wave's number in its workgroup, as the scalar it is
__device__ __forceinline__ u32 wave_id() { return (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// inclusive prefix sum over each row of 16 consecutive lanes (the wave tables below have 16 entries, one per wave of the workgroup):
// four DPP row shifts that read zero in front of the row's first lane, no LDS and no shuffle. Every lane of the wave has to be active.
template <int S>
__device__ __forceinline__ u32 row_shr(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + S, 0xF, 0xF, true); }
template <int S>
__device__ __forceinline__ u64 row_shr(u64 v) { return (u64)row_shr<S>((u32)v) | (u64)row_shr<S>((u32)(v >> 32)) << 32; }
template <typename T>
__device__ __forceinline__ T scan16(T v) {
  v += row_shr<1>(v); v += row_shr<2>(v); v += row_shr<4>(v); v += row_shr<8>(v);
  return v;
}

// v of lane l of the wave (l the same in every lane), as a scalar
__device__ __forceinline__ u32 lane_value(u32 v, u32 l) { return (u32)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ u64 lane_value(u64 v, u32 l) { return (u64)lane_value((u32)v, l) | (u64)lane_value((u32)(v >> 32), l) << 32; }

// rank[c] = the lanes in front of this one (thread order) whose p[c] holds, total[c] = all lanes whose p[c] holds: ballot and popcount
// per wave, a table of N x 16 wave counts in LDS, one barrier pair for all N.
template <int N>
__device__ __forceinline__ void block_rank(const bool (&p)[N], u32 (&rank)[N], u32 (&total)[N]) {
  __shared__ u32 sCnt[N][16];
  const u32 lane = threadIdx.x & 63, wave = wave_id();
#pragma unroll
  for (int c = 0; c < N; c++) {
    const u64 m = __ballot(p[c]);
    rank[c] = (u32)__popcll(m & ((1ull << lane) - 1));                // (in the wave, taken now: no mask lives across the barrier)
    if (lane == 0) sCnt[c][wave] = (u32)__popcll(m);
  }
  __syncthreads();
  // (every lane reads ONE count, that of wave lane & 15, and the 16 are scanned across lanes: a walk over all 16 in every lane keeps
  //  them and the 16 `w < wave` masks in scalar registers, which a kernel with many arguments does not have)
#pragma unroll
  for (int c = 0; c < N; c++) {
    const u32 x = sCnt[c][lane & 15], inc = scan16(x);
    rank[c] += lane_value(inc - x, wave);
    total[c] = lane_value(inc, 15);
  }
  __syncthreads();                                                    // (sCnt of the next call)
}

// Job `job` decodes frame f of an archive with frames of fs bytes and U bytes of content: its seek-table span, taken as the table says
// (the decoder refuses a span that runs backwards or leaves the body), has to regenerate that frame's share of the content, and lands
// in slot `slot` of the staging window. outOff == nullptr: the destinations are written elsewhere.
__device__ __forceinline__ void emit_job(const u8* table, u64 f, u64 fs, u64 U, size_t job, u64 slot, u64* frameOff, u64* outOff, u32* expect) {
  frameOff[2 * job] = seek_entry(table, f); frameOff[2 * job + 1] = seek_entry(table, f + 1);
  expect[job] = (u32)frame_expect(f, fs, U);
  if (outOff) outOff[job] = slot * fs;
}

// inclusive prefix sum over the 64 lanes of a wave: the four rows scanned, then the totals of the rows in front added
__device__ __forceinline__ u64 wave_incl_scan64(u64 v, int lane) {
  v = scan16(v);
  const u64 r0 = lane_value(v, 15), r1 = lane_value(v, 31), r2 = lane_value(v, 47);
  return v + (lane >= 16 ? r0 : 0) + (lane >= 32 ? r1 : 0) + (lane >= 48 ? r2 : 0);
}

// v[c] becomes the sum of column c over the lanes in front of this one, tot[c] the sum over all lanes: an inclusive scan per wave and
// 16 wave sums per column in LDS.
template <int N>
__device__ __forceinline__ void block_excl_scan(u64 (&v)[N], u64 (&tot)[N]) {
  __shared__ u64 sSum[N][16];
  const u32 wave = wave_id(); const int lane = (int)(threadIdx.x & 63);
  u64 inc[N];
#pragma unroll
  for (int c = 0; c < N; c++) {
    inc[c] = wave_incl_scan64(v[c], lane);
    if (lane == 63) sSum[c][wave] = inc[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; c++) {                                       // (one wave sum per lane, scanned across lanes, as in block_rank)
    const u64 x = sSum[c][lane & 15], s = scan16(x);
    v[c] = lane_value(s - x, wave) + inc[c] - v[c]; tot[c] = lane_value(s, 15);
  }
  __syncthreads();                                                    // (sSum of the next call)
}

// A table of n items of N columns becomes, in place, totIn[] + the exclusive prefixes of its columns, for i = 0 .. n: entry n is behind
// all items (an item's own counts are the difference to the next entry), and totOut[] = that entry (nullptr: not wanted). totIn
// nullptr: zeros. 2048 items at a time behind a running total, a lane takes two neighbours: half the scans and barriers per item. totIn
// and totOut may be the same words.
template <int N>
__device__ __forceinline__ void scan_in_place(u64* tab, u32 n, const u64* totIn, u64* totOut) {
  u64 run[N];
#pragma unroll
  for (int c = 0; c < N; c++) run[c] = totIn ? totIn[c] : 0;
  for (u32 base = 0; base < n; base += 2048) {
    const u32 i = base + 2 * threadIdx.x;                            // (no overflow: a launch has far fewer than 2^32 - 2048 items)
    u64* const e = tab + N * (size_t)i;
    u64 a[N], v[N], tot[N];
#pragma unroll
    for (int c = 0; c < N; c++) { a[c] = i < n ? e[c] : 0; v[c] = a[c] + (i + 1 < n ? e[N + c] : 0); }
    block_excl_scan<N>(v, tot);
#pragma unroll
    for (int c = 0; c < N; c++) {
      if (i < n) e[c] = run[c] + v[c];
      if (i + 1 < n) e[N + c] = run[c] + v[c] + a[c];
      run[c] += tot[c];
    }
  }
  if (threadIdx.x == 0)
    for (int c = 0; c < N; c++) { tab[N * (size_t)n + c] = run[c]; if (totOut) totOut[c] = run[c]; }
}

// A pass through an archive handle: entry k of [0, n) is frame frameOf(k) in slot k of the staging window, entries ascending by frame.
// A frame that is not resident (cacheSlotOf, readable for nFrames frames) gets a decode job, ranked in entry order from job 0
// (emit_job). A resident one gets a copy entry {k, arena slot, length, frame}, ranked the same way (zra_upd_stage_cached_kernel's
// format). counts = {jobs, copies, bytes the jobs are to regenerate (low, high word)}. Nothing of the cache is written.
template <typename FrameOf>
__device__ __forceinline__ void split_by_residency(u32 n, FrameOf frameOf, const u32* cacheSlotOf, u32 nFrames, const u8* table, u64 fs, u64 U, u64* frameOff,
                                                   u64* outOff, u32* expect, u32* copies, u32* counts) {
  u32 jobBase = 0, copyBase = 0;
  u64 bytes[1] = {0}, allBytes[1];
  for (u32 base = 0; base < n; base += 1024) {
    const u32 k = base + threadIdx.x;
    const bool in = k < n;
    const u64 f = in ? (u64)frameOf(k) : 0;
    const u32 cs = in && f < nFrames ? cacheSlotOf[f] : kFrameNotResident;
    const bool p[2] = {in && cs == kFrameNotResident, in && cs != kFrameNotResident};
    u32 rank[2], total[2];
    block_rank<2>(p, rank, total);
    if (p[0]) {
      emit_job(table, f, fs, U, jobBase + rank[0], k, frameOff, outOff, expect);
      bytes[0] += frame_expect(f, fs, U);
    }
    if (p[1]) {
      u32* e = copies + 4 * (size_t)(copyBase + rank[1]);
      e[0] = k; e[1] = cs; e[2] = (u32)frame_expect(f, fs, U); e[3] = (u32)f;
    }
    jobBase += total[0]; copyBase += total[1];
  }
  block_excl_scan<1>(bytes, allBytes);
  if (threadIdx.x == 0) { counts[0] = jobBase; counts[1] = copyBase; counts[2] = (u32)allBytes[0]; counts[3] = (u32)(allBytes[0] >> 32); }
}

}  // namespace zra_dev
