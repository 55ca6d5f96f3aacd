// zra_amd — the tile of the range scans (zra_search.hip, through zra_patterns.h zra_msearch.hip, zra_grep.hip, zra_grep_where.hip and
// zra_extract.hip, through zra_regex_tile.h the two regex files): how many start positions a workgroup takes, how a tile of the
// staging window's plaintext gets into LDS and how a lane reads it there; the record scans' list entry.
// Device code: included by .hip translation units only.
#pragma once
#include "zra_host.h"
#include "zra_dev.h"

using namespace zra_dev;

namespace {
constexpr u32 kMaxPattern = zra_eng::kScanMaxPattern;   // ZRA_HIP_SEARCH_MAX_PATTERN
// Start positions of one workgroup. 8 KiB: the halo of up to 255 bytes a tile stages beyond its own positions is then 3 % of its global
// reads, tile + halo take 8.5 KiB of LDS (a CU holds its 8 workgroups of 256 lanes with room to spare), 1 GiB of plaintext is 131,072
// workgroups, and the per-tile tables cost well under 1 % of the window.
constexpr u32 kTile = zra_eng::kScanTile;
constexpr u32 kWavePos = kTile / 4;       // consecutive start positions of one wave
constexpr u32 kWaveIters = kWavePos / 64;
// staged bytes: up to 15 in front (the 16-byte alignment of the first global load), the tile, M - 1 halo bytes, rounded up to 16; the
// compare reads whole words and may look up to 7 bytes beyond a pattern's end (masked off)
constexpr u32 kLdsWords = (kTile + kMaxPattern + 64) / 4;
constexpr u32 kGroup = 8;                 // consecutive tiles of one workgroup, in every call but the single search
struct __attribute__((aligned(16))) Range { u64 offset, size; };   // a list entry of the record scans: ZraHipContentRange

// the four bytes at byte index i of an LDS word array
__device__ __forceinline__ u32 lds_word(const u32* s, u32 i) {
  const u64 pair = ((u64)s[(i >> 2) + 1] << 32) | s[i >> 2];
  return (u32)(pair >> ((i & 3) * 8));
}

// `bytes` bytes at src -> sTile, 16-byte global loads from the aligned address at or below src: at most 15 bytes in front (inside the
// carry area) and 15 behind (inside the run or the buffer's slack). Returns the index of src's first byte in sTile.
__device__ __forceinline__ u32 stage_tile(const u8* src, u32 bytes, u32* sTile) {
  const u32 d = (u32)((size_t)src & 15);
  const uint4* const g = (const uint4*)(src - d);
  const u32 chunks = (d + bytes + 15) >> 4;
  for (u32 c = threadIdx.x; c < chunks; c += 256) lds_st128((u8*)sTile + 16 * (size_t)c, g[c]);
  return d;
}
}  // namespace
