// zra_amd — the pattern table of the calls that look for several byte patterns in one pass over a staging window's plaintext
// (zra_msearch.hip: ZraHipSearchArchiveMulti; zra_grep.hip: ZraHipGrepArchive; zra_extract.hip: ZraHipExtractRecords): its layout in
// device memory and in LDS, the host code that builds it, and the device code that stages it and a tile of the window and tests one
// position. Included by those three files only (device code: a .hip translation unit).
//  (filter) a 65,536-bit table in LDS: bit (b0 | b1 << 8) is set iff some pattern begins with b0 and is one byte long or goes on with
//      b1. A position whose byte pair has no bit costs that one bit test; only a survivor is compared, against the patterns that begin
//      with its first byte (bucketed on the host). The position hi - 1 has no second byte: it is a survivor iff a 1-byte pattern
//      matches it. A survivor's hits are a 64-bit mask over the pattern indices.
#pragma once
#include "zra_host.h"
#include "zra_dev.h"
#include <algorithm>
#include <cstring>

using namespace zra_dev;

namespace {
constexpr u32 kMaxPattern = 256;          // ZRA_HIP_SEARCH_MAX_PATTERN
constexpr u32 kMaxPatterns = 64;          // ZRA_HIP_SEARCH_MAX_PATTERNS
constexpr u32 kMaxPatternBytes = 4096;    // ZRA_HIP_SEARCH_MAX_PATTERN_BYTES
// the tile of zra_search.hip: 8 KiB of start positions per trip of a 256-lane workgroup, a wave takes 2,048 consecutive ones
constexpr u32 kTile = 8192;
constexpr u32 kWavePos = kTile / 4;
constexpr u32 kWaveIters = kWavePos / 64;
constexpr u32 kGroup = 8;                 // consecutive tiles of one workgroup
// staged bytes: up to 15 in front (the 16-byte alignment of the first global load), the tile, M - 1 halo bytes, rounded up to 16; the
// compare reads whole words and may look up to 7 bytes beyond a pattern's end (masked off)
constexpr u32 kLdsWords = (kTile + kMaxPattern + 64) / 4;

// What the host makes of the patterns, as it lies in device memory and in LDS (13,376 bytes).
struct __attribute__((aligned(16))) Table {
  u32 filter[65536 / 32];
  u32 pat[(kMaxPatternBytes + 4 * kMaxPatterns) / 4];   // every pattern begins on a word; the bytes behind its end are zero
  u16 off[kMaxPatterns];                                 // pattern i: word index into pat
  u16 len[kMaxPatterns];
  u16 bucket[256];                                       // first byte b: the patterns order[bucket & 255 .. + (bucket >> 8))
  u8 order[kMaxPatterns];                                // pattern indices sorted by first byte
};
static_assert(sizeof(Table) % 16 == 0 && sizeof(Table) == 13376, "staged 16 bytes at a time");

// Rule 1 of both calls as far as the sizes go: 1 .. 64 patterns of 1 .. 256 bytes, 4,096 bytes in all. *M: the longest, *mMin: the shortest.
inline bool pattern_sizes_ok(const uint32_t* hSizes, size_t nPat, uint32_t* M, uint32_t* mMin) {
  if (nPat == 0 || nPat > kMaxPatterns) return false;
  uint32_t sum = 0;
  *M = 0; *mMin = kMaxPattern;
  for (size_t i = 0; i < nPat; i++) {
    if (hSizes[i] == 0 || hSizes[i] > kMaxPattern) return false;
    *M = std::max(*M, hSizes[i]); *mMin = std::min(*mMin, hSizes[i]); sum += hSizes[i];
  }
  return sum <= kMaxPatternBytes;
}

// The table of the nPat patterns laid end to end at hPat, into T (zeroed by the caller).
inline void build_table(Table& T, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat) {
  uint8_t* const pb = (uint8_t*)T.pat;
  uint32_t at = 0, first[257] = {0};
  const uint8_t* src = hPat;
  for (size_t i = 0; i < nPat; i++) {
    const uint32_t m = hSizes[i];
    std::memcpy(pb + at, src, m);
    T.off[i] = (u16)(at / 4); T.len[i] = (u16)m;
    for (uint32_t b1 = 0; b1 < 256; b1++) {
      if (m > 1 && b1 != src[1]) continue;
      const uint32_t bit = src[0] | b1 << 8;
      T.filter[bit >> 5] |= 1u << (bit & 31);
    }
    first[src[0] + 1]++;
    at += (m + 3) & ~3u; src += m;
  }
  for (int b = 0; b < 256; b++) { T.bucket[b] = (u16)(first[b] | first[b + 1] << 8); first[b + 1] += first[b]; }
  src = hPat;
  for (size_t i = 0; i < nPat; i++) { T.order[first[src[0]]++] = (u8)i; src += hSizes[i]; }
}

// the four bytes at byte index i of an LDS word array
__device__ __forceinline__ u32 lds_word(const u32* s, u32 i) {
  const u64 pair = ((u64)s[(i >> 2) + 1] << 32) | s[i >> 2];
  return (u32)(pair >> ((i & 3) * 8));
}

__device__ __forceinline__ void stage_table(const Table* tbl, Table* sT) {
  for (u32 c = threadIdx.x; c < sizeof(Table) / 16; c += 256) lds_st128((u8*)sT + 16 * (size_t)c, ((const uint4*)tbl)[c]);
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

// The patterns that occur at the position whose first byte is byte i of sTile, as a mask over their indices; avail = min(hi - p, 256)
// bytes of the range lie at and behind the position. *surv: (filter)'s survivor.
__device__ __forceinline__ u64 position_mask(const Table* sT, const u32* sTile, u32 i, u32 avail, bool* surv) {
  const u32 w = lds_word(sTile, i), pair = w & 0xFFFF;
  u64 mask = 0;
  *surv = avail >= 2 && ((sT->filter[pair >> 5] >> (pair & 31)) & 1);
  if (*surv || avail < 2) {
    const u32 bk = sT->bucket[w & 0xFF];
    for (u32 k = bk & 0xFF, e = k + (bk >> 8); k < e; k++) {
      const u32 pi = sT->order[k], m = sT->len[pi];
      if (m > avail) continue;
      const u32* const pw = sT->pat + sT->off[pi];
      bool hit = true;
      for (u32 q = 0; q < m; q += 4) {
        const u32 mm = m - q >= 4 ? 0xFFFFFFFFu : (1u << (8 * (m - q))) - 1;
        if ((lds_word(sTile, i + q) ^ pw[q >> 2]) & mm) { hit = false; break; }
      }
      if (hit) mask |= 1ull << pi;
    }
    if (avail < 2) *surv = mask != 0;
  }
  return mask;
}
}  // namespace
