// zra_amd — the pattern table of the calls that look for several byte patterns in one pass over a staging window's plaintext
// (zra_msearch.hip: ZraHipSearchArchiveMulti; zra_grep.hip: ZraHipGrepArchive; zra_extract.hip: ZraHipExtractRecords): its layout in
// device memory and in LDS, the host code that builds it, and the device code that stages it and a tile of the window and tests one
// position; for the calls that cut the range into records, the two flags of a position. Included by those files, zra_grep_where.hip
// and, for the selectors of zra_record_scan.h, the two regex files (device code: a .hip translation unit). The tile, its staging and
// the list entry: zra_scan_tile.h, shared with zra_search.hip.
//  (filter) a 65,536-bit table in LDS: bit (b0 | b1 << 8) is set iff some pattern begins with b0 and is one byte long or goes on with
//      b1. A position whose byte pair has no bit costs that one bit test; only a survivor is compared, against the patterns that begin
//      with its first byte (bucketed on the host). The position hi - 1 has no second byte: it is a survivor iff a 1-byte pattern
//      matches it. A survivor's hits are a 64-bit mask over the pattern indices.
//  (classes) the calls with a syntax word (zra_pattern_expr.h: every element of a pattern is a byte set) use ClassTable and
//      position_mask's overload for it, through the same kernel bodies: two 256-entry tables of 64-bit pattern masks, indexed by the position's
//      first and second byte, are exact on two elements; their AND is the candidates, each verified element by element from the third.
#pragma once
#include "zra_scan.h"
#include "zra_scan_tile.h"
#include "zra_pattern_expr.h"
#include <algorithm>
#include <cstring>

namespace {
constexpr u32 kMaxPatterns = 64;          // ZRA_HIP_SEARCH_MAX_PATTERNS
constexpr u32 kMaxPatternBytes = 4096;    // ZRA_HIP_SEARCH_MAX_PATTERN_BYTES

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

// Rule 1 of the three calls as far as the sizes go: 1 .. 64 patterns of 1 .. 256 bytes, 4,096 bytes in all. *M: the longest, *mMin: the shortest.
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

// Rule 1 of the grep and the extract: the sizes, and no pattern holds the delimiter, so that an occurrence lies inside one record.
inline bool record_patterns_ok(const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint8_t delimiter, uint32_t* M, uint32_t* mMin) {
  if (!pattern_sizes_ok(hSizes, nPat, M, mMin)) return false;
  size_t bytes = 0;
  for (size_t i = 0; i < nPat; i++) bytes += hSizes[i];
  return std::memchr(hPat, delimiter, bytes) == nullptr;
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

// (classes) What the host makes of compiled expressions, as it lies in device memory and in LDS (13,584 bytes).
struct __attribute__((aligned(16))) ClassTable {
  u64 first[256];                 // byte b: the patterns whose element 0 admits b
  u64 second[256];                // byte b: the patterns whose element 1 admits b; a one-element pattern has its bit set everywhere
  u32 member[256];                // byte b: bit c is set iff b is in counted set c (ZRA_HIP_PATTERN_MAX_SETS = 32)
  u16 elem[kMaxPatternBytes];     // zra_expr's codes: a byte, a letter in either case, or a counted set's number
  u16 off[kMaxPatterns];          // pattern i: elem[off .. off + len)
  u16 len[kMaxPatterns];
  u64 one, pad;                   // the one-element patterns
};
static_assert(sizeof(ClassTable) % 16 == 0 && sizeof(ClassTable) == 13584 && zra_expr::kMaxSets == 32 && zra_expr::kMaxElementsAll == kMaxPatternBytes, "staged 16 bytes at a time");

inline void build_class_table(ClassTable& T, const zra_expr::Compiled& C) {
  std::copy(C.codes.begin(), C.codes.end(), T.elem);
  for (size_t i = 0; i < C.len.size(); i++) {
    const zra_expr::ByteSet* const e = &C.elems[C.off[i]];
    T.off[i] = (u16)C.off[i]; T.len[i] = (u16)C.len[i];
    if (C.len[i] == 1) T.one |= 1ull << i;
    for (uint32_t b = 0; b < 256; b++) {
      if (e[0].has(b)) T.first[b] |= 1ull << i;
      if (C.len[i] == 1 || e[1].has(b)) T.second[b] |= 1ull << i;
    }
  }
  for (size_t c = 0; c < C.sets.size(); c++)
    for (uint32_t b = 0; b < 256; b++) if (C.sets[c].has(b)) T.member[b] |= 1u << c;
}

// Rule 1 of the three calls as far as the patterns go, for every syntax word, and what the passes need of the patterns: their lengths
// (in elements), the longest, the shortest, and the table that heads the call's device tables. syntax 0 is the literal calls' path,
// byte for byte: Table and the literal kernels; any other accepted word compiles expressions and takes ClassTable and the class kernels.
struct PatternSet {
  bool classes = false;
  uint32_t M = 0, mMin = kMaxPattern;
  const uint32_t* len = nullptr;   // per pattern, in elements
  zra_expr::Compiled C;
  size_t table_bytes() const { return classes ? sizeof(ClassTable) : sizeof(Table); }
};
// delimiter: the grep's and the extract's, -1: none (the multi search). hPat and hSizes are not null.
inline bool patterns_ok(const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, int delimiter, PatternSet* ps) {
  if (syntax == 0) {
    ps->len = hSizes;
    return delimiter < 0 ? pattern_sizes_ok(hSizes, nPat, &ps->M, &ps->mMin) : record_patterns_ok(hPat, hSizes, nPat, (uint8_t)delimiter, &ps->M, &ps->mMin);
  }
  if (!zra_expr::compile(hPat, hSizes, nPat, syntax, delimiter, &ps->C)) return false;
  ps->classes = true; ps->M = ps->C.M; ps->mMin = ps->C.mMin; ps->len = ps->C.len.data();
  return true;
}
// the table into dst (table_bytes() zeroed bytes)
inline void build_pattern_table(void* dst, const PatternSet& ps, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat) {
  if (ps.classes) build_class_table(*(ClassTable*)dst, ps.C); else build_table(*(Table*)dst, hPat, hSizes, nPat);
}

template <class TB>
__device__ __forceinline__ void stage_table(const TB* tbl, TB* sT) {
  for (u32 c = threadIdx.x; c < sizeof(TB) / 16; c += 256) lds_st128((u8*)sT + 16 * (size_t)c, ((const uint4*)tbl)[c]);
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

// (classes) does the element with this code admit the byte b
__device__ __forceinline__ bool admits(const ClassTable* sT, u32 code, u32 b) {
  return code < zra_expr::kCodePair ? b == code : code < zra_expr::kCodeSet ? (b | 0x20) == (code & 0xFF) : ((sT->member[b] >> (code & 31)) & 1) != 0;
}

// (classes) position_mask over a ClassTable. The candidates are first[b0] & second[b1], exact on two elements (with avail < 2: first[b0]
// of the one-element patterns); *surv: there is one. A candidate is verified from element 2 and leaves at the first miss; elements 2
// and 3, where most candidates leave, take their bytes from the word the candidates came from. Only elements q < m <= avail are
// tested, so no tile byte is read that the literal compare does not read.
__device__ __forceinline__ u64 position_mask(const ClassTable* sT, const u32* sTile, u32 i, u32 avail, bool* surv) {
  const u32 w = lds_word(sTile, i);
  u64 cand = sT->first[w & 0xFF] & (avail >= 2 ? sT->second[(w >> 8) & 0xFF] : sT->one);
  *surv = cand != 0;
  u64 mask = 0;
  for (; cand; cand &= cand - 1) {
    const u32 pi = (u32)__builtin_ctzll(cand), m = sT->len[pi];
    if (m > avail) continue;
    const u16* const el = sT->elem + sT->off[pi];
    bool hit = m < 3 || admits(sT, el[2], (w >> 16) & 0xFF);
    if (hit && m > 3) hit = admits(sT, el[3], w >> 24);
    for (u32 q = 4; q < m && hit; q++) {
      const u32 at = i + q;
      hit = admits(sT, el[q], (sTile[at >> 2] >> ((at & 3) * 8)) & 0xFF);
    }
    if (hit) mask |= 1ull << pi;
  }
  return mask;
}

// ---- the grep and the extract: a position's two flags (the list entry, Range, is zra_scan_tile.h's)
constexpr u64 kHitBit = 1ull << 63;                                // the hit bit of the record open at a tile's head, beside its start

// The two ballots of trip t of a wave (tile position j = w0 + 64 t + lane; d = the index of the tile's first byte in sTile; toHi = the
// bytes of the range at and behind the tile's first position): `delimiter` (its byte) and `hit` (a match starts here), and the lane's
// matches as (position, pattern) pairs.
template <class TB>
__device__ __forceinline__ void trip_flags(const TB* sT, const u32* sTile, u32 d, u32 j, u32 n, long long toHi, u32 delim, u64* dm, u64* hm, u32* pairs) {
  bool isD = false, hit = false;
  if (j < n) {
    isD = (lds_word(sTile, d + j) & 0xFF) == delim;
    bool surv;
    const u64 mask = position_mask(sT, sTile, d + j, (u32)min(toHi - (long long)j, (long long)kMaxPattern), &surv);
    hit = mask != 0;
    *pairs += (u32)__popcll(mask);
  }
  *dm = __ballot(isD);
  *hm = __ballot(hit);
}
}  // namespace
