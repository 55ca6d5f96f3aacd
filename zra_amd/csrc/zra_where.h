// zra_amd — the record predicate of the grep with clauses (zra_hip.h: ZraHipGrepArchiveWhere, ZraHipArchiveGrepWhere,
// ZraHipCheckRecordClauses): its rule-1 checks, the block the kernels take by value, and the test of one record's hit set.
// A record's hit set H has bit i when a match of pattern i starts inside the record. A clause {all, any, none} holds for H when
// (H & all) == all, any == 0 || (H & any) != 0, and (H & none) == 0; a record is selected when some clause holds, and the mode's invert
// bit complements that answer.
// Plain C++17, no HIP types and nothing of the engine: tools/model/where_check.cpp walks it on the CPU under the host sanitizers, and
// zra_grep_where.hip includes it for the device (where_selected is compiled for both sides there).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZRA_WHERE_FN __host__ __device__ __forceinline__
#else
#define ZRA_WHERE_FN inline
#endif

namespace zra_where {

constexpr uint32_t kMaxClauses = 8;       // ZRA_HIP_WHERE_MAX_CLAUSES
constexpr uint32_t kMaxPatterns = 64;     // ZRA_HIP_SEARCH_MAX_PATTERNS: a set is one 64-bit word

struct Clause { uint64_t all, any, none; };   // ZraHipRecordClause: bit i = pattern i

// What a kernel takes by value: the clauses as three columns, their number, the invert bit. The columns behind n are zero and never read.
struct Block {
  uint64_t all[kMaxClauses], any[kMaxClauses], none[kMaxClauses];
  uint32_t n, inv;
};
static_assert(sizeof(Block) == 200 && sizeof(Clause) == 24, "three columns of eight words, two 32-bit words");

// the patterns 0 .. nPatterns - 1 as a set
inline uint64_t full_set(size_t nPatterns) { return nPatterns >= 64 ? ~0ull : (1ull << nPatterns) - 1; }

// Rule 1 as far as the clauses go: 1 .. 8 of them, no bit at or above nPatterns (1 .. 64), and no pattern both demanded and forbidden
// by one clause (such a clause never holds: a mistake, not a predicate).
inline bool clauses_ok(const Clause* c, size_t nClauses, size_t nPatterns) {
  if (!c || nClauses == 0 || nClauses > kMaxClauses || nPatterns == 0 || nPatterns > kMaxPatterns) return false;
  const uint64_t outside = ~full_set(nPatterns);
  for (size_t i = 0; i < nClauses; i++) {
    if ((c[i].all | c[i].any | c[i].none) & outside) return false;
    if ((c[i].all & c[i].none) || (c[i].any & c[i].none)) return false;
  }
  return true;
}

// the block of checked clauses
inline Block make_block(const Clause* c, size_t nClauses, bool invert) {
  Block b = {};
  for (size_t i = 0; i < nClauses; i++) { b.all[i] = c[i].all; b.any[i] = c[i].any; b.none[i] = c[i].none; }
  b.n = (uint32_t)nClauses; b.inv = invert ? 1u : 0u;
  return b;
}

// Is the record with hit set H selected. The loop runs over the n clauses in use and reads a clause's three words where it tests
// them: in a kernel the block stays in the argument segment and costs three scalar loads per clause, not 50 registers for the call.
ZRA_WHERE_FN bool where_selected(const Block& b, uint64_t H) {
  bool some = false;
  for (uint32_t i = 0; i < b.n; i++)
    some |= (H & b.all[i]) == b.all[i] && (b.any[i] == 0 || (H & b.any[i]) != 0) && (H & b.none[i]) == 0;
  return some != (b.inv != 0);
}

}  // namespace zra_where
