// zra_amd — the summary algebra of the regex grep with context records (zra_grep_regex_context.hip): zra_context.h's
// Ctx carried through DESIGN.md §28's run summary in the place of its count. Compiles on the host as well, so that
// tools/model/regex_context_check.cpp folds random texts through the very functions the kernels call.
//  (summary) a run of positions reduces to Run = {has a delimiter, tail, last, c} and a map F of 64 states kept apart (the kernels hold
//      it as 16 words of registers, the host as 64 bytes): F[s] the state reached from s over the bytes in front of the run's first
//      delimiter (without one: over the whole run), tail the state of the record open behind the last delimiter (from the start state),
//      last the position behind the last delimiter, c the Ctx of the records that end inside the run APART from the first. Those
//      records begin at the start state, so which of them are selected does not depend on what lies in front of the run: Ctx's "as if
//      no record outside the run were selected" holds for them whatever the run is joined to.
//  (combine) A followed by B, `through` = B.F[A.tail]. B without a delimiter: A.tail = through if A has one, else the maps compose
//      (A.F = B.F o A.F, the caller's, combine() returns true); A without one: B, under the composed map; both: the record that B's
//      first delimiter ends is selected iff accept(through) ^ invert, and A.c = A.c + single(that) + B.c. Associative; the run of no
//      positions {0, 0, 0, {}} under the identity map is its identity. Only delimiter-free runs compose maps.
//  (front) what lies in front of a point of the stream: the start and the DFA state of the record open there and the Ctx of every
//      record that has ended. advance() moves it over a run, `through` = F[front.state]: this is where a run's first record is resolved.
//      finish() ends the record open at the range's end.
#pragma once
#include "zra_context.h"

namespace zra_rxc {
using zra_ctx::Ctx;

struct Run { uint64_t last; uint32_t has, tail; Ctx c; };
struct Front { uint64_t start; uint32_t state; Ctx c; };

ZRA_CTX_FN uint32_t accepts(uint64_t accept, uint32_t state) { return (uint32_t)(accept >> state) & 1u; }
// the selection bit of a record that ends in `state`
ZRA_CTX_FN uint32_t selected(uint64_t accept, uint32_t state, uint32_t inv) { return accepts(accept, state) ^ inv; }

// (combine); true: A had no delimiter, the caller composes the maps
ZRA_CTX_FN bool combine(Run& A, const Run& B, uint32_t through, uint64_t accept, uint32_t inv, uint32_t before, uint32_t after) {
  if (!A.has) { A = B; return true; }
  if (!B.has) { A.tail = through; return false; }
  zra_ctx::push(A.c, selected(accept, through, inv), before, after);
  zra_ctx::append(A.c, B.c, before, after);
  A.tail = B.tail; A.last = B.last;
  return false;
}

// (front) over the run r; returns whether the record that r's first delimiter ends MATCHES (before the inversion), 0 without one
ZRA_CTX_FN uint32_t advance(Front& f, const Run& r, uint32_t through, uint64_t accept, uint32_t inv, uint32_t before, uint32_t after) {
  if (!r.has) { f.state = through; return 0; }
  const uint32_t m = accepts(accept, through);
  zra_ctx::push(f.c, m ^ inv, before, after);
  zra_ctx::append(f.c, r.c, before, after);
  f.state = r.tail; f.start = r.last;
  return m;
}

// the record open at hi, if there is one, ends there
ZRA_CTX_FN bool finish(Front& f, uint64_t hi, uint64_t accept, uint32_t inv, uint32_t before, uint32_t after) {
  if (f.start >= hi) return false;
  zra_ctx::push(f.c, selected(accept, f.state, inv), before, after);
  return true;
}

// the (look) of a run whose first record is resolved, and of a run of resolved records: zra_context.h's
using zra_ctx::resolved_look;
using zra_ctx::ctx_look;

// F := m o F over the 64 states, a byte each (the host's form of zra_regex_tile.h's compose)
ZRA_CTX_FN void compose_bytes(uint8_t* F, const uint8_t* m) {
  for (uint32_t s = 0; s < 64; s++) F[s] = m[F[s]];
}
}  // namespace zra_rxc
