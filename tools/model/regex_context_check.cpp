// Host check of zra_amd/csrc/zra_regex_context.h, the summary algebra of the regex grep with context records: the very
// combine(), advance() and finish() the kernels call, folded over random texts and held against a walk that knows nothing of
// summaries. Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zra_amd/csrc tools/model/regex_context_check.cpp
// A case: a text over {a, b, c, delimiter}, one of a few hand-written automata, widths before and after in 0 .. 64, the inversion, the
// text cut into 1 .. 3 passes and every pass into runs of 0 .. 64 positions. Every pass is folded twice, from the left and in a random
// bracketing, and the two must agree word for word (associativity, maps included); the carried front moves over the passes and ends the
// record open at the text's end. |S|, |O| and the groups must be the brute-force walk's. Ends with "regex_context_check: N cases ok".
#include "zra_regex_context.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {
using zra_ctx::Ctx;
using zra_rxc::Front;
using zra_rxc::Run;

constexpr uint8_t kDelim = '\n';
// a complete automaton over the three letters: next[state][letter - 'a']
struct Automaton { const char* name; uint32_t states, start; uint64_t accept; uint8_t next[6][3]; };
const Automaton kAutomata[] = {
    {"ab", 3, 0, 1ull << 2, {{1, 0, 0}, {1, 2, 0}, {2, 2, 2}}},                       // holds `ab`: 2 is the accepting sink
    {"^a", 3, 0, 1ull << 1, {{1, 2, 2}, {1, 1, 1}, {2, 2, 2}}},                       // begins with a: 2 is the dead state
    {"b$", 2, 0, 1ull << 1, {{0, 1, 0}, {0, 1, 0}}},                                  // ends in b
    {"^$", 2, 0, 1ull << 0, {{1, 1, 1}, {1, 1, 1}}},                                  // the empty record
    {"^(b|c)*(a(b|c)*a(b|c)*)*$", 2, 0, 1ull << 0, {{1, 0, 0}, {0, 1, 1}}},           // an even number of a: every map is a permutation
    {"six states", 6, 0, 1ull << 3 | 1ull << 5, {{1, 4, 4}, {1, 2, 3}, {4, 4, 3}, {4, 4, 5}, {4, 4, 4}, {5, 5, 5}}},
};
// (the last one: 0 start, 1 behind a+, 2 behind a+b, 3 accepting at a record's end only, 4 a state that is left for 3 by c, 5 the
// accepting sink. It is no expression's minimal automaton: the check needs transitions and accepting states, not a compiler.)

struct Summary { Run r; uint8_t F[64]; };

Summary identity() {
  Summary s;
  s.r = Run{0, 0, 0, Ctx{0, 0, 0, 0, 0}};
  for (uint32_t q = 0; q < 64; q++) s.F[q] = (uint8_t)q;
  return s;
}

// the summary of the positions [p, q) of the text, by its definition
Summary leaf(const Automaton& A, const std::vector<uint8_t>& text, size_t p, size_t q, uint32_t inv, uint32_t before, uint32_t after) {
  Summary s = identity();
  uint32_t state = A.start;
  for (size_t i = p; i < q; i++) {
    const uint8_t b = text[i];
    if (b == kDelim) {
      if (s.r.has) zra_ctx::push(s.r.c, zra_rxc::selected(A.accept, state, inv), before, after);
      s.r.has = 1; s.r.last = i + 1; state = A.start;
    } else if (!s.r.has) {
      for (uint32_t k = 0; k < A.states; k++) s.F[k] = A.next[s.F[k]][b - 'a'];
    } else state = A.next[state][b - 'a'];
  }
  s.r.tail = s.r.has ? state : 0;
  return s;
}

void join(Summary& a, const Summary& b, const Automaton& A, uint32_t inv, uint32_t before, uint32_t after) {
  if (zra_rxc::combine(a.r, b.r, b.F[a.r.tail], A.accept, inv, before, after)) zra_rxc::compose_bytes(a.F, b.F);
}

Summary fold(std::mt19937& rng, const std::vector<Summary>& leaves, size_t i, size_t j, const Automaton& A, uint32_t inv, uint32_t before, uint32_t after) {
  if (j - i == 1) return leaves[i];
  const size_t k = i + 1 + rng() % (j - i - 1);
  Summary l = fold(rng, leaves, i, k, A, inv, before, after);
  const Summary r = fold(rng, leaves, k, j, A, inv, before, after);
  join(l, r, A, inv, before, after);
  return l;
}

bool same(const Summary& a, const Summary& b, uint32_t states) {
  return a.r.has == b.r.has && a.r.tail == b.r.tail && a.r.last == b.r.last && a.r.c.sel == b.r.c.sel && a.r.c.out == b.r.c.out && a.r.c.groups == b.r.c.groups &&
         a.r.c.head == b.r.c.head && a.r.c.tail == b.r.c.tail && std::memcmp(a.F, b.F, states) == 0;
}

int fail(const char* what, unsigned long long n, const Automaton& A, const std::vector<uint8_t>& text, uint32_t inv, uint32_t before, uint32_t after) {
  std::printf("regex_context_check: case %llu FAILED (%s): automaton %s inv %u before %u after %u text ", n, what, A.name, inv, before, after);
  for (uint8_t b : text) std::printf("%c", b == kDelim ? '/' : b);
  std::printf("\n");
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  const unsigned long long want = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 120000;
  std::mt19937 rng(20240531);
  unsigned long long done = 0;
  for (; done < want; done++) {
    const Automaton& A = kAutomata[rng() % (sizeof(kAutomata) / sizeof(kAutomata[0]))];
    const uint32_t inv = rng() & 1;
    const uint32_t before = (rng() & 3) ? rng() % 5 : rng() % 65, after = (rng() & 3) ? rng() % 5 : rng() % 65;
    const size_t n = rng() % ((rng() & 7) ? 120 : 700);
    const uint32_t pd = 1 + rng() % 10;                                       // a delimiter in pd of 12 bytes
    std::vector<uint8_t> text(n);
    for (auto& b : text) b = rng() % 12 < pd ? kDelim : (uint8_t)('a' + rng() % 3);
    if ((rng() & 7) == 0 && n > 70) std::memset(text.data() + rng() % (n - 70), 'a' + rng() % 3, 70);   // a stretch without a delimiter
    // ---- the brute-force walk
    std::vector<uint32_t> sel;
    {
      uint32_t state = A.start;
      size_t start = 0;
      for (size_t i = 0; i < n; i++) {
        if (text[i] == kDelim) { sel.push_back(zra_rxc::selected(A.accept, state, inv)); state = A.start; start = i + 1; }
        else state = A.next[state][text[i] - 'a'];
      }
      if (start < n) sel.push_back(zra_rxc::selected(A.accept, state, inv));
    }
    const long long R = (long long)sel.size();
    std::vector<uint8_t> inO(sel.size(), 0);
    uint64_t nSel = 0, nOut = 0, nGroups = 0;
    for (long long j = 0; j < R; j++)
      if (sel[j]) {
        nSel++;
        for (long long k = std::max(0ll, j - (long long)before); k <= std::min(R - 1, j + (long long)after); k++) inO[k] = 1;
      }
    for (long long k = 0; k < R; k++) { nOut += inO[k]; nGroups += inO[k] && (k == 0 || !inO[k - 1]); }
    // ---- the passes
    Front f; f.start = 0; f.state = A.start; f.c = Ctx{0, 0, 0, 0, 0};
    const uint32_t passes = 1 + rng() % 3;
    size_t p = 0;
    for (uint32_t ps = 0; ps < passes; ps++) {
      const size_t pEnd = ps + 1 == passes ? n : p + rng() % (n - p + 1);
      std::vector<Summary> leaves;
      for (size_t q = p; q < pEnd || leaves.empty();) {
        const size_t w = std::min<size_t>(rng() % 65, pEnd - q);
        leaves.push_back(leaf(A, text, q, q + w, inv, before, after));
        q += w;
        if (q >= pEnd) break;
      }
      Summary left = leaves[0];
      for (size_t i = 1; i < leaves.size(); i++) join(left, leaves[i], A, inv, before, after);
      const Summary any = fold(rng, leaves, 0, leaves.size(), A, inv, before, after);
      if (!same(left, any, A.states)) return fail("two bracketings differ", done, A, text, inv, before, after);
      const Summary whole = leaf(A, text, p, pEnd, inv, before, after);
      if (!same(left, whole, A.states)) return fail("the fold is not the run's own summary", done, A, text, inv, before, after);
      zra_rxc::advance(f, left.r, left.F[f.state], A.accept, inv, before, after);
      p = pEnd;
    }
    zra_rxc::finish(f, n, A.accept, inv, before, after);
    if (f.c.sel != nSel) return fail("|S|", done, A, text, inv, before, after);
    if (f.c.out != nOut) return fail("|O|", done, A, text, inv, before, after);
    if (f.c.groups != nGroups) return fail("groups", done, A, text, inv, before, after);
  }
  std::printf("regex_context_check: %llu cases ok\n", done);
  return 0;
}
