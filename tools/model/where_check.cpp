// Walks zra_amd/csrc/zra_where.h on the CPU: the rule-1 refusals of the record clauses at and one past their edges, and
// where_selected() against a second formulation that shares no bit arithmetic with it: every clause is expanded into explicit terms
// (a list of pattern numbers that must be in the set and a list that must not, one term per member of `any`), and a hit set is an
// array of 6 booleans. Every hit set of a 6-pattern universe is held against every clause list of a fixed random sample, plain and
// inverted. The clause arrays lie in heap blocks of exactly their size, so that under -fsanitize=address,undefined a read behind
// hClauses + nClauses ends the run. Includes only that header.
//   g++ -std=c++17 -fsanitize=address,undefined -I zra_amd/csrc tools/model/where_check.cpp -o where_check
//   ./where_check          exit 0 and "where_check: N cases ok", or the failing cases and exit 1
#include "zra_where.h"

#include <cstdio>
#include <memory>
#include <vector>

using namespace zra_where;

namespace {
int g_cases = 0, g_failed = 0;

void expect(bool got, bool want, const char* what, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
  g_cases++;
  if (got == want) return;
  g_failed++;
  std::printf("FAILED %s (%llx %llx %llx): got %d, want %d\n", what, a, b, c, (int)got, (int)want);
}

// clauses_ok on an exact-size heap copy
bool ok(const std::vector<Clause>& c, size_t nPatterns) {
  std::unique_ptr<Clause[]> h(new Clause[c.size() ? c.size() : 1]);
  for (size_t i = 0; i < c.size(); i++) h[i] = c[i];
  return clauses_ok(c.size() ? h.get() : h.get() + 1, c.size(), nPatterns);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

constexpr int kUniverse = 6;
struct Term { std::vector<int> must, mustNot; };

// a clause as terms: all of `all`, none of `none`, and, when `any` has members, one term per member
std::vector<Term> expand(const Clause& c) {
  Term base;
  for (int i = 0; i < kUniverse; i++) {
    if ((c.all >> i) & 1) base.must.push_back(i);
    if ((c.none >> i) & 1) base.mustNot.push_back(i);
  }
  std::vector<Term> out;
  if (c.any == 0) { out.push_back(base); return out; }
  for (int i = 0; i < kUniverse; i++)
    if ((c.any >> i) & 1) { Term t = base; t.must.push_back(i); out.push_back(t); }
  return out;
}

bool term_holds(const Term& t, const bool in[kUniverse]) {
  for (int i : t.must) if (!in[i]) return false;
  for (int i : t.mustNot) if (in[i]) return false;
  return true;
}
}  // namespace

int main() {
  // ---- the refusals
  expect(clauses_ok(nullptr, 1, 4), false, "hClauses NULL");
  expect(ok({}, 4), false, "no clause");
  expect(ok(std::vector<Clause>(8, Clause{1, 2, 4}), 4), true, "8 clauses");
  expect(ok(std::vector<Clause>(9, Clause{1, 2, 4}), 4), false, "9 clauses");
  expect(ok({{0, 0, 0}}, 0), false, "no pattern");
  expect(ok({{0, 0, 0}}, 65), false, "65 patterns");
  expect(ok({{0, 0, 0}}, 1), true, "the empty clause");
  for (size_t n : {(size_t)1, (size_t)2, (size_t)6, (size_t)63, (size_t)64}) {
    const uint64_t top = 1ull << (n - 1);
    expect(full_set(n) == (n == 64 ? ~0ull : (1ull << n) - 1), true, "full_set", n);
    for (int field = 0; field < 3; field++) {
      Clause in = {0, 0, 0}, out = {0, 0, 0};
      (field == 0 ? in.all : field == 1 ? in.any : in.none) = top;
      expect(ok({in}, n), true, "bit nPatterns - 1", n, field);
      expect(ok({{1, 0, 0}, in}, n), true, "bit nPatterns - 1 in the second clause", n, field);
      if (n == 64) continue;
      (field == 0 ? out.all : field == 1 ? out.any : out.none) = top << 1;
      expect(ok({out}, n), false, "bit nPatterns", n, field);
      expect(ok({{1, 0, 0}, out}, n), false, "bit nPatterns in the second clause", n, field);
      (field == 0 ? out.all : field == 1 ? out.any : out.none) = 1ull << 63;
      expect(ok({out}, n), false, "bit 63", n, field);
    }
  }
  expect(ok({{3, 0, 2}}, 4), false, "all & none");
  expect(ok({{0, 3, 1}}, 4), false, "any & none");
  expect(ok({{1, 2, 4}, {0, 8, 8}}, 4), false, "any & none in the second clause");
  expect(ok({{3, 3, 4}}, 4), true, "all & any");
  expect(ok({{~0ull, 0, 0}, {0, ~0ull, 0}, {0, 0, ~0ull}}, 64), true, "full words at 64 patterns");

  // ---- the named predicates
  for (uint64_t H = 0; H < 16; H++) {
    const Clause any = {0, 15, 0}, none = {0, 0, 15}, every = {0, 0, 0};
    expect(where_selected(make_block(&any, 1, false), H), H != 0, "the plain grep", H);
    expect(where_selected(make_block(&any, 1, true), H), H == 0, "the plain grep, inverted", H);
    expect(where_selected(make_block(&none, 1, false), H), H == 0, "grep -v", H);
    expect(where_selected(make_block(&every, 1, false), H), true, "every record", H);
    expect(where_selected(make_block(&every, 1, true), H), false, "no record", H);
  }
  const Clause hi = {1ull << 63, 0, 1ull << 62};
  expect(where_selected(make_block(&hi, 1, false), 1ull << 63), true, "bit 63");
  expect(where_selected(make_block(&hi, 1, false), 3ull << 62), false, "bit 62 forbidden");

  // ---- the sample: 400 clause lists of 1 .. 8 clauses over 6 patterns, every one of the 64 hit sets, both modes
  for (int s = 0; s < 400; s++) {
    const size_t n = 1 + rnd() % kMaxClauses;
    std::vector<Clause> c(n);
    for (auto& k : c) {
      k = Clause{0, 0, 0};
      for (int i = 0; i < kUniverse; i++)
        switch (rnd() % 5) { case 0: k.all |= 1ull << i; break; case 1: k.any |= 1ull << i; break; case 2: k.none |= 1ull << i; break; default: break; }
      if (rnd() % 4 == 0) k.any |= k.all & (rnd() % 64);                   // (all and any may share a pattern)
    }
    expect(ok(c, kUniverse), true, "a sampled list", s);
    std::unique_ptr<Clause[]> h(new Clause[n]);
    for (size_t i = 0; i < n; i++) h[i] = c[i];
    const Block plain = make_block(h.get(), n, false), inverted = make_block(h.get(), n, true);
    std::vector<std::vector<Term>> terms;
    for (auto& k : c) terms.push_back(expand(k));
    for (uint64_t H = 0; H < (1u << kUniverse); H++) {
      bool in[kUniverse];
      for (int i = 0; i < kUniverse; i++) in[i] = (H >> i) & 1;
      bool want = false;
      for (auto& list : terms) for (auto& t : list) want = want || term_holds(t, in);
      expect(where_selected(plain, H), want, "where_selected", s, H);
      expect(where_selected(inverted, H), !want, "where_selected, inverted", s, H);
    }
  }

  if (g_failed) { std::printf("where_check: %d of %d cases FAILED\n", g_failed, g_cases); return 1; }
  std::printf("where_check: %d cases ok\n", g_cases);
  return 0;
}
