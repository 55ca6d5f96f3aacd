// zra_amd — the regular expressions of the regex grep (zra_hip.h: ZraHipGrepArchiveRegex, ZraHipArchiveGrepRegex, ZraHipCheckRegex;
// DESIGN.md §28): caller-supplied expressions, the syntax word and the delimiter become the minimal complete DFA of the set of matched
// records, or a refusal with its reason. POSIX ERE over bytes on top of zra_pattern_expr.h's atoms: * + ? {n} {n,} {n,m} ( ) | ^ $.
// Plain C++17, host only, no HIP types and nothing of the engine: tools/model/regex_check.cpp walks it on the CPU under the address
// and undefined-behaviour sanitizers (tests/test_regex_abi.py). The regex selector of zra_record_scan.h uploads the table it makes.
//
//  (parser) one loop over the bytes with an explicit stack of open groups: no recursion on what a caller wrote. Every read is behind a
//      test against the expression's end, and the sizes are summed (in 64 bits) and bounded before the first byte is looked at. Nodes
//      are made by constructors that keep the tree small: a subtree without a position is the empty word, x{1} is x, a simple
//      quantifier (* + ?) over a simple quantifier is one, an empty alternative becomes a ?. What is left of unary chains is bounded by
//      the position limit: every counted repetition with two or more copies at least doubles its subtree's positions.
//  (positions) an atom or an anchor is one position; x* x+ x? keep x's count, x{n,m} has m copies, x{n,} has max(n, 1), a
//      concatenation and an alternation add up. The count is taken (saturating) before anything is expanded.
//  (anchors) BOL and EOL are two symbols that no atom admits; ^ reads BOL, $ reads EOL. The language of a call is S* (e_1|...|e_K) S*
//      over the bytes and the two symbols, and a record r is matched iff BOL r EOL is in it. So `^^a` and `a^b` match nothing, by
//      the same rule that makes `^a` match at the record's start, and no anchor is a special case.
//  (automaton) Thompson's construction over the expanded tree; the subset construction runs on sets of POSITIONS (the symbol-reading
//      states of an epsilon closure) plus "accepted", which is one sink: behind a match the trailing S* takes everything. The leading
//      S* adds the initial closure to every state. The device's start state is the state behind BOL, its accepting states those from
//      which EOL leads to the sink. Bytes are grouped into classes by the atoms' sets first, so a step costs the state's positions,
//      not 255 columns. The construction stops at kMaxSubsets distinct sets (reason 4). Moore's refinement then merges equivalent
//      states and stops as soon as it holds more than 64 blocks.
#pragma once
#include "zra_pattern_expr.h"

#include <algorithm>
#include <cstring>
#include <map>

namespace zra_regex {

using zra_expr::ByteSet;

constexpr uint32_t kMaxStates = 64;         // ZRA_HIP_REGEX_MAX_STATES
constexpr uint32_t kMaxPositions = 4096;    // ZRA_HIP_REGEX_MAX_POSITIONS
constexpr uint32_t kMaxSubsets = 4096;      // the construction bound
constexpr uint32_t kMaxRepeat = 255;
enum : uint32_t { kAccepted = 0, kWhyArguments = 1, kWhySyntax = 2, kWhyEmptyAtom = 3, kWhyStates = 4 };

struct Info { uint32_t states, classes, positions, why, pattern; };   // ZraHipRegexInfo

// What the device steps through (zra_regex_tile.h): uploaded as the head of the call's tables. Rows behind `classes` and columns
// behind `states` are zero: state 0 exists, so every entry is a state.
struct alignas(16) Table {
  uint8_t classOf[256];          // the delimiter's entry is 0 and never read: the delimiter belongs to no class
  uint8_t next[256][64];         // class-major: the 64 lanes of a map step read consecutive bytes
  uint64_t accept;               // bit s: a record that ends in state s is matched
  uint64_t settled;              // bit s: every byte leads from s to s (the dead state, the accepting sink)
  uint32_t start, states, classes, pad;
};
static_assert(sizeof(Table) == 256 + 16384 + 32, "16-byte chunks");

namespace detail {
enum : uint8_t { kEps, kSet, kBol, kEol, kCat, kAlt, kStar, kPlus, kOpt, kRep };
struct Node { uint8_t type; int32_t a, b; uint32_t kids, nKids; uint64_t pos; };   // kSet: a = set; unary: a = child; kRep: kids[0], a = min, b = max (-1: none)
constexpr uint64_t kSat = 1ull << 32;

struct Tree {
  std::vector<Node> n;
  std::vector<int32_t> kids;
  std::vector<ByteSet> sets;               // distinct
  std::map<std::vector<uint64_t>, int32_t> setIndex;
  int32_t eps = -1;
  int32_t add(uint8_t type, int32_t a, int32_t b, uint64_t pos) { n.push_back(Node{type, a, b, 0, 0, pos < kSat ? pos : kSat}); return (int32_t)n.size() - 1; }
  int32_t mk_eps() { if (eps < 0) eps = add(kEps, 0, 0, 0); return eps; }
  int32_t mk_set(const ByteSet& s) {
    const std::vector<uint64_t> key(s.w, s.w + 4);
    auto it = setIndex.find(key);
    if (it == setIndex.end()) { it = setIndex.emplace(key, (int32_t)sets.size()).first; sets.push_back(s); }
    return add(kSet, it->second, 0, 1);
  }
  int32_t mk_list(uint8_t type, const std::vector<int32_t>& items, bool* hadEps) {
    std::vector<int32_t> keep;
    uint64_t pos = 0;
    for (int32_t k : items) { if (n[k].type == kEps) { *hadEps = true; continue; } keep.push_back(k); pos += n[k].pos; }
    if (keep.empty()) return mk_eps();
    if (keep.size() == 1) return keep[0];
    const int32_t id = add(type, 0, 0, pos);
    n[id].kids = (uint32_t)kids.size(); n[id].nKids = (uint32_t)keep.size();
    kids.insert(kids.end(), keep.begin(), keep.end());
    return id;
  }
  int32_t mk_cat(const std::vector<int32_t>& items) { bool e = false; return mk_list(kCat, items, &e); }
  int32_t mk_alt(const std::vector<int32_t>& items) { bool e = false; const int32_t id = mk_list(kAlt, items, &e); return e ? mk_quant(id, 0, 1) : id; }
  // x{mn,mx}, mx < 0: no upper bound
  int32_t mk_quant(int32_t x, int32_t mn, int32_t mx) {
    if (n[x].type == kEps || mx == 0) return mk_eps();
    if (mn == 1 && mx == 1) return x;
    const uint8_t t = n[x].type;
    const bool inner = t == kStar || t == kPlus || t == kOpt;
    const int32_t in = inner ? n[x].a : x;
    const uint64_t pos = n[in].pos;
    if (mn == 0 && mx == 1) return t == kOpt || t == kStar ? x : t == kPlus ? add(kStar, in, 0, pos) : add(kOpt, x, 0, pos);
    if (mn == 0 && mx < 0) return t == kStar ? x : add(kStar, in, 0, pos);
    if (mn == 1 && mx < 0) return t == kPlus || t == kStar ? x : t == kOpt ? add(kStar, in, 0, pos) : add(kPlus, x, 0, pos);
    const int32_t id = add(kRep, mn, mx, n[x].pos * (uint64_t)(mx < 0 ? mn : mx));
    n[id].kids = (uint32_t)kids.size(); n[id].nKids = 1;
    kids.push_back(x);
    return id;
  }
};

// the bound behind a '{' at p: digits, then '}' or ',' digits? '}'; 0 <= mn <= mx <= 255
inline bool bound(const uint8_t*& p, const uint8_t* e, int32_t* mn, int32_t* mx) {
  auto number = [&](int32_t* v) {
    if (p >= e || *p < '0' || *p > '9') return false;
    uint32_t x = 0;
    while (p < e && *p >= '0' && *p <= '9') { x = x * 10 + (uint32_t)(*p++ - '0'); if (x > kMaxRepeat) return false; }
    *v = (int32_t)x;
    return true;
  };
  if (!number(mn)) return false;
  if (p >= e) return false;
  if (*p == '}') { p++; *mx = *mn; return true; }
  if (*p++ != ',') return false;
  if (p >= e) return false;
  if (*p == '}') { p++; *mx = -1; return true; }
  if (!number(mx) || p >= e || *p++ != '}') return false;
  return *mn <= *mx;
}

// One expression [p, e) into the tree. 0: its root in *root; else the reason.
inline uint32_t parse(Tree& T, const uint8_t* p, const uint8_t* e, uint32_t syntax, int delimiter, int32_t* root) {
  struct Open { std::vector<int32_t> branches, items; };
  std::vector<Open> st(1);
  bool canQuant = false;                     // the last item is an atom or a group without a quantifier
  while (p < e) {
    const uint8_t c = *p++;
    Open& o = st.back();
    switch (c) {
      case '(': st.emplace_back(); canQuant = false; break;
      case ')': {
        if (st.size() == 1 || o.items.empty()) return kWhySyntax;
        o.branches.push_back(T.mk_cat(o.items));
        const int32_t g = T.mk_alt(o.branches);
        st.pop_back();
        st.back().items.push_back(g);
        canQuant = true;
        break;
      }
      case '|':
        if (o.items.empty()) return kWhySyntax;
        o.branches.push_back(T.mk_cat(o.items));
        o.items.clear();
        canQuant = false;
        break;
      case '*': case '+': case '?': case '{': {
        if (!canQuant) return kWhySyntax;
        int32_t mn = c == '+' ? 1 : 0, mx = c == '?' ? 1 : -1;
        if (c == '{' && !bound(p, e, &mn, &mx)) return kWhySyntax;
        o.items.back() = T.mk_quant(o.items.back(), mn, mx);
        canQuant = false;
        break;
      }
      case '^': o.items.push_back(T.add(kBol, 0, 0, 1)); canQuant = false; break;
      case '$': o.items.push_back(T.add(kEol, 0, 0, 1)); canQuant = false; break;
      case ']': case '}': return kWhySyntax;
      default: {
        ByteSet s;
        bool neg = false;
        if (c == '.') s.complement();
        else if (c == '[') { if (!zra_expr::detail::bracket(p, e, &s, &neg)) return kWhySyntax; }
        else if (c == '\\') { uint32_t b = 0; const int k = zra_expr::detail::escape(p, e, &b, &s); if (!k) return kWhySyntax; if (k == 1) s.add(b); }
        else s.add(c);
        if (!zra_expr::detail::finish(&s, neg, true, syntax, delimiter)) return kWhyEmptyAtom;
        o.items.push_back(T.mk_set(s));
        canQuant = true;
      }
    }
  }
  if (st.size() != 1 || st[0].items.empty()) return kWhySyntax;
  st[0].branches.push_back(T.mk_cat(st[0].items));
  *root = T.mk_alt(st[0].branches);
  return 0;
}

// Thompson's automaton. A state reads a symbol (sym >= 0: a set's index, nSets: BOL, nSets + 1: EOL) into out1, or has up to two
// epsilon moves. A fragment ends in a state without moves.
struct Nfa {
  struct State { int32_t sym, out1, out2; };
  std::vector<State> s;
  int32_t state(int32_t sym) { s.push_back(State{sym, -1, -1}); return (int32_t)s.size() - 1; }
  struct Frag { int32_t in, out; };
};

// The depth of the recursion is the tree's: at most two levels per position beside the bounded unary chains, (parser).
inline Nfa::Frag build(const Tree& T, Nfa& N, int32_t id) {
  const Node& nd = T.n[id];
  const int32_t nSets = (int32_t)T.sets.size();
  switch (nd.type) {
    case kEps: { const int32_t a = N.state(-1); return {a, a}; }
    case kSet: case kBol: case kEol: {
      const int32_t a = N.state(nd.type == kSet ? nd.a : nd.type == kBol ? nSets : nSets + 1), b = N.state(-1);
      N.s[a].out1 = b;
      return {a, b};
    }
    case kCat: {
      Nfa::Frag f = build(T, N, T.kids[nd.kids]);
      for (uint32_t k = 1; k < nd.nKids; k++) { const Nfa::Frag g = build(T, N, T.kids[nd.kids + k]); N.s[f.out].out1 = g.in; f.out = g.out; }
      return f;
    }
    case kAlt: {
      const int32_t in = N.state(-1), out = N.state(-1);
      int32_t split = in;
      for (uint32_t k = 0; k < nd.nKids; k++) {
        const Nfa::Frag g = build(T, N, T.kids[nd.kids + k]);
        N.s[g.out].out1 = out;
        N.s[split].out1 = g.in;
        if (k + 2 < nd.nKids) { const int32_t nx = N.state(-1); N.s[split].out2 = nx; split = nx; }
        else if (k + 2 == nd.nKids) { const Nfa::Frag h = build(T, N, T.kids[nd.kids + k + 1]); N.s[h.out].out1 = out; N.s[split].out2 = h.in; break; }
      }
      return {in, out};
    }
    case kStar: case kOpt: {
      const Nfa::Frag g = build(T, N, nd.a);
      const int32_t in = N.state(-1), out = N.state(-1);
      N.s[in].out1 = g.in; N.s[in].out2 = out;
      N.s[g.out].out1 = out;
      if (nd.type == kStar) N.s[g.out].out2 = g.in;
      return {in, out};
    }
    case kPlus: {
      const Nfa::Frag g = build(T, N, nd.a);
      const int32_t out = N.state(-1);
      N.s[g.out].out1 = g.in; N.s[g.out].out2 = out;
      return {g.in, out};
    }
    default: {   // kRep: mn copies, then a + of one more copy (no upper bound) or mx - mn optional copies that all skip to the end
      const int32_t x = T.kids[nd.kids], mn = nd.a, mx = nd.b;
      const int32_t in = N.state(-1), out = N.state(-1);
      int32_t at = in;
      const int32_t plain = mx < 0 ? mn - 1 : mn;
      for (int32_t k = 0; k < plain; k++) { const Nfa::Frag g = build(T, N, x); N.s[at].out1 = g.in; at = g.out; }
      if (mx < 0) {
        const Nfa::Frag g = build(T, N, x);
        N.s[at].out1 = g.in;
        N.s[g.out].out1 = g.in; N.s[g.out].out2 = out;
        return {in, out};
      }
      for (int32_t k = mn; k < mx; k++) {
        const Nfa::Frag g = build(T, N, x);
        const int32_t split = N.state(-1);
        N.s[at].out1 = split;
        N.s[split].out1 = g.in; N.s[split].out2 = out;
        at = g.out;
      }
      N.s[at].out1 = out;
      return {in, out};
    }
  }
}
}  // namespace detail

struct Compiled {
  Info info{0, 0, 0, kWhyArguments, 0};
  Table table;
};

inline bool refuse(Compiled* out, uint32_t why, uint32_t pattern = 0) { out->info = Info{0, 0, 0, why, pattern}; return false; }

// Rule 1 of the regex grep as far as the expressions go, and the table. hPat: the expressions laid end to end, hSizes their sizes.
inline bool compile(const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, int delimiter, Compiled* out) {
  using namespace detail;
  std::memset(&out->table, 0, sizeof(Table));
  if (!hPat || !hSizes || nPat == 0 || nPat > zra_expr::kMaxPatterns || (syntax & ~zra_expr::kFoldCase) || delimiter < 0 || delimiter > 255) return refuse(out, kWhyArguments);
  uint64_t bytes = 0;
  for (size_t i = 0; i < nPat; i++) { if (hSizes[i] == 0) return refuse(out, kWhyArguments); bytes += hSizes[i]; }
  if (bytes > zra_expr::kMaxExprBytes) return refuse(out, kWhyArguments);
  Tree T;
  std::vector<int32_t> roots;
  const uint8_t* p = hPat;
  for (size_t i = 0; i < nPat; p += hSizes[i], i++) {
    int32_t root = 0;
    const uint32_t why = parse(T, p, p + hSizes[i], syntax, delimiter, &root);
    if (why) return refuse(out, why, (uint32_t)i);
    roots.push_back(root);
  }
  uint64_t positions = 0;
  for (int32_t r : roots) positions += T.n[r].pos;
  if (positions > kMaxPositions) return refuse(out, kWhyArguments);
  const int32_t top = T.mk_alt(roots);

  // ---- the automaton; the symbol-reading states, numbered: the positions
  Nfa N;
  const Nfa::Frag F = build(T, N, top);
  const int32_t nSets = (int32_t)T.sets.size();
  std::vector<int32_t> posOf(N.s.size(), -1), stateOf;
  for (size_t k = 0; k < N.s.size(); k++) if (N.s[k].sym >= 0) { posOf[k] = (int32_t)stateOf.size(); stateOf.push_back((int32_t)k); }
  const size_t P = stateOf.size(), kFinal = P, W = (P + 1 + 63) / 64;
  typedef std::vector<uint64_t> Bits;
  // the closure of a state: the positions and "final" that its epsilon moves reach
  std::vector<uint32_t> seen(N.s.size(), 0);
  uint32_t stamp = 0;
  std::vector<int32_t> todo;
  auto closure = [&](int32_t from, Bits* b) {
    stamp++;
    todo.assign(1, from);
    seen[from] = stamp;
    while (!todo.empty()) {
      const int32_t k = todo.back(); todo.pop_back();
      if (k == F.out) (*b)[kFinal >> 6] |= 1ull << (kFinal & 63);
      if (N.s[k].sym >= 0) { (*b)[posOf[k] >> 6] |= 1ull << (posOf[k] & 63); continue; }
      for (int32_t nx : {N.s[k].out1, N.s[k].out2}) if (nx >= 0 && seen[nx] != stamp) { seen[nx] = stamp; todo.push_back(nx); }
    }
  };
  Bits init(W, 0);
  closure(F.in, &init);
  std::vector<Bits> follow(P, Bits(W, 0));
  for (size_t q = 0; q < P; q++) closure(N.s[stateOf[q]].out1, &follow[q]);
  auto has_final = [&](const Bits& b) { return ((b[kFinal >> 6] >> (kFinal & 63)) & 1) != 0; };

  // ---- byte classes by the atoms' sets (a refinement of the final classes), the delimiter left out
  std::vector<int32_t> preOf(256, -1);
  std::vector<uint32_t> rep;
  {
    std::map<std::vector<uint64_t>, int32_t> sig;
    const size_t SW = ((size_t)nSets + 63) / 64;
    for (uint32_t b = 0; b < 256; b++) {
      if ((int)b == delimiter) continue;
      std::vector<uint64_t> key(SW, 0);
      for (int32_t k = 0; k < nSets; k++) if (T.sets[k].has(b)) key[k >> 6] |= 1ull << (k & 63);
      auto it = sig.find(key);
      if (it == sig.end()) { it = sig.emplace(key, (int32_t)rep.size()).first; rep.push_back(b); }
      preOf[b] = it->second;
    }
  }
  const size_t C = rep.size();
  std::vector<std::vector<uint32_t>> classesOfSet((size_t)nSets);
  for (int32_t k = 0; k < nSets; k++) for (size_t c = 0; c < C; c++) if (T.sets[k].has(rep[c])) classesOfSet[k].push_back((uint32_t)c);

  // ---- the subset construction over the bytes. Subset 0 is the sink "accepted".
  auto step_symbol = [&](const Bits& from, int32_t sym) {   // BOL or EOL
    Bits to = init;
    for (size_t q = 0; q < P; q++) if (((from[q >> 6] >> (q & 63)) & 1) && N.s[stateOf[q]].sym == sym) for (size_t w = 0; w < W; w++) to[w] |= follow[q][w];
    return to;
  };
  std::vector<Bits> subsets(1, Bits());
  std::vector<std::vector<uint32_t>> delta(1, std::vector<uint32_t>(C, 0));
  std::vector<uint8_t> accepting(1, 1);
  std::map<Bits, uint32_t> index;
  uint32_t start = 0;
  if (!has_final(init)) {
    const Bits first = step_symbol(init, nSets);
    if (!has_final(first)) { start = 1; subsets.push_back(first); index.emplace(first, 1u); }
  }
  std::vector<Bits> nextOf(C, Bits(W, 0));
  for (size_t d = 1; d < subsets.size(); d++) {
    const Bits cur = subsets[d];
    accepting.push_back(has_final(step_symbol(cur, nSets + 1)) ? 1 : 0);
    for (size_t c = 0; c < C; c++) nextOf[c] = init;
    for (size_t q = 0; q < P; q++) {
      if (!((cur[q >> 6] >> (q & 63)) & 1)) continue;
      const int32_t sym = N.s[stateOf[q]].sym;
      if (sym >= nSets) continue;
      for (uint32_t c : classesOfSet[sym]) for (size_t w = 0; w < W; w++) nextOf[c][w] |= follow[q][w];
    }
    delta.emplace_back(C, 0);
    for (size_t c = 0; c < C; c++) {
      if (has_final(nextOf[c])) continue;                                    // (the sink)
      auto it = index.find(nextOf[c]);
      if (it == index.end()) {
        if (subsets.size() > kMaxSubsets) return refuse(out, kWhyStates);    // (the sink is not counted)
        it = index.emplace(nextOf[c], (uint32_t)subsets.size()).first;
        subsets.push_back(nextOf[c]);
      }
      delta[d][c] = it->second;
    }
  }
  const size_t D = subsets.size();

  // ---- Moore's refinement; only states reachable from the start count (the sink may not be)
  std::vector<uint8_t> reach(D, 0);
  {
    std::vector<uint32_t> q(1, start);
    reach[start] = 1;
    while (!q.empty()) { const uint32_t d = q.back(); q.pop_back(); for (uint32_t t : delta[d]) if (!reach[t]) { reach[t] = 1; q.push_back(t); } }
  }
  std::vector<uint32_t> block(D, 0);
  for (size_t d = 0; d < D; d++) block[d] = accepting[d];
  size_t nBlocks = 0;
  for (;;) {
    std::map<std::vector<uint32_t>, uint32_t> sigs;
    std::vector<uint32_t> nb(D, 0), key(C + 1);
    for (size_t d = 0; d < D; d++) {
      if (!reach[d]) continue;
      key[0] = block[d];
      for (size_t c = 0; c < C; c++) key[c + 1] = block[delta[d][c]];
      nb[d] = sigs.emplace(key, (uint32_t)sigs.size()).first->second;
    }
    const bool stable = sigs.size() == nBlocks;
    nBlocks = sigs.size();
    block.swap(nb);
    if (nBlocks > kMaxStates) return refuse(out, kWhyStates);
    if (stable) break;
  }

  // ---- the table: the final classes are the distinct columns
  Table& tb = out->table;
  std::vector<uint32_t> repState(nBlocks, 0);
  for (size_t d = D; d-- > 0;) if (reach[d]) repState[block[d]] = (uint32_t)d;
  std::map<std::vector<uint32_t>, uint32_t> cols;
  std::vector<uint32_t> classOfPre(C, 0);
  for (size_t c = 0; c < C; c++) {
    std::vector<uint32_t> col(nBlocks);
    for (size_t s = 0; s < nBlocks; s++) col[s] = block[delta[repState[s]][c]];
    auto it = cols.find(col);
    if (it == cols.end()) {
      it = cols.emplace(col, (uint32_t)cols.size()).first;
      for (size_t s = 0; s < nBlocks; s++) tb.next[it->second][s] = (uint8_t)col[s];
    }
    classOfPre[c] = it->second;
  }
  for (uint32_t b = 0; b < 256; b++) if (preOf[b] >= 0) tb.classOf[b] = (uint8_t)classOfPre[preOf[b]];
  for (size_t s = 0; s < nBlocks; s++) {
    if (accepting[repState[s]]) tb.accept |= 1ull << s;
    bool settled = true;
    for (size_t c = 0; c < C; c++) settled = settled && block[delta[repState[s]][c]] == s;
    if (settled) tb.settled |= 1ull << s;
  }
  tb.start = block[start]; tb.states = (uint32_t)nBlocks; tb.classes = (uint32_t)cols.size();
  out->info = Info{(uint32_t)nBlocks, (uint32_t)cols.size(), (uint32_t)positions, kAccepted, 0};
  return true;
}

// Is the record [r, r + n) matched: the table walked on the host (the checker and the tools; the device walks it in zra_regex_tile.h)
inline bool matches(const Table& t, const uint8_t* r, size_t n) {
  uint32_t s = t.start;
  for (size_t i = 0; i < n; i++) s = t.next[t.classOf[r[i]]][s];
  return ((t.accept >> s) & 1) != 0;
}

}  // namespace zra_regex
