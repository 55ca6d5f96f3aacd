// zra_amd — the pattern expressions of the multi-pattern scans (zra_hip.h: ZraHipSearchArchiveMultiExpr, ZraHipGrepArchiveExpr,
// ZraHipExtractRecordsExpr and their handle twins; ZraHipCheckPatternExpr): caller-supplied bytes, sizes, the syntax word and the
// delimiter become one 256-bit byte set per pattern element, or a refusal. Every element matches exactly one byte, so a pattern keeps
// a fixed length and the pass geometry of the literal calls holds with lengths counted in elements.
// Plain C++17, host only, no HIP types and nothing of the engine: tools/model/pattern_expr_check.cpp walks it on the CPU under the
// address and undefined-behaviour sanitizers (tests/test_pattern_expr.py). zra_patterns.h makes the device table from the result.
//
// The parser reads bytes a caller supplied: every read is behind a test against the expression's end, so nothing behind
// hPatterns + the sum of the sizes is read whatever the bytes are, and the sizes are summed (in 64 bits) and bounded before the first
// byte is looked at.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zra_expr {

constexpr uint32_t kFoldCase = 1, kClasses = 2;     // ZRA_HIP_PATTERN_FOLD_CASE, ZRA_HIP_PATTERN_CLASSES
constexpr uint32_t kMaxPatterns = 64;               // ZRA_HIP_SEARCH_MAX_PATTERNS
constexpr uint32_t kMaxElements = 256;              // ZRA_HIP_SEARCH_MAX_PATTERN, in elements
constexpr uint32_t kMaxElementsAll = 4096;          // ZRA_HIP_SEARCH_MAX_PATTERN_BYTES, in elements
constexpr uint32_t kMaxSets = 32;                   // ZRA_HIP_PATTERN_MAX_SETS
constexpr uint32_t kMaxExprBytes = 16384;           // ZRA_HIP_PATTERN_MAX_EXPR_BYTES

struct ByteSet {
  uint64_t w[4] = {0, 0, 0, 0};
  void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
  void add(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; b++) add(b); }
  void remove(uint32_t b) { w[b >> 6] &= ~(1ull << (b & 63)); }
  bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
  void join(const ByteSet& o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
  void complement() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
  uint32_t count() const { uint32_t n = 0; for (int i = 0; i < 4; i++) n += (uint32_t)__builtin_popcountll(w[i]); return n; }
  uint32_t lowest() const { for (int i = 0; i < 4; i++) if (w[i]) return 64 * i + (uint32_t)__builtin_ctzll(w[i]); return 256; }
  bool operator==(const ByteSet& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
  // closed under the case swap of its ASCII letters
  void fold() { for (uint32_t c = 'A'; c <= 'Z'; c++) { if (has(c)) add(c | 0x20); else if (has(c | 0x20)) add(c); } }
};

inline bool is_letter(uint32_t b) { return (b | 0x20) >= 'a' && (b | 0x20) <= 'z'; }

// How the device tests an element (zra_patterns.h: ClassTable::elem): one byte, one ASCII letter in either case, or a counted set.
enum : uint16_t { kCodeByte = 0x000, kCodePair = 0x100, kCodeSet = 0x200 };

struct Compiled {
  std::vector<ByteSet> elems;        // all patterns' elements, pattern after pattern
  std::vector<uint16_t> codes;       // beside elems: kCodeByte | byte, kCodePair | lower-case letter, kCodeSet | index into sets
  std::vector<uint32_t> off, len;    // pattern i: elems[off[i] .. off[i] + len[i])
  std::vector<ByteSet> sets;         // the counted sets: distinct, neither a single byte nor one letter pair
  uint32_t M = 0, mMin = kMaxElements;
  int bad = -1;                      // the refused pattern's index, -1: the counts, the sizes or the syntax word
};

namespace detail {
inline int hexval(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : (c | 0x20) >= 'a' && (c | 0x20) <= 'f' ? (c | 0x20) - 'a' + 10 : -1; }

// The escape behind a backslash at p (p < e is tested here). 1: one byte -> *byte, 2: a class -> *cls, 0: refused.
inline int escape(const uint8_t*& p, const uint8_t* e, uint32_t* byte, ByteSet* cls) {
  if (p >= e) return 0;
  const uint8_t c = *p++;
  switch (c) {
    case 'x': {
      if (e - p < 2) return 0;
      const int h = hexval(p[0]), l = hexval(p[1]);
      if (h < 0 || l < 0) return 0;
      p += 2; *byte = (uint32_t)(h * 16 + l);
      return 1;
    }
    case 'n': *byte = '\n'; return 1;
    case 't': *byte = '\t'; return 1;
    case 'r': *byte = '\r'; return 1;
    case 'd': cls->add('0', '9'); return 2;
    case 'w': cls->add('0', '9'); cls->add('A', 'Z'); cls->add('a', 'z'); cls->add('_'); return 2;
    case 's': cls->add(' '); cls->add('\t', '\r'); return 2;
    case '.': case '[': case ']': case '\\': case '*': case '+': case '?': case '{': case '}': case '(': case ')': case '|': case '^': case '$': case '-':
      *byte = c; return 1;
    default: return 0;
  }
}

// The set behind a '[' at p, up to and including its ']'. *neg: it began with '^' (not yet complemented).
inline bool bracket(const uint8_t*& p, const uint8_t* e, ByteSet* s, bool* neg) {
  if (p < e && *p == ':') return false;                                    // [: is reserved (POSIX classes)
  *neg = p < e && *p == '^';
  if (*neg) p++;
  for (bool first = true;; first = false) {
    if (p >= e) return false;                                              // unterminated
    uint32_t lo = *p++;
    if (lo == ']' && !first) return true;
    if (lo == '[' && p < e && *p == ':') return false;                     // [[:alpha:]] is reserved
    bool cls = false;
    if (lo == '\\') {
      ByteSet c;
      const int k = escape(p, e, &lo, &c);
      if (!k) return false;
      if (k == 2) { s->join(c); cls = true; }
    }
    const bool range = e - p >= 2 && p[0] == '-' && p[1] != ']';           // a '-' that is neither first nor last
    if (cls) { if (range) return false; continue; }                        // a class is no range end
    if (!range) { s->add(lo); continue; }
    p++;
    uint32_t hi = *p++;
    if (hi == '[' && p < e && *p == ':') return false;
    if (hi == '\\') {
      ByteSet c;
      if (escape(p, e, &hi, &c) != 1) return false;
    }
    if (lo > hi) return false;
    s->add(lo, hi);
  }
}

// One element's final set from what the syntax gave: fold, complement, delimiter. soft: '.' or a complemented set loses the
// delimiter silently; anything else that holds it is refused, and so is an empty set.
inline bool finish(ByteSet* s, bool neg, bool soft, uint32_t syntax, int delimiter) {
  if (syntax & kFoldCase) s->fold();
  if (neg) s->complement();
  if (delimiter >= 0 && s->has((uint32_t)delimiter)) {
    if (!soft) return false;
    s->remove((uint32_t)delimiter);
  }
  return s->count() != 0;
}
}  // namespace detail

// The elements of one expression [p, e) behind out->elems. false: refused.
inline bool parse_expr(const uint8_t* p, const uint8_t* e, uint32_t syntax, int delimiter, std::vector<ByteSet>* out) {
  const size_t at = out->size();
  while (p < e) {
    ByteSet s;
    bool neg = false, soft = false;
    const uint8_t c = *p++;
    if (!(syntax & kClasses)) s.add(c);
    else switch (c) {
      case '.': s.complement(); soft = true; break;
      case '[': if (!detail::bracket(p, e, &s, &neg)) return false; soft = neg; break;
      case '\\': { uint32_t b = 0; const int k = detail::escape(p, e, &b, &s); if (!k) return false; if (k == 1) s.add(b); break; }
      case ']': case '*': case '+': case '?': case '{': case '}': case '(': case ')': case '|': case '^': case '$': return false;   // reserved
      default: s.add(c);
    }
    if (!detail::finish(&s, neg, soft, syntax, delimiter)) return false;
    if (out->size() - at == kMaxElements) return false;
    out->push_back(s);
  }
  return out->size() > at;
}

// Rule 1 of the calls as far as the patterns go. hPat: the patterns (syntax without kClasses) or expressions laid end to end, hSizes
// their sizes in bytes; delimiter: the grep's and the extract's byte, -1: none (the multi search).
inline bool compile(const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, int delimiter, Compiled* out) {
  *out = Compiled();
  if (!hPat || !hSizes || nPat == 0 || nPat > kMaxPatterns || (syntax & ~(kFoldCase | kClasses)) || delimiter < -1 || delimiter > 255) return false;
  const uint64_t maxBytes = (syntax & kClasses) ? kMaxExprBytes : kMaxElementsAll;
  uint64_t bytes = 0;
  for (size_t i = 0; i < nPat; i++) {
    if (hSizes[i] == 0 || hSizes[i] > maxBytes) { out->bad = (int)i; return false; }
    bytes += hSizes[i];
  }
  if (bytes > maxBytes) return false;
  const uint8_t* p = hPat;
  for (size_t i = 0; i < nPat; p += hSizes[i], i++) {
    out->bad = (int)i;
    const size_t at = out->elems.size();
    if (!parse_expr(p, p + hSizes[i], syntax, delimiter, &out->elems)) return false;
    const uint32_t m = (uint32_t)(out->elems.size() - at);
    if (out->elems.size() > kMaxElementsAll) return false;
    out->off.push_back((uint32_t)at); out->len.push_back(m);
    if (m > out->M) out->M = m;
    if (m < out->mMin) out->mMin = m;
  }
  out->codes.reserve(out->elems.size());
  for (size_t k = 0, i = 0; k < out->elems.size(); k++) {
    while (k >= (size_t)out->off[i] + out->len[i]) i++;
    out->bad = (int)i;
    const ByteSet& s = out->elems[k];
    const uint32_t n = s.count(), b = s.lowest();
    if (n == 1) { out->codes.push_back((uint16_t)(kCodeByte | b)); continue; }
    if (n == 2 && is_letter(b) && b < 'a' && s.has(b | 0x20)) { out->codes.push_back((uint16_t)(kCodePair | b | 0x20)); continue; }
    size_t c = 0;
    while (c < out->sets.size() && !(out->sets[c] == s)) c++;
    if (c == out->sets.size()) {
      if (c == kMaxSets) return false;
      out->sets.push_back(s);
    }
    out->codes.push_back((uint16_t)(kCodeSet | c));
  }
  out->bad = -1;
  return true;
}

}  // namespace zra_expr
