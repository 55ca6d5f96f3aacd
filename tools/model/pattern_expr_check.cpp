// Walks zra_amd/csrc/zra_pattern_expr.h on the CPU: a table of expressions with the byte sets they must compile to, or their refusal;
// the limits at and one past their edge; and every truncation of every accepted expression, which must parse or be refused and nothing
// else. Every input lies in a heap block of exactly its size, so that under -fsanitize=address,undefined a read behind
// hPatterns + the sum of the sizes ends the run. Includes only that header.
//   g++ -std=c++17 -fsanitize=address,undefined -I zra_amd/csrc tools/model/pattern_expr_check.cpp -o pattern_expr_check
//   ./pattern_expr_check          exit 0 and "pattern_expr_check: N cases ok", or the failing cases and exit 1
//   ./pattern_expr_check --list   the table's single-expression cases, one per line: syntax delimiter hex(expression) ok|refused
//                                 (tests/test_pattern_expr.py holds ZraHipCheckPatternExpr and the Python model against the same table)
#include "zra_pattern_expr.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

using namespace zra_expr;

namespace {
int g_cases = 0, g_failed = 0;

struct Case {
  std::string expr;
  uint32_t syntax;
  int delim;
  const char* want;   // nullptr: refused; else one element per '|', each a list of hex bytes and ranges: "30-39 5f|61"
};

std::string B(std::initializer_list<int> v) { std::string s; for (int b : v) s.push_back((char)b); return s; }

// compile() on exact-size heap copies of the patterns and their sizes
bool run(const std::vector<std::string>& pats, uint32_t syntax, int delim, Compiled* C) {
  size_t bytes = 0;
  for (auto& p : pats) bytes += p.size();
  std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes ? bytes : 1]);
  std::unique_ptr<uint32_t[]> sizes(new uint32_t[pats.size() ? pats.size() : 1]);
  size_t at = 0;
  for (size_t i = 0; i < pats.size(); i++) { std::memcpy(buf.get() + at, pats[i].data(), pats[i].size()); at += pats[i].size(); sizes[i] = (uint32_t)pats[i].size(); }
  // (the block has `bytes` bytes: with none, a pointer one behind a one-byte block)
  return compile(bytes ? buf.get() : buf.get() + 1, sizes.get(), pats.size(), syntax, delim, C);
}

bool parse_want(const char* w, std::vector<ByteSet>* out) {
  ByteSet s;
  for (const char* p = w;; ) {
    if (*p == '|' || *p == 0) { out->push_back(s); s = ByteSet(); if (!*p) return true; p++; continue; }
    if (*p == ' ') { p++; continue; }
    char* e;
    const unsigned long lo = std::strtoul(p, &e, 16);
    unsigned long hi = lo;
    if (*e == '-') hi = std::strtoul(e + 1, &e, 16);
    if (e == p || lo > hi || hi > 255) return false;
    s.add((uint32_t)lo, (uint32_t)hi);
    p = e;
  }
}

std::string hex(const std::string& s) { std::string o; char b[3]; for (unsigned char c : s) { std::snprintf(b, 3, "%02x", c); o += b; } return o; }

void fail(const char* what, const std::string& expr, uint32_t syntax, int delim) {
  g_failed++;
  std::printf("FAIL %s: syntax %u delimiter %d expression %s\n", what, syntax, delim, hex(expr).c_str());
}

void check(const Case& c) {
  g_cases++;
  Compiled C;
  const bool ok = run({c.expr}, c.syntax, c.delim, &C);
  if (!c.want) { if (ok) fail("accepted", c.expr, c.syntax, c.delim); return; }
  if (!ok) { fail("refused", c.expr, c.syntax, c.delim); return; }
  std::vector<ByteSet> want;
  if (!parse_want(c.want, &want)) { fail("table", c.expr, c.syntax, c.delim); return; }
  if (C.elems.size() != want.size() || C.len.size() != 1 || C.len[0] != want.size() || C.off[0] != 0 || C.M != want.size() || C.mMin != want.size()) {
    fail("length", c.expr, c.syntax, c.delim);
    return;
  }
  for (size_t k = 0; k < want.size(); k++) {
    if (!(C.elems[k] == want[k])) { fail("set", c.expr, c.syntax, c.delim); return; }
    // the element's code says the same as its set
    const uint16_t code = C.codes[k];
    ByteSet s;
    if (code < kCodePair) s.add(code);
    else if (code < kCodeSet) { s.add(code & 0xFF); s.add((code & 0xFF) ^ 0x20); }
    else if ((size_t)(code & 0xFF) < C.sets.size()) s = C.sets[code & 0xFF];
    if (!(s == want[k])) { fail("code", c.expr, c.syntax, c.delim); return; }
  }
  // every truncation parses or is refused (and reads nothing behind its end: the block is exactly as long)
  for (size_t n = 0; n < c.expr.size(); n++) { Compiled T; run({c.expr.substr(0, n)}, c.syntax, c.delim, &T); g_cases++; }
}

void expect(bool got, bool want, const char* what) {
  g_cases++;
  if (got != want) { g_failed++; std::printf("FAIL %s: %s\n", what, got ? "accepted" : "refused"); }
}

const char* kAll = "00-ff";
const char* kW = "30-39 41-5a 5f 61-7a";

std::vector<Case> table() {
  std::vector<Case> t = {
    // ---- escapes
    {"\\x41", 2, -1, "41"}, {"\\x4a", 2, -1, "4a"}, {"\\x4A", 2, -1, "4a"}, {"\\xfF", 2, -1, "ff"}, {"\\x00", 2, -1, "00"},
    {"\\n", 2, -1, "0a"}, {"\\t", 2, -1, "09"}, {"\\r", 2, -1, "0d"},
    {"\\d", 2, -1, "30-39"}, {"\\w", 2, -1, kW}, {"\\s", 2, -1, "09-0d 20"}, {"\\d\\d\\d", 2, -1, "30-39|30-39|30-39"},
    {"\\q", 2, -1, nullptr}, {"\\", 2, -1, nullptr}, {"a\\", 2, -1, nullptr}, {"\\x4", 2, -1, nullptr}, {"\\x", 2, -1, nullptr}, {"\\xg0", 2, -1, nullptr},
    {"\\x0g", 2, -1, nullptr}, {"\\0", 2, -1, nullptr}, {"\\a", 2, -1, nullptr}, {"\\D", 2, -1, nullptr}, {"\\W", 2, -1, nullptr}, {"\\S", 2, -1, nullptr},
    {"\\v", 2, -1, nullptr}, {"\\f", 2, -1, nullptr}, {"\\:", 2, -1, nullptr}, {B({'\\', 0x80}), 2, -1, nullptr}, {B({'\\', 0}), 2, -1, nullptr},
    // ---- sets
    {"[]]", 2, -1, "5d"}, {"[^]]", 2, -1, "00-5c 5e-ff"}, {"[a-]", 2, -1, "2d 61"}, {"[-a]", 2, -1, "2d 61"}, {"[z-a]", 2, -1, nullptr},
    {"[\\d-z]", 2, -1, nullptr}, {"[a-\\d]", 2, -1, nullptr}, {"[\\w-]", 2, -1, "2d 30-39 41-5a 5f 61-7a"}, {"[a-c]", 2, -1, "61-63"}, {"[a-a]", 2, -1, "61"},
    {"[\\x30-\\x39]", 2, -1, "30-39"}, {"[^\\x00-\\xff]", 2, -1, nullptr}, {"[\\x00-\\xff]", 2, -1, kAll}, {"[", 2, -1, nullptr}, {"[a", 2, -1, nullptr},
    {"[a-", 2, -1, nullptr}, {"[a-z", 2, -1, nullptr}, {"[^", 2, -1, nullptr}, {"[]", 2, -1, nullptr}, {"[^]", 2, -1, nullptr}, {"[a\\", 2, -1, nullptr},
    {"[a-\\", 2, -1, nullptr}, {"[a-\\x4", 2, -1, nullptr}, {"[\\x4]", 2, -1, nullptr},
    {"[:alpha:]", 2, -1, nullptr}, {"[[:alpha:]]", 2, -1, nullptr}, {"[a[:]", 2, -1, nullptr}, {"[a-[:]", 2, -1, nullptr}, {"[^:]", 2, -1, "00-39 3b-ff"},
    {"[a:]", 2, -1, "3a 61"}, {"[[]", 2, -1, "5b"}, {"[[a]", 2, -1, "5b 61"},
    {"[\\d\\s]", 2, -1, "09-0d 20 30-39"}, {"[.]", 2, -1, "2e"}, {"[*+?{}()|$]", 2, -1, "24 28-2b 3f 7b-7d"}, {"[a^]", 2, -1, "5e 61"}, {"[\\]]", 2, -1, "5d"},
    {"[\\\\]", 2, -1, "5c"}, {"[a\\-z]", 2, -1, "2d 61 7a"}, {"[a-c-e]", 2, -1, "2d 61-63 65"}, {"[--0]", 2, -1, "2d-30"}, {"[0-9a-f]", 2, -1, "30-39 61-66"},
    {"[\\n-\\r]", 2, -1, "0a-0d"}, {"[^0-9]", 2, -1, "00-2f 3a-ff"}, {"x[0-9].", 2, -1, "78|30-39|00-ff"},
    // ---- every other byte is a literal
    {".", 2, -1, kAll}, {B({0}), 2, -1, "00"}, {B({0x80}), 2, -1, "80"}, {B({0xff, 'a', 0}), 2, -1, "ff|61|00"}, {"a-b", 2, -1, "61|2d|62"}, {"-", 2, -1, "2d"},
    {":", 2, -1, "3a"}, {"a b", 2, -1, "61|20|62"}, {"status=5[0-9][0-9]", 2, -1, "73|74|61|74|75|73|3d|35|30-39|30-39"}, {"\\x3d", 2, -1, "3d"},
    {"20..-..-.. ", 2, -1, "32|30|00-ff|00-ff|2d|00-ff|00-ff|2d|00-ff|00-ff|20"},
    // ---- without CLASSES every byte is a literal
    {"a.[", 0, -1, "61|2e|5b"}, {"\\", 0, -1, "5c"}, {"*", 1, -1, "2a"}, {"aB.", 1, -1, "41 61|42 62|2e"}, {"[", 1, -1, "5b"},
    // ---- fold
    {"a", 3, -1, "41 61"}, {"A", 3, -1, "41 61"}, {"z", 3, -1, "5a 7a"}, {"Z", 1, -1, "5a 7a"}, {"@[`{", 1, -1, "40|5b|60|7b"}, {"@\\[`\\{", 3, -1, "40|5b|60|7b"},
    {B({0xc1}), 3, -1, "c1"}, {B({0xe1}), 3, -1, "e1"}, {B({0xc1, 0xe1}), 1, -1, "c1|e1"}, {"\\xc1", 3, -1, "c1"}, {"\\xe1", 3, -1, "e1"},
    {"[a-c]", 3, -1, "41-43 61-63"}, {"[^a]", 3, -1, "00-40 42-60 62-ff"}, {"[^A]", 3, -1, "00-40 42-60 62-ff"}, {"[@-\\x5b]", 3, -1, "40-5b 61-7a"},
    {"[\\xc1]", 3, -1, "c1"}, {"\\w", 3, -1, kW}, {"\\d", 3, -1, "30-39"}, {".", 3, -1, kAll}, {"eRrOr", 3, -1, "45 65|52 72|52 72|4f 6f|52 72"},
    {"[`{]", 3, -1, "60 7b"}, {"\\x41", 3, -1, "41 61"},
    // ---- the delimiter
    {".", 2, 10, "00-09 0b-ff"}, {"[^a]", 2, 10, "00-09 0b-60 62-ff"}, {"[\\n]", 2, 10, nullptr}, {"\\n", 2, 10, nullptr}, {"a\nb", 2, 10, nullptr},
    {"a\nb", 0, 10, nullptr}, {"a\nb", 1, 10, nullptr}, {"a\nb", 2, -1, "61|0a|62"}, {"\\s", 2, 10, nullptr}, {"[^\\s]", 2, 10, "00-08 0e-1f 21-ff"},
    {"[\\x00-\\x20]", 2, 10, nullptr}, {"[^\\x00-\\x09\\x0b-\\xff]", 2, 10, nullptr}, {"[^\\x00-\\x09\\x0b-\\xff]", 2, -1, "0a"},
    {"a", 1, 'A', nullptr}, {"A", 3, 'a', nullptr}, {"[a-c]", 3, 'B', nullptr}, {"[^a]", 3, 'A', "00-40 42-60 62-ff"}, {"[^b]", 3, 'A', "00-40 43-61 63-ff"},
    {"a", 0, 'A', "61"}, {"a", 2, 'A', "61"}, {".", 2, 0, "01-ff"}, {B({'a', 0}), 2, 0, nullptr}, {".", 2, 255, "00-fe"}, {"x;y", 2, ';', nullptr},
    // ---- the syntax word and the delimiter's range
    {"a", 4, -1, nullptr}, {"a", 0x80000000u, -1, nullptr}, {"a", 7, -1, nullptr}, {"a", 2, 256, nullptr}, {"a", 2, -2, nullptr},
  };
  // every escapable byte, escaped outside and inside a set; every reserved byte, alone and behind a literal
  for (const char* p = ".[]\\*+?{}()|^$-"; *p; p++) {
    static char want[16][3];
    char* w = want[p - ".[]\\*+?{}()|^$-"];
    std::snprintf(w, 3, "%02x", (unsigned)*p);
    t.push_back({std::string("\\") + *p, 2, -1, w});
    t.push_back({std::string("[\\") + *p + "]", 2, -1, w});
  }
  for (const char* p = "]*+?{}()|^$"; *p; p++) {
    t.push_back({std::string(1, *p), 2, -1, nullptr});
    t.push_back({std::string("a") + *p, 3, -1, nullptr});
  }
  return t;
}

std::string set_expr(int k) { char b[16]; std::snprintf(b, sizeof b, "[\\x%02x\\x%02x]", 0x80 + k, 0xC0 + k); return b; }   // 64 distinct two-byte sets

void limits() {
  Compiled C;
  // ---- counted sets: 32 accepted, 33 refused, in one pattern and across patterns; what does not count; equal sets once
  std::string e32, e33;
  std::vector<std::string> p32, p33;
  for (int k = 0; k < 33; k++) { if (k < 32) { e32 += set_expr(k); p32.push_back(set_expr(k)); } e33 += set_expr(k); p33.push_back(set_expr(k)); }
  expect(run({e32}, 2, -1, &C) && C.sets.size() == 32, true, "32 sets in one pattern");
  expect(run({e33}, 2, -1, &C), false, "33 sets in one pattern");
  expect(run(p32, 2, -1, &C) && C.sets.size() == 32, true, "32 sets in 32 patterns");
  expect(run(p33, 2, -1, &C), false, "33 sets in 33 patterns");
  expect(run({e32 + "[aA][b]x[Zz]" + e32 + "\\x41"}, 2, -1, &C) && C.sets.size() == 32 && C.len[0] == 69, true, "single bytes, letter pairs and repeats are not counted");
  expect(run({e32 + "abc[q]"}, 3, -1, &C) && C.sets.size() == 32, true, "folded letters are not counted");
  expect(run({e32 + "[ab]"}, 2, -1, &C), false, "a two-byte set that is no letter pair counts");
  expect(run({e32 + "[a-b]"}, 3, -1, &C), false, "two folded letters count");
  expect(run({e32 + "[@`]"}, 2, -1, &C), false, "@ and ` are no letter pair");
  expect(run({e32 + B({'[', 0xC1, 0xE1, ']'})}, 2, -1, &C), false, "0xC1 and 0xE1 are no letter pair");
  expect(run({std::string("[0-9]\\d[0-9][9876543210]"), std::string("\\d."), std::string(".[\\x00-\\xff]")}, 2, -1, &C) && C.sets.size() == 2, true, "equal sets count once");
  expect(run({std::string("..")}, 2, 10, &C) && C.sets.size() == 1, true, "two dots are one set");
  // ---- patterns: 1 .. 64
  expect(run({}, 2, -1, &C), false, "no pattern");
  expect(run(std::vector<std::string>(64, "a"), 2, -1, &C) && C.len.size() == 64, true, "64 patterns");
  expect(run(std::vector<std::string>(65, "a"), 2, -1, &C), false, "65 patterns");
  expect(run({"a", ""}, 2, -1, &C), false, "an empty expression");
  expect(run({"a", ""}, 0, -1, &C), false, "an empty pattern");
  // ---- elements: 256 per pattern, 4,096 in all
  for (uint32_t syntax : {0u, 1u, 2u, 3u}) {
    expect(run({std::string(256, 'a')}, syntax, -1, &C) && C.M == 256, true, "256 elements");
    expect(run({std::string(257, 'a')}, syntax, -1, &C), false, "257 elements");
    std::vector<std::string> all(16, std::string(256, '.'));
    expect(run(all, syntax, -1, &C) && C.elems.size() == 4096 && C.mMin == 256, true, "4,096 elements in all");
    all.push_back("a");
    expect(run(all, syntax, -1, &C), false, "4,097 elements in all");
  }
  expect(run({std::string(255, '.') + "[ab]"}, 2, -1, &C) && C.M == 256, true, "256 elements, the last a set");
  expect(run({std::string(255, '.') + "[ab]c"}, 2, -1, &C), false, "257 elements, a set among them");
  // ---- expression bytes: 16,384 in all, with no more than 4,095 elements either way
  for (int over = 0; over < 2; over++) {
    std::vector<std::string> pats;
    std::string cur;
    uint32_t elems = 0;
    auto add = [&](const std::string& e) { if (elems && elems % 256 == 0) { pats.push_back(cur); cur.clear(); } cur += e; elems++; };
    for (int k = 0; k < 4093; k++) add("\\x41");
    add("[\\x41a]");
    add(over ? "[\\x41]" : "[abc]");
    pats.push_back(cur);
    size_t bytes = 0;
    for (auto& p : pats) bytes += p.size();
    expect(bytes == (over ? 16385u : 16384u) && elems == 4095, true, "the sizes of the expression-bytes case");
    expect(run(pats, 2, -1, &C), !over, over ? "16,385 expression bytes" : "16,384 expression bytes");
  }
  expect(run({std::string(16385, 'a')}, 2, -1, &C), false, "one expression of 16,385 bytes");
  expect(run({std::string(4097, 'a')}, 0, -1, &C), false, "one literal pattern of 4,097 bytes");
  // ---- null arguments
  uint32_t one = 1;
  const uint8_t a = 'a';
  expect(compile(nullptr, &one, 1, 2, -1, &C), false, "hPatterns NULL");
  expect(compile(&a, nullptr, 1, 2, -1, &C), false, "hPatternSizes NULL");
  // ---- a refused pattern is named
  expect(!run({"a", "b", "c)"}, 2, -1, &C) && C.bad == 2, true, "the refused pattern's index");
  expect(!run({"a", "[z-a]", "c"}, 2, -1, &C) && C.bad == 1, true, "the refused pattern's index");
}
}  // namespace

int main(int argc, char** argv) {
  const std::vector<Case> t = table();
  if (argc > 1 && !std::strcmp(argv[1], "--list")) {
    for (const Case& c : t) std::printf("%u %d %s %s\n", c.syntax, c.delim, hex(c.expr).c_str(), c.want ? c.want : "refused");
    return 0;
  }
  for (const Case& c : t) check(c);
  limits();
  if (g_failed) { std::printf("pattern_expr_check: %d of %d cases FAILED\n", g_failed, g_cases); return 1; }
  std::printf("pattern_expr_check: %d cases ok\n", g_cases);
  return 0;
}
