// Walks zra_amd/csrc/zra_regex.h on the CPU: every refusal of ZraHipCheckRegex with its reason and expression index, the limits at
// and one beyond each bound (64 / 65 expressions, 16,384 / 16,385 bytes, 4,096 / 4,097 positions, 64 / 65 states, {255} / {256}), the
// construction bound, answers pinned by hand for the accepted expressions, and every truncation of every accepted expression. The
// expression bytes and the sizes lie in heap blocks of exactly their size, so that under -fsanitize=address,undefined a read behind
// hPatterns + the sum of the sizes ends the run. Includes only that header.
//   g++ -std=c++17 -fsanitize=address,undefined -I zra_amd/csrc tools/model/regex_check.cpp -o regex_check
//   ./regex_check          exit 0 and "regex_check: N cases ok", or the failing cases and exit 1
//   ./regex_check --dump   also one line per compiled list: "case <fold> <delimiter> <hex,hex,...> <ok> <why> <pattern> <states>
//                          <classes> <positions>", for a second implementation to be held against (tests/test_regex_abi.py)
#include "zra_regex.h"

#include <cstdio>
#include <memory>
#include <string>

using namespace zra_regex;

namespace {
int g_cases = 0, g_failed = 0;
bool g_dump = false, g_deep = false;   // g_deep: nesting that a recursive second implementation need not follow, left out of the dump

typedef std::vector<std::string> List;

struct Result { bool ok; Info info; std::unique_ptr<Compiled> c; };

// compile() on exact-size heap copies
Result run(const List& list, bool fold, int delim) {
  size_t bytes = 0;
  for (auto& s : list) bytes += s.size();
  std::unique_ptr<uint8_t[]> pat(new uint8_t[bytes ? bytes : 1]);
  std::unique_ptr<uint32_t[]> sizes(new uint32_t[list.size() ? list.size() : 1]);
  size_t at = 0;
  for (size_t i = 0; i < list.size(); i++) { std::memcpy(pat.get() + at, list[i].data(), list[i].size()); at += list[i].size(); sizes[i] = (uint32_t)list[i].size(); }
  Result r;
  r.c.reset(new Compiled());
  r.ok = compile(bytes ? pat.get() : pat.get() + 1, list.size() ? sizes.get() : sizes.get() + 1, list.size(), fold ? 1u : 0u, delim, r.c.get());
  r.info = r.c->info;
  g_cases++;
  if (g_dump && !g_deep) {
    std::printf("case %d %d ", (int)fold, delim);
    for (size_t i = 0; i < list.size(); i++) {
      if (i) std::printf(",");
      for (unsigned char ch : list[i]) std::printf("%02x", ch);
    }
    std::printf(" %d %u %u %u %u %u\n", (int)r.ok, r.info.why, r.info.pattern, r.info.states, r.info.classes, r.info.positions);
  }
  if (r.ok != (r.info.why == kAccepted)) { g_failed++; std::printf("FAILED: the status and why disagree\n"); }
  return r;
}

void fail(const char* what, const List& list) {
  g_failed++;
  std::printf("FAILED %s:", what);
  for (auto& s : list) std::printf(" '%.60s'", s.c_str());
  std::printf("\n");
}

void refused(const List& list, uint32_t why, uint32_t pattern = 0, bool fold = false, int delim = '\n') {
  const Result r = run(list, fold, delim);
  if (r.ok || r.info.why != why || r.info.pattern != pattern || r.info.states || r.info.classes || r.info.positions) fail("a refusal", list);
}

std::vector<List> g_accepted;

// accepted, with answers: yes / no are records
Result accepted(const List& list, const List& yes, const List& no, bool fold = false, int delim = '\n') {
  Result r = run(list, fold, delim);
  if (!r.ok) { fail("an accepted list", list); return r; }
  const Table& t = r.c->table;
  if (t.states != r.info.states || t.classes != r.info.classes || t.start >= t.states || t.states > kMaxStates || t.classes > 255) fail("the table's head", list);
  for (uint32_t c = 0; c < 256; c++) for (uint32_t s = 0; s < 64; s++) if (t.next[c][s] >= t.states || (c >= t.classes && t.next[c][s])) fail("the table's rows", list);
  for (uint32_t b = 0; b < 256; b++) if (t.classOf[b] >= t.classes) fail("the table's classes", list);
  for (auto& s : yes) { g_cases++; if (!matches(t, (const uint8_t*)s.data(), s.size())) fail(("no match in '" + s + "'").c_str(), list); }
  for (auto& s : no) { g_cases++; if (matches(t, (const uint8_t*)s.data(), s.size())) fail(("a match in '" + s + "'").c_str(), list); }
  if (!fold && delim == '\n') g_accepted.push_back(list);
  return r;
}

std::string times(const std::string& s, size_t n) { std::string r; for (size_t i = 0; i < n; i++) r += s; return r; }
}  // namespace

int main(int argc, char** argv) {
  g_dump = argc > 1 && std::string(argv[1]) == "--dump";

  // ---- arguments and size limits (reason 1)
  { Compiled c; g_cases++; uint32_t one = 1; if (compile(nullptr, &one, 1, 0, '\n', &c) || c.info.why != kWhyArguments) fail("hPatterns NULL", {}); }
  { Compiled c; g_cases++; if (compile((const uint8_t*)"a", nullptr, 1, 0, '\n', &c) || c.info.why != kWhyArguments) fail("hPatternSizes NULL", {}); }
  refused({}, kWhyArguments);
  refused({"a", ""}, kWhyArguments);
  { Compiled c; g_cases++; uint32_t one = 1; if (compile((const uint8_t*)"a", &one, 1, 2, '\n', &c) || c.info.why != kWhyArguments) fail("syntax bit 2", {}); }
  { Compiled c; g_cases++; uint32_t one = 1; if (compile((const uint8_t*)"a", &one, 1, 4, '\n', &c) || c.info.why != kWhyArguments) fail("syntax bit 4", {}); }
  { Compiled c; g_cases++; uint32_t one = 1; if (compile((const uint8_t*)"a", &one, 1, 0, -1, &c) || c.info.why != kWhyArguments) fail("delimiter -1", {}); }
  { Compiled c; g_cases++; uint32_t one = 1; if (compile((const uint8_t*)"a", &one, 1, 0, 256, &c) || c.info.why != kWhyArguments) fail("delimiter 256", {}); }
  accepted(List(64, "a"), {"a", "ba"}, {"", "b"});
  refused(List(65, "a"), kWhyArguments);
  accepted({"[" + times("a", 16382) + "]"}, {"a"}, {"b"});                                     // 16,384 bytes, one position
  refused({"[" + times("a", 16383) + "]"}, kWhyArguments);
  refused({"[" + times("a", 16382) + "]", "("}, kWhyArguments);                                // (the sizes are summed before a byte is read)
  { List l(64, "a^b{62}"); const Result r = accepted(l, {}, {"", "ab", "a"}); if (r.ok && (r.info.positions != 4096 || r.info.states != 1)) fail("4,096 positions", l); }
  { List l(64, "a^b{62}"); l[63] = "a^b{63}"; refused(l, kWhyArguments); }
  { List l(64, "a^b{62}"); l[0] = "a^b{63}"; l[63] = ")"; refused(l, kWhySyntax, 63); }        // (syntax is checked before the positions are counted)
  refused({"((a{255}){255}){255}"}, kWhyArguments);                                            // (counted without being expanded)
  refused({"(((((((a{255}){255}){255}){255}){255}){255}){255}){255}"}, kWhyArguments);         // (and without overflow)
  accepted({"((a{255}){255}){0}b"}, {"b"}, {"a", ""});

  // ---- syntax (reason 2), with the expression's index
  for (const char* e : {"*a", "+a", "?a", "{2}a", "(*a)", "(+a)", "a|*b", "a|?", "a**", "a*?", "a+?", "a*+", "a?*", "a{2}*", "a*{2}", "a{2}{3}", "^*", "$+", "^?", "a$*",
                        "^{2}", "()", "a()", "(())", "a|", "|a", "(a|)", "(|a)", "a||b", "(a", "a)", "((a)", "(a))", ")", "(", "a{", "a{}", "a{,3}", "a{,}", "a{2", "a{2,",
                        "a{2,3", "a{3,2}", "a{256}", "a{0,256}", "a{1000}", "a{2,x}", "a{x}", "a{2 }", "a{-1}", "a]", "]", "a}", "}", "a{2}}", "[:alpha:]", "[[:alpha:]]",
                        "[a", "[", "[^", "[]", "[b-a]", "[a-\\d]", "[\\d-z]", "\\", "a\\", "\\q", "\\x4", "\\xg0", "\\", "[\\q]", "(a|b", "a|b)", "|", "(|)"}) {
    refused({e}, kWhySyntax, 0);
    refused({"ok", e}, kWhySyntax, 1);
    refused({"ok", "(fine)+", e, "*"}, kWhySyntax, 2);
  }
  // ---- an atom that only the delimiter would match (reason 3)
  for (const char* e : {"\\n", "[\\n]", "a\\nb", "[\\n\\n]", "(a|\\n)", "\\x0a", "\\x0A+", "[\\x0a-\\x0a]"}) { refused({e}, kWhyEmptyAtom, 0); refused({"a", e}, kWhyEmptyAtom, 1); }
  refused({"a"}, kWhyEmptyAtom, 0, false, 'a');
  refused({"A"}, kWhyEmptyAtom, 0, false, 'A');
  accepted({"A"}, {"a"}, {"b"}, true, 'A');                                                    // (folded first, then the delimiter leaves: a is left)
  refused({"[^\\x00-\\xff]"}, kWhyEmptyAtom, 0);
  refused({"[a", "\\n"}, kWhySyntax, 0);                                                        // (the first refusal in reading order)
  refused({"\\n", "[a"}, kWhyEmptyAtom, 0);
  refused({"\\n)"}, kWhyEmptyAtom, 0);
  refused({"*\\n"}, kWhySyntax, 0);
  accepted({"a"}, {"a", "A"}, {"c"}, true, 'b');
  accepted({"[ab]"}, {"b"}, {"c", ""}, false, 'a');                                            // (the delimiter leaves silently)
  accepted({"\\s+x", "[ \\n]y"}, {" x", "\t\tx", " y"}, {"x", "y", "\ty"});
  accepted({".", "[^a]"}, {"a", "b"}, {""});

  // ---- the state limit and the construction bound (reason 4)
  { const Result r = accepted({"^.{62}$"}, {times("x", 62)}, {times("x", 61), times("x", 63), ""}); if (r.ok && r.info.states != 64) fail("64 states", {"^.{62}$"}); }
  refused({"^.{63}$"}, kWhyStates);
  refused({"(a|b)*a(a|b){10}$"}, kWhyStates);                                                   // 2,048 states from fewer than 4,096 sets
  refused({"(a|b)*a(a|b){12}$"}, kWhyStates);                                                   // the construction bound
  refused({"(a|b)*a(a|b){40}$"}, kWhyStates);
  refused({"a{255}"}, kWhyStates);
  accepted({"a{255}", "a*"}, {"", "b"}, {});
  refused({"a{256}", "a*"}, kWhySyntax, 0);

  // ---- answers pinned by hand
  accepted({"status=5[0-9]+ .*timeout"}, {"x status=503 upstream timeout", "status=50 timeout"}, {"status=5 timeout", "status=503timeout", "status=403 timeout"});
  accepted({"^(GET|POST) /api/"}, {"GET /api/x", "POST /api/"}, {" GET /api/", "PUT /api/", "GET/api/"});
  accepted({"took [0-9]{4,}ms$"}, {"took 1234ms", "x took 123456ms"}, {"took 123ms", "took 1234ms "});
  accepted({"^$"}, {""}, {"a", " "});
  accepted({"a*"}, {"", "b", "aaa"}, {});
  accepted({"a^b"}, {}, {"", "ab", "b", "a"});
  accepted({"^^a"}, {}, {"a", ""});
  accepted({"$$"}, {}, {"", "a"});
  accepted({"(^)+a"}, {"ab"}, {"ba"});
  accepted({"(^a|b$)"}, {"ax", "xb"}, {"xa", "bx"});
  accepted({"^(..)*$"}, {"", "ab", "abcd"}, {"a", "abc"});
  accepted({"a{0}b"}, {"b", "ab"}, {"a"});
  accepted({"a{0,0}"}, {"", "x"}, {});
  accepted({"^a{2,3}$"}, {"aa", "aaa"}, {"a", "aaaa", ""});
  accepted({"^a{2,}$"}, {"aa", "aaaaa"}, {"a", ""});
  accepted({"^(ab|c)?d$"}, {"d", "abd", "cd"}, {"ad", "abcd"});
  accepted({"^((a|b)c)+$"}, {"ac", "acbc"}, {"", "a", "acb"});
  accepted({"x(a|^)^b"}, {}, {"b", "xab", "xb"});
  accepted({"^[^a-c]\\.[\\]x-]$"}, {"d.]", "z.-", "d.x"}, {"a.]", "dx]", "d.y"});
  accepted({"^\\x41\\t\\w\\d\\s$"}, {"A\t_0 ", "A\tz9\r"}, {"a\t_0 ", "A\t-0 "});
  accepted({"^abc$"}, {"abc", "ABC", "aBc"}, {"abcd"}, true);
  accepted({"^[^a]$"}, {"b"}, {"a", "A"}, true);
  accepted({"^[A-C]+$"}, {"abc", "CBA"}, {"d"}, true);
  accepted({"^[@-\\[]$"}, {"@", "[", "a"}, {"`", "{"}, true);
  accepted({"((((((((a))))))))"}, {"a"}, {""});
  accepted({"(a?)?", "b"}, {""}, {});
  accepted({"(a|b)*a(a|b){4}$"}, {"abbbb", "bbabaaa"}, {"bbbbb", "a"});
  accepted({"^(a(b(c(d)?)?)?)$"}, {"a", "ab", "abcd"}, {"abd", ""});
  accepted({"foo", "bar$", "^baz"}, {"xfoox", "xbar", "bazx"}, {"barx", "xbaz", "fo"});

  // ---- deep nesting: the parser keeps its own stack, and what recursion is left follows the positions, not the bytes
  g_deep = true;
  { const Result r = accepted({times("(a|", 1300) + "b" + times(")", 1300)}, {"a", "xb"}, {"c", ""}); if (r.ok && r.info.positions != 1301) fail("1,300 nested alternations", {}); }
  { const Result r = accepted({times("(", 8000) + "a" + times(")", 8000)}, {"a"}, {""}); if (r.ok && (r.info.positions != 1 || r.info.states != 2)) fail("8,000 nested groups", {}); }
  {
    std::string s = "a";
    for (int i = 0; i < 2000; i++) s = "(" + s + ")?b";
    const Result r = accepted({s}, {"b", "ab"}, {"a", ""});
    if (r.ok && (r.info.positions != 2001 || r.info.states != 2)) fail("2,000 nested optional groups", {});
  }
  refused({times("(", 8000) + "a" + times(")", 7999)}, kWhySyntax, 0);
  g_deep = false;

  // ---- every truncation of every accepted expression (each list's last expression, cut): accepted or refused, never a wild read
  const std::vector<List> full = g_accepted;
  for (const List& l : full) {
    if (l.back().size() > 64) continue;
    for (size_t n = 1; n < l.back().size(); n++) { List cut = l; cut.back() = l.back().substr(0, n); run(cut, false, '\n'); }
  }

  if (g_failed) { std::printf("regex_check: %d of %d cases FAILED\n", g_failed, g_cases); return 1; }
  std::printf("regex_check: %d cases ok\n", g_cases);
  return 0;
}
