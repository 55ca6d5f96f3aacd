// zratool_amd — command-line counterpart of the reference's programs/zratool.cpp: same modes, same argv, same output names
//   zratool_amd c|imc|d|imd|b {file} ...     (zratool.cpp:98-286; the positions are listed above main)
// written against include/zra.hpp only, so it doubles as a source-compatibility check of the C++ API.
//   c   : streaming compress  (Compressor, 10 MB chunks rounded to the frame size, header written last at offset 0)
//   d   : streaming decompress (FullDecompressor)
//   imc : in-memory CompressBuffer          imd : in-memory DecompressBuffer
//   b   : benchmark of all four + one random-access query with a memcmp check
// and four modes of its own, against include/zra_hip.h:
//   t   : test an archive like `zstd -t` (ZraHipVerifyArchive, content verification on the device); one line per faulty frame and a
//         summary; exit status 0 clean, 1 faults, 2 the call failed
//   g   : search an archive like `zstdgrep -F -b -o` (ZraHipSearchArchive, decode and scan on the device); one content offset per line
//         and a summary; exit status as grep: 0 matches, 1 none, 2 trouble
//   gm  : the same for 1 to 64 patterns in one pass, like `grep -F -f` (ZraHipSearchArchiveMulti); `offset<TAB>pattern index` per line
//         and a summary; exit status as g
//   gl  : the records (lines) that hold a match, like `grep -F -f -b` without the text (ZraHipGrepArchive); -v: the records that hold
//         none, -d {hex byte}: the delimiter (default 0a); `offset<TAB>size` per selected record (the first 2^20; the summary counts
//         all) and a summary; exit status as grep: 0 some, 1 none, 2 trouble
//   gx  : the text of those records, what `grep -F -f` prints (ZraHipExtractRecords): every selected record and its delimiter, packed on
//         the device, to stdout or with -o {file} to a file; -v and -d as gl; exit status as grep, and no output when nothing is selected
//   gme, gle, gxe: gm, gl and gx with pattern expressions (ZraHipSearchArchiveMultiExpr, ZraHipGrepArchiveExpr, ZraHipExtractRecordsExpr):
//         a pattern is an expression of fixed length, . [set] [^set] \escape (zra_hip.h: ZraHipCheckPatternExpr); -i: ASCII letters
//         match either case, -F: the patterns are literal after all; behind "hex:" a pattern is literal bytes either way. A refused
//         expression is exit status 2 with a message that names the pattern's index; otherwise output and exit status of gm, gl, gx
//   glw : gle with a record predicate (ZraHipGrepArchiveWhere): one or more -w {clause}; a clause is comma-separated items +i (pattern i
//         must occur in the record), ?i (one of the ?-patterns must), -i (pattern i must not), i = the pattern's position on the command
//         line from 0; a record is selected when some clause holds, -v complements that. Output and exit status of gl; a refused
//         clause is exit status 2
//   gxw : gxe with glw's record predicate (ZraHipExtractRecordsWhere): the text `grep A | grep B | grep -v C` prints; -w as glw, -o, -v,
//         -d, -i, -F as gxe. Output and exit status of gx; a refused clause is exit status 2
//   cut : gx with cut's field selection (ZraHipCutRecords): of every selected record only the fields of LIST (cut's: 1,3,5-7,9-), cut
//         at the separator byte; both stand in front of the patterns, and no pattern at all selects every record. -o, -v, -d as gx.
//         Output and exit status of gx; a refused separator or list is exit status 2
//   tally : cut, counted (ZraHipTallyFields): one line per distinct value of the cut's output in order of first appearance, `count key`:
//         the counts `cut ... | sort | uniq -c` prints. Separator, list and patterns as cut; -v, -d as gx. Exit status of gx
//   glr : gl with regular expressions (ZraHipGrepArchiveRegex): POSIX extended expressions over bytes, * + ? {n,m} ( ) | ^ $ on top of
//         gle's atoms (zra_hip.h: ZraHipCheckRegex); several expressions are alternatives; -i: ASCII letters match either case, -v, -d as
//         gl; -c: only the count. Output and exit status of gl; a refused expression is exit status 2 with the reason and its index
//   gxr : gx with glr's regular expressions (ZraHipExtractRecordsRegex): the text `grep -E` prints; -i, -v, -d as glr, -o as gx. Output
//         and exit status of gx; a refused expression as glr
//   cmp : compare the contents of two archives like `cmp` (ZraHipCompareArchives, on the device); one line `offset size` per differing
//         range (the first 2^20; the summary counts all) and a summary; exit status as cmp: 0 equal content and equal length, 1 different, 2 trouble
//   diff: the patch that turns the content of archive A into that of archive B (ZraHipDiffArchives, on the device); one line `offset size`
//         per write, the tail and a summary; -g {grain}: a power of two from 1 to 8192 (default 1); exit status 0 empty patch, 1 not empty, 2 trouble
//   sign: the content signature of an archive (ZraHipSignArchive, on the device) into a file: the 40-byte little-endian ZraHipSignature,
//         then its words; -g {grain}: a power of two from 64 to 8192 (default 4096), -s {seed} (default 0); exit status 0 written, 2 trouble
//   sigdiff: diff with archive A given by its signature file (ZraHipDiffSignature): output and exit status of diff at the signature's grain
#include <zra.hpp>
#include <zra.h>
#include <zra_hip.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

zra::Buffer read_file(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) { std::perror(path); std::exit(2); }
  zra::Buffer b((size_t)f.tellg());
  f.seekg(0);
  f.read(reinterpret_cast<char*>(b.data()), (std::streamsize)b.size());
  return b;
}
void write_file(const char* path, const zra::u8* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)n);
}

size_t stream_compress(const char* in, const char* out, zra::i8 level, zra::u32 frameSize, size_t bufferSize) {
  std::ifstream fi(in, std::ios::binary | std::ios::ate);
  if (!fi) { std::perror(in); std::exit(2); }
  const size_t size = (size_t)fi.tellg();
  fi.seekg(0);
  std::ofstream fo(out, std::ios::binary);
  zra::Compressor comp(size, level, frameSize);
  const size_t chunk = bufferSize - (bufferSize % frameSize) + frameSize;      // zratool.cpp:131
  zra::Buffer ibuf(chunk), obuf;
  fo.seekp((std::streamoff)comp.GetHeaderSize());
  size_t done = 0, body = 0;
  while (done < size) {
    const size_t n = std::min(chunk, size - done);
    fi.read(reinterpret_cast<char*>(ibuf.data()), (std::streamsize)n);
    comp.Compress(zra::BufferView(ibuf.data(), n), obuf);
    fo.write(reinterpret_cast<const char*>(obuf.data()), (std::streamsize)obuf.size());
    body += obuf.size();
    done += n;
  }
  if (size == 0) comp.Compress(zra::BufferView(ibuf.data(), 0), obuf);
  const zra::Buffer& h = comp.GetHeader();
  fo.seekp(0);
  fo.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)h.size());
  return body + h.size();
}

size_t stream_decompress(const char* in, const char* out, size_t bufferSize) {
  std::ifstream fi(in, std::ios::binary);
  if (!fi) { std::perror(in); std::exit(2); }
  std::ofstream fo(out, std::ios::binary);
  zra::FullDecompressor dec([&fi](size_t off, size_t n, void* buf) {
    fi.seekg((std::streamoff)off);
    fi.read(static_cast<char*>(buf), (std::streamsize)n);
  });
  zra::Buffer obuf(bufferSize);                                                // zratool.cpp:195
  size_t total = 0;
  for (;;) {
    const size_t n = dec.Decompress(obuf);
    if (!n) break;
    fo.write(reinterpret_cast<const char*>(obuf.data()), (std::streamsize)n);
    total += n;
  }
  return total;
}

// output name of the decompress modes: the ".zra" suffix removed (zratool.cpp:90-95; a name without it is used as it is)
std::string remove_extension(std::string name) {
  const auto pos = name.find_last_of('.');
  if (pos != std::string::npos && name.substr(pos) == ".zra") return name.substr(0, pos);
  return name;
}

// mode t: the file goes to device memory as it is, the verification runs there
int test_archive(const char* path) {
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!arc.empty() && (hipMalloc(&dArc, arc.size()) != hipSuccess || hipMemcpy(dArc, arc.data(), arc.size(), hipMemcpyHostToDevice) != hipSuccess)) {
    std::fprintf(stderr, "%s: no device memory for %zu bytes\n", path, arc.size());
    if (dArc) (void)hipFree(dArc);
    ZraHipDestroyEngine(eng);
    return 2;
  }
  std::vector<ZraHipFrameFault> faults(1u << 16);
  size_t n = 0;
  st = ZraHipVerifyArchive(eng, dArc, arc.size(), ZRA_HIP_VERIFY_CONTENT, 0, UINT64_MAX, 0, faults.data(), faults.size(), &n);
  uint64_t s8[8] = {0};
  ZraHipGetVerifyStats(eng, s8);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot verify: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min(n, faults.size()); i++)
    std::printf("frame %llu: zstd error %u (%s)\n", (unsigned long long)faults[i].frame, faults[i].code,
                faults[i].stage == ZRA_HIP_VERIFY_STRUCTURE ? "structure" : "content");
  if (n > faults.size()) std::printf("... and %zu more\n", n - faults.size());
  std::printf("%s: %llu frames, %llu decoded, %zu faulty: %s\n", path, (unsigned long long)s8[1], (unsigned long long)s8[4], n, n ? "DAMAGED" : "ok");
  return n ? 1 : 0;
}

// mode g's archive: file -> device memory. false: message printed, nothing held
bool to_device(const char* path, const zra::Buffer& arc, void** dArc) {
  *dArc = nullptr;
  if (arc.empty()) return true;
  if (hipMalloc(dArc, arc.size()) == hipSuccess && hipMemcpy(*dArc, arc.data(), arc.size(), hipMemcpyHostToDevice) == hipSuccess) return true;
  std::fprintf(stderr, "%s: no device memory for %zu bytes\n", path, arc.size());
  if (*dArc) (void)hipFree(*dArc);
  *dArc = nullptr;
  return false;
}

// A pattern of modes g and gm is taken literally; behind a leading "hex:" it is pairs of hex digits. false: message printed
bool parse_pattern(const char* text, std::string* out) {
  std::string pat = text;
  if (pat.rfind("hex:", 0) == 0) {
    const std::string digits = pat.substr(4);
    pat.clear();
    if (digits.size() % 2 || digits.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) {
      std::fprintf(stderr, "%s: not pairs of hex digits\n", text);
      return false;
    }
    for (size_t i = 0; i < digits.size(); i += 2) pat.push_back((char)std::stoul(digits.substr(i, 2), nullptr, 16));
  }
  if (pat.empty() || pat.size() > ZRA_HIP_SEARCH_MAX_PATTERN) {
    std::fprintf(stderr, "a pattern has 1 to %u bytes\n", ZRA_HIP_SEARCH_MAX_PATTERN);
    return false;
  }
  *out = pat;
  return true;
}

// The modes with pattern expressions (gme, gle, gxe): -i and -F. Null for gm, gl and gx.
struct ExprOpt { bool fold, fixed; };
struct RegexOpt { bool fold; };                                                // gxr: the patterns are regular expressions

// The patterns texts[0 .. n) of a multi-pattern mode laid end to end, their sizes and the calls' syntax word. delimiter: gl's and gx's,
// -1 for gm. Without ex the patterns are literal (syntax 0). With ex a pattern is an expression unless -F was given; a "hex:" pattern
// becomes \xHH escapes, so that it stays literal bytes. false: message printed, for an expression with the pattern's index.
bool gather_patterns(char** texts, int n, int delimiter, const ExprOpt* ex, std::string* all, std::vector<uint32_t>* sizes, uint32_t* syntax) {
  *syntax = !ex ? 0u : (ex->fold ? ZRA_HIP_PATTERN_FOLD_CASE : 0u) | (ex->fixed ? 0u : ZRA_HIP_PATTERN_CLASSES);
  const bool expr = (*syntax & ZRA_HIP_PATTERN_CLASSES) != 0;
  for (int i = 0; i < n; i++) {
    std::string pat;
    if (!expr || std::string(texts[i]).rfind("hex:", 0) == 0) {
      if (!parse_pattern(texts[i], &pat)) return false;
      if (expr) {
        std::string esc;
        char b[8];
        for (unsigned char c : pat) { std::snprintf(b, sizeof b, "\\x%02x", c); esc += b; }
        pat = esc;
      }
    } else pat = texts[i];
    if (ex) {
      const uint32_t size = (uint32_t)pat.size();
      if (ZraHipCheckPatternExpr(pat.data(), &size, 1, *syntax, delimiter, nullptr, nullptr).zra != Success) {
        std::fprintf(stderr, "pattern %d: not a pattern expression of 1 to %u elements%s\n", i, ZRA_HIP_SEARCH_MAX_PATTERN, delimiter >= 0 ? ", or it matches the delimiter" : "");
        return false;
      }
    }
    *all += pat;
    sizes->push_back((uint32_t)pat.size());
  }
  if (ex) {
    if (n >= 1 && ZraHipCheckPatternExpr(all->data(), sizes->data(), sizes->size(), *syntax, delimiter, nullptr, nullptr).zra == Success) return true;
    std::fprintf(stderr, "1 to %u patterns of %u elements, %u expression bytes and %u byte sets in all\n", ZRA_HIP_SEARCH_MAX_PATTERNS, ZRA_HIP_SEARCH_MAX_PATTERN_BYTES,
                 ZRA_HIP_PATTERN_MAX_EXPR_BYTES, ZRA_HIP_PATTERN_MAX_SETS);
    return false;
  }
  if (n < 1 || n > (int)ZRA_HIP_SEARCH_MAX_PATTERNS || all->size() > ZRA_HIP_SEARCH_MAX_PATTERN_BYTES) {
    std::fprintf(stderr, "1 to %u patterns of %u bytes in all\n", ZRA_HIP_SEARCH_MAX_PATTERNS, ZRA_HIP_SEARCH_MAX_PATTERN_BYTES);
    return false;
  }
  if (delimiter >= 0 && all->find((char)delimiter) != std::string::npos) { std::fprintf(stderr, "a pattern holds the delimiter %02x\n", delimiter); return false; }
  return true;
}

// mode g
int search_archive(const char* path, const char* text) {
  std::string pat;
  if (!parse_pattern(text, &pat)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<uint64_t> at(1u << 20);
  uint64_t n = 0;
  st = ZraHipSearchArchive(eng, dArc, arc.size(), pat.data(), pat.size(), 0, UINT64_MAX, 0, at.data(), at.size(), &n);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot search: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(n, at.size()); i++) std::printf("%llu\n", (unsigned long long)at[i]);
  if (n > at.size()) std::printf("... and %llu more\n", (unsigned long long)(n - at.size()));
  std::printf("%llu matches\n", (unsigned long long)n);
  return n ? 0 : 1;
}

// modes gm and (ex) gme: the patterns texts[0 .. n), their indices in that order
int search_archive_multi(const char* path, char** texts, int n, const ExprOpt* ex) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (!gather_patterns(texts, n, -1, ex, &all, &sizes, &syntax)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipPatternMatch> at(1u << 20);
  uint64_t total = 0;
  st = ex ? ZraHipSearchArchiveMultiExpr(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, 0, UINT64_MAX, 0, at.data(), at.size(), &total, nullptr)
          : ZraHipSearchArchiveMulti(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), 0, UINT64_MAX, 0, at.data(), at.size(), &total, nullptr);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot search: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(total, at.size()); i++) std::printf("%llu\t%u\n", (unsigned long long)at[i].offset, at[i].pattern);
  if (total > at.size()) std::printf("... and %llu more\n", (unsigned long long)(total - at.size()));
  std::printf("%llu matches\n", (unsigned long long)total);
  return total ? 0 : 1;
}

// mode glw: "+0,-1,?2,?3" -> {all, any, none}
bool parse_clause(const char* text, ZraHipRecordClause* c) {
  *c = ZraHipRecordClause{0, 0, 0};
  for (const char* p = text; *p;) {
    const char kind = *p++;
    char* end = nullptr;
    const unsigned long i = (*p >= '0' && *p <= '9') ? std::strtoul(p, &end, 10) : ZRA_HIP_SEARCH_MAX_PATTERNS;
    if ((kind != '+' && kind != '?' && kind != '-') || i >= ZRA_HIP_SEARCH_MAX_PATTERNS || (*end && *end != ',') || (*end == ',' && !end[1])) {
      std::fprintf(stderr, "a clause is +i, ?i or -i items with commas between them, i below %u: %s\n", ZRA_HIP_SEARCH_MAX_PATTERNS, text);
      return false;
    }
    (kind == '+' ? c->all : kind == '?' ? c->any : c->none) |= 1ull << i;
    p = *end ? end + 1 : end;
  }
  return true;
}

// modes gl, (ex) gle and (where) glw: the patterns texts[0 .. n)
int grep_archive(const char* path, bool invert, uint8_t delimiter, char** texts, int n, const ExprOpt* ex, const std::vector<ZraHipRecordClause>* where = nullptr) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (!gather_patterns(texts, n, delimiter, ex, &all, &sizes, &syntax)) return 2;
  if (where && ZraHipCheckRecordClauses(where->data(), where->size(), sizes.size()).zra != Success) {
    std::fprintf(stderr, "1 to %u clauses over the patterns 0 .. %d, none with a pattern both wanted and unwanted\n", ZRA_HIP_WHERE_MAX_CLAUSES, n - 1);
    return 2;
  }
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipContentRange> at(1u << 20);
  uint64_t total = 0;
  const uint32_t mode = invert ? ZRA_HIP_GREP_INVERT : 0u;
  st = where ? ZraHipGrepArchiveWhere(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, where->data(), where->size(), 0, UINT64_MAX,
                                      0, at.data(), at.size(), &total)
     : ex ? ZraHipGrepArchiveExpr(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, 0, UINT64_MAX, 0, at.data(), at.size(), &total)
          : ZraHipGrepArchive(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), delimiter, mode, 0, UINT64_MAX, 0, at.data(), at.size(), &total);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot grep: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(total, at.size()); i++) std::printf("%llu\t%llu\n", (unsigned long long)at[i].offset, (unsigned long long)at[i].size);
  if (total > at.size()) std::printf("... and %llu more\n", (unsigned long long)(total - at.size()));
  std::printf("%llu records\n", (unsigned long long)total);
  return total ? 0 : 1;
}

// mode glc: gle's patterns with `before` records in front of and `after` records behind every selected one; a selected record's line
// ends in a tab and `*`, and `--` stands between two groups, as grep prints it
int grep_archive_context(const char* path, bool invert, uint8_t delimiter, uint32_t before, uint32_t after, char** texts, int n, const ExprOpt* ex) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (!gather_patterns(texts, n, delimiter, ex, &all, &sizes, &syntax)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipContentRange> at(1u << 20);
  uint64_t total = 0, selected = 0, groups = 0;
  st = ZraHipGrepArchiveContext(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, invert ? ZRA_HIP_GREP_INVERT : 0u, before, after, 0,
                                UINT64_MAX, 0, at.data(), at.size(), &total, &selected, &groups);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot grep: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(total, at.size()); i++) {
    const uint64_t size = at[i].size & ~ZRA_HIP_CONTEXT_SELECTED;
    // neighbours in the range lie one delimiter apart: a record that does not begin there opens a group
    if (i && at[i].offset != at[i - 1].offset + (at[i - 1].size & ~ZRA_HIP_CONTEXT_SELECTED) + 1) std::printf("--\n");
    std::printf("%llu\t%llu%s\n", (unsigned long long)at[i].offset, (unsigned long long)size, (at[i].size & ZRA_HIP_CONTEXT_SELECTED) ? "\t*" : "");
  }
  if (total > at.size()) std::printf("... and %llu more\n", (unsigned long long)(total - at.size()));
  std::printf("%llu records, %llu selected, %llu groups\n", (unsigned long long)total, (unsigned long long)selected, (unsigned long long)groups);
  return total ? 0 : 1;
}

// glr's and gxr's expressions texts[0 .. n), alternatives: laid end to end and checked on the host
bool gather_regex(char** texts, int n, bool fold, uint8_t delimiter, std::string* all, std::vector<uint32_t>* sizes, uint32_t* syntax) {
  for (int i = 0; i < n; i++) { *all += texts[i]; sizes->push_back((uint32_t)std::strlen(texts[i])); }
  *syntax = fold ? ZRA_HIP_PATTERN_FOLD_CASE : 0u;
  ZraHipRegexInfo info;
  if (ZraHipCheckRegex(all->data(), sizes->data(), sizes->size(), *syntax, delimiter, &info).zra == Success) return true;
  static const char* const why[] = {"", "1 to 64 expressions of 1 byte or more, 16384 bytes and 4096 positions in all", "not a regular expression",
                                    "an atom matches only the delimiter", "more than 64 states"};
  if (info.why == 2 || info.why == 3) std::fprintf(stderr, "expression %u: %s\n", info.pattern, why[info.why]);
  else std::fprintf(stderr, "%s\n", why[info.why <= 4 ? info.why : 1]);
  return false;
}

// mode glrc: glr's expressions, glc's context, output and exit status
int grep_archive_regex_context(const char* path, bool invert, bool fold, uint8_t delimiter, uint32_t before, uint32_t after, char** texts, int n) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (!gather_regex(texts, n, fold, delimiter, &all, &sizes, &syntax)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipContentRange> at(1u << 20);
  uint64_t total = 0, selected = 0, groups = 0;
  st = ZraHipGrepArchiveRegexContext(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, invert ? ZRA_HIP_GREP_INVERT : 0u, before, after, 0,
                                     UINT64_MAX, 0, at.data(), at.size(), &total, &selected, &groups);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot grep: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(total, at.size()); i++) {
    const uint64_t size = at[i].size & ~ZRA_HIP_CONTEXT_SELECTED;
    if (i && at[i].offset != at[i - 1].offset + (at[i - 1].size & ~ZRA_HIP_CONTEXT_SELECTED) + 1) std::printf("--\n");   // (as glc: a group opens)
    std::printf("%llu\t%llu%s\n", (unsigned long long)at[i].offset, (unsigned long long)size, (at[i].size & ZRA_HIP_CONTEXT_SELECTED) ? "\t*" : "");
  }
  if (total > at.size()) std::printf("... and %llu more\n", (unsigned long long)(total - at.size()));
  std::printf("%llu records, %llu selected, %llu groups\n", (unsigned long long)total, (unsigned long long)selected, (unsigned long long)groups);
  return total ? 0 : 1;
}

// mode glr
int grep_archive_regex(const char* path, bool invert, bool fold, bool countOnly, uint8_t delimiter, char** texts, int n) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (!gather_regex(texts, n, fold, delimiter, &all, &sizes, &syntax)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipContentRange> at(countOnly ? 0 : 1u << 20);
  uint64_t total = 0;
  st = ZraHipGrepArchiveRegex(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, invert ? ZRA_HIP_GREP_INVERT : 0u, 0, UINT64_MAX, 0,
                              countOnly ? nullptr : at.data(), at.size(), &total);
  if (dArc) (void)hipFree(dArc);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot grep: %s\n", path, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(total, at.size()); i++) std::printf("%llu\t%llu\n", (unsigned long long)at[i].offset, (unsigned long long)at[i].size);
  if (!countOnly && total > at.size()) std::printf("... and %llu more\n", (unsigned long long)(total - at.size()));
  std::printf("%llu records\n", (unsigned long long)total);
  return total ? 0 : 1;
}

struct CutOpt { uint8_t separator; uint64_t mask; };

// modes gx, (ex) gxe, (where) gxw, (rx) gxr and (cut) cut: a sizing call, then the call with a buffer of exactly that size; the packed bytes go to
// outPath, or to stdout when it is null. Nothing is written when a call fails or when nothing is selected.
int extract_records(const char* path, bool invert, uint8_t delimiter, const char* outPath, char** texts, int n, const ExprOpt* ex, const RegexOpt* rx = nullptr,
                    const std::vector<ZraHipRecordClause>* where = nullptr, const CutOpt* cut = nullptr) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (cut && n == 0) {}                                                       // (every record)
  else if (rx ? !gather_regex(texts, n, rx->fold, delimiter, &all, &sizes, &syntax) : !gather_patterns(texts, n, delimiter, ex, &all, &sizes, &syntax)) return 2;
  if (where && ZraHipCheckRecordClauses(where->data(), where->size(), sizes.size()).zra != Success) {
    std::fprintf(stderr, "1 to %u clauses over the patterns 0 .. %d, none with a pattern both wanted and unwanted\n", ZRA_HIP_WHERE_MAX_CLAUSES, n - 1);
    return 2;
  }
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr; void* dData = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  const uint32_t mode = invert ? ZRA_HIP_GREP_INVERT : 0u;
  uint64_t total = 0, bytes = 0;
  std::string text;
  auto extract = [&](void* dOut, size_t cap) {
    if (cut)
      return ZraHipCutRecords(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, cut->separator, cut->mask, 0, UINT64_MAX, 0, nullptr,
                              0, &total, dOut, cap, &bytes);
    if (where)
      return ZraHipExtractRecordsWhere(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, where->data(), where->size(), 0, UINT64_MAX,
                                       0, nullptr, 0, &total, dOut, cap, &bytes);
    if (rx)
      return ZraHipExtractRecordsRegex(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, 0, UINT64_MAX, 0, nullptr, 0, &total, dOut,
                                       cap, &bytes);
    return ex ? ZraHipExtractRecordsExpr(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, 0, UINT64_MAX, 0, nullptr, 0, &total, dOut,
                                         cap, &bytes)
              : ZraHipExtractRecords(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), delimiter, mode, 0, UINT64_MAX, 0, nullptr, 0, &total, dOut, cap, &bytes);
  };
  st = extract(nullptr, 0);
  if (st.zra == OutputBufferTooSmall) {
    text.resize(bytes);
    if (hipMalloc(&dData, bytes) != hipSuccess) { dData = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else {
      st = extract(dData, bytes);
      if (st.zra == Success && hipMemcpy(&text[0], dData, bytes, hipMemcpyDeviceToHost) != hipSuccess) { st.zra = ZStdError; st.zstd = 1; }
    }
  }
  if (dArc) (void)hipFree(dArc);
  if (dData) (void)hipFree(dData);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot extract: %s\n", path, ZraGetErrorString(st)); return 2; }
  if (!total) return 1;
  if (outPath) {
    std::ofstream out(outPath, std::ios::binary);
    out.write(text.data(), (std::streamsize)text.size());
    out.close();
    if (!out) { std::fprintf(stderr, "%s: cannot write\n", outPath); return 2; }
  } else if (std::fwrite(text.data(), 1, text.size(), stdout) != text.size() || std::fflush(stdout) != 0) {
    std::fprintf(stderr, "cannot write to stdout\n");
    return 2;
  }
  return 0;
}

// mode tally: the cut's selection into a workspace of exactly the size a first call names (ZraHipTallyFields), then the sizes of the tally
// and the tally itself on that workspace (ZraHipTallyRecords); one line per distinct key in order of first appearance: the count, a
// space, the key, the delimiter. Nothing goes to stdout when a call fails.
int tally_fields(const char* path, bool invert, uint8_t delimiter, const CutOpt& cut, char** texts, int n) {
  std::string all;
  std::vector<uint32_t> sizes;
  uint32_t syntax = 0;
  if (n && !gather_patterns(texts, n, delimiter, nullptr, &all, &sizes, &syntax)) return 2;
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr; void* dWork = nullptr; void* dKeys = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  const uint32_t mode = invert ? ZRA_HIP_GREP_INVERT : 0u;
  uint64_t work = 0, records = 0, distinct = 0, skipped = 0, keyBytes = 0;
  std::vector<ZraHipTallyEntry> entries;
  std::string keys;
  auto fields = [&](void* w, size_t cap) {
    return ZraHipTallyFields(eng, dArc, arc.size(), all.data(), sizes.data(), sizes.size(), syntax, delimiter, mode, cut.separator, cut.mask, 0, UINT64_MAX, 0, w, cap, &work,
                             0, nullptr, 0, nullptr, 0, &records, &distinct, &skipped, &keyBytes);
  };
  st = fields(nullptr, 0);
  if (st.zra == OutputBufferTooSmall && work) {
    const uint64_t need = work;
    if (hipMalloc(&dWork, need) != hipSuccess) { dWork = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else st = fields(dWork, need);                                            // (both capacities 0: the tally's sizes)
    if (st.zra == Success && distinct) {
      entries.resize(distinct); keys.resize(keyBytes);
      if (hipMalloc(&dKeys, keyBytes) != hipSuccess) { dKeys = nullptr; st.zra = ZStdError; st.zstd = 64; }
      else {
        st = ZraHipTallyRecords(eng, dWork, work, delimiter, 0, entries.data(), entries.size(), dKeys, keyBytes, &records, &distinct, &skipped, &keyBytes);
        if (st.zra == Success && hipMemcpy(&keys[0], dKeys, keyBytes, hipMemcpyDeviceToHost) != hipSuccess) { st.zra = ZStdError; st.zstd = 1; }
      }
    }
  }
  if (dArc) (void)hipFree(dArc);
  if (dWork) (void)hipFree(dWork);
  if (dKeys) (void)hipFree(dKeys);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot tally: %s\n", path, ZraGetErrorString(st)); return 2; }
  if (skipped) std::fprintf(stderr, "%s: %llu records longer than %u bytes are not counted\n", path, (unsigned long long)skipped, ZRA_HIP_TALLY_MAX_KEY);
  if (!distinct) return 1;
  std::string out;
  size_t at = 0;
  for (const ZraHipTallyEntry& e : entries) {                                 // (the keys lie in entry order, each with its delimiter)
    out += std::to_string(e.count); out += ' ';
    out.append(keys, at, (size_t)e.size + 1);
    at += (size_t)e.size + 1;
  }
  if (std::fwrite(out.data(), 1, out.size(), stdout) != out.size() || std::fflush(stdout) != 0) { std::fprintf(stderr, "cannot write to stdout\n"); return 2; }
  return 0;
}

// mode cmp. Nothing goes to stdout when the call fails.
int compare_archives(const char* pathA, const char* pathB) {
  zra::Buffer a = read_file(pathA), b = read_file(pathB);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", pathA, ZraGetErrorString(st)); return 2; }
  void* dA = nullptr; void* dB = nullptr;
  if (!to_device(pathA, a, &dA)) { ZraHipDestroyEngine(eng); return 2; }
  if (!to_device(pathB, b, &dB)) { if (dA) (void)hipFree(dA); ZraHipDestroyEngine(eng); return 2; }
  std::vector<ZraHipContentRange> at(1u << 20);
  uint64_t n = 0, bytes = 0, u2[2] = {0, 0};
  st = ZraHipCompareArchives(eng, dA, a.size(), dB, b.size(), 0, 0, UINT64_MAX, 0, at.data(), at.size(), &n, &bytes);
  ZraHipGetCompareSizes(eng, u2);
  if (dA) (void)hipFree(dA);
  if (dB) (void)hipFree(dB);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s %s: cannot compare: %s\n", pathA, pathB, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < std::min<uint64_t>(n, at.size()); i++) std::printf("%llu %llu\n", (unsigned long long)at[i].offset, (unsigned long long)at[i].size);
  std::printf("%llu ranges, %llu bytes differ\n", (unsigned long long)n, (unsigned long long)bytes);
  if (u2[0] != u2[1]) std::printf("sizes differ: %llu %llu\n", (unsigned long long)u2[0], (unsigned long long)u2[1]);
  return n || u2[0] != u2[1] ? 1 : 0;
}

// mode diff: a sizing call, then the call with buffers of exactly that size. Nothing goes to stdout when a call fails.
int diff_archives(const char* pathA, const char* pathB, uint32_t grain) {
  zra::Buffer a = read_file(pathA), b = read_file(pathB);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", pathA, ZraGetErrorString(st)); return 2; }
  void* dA = nullptr; void* dB = nullptr; void* dData = nullptr;
  if (!to_device(pathA, a, &dA)) { ZraHipDestroyEngine(eng); return 2; }
  if (!to_device(pathB, b, &dB)) { if (dA) (void)hipFree(dA); ZraHipDestroyEngine(eng); return 2; }
  uint64_t n = 0, bytes = 0, at = 0, app = 0;
  std::vector<uint64_t> off, size, dataOff;
  st = ZraHipDiffArchives(eng, dA, a.size(), dB, b.size(), 0, grain, 0, nullptr, nullptr, nullptr, 0, &n, nullptr, 0, &bytes, &at, &app);
  if (st.zra == OutputBufferTooSmall) {
    off.resize(n); size.resize(n); dataOff.resize(n);
    if (bytes && hipMalloc(&dData, bytes) != hipSuccess) { dData = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else st = ZraHipDiffArchives(eng, dA, a.size(), dB, b.size(), 0, grain, 0, off.data(), size.data(), dataOff.data(), off.size(), &n, dData, bytes, &bytes, &at, &app);
  }
  if (dA) (void)hipFree(dA);
  if (dB) (void)hipFree(dB);
  if (dData) (void)hipFree(dData);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s %s: cannot diff: %s\n", pathA, pathB, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < n; i++) std::printf("%llu %llu\n", (unsigned long long)off[i], (unsigned long long)size[i]);
  std::printf("append %llu\n", (unsigned long long)app);
  std::printf("%llu writes, %llu bytes written, %llu bytes of patch data\n", (unsigned long long)n, (unsigned long long)at, (unsigned long long)bytes);
  return n || app ? 1 : 0;
}

// mode sign: the 40-byte little-endian ZraHipSignature, then the words. Nothing goes to stdout when a call fails.
int sign_archive(const char* path, const char* outPath, uint32_t grain, uint64_t seed) {
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr; void* dSig = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  ZraHipSignature info;
  std::vector<uint64_t> words;
  st = ZraHipSignArchive(eng, dArc, arc.size(), grain, seed, 0, UINT64_MAX, 0, nullptr, 0, &info);
  if (st.zra == OutputBufferTooSmall) {
    words.resize(info.words);
    if (hipMalloc(&dSig, info.words * 8) != hipSuccess) { dSig = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else {
      st = ZraHipSignArchive(eng, dArc, arc.size(), grain, seed, 0, UINT64_MAX, 0, (uint64_t*)dSig, info.words, &info);
      if (st.zra == Success && hipMemcpy(words.data(), dSig, info.words * 8, hipMemcpyDeviceToHost) != hipSuccess) { st.zra = ZStdError; st.zstd = 1; }
    }
  }
  if (dArc) (void)hipFree(dArc);
  if (dSig) (void)hipFree(dSig);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot sign: %s\n", path, ZraGetErrorString(st)); return 2; }
  std::vector<uint64_t> head = {info.contentSize, (uint64_t)info.frameSize | ((uint64_t)info.grain << 32), info.seed, info.frames, info.words};
  std::string bytes;
  for (const std::vector<uint64_t>* v : {&head, &words})
    for (uint64_t w : *v) for (int i = 0; i < 8; i++) bytes.push_back((char)(w >> (8 * i)));
  std::ofstream out(outPath, std::ios::binary);
  out.write(bytes.data(), (std::streamsize)bytes.size());
  out.close();
  if (!out) { std::fprintf(stderr, "%s: cannot write\n", outPath); return 2; }
  std::printf("%llu frames, %llu words, grain %u\n", (unsigned long long)info.frames, (unsigned long long)info.words, info.grain);
  return 0;
}

// mode sigdiff: the diff mode with A given by a signature file. Nothing goes to stdout when a call fails.
int diff_signature(const char* pathSig, const char* pathB) {
  std::ifstream in(pathSig, std::ios::binary);
  std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (!in.good() && !in.eof()) raw.clear();
  if (raw.size() < 40 || raw.size() % 8) { std::fprintf(stderr, "%s: not a signature file\n", pathSig); return 2; }
  std::vector<uint64_t> w(raw.size() / 8);
  for (size_t i = 0; i < w.size(); i++) { uint64_t x = 0; for (int k = 0; k < 8; k++) x |= (uint64_t)(uint8_t)raw[8 * i + k] << (8 * k); w[i] = x; }
  const ZraHipSignature sig = {w[0], (uint32_t)w[1], (uint32_t)(w[1] >> 32), w[2], w[3], w[4]};
  const size_t sigWords = w.size() - 5;
  zra::Buffer b = read_file(pathB);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", pathSig, ZraGetErrorString(st)); return 2; }
  void* dSig = nullptr; void* dB = nullptr; void* dData = nullptr;
  if (!to_device(pathB, b, &dB)) { ZraHipDestroyEngine(eng); return 2; }
  if (sigWords && (hipMalloc(&dSig, sigWords * 8) != hipSuccess || hipMemcpy(dSig, w.data() + 5, sigWords * 8, hipMemcpyHostToDevice) != hipSuccess)) {
    std::fprintf(stderr, "%s: no device memory\n", pathSig);
    if (dSig) (void)hipFree(dSig);
    if (dB) (void)hipFree(dB);
    ZraHipDestroyEngine(eng);
    return 2;
  }
  uint64_t n = 0, bytes = 0, at = 0, app = 0;
  std::vector<uint64_t> off, size, dataOff;
  st = ZraHipDiffSignature(eng, &sig, (const uint64_t*)dSig, sigWords, dB, b.size(), 0, 0, nullptr, nullptr, nullptr, 0, &n, nullptr, 0, &bytes, &at, &app);
  if (st.zra == OutputBufferTooSmall) {
    off.resize(n); size.resize(n); dataOff.resize(n);
    if (bytes && hipMalloc(&dData, bytes) != hipSuccess) { dData = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else st = ZraHipDiffSignature(eng, &sig, (const uint64_t*)dSig, sigWords, dB, b.size(), 0, 0, off.data(), size.data(), dataOff.data(), off.size(), &n, dData, bytes,
                                  &bytes, &at, &app);
  }
  if (dSig) (void)hipFree(dSig);
  if (dB) (void)hipFree(dB);
  if (dData) (void)hipFree(dData);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s %s: cannot diff: %s\n", pathSig, pathB, ZraGetErrorString(st)); return 2; }
  for (size_t i = 0; i < n; i++) std::printf("%llu %llu\n", (unsigned long long)off[i], (unsigned long long)size[i]);
  std::printf("append %llu\n", (unsigned long long)app);
  std::printf("%llu writes, %llu bytes written, %llu bytes of patch data\n", (unsigned long long)n, (unsigned long long)at, (unsigned long long)bytes);
  return n || app ? 1 : 0;
}

// modes ix and rr: index the whole archive on the device (a sizing call, then the call), then, for rr, read records
// [first, first + count) (clipped to the records there are) and write their text, each with its delimiter, to stdout. Nothing goes
// to stdout when a call fails.
int index_records(const char* path, uint8_t delimiter, bool read, uint64_t first, uint64_t count) {
  zra::Buffer arc = read_file(path);
  ZraHipEngine* eng = nullptr;
  ZraStatus st = ZraHipCreateEngine(&eng, 0);
  if (st.zra != Success) { std::fprintf(stderr, "%s: no engine: %s\n", path, ZraGetErrorString(st)); return 2; }
  void* dArc = nullptr; void* dIndex = nullptr; void* dData = nullptr;
  if (!to_device(path, arc, &dArc)) { ZraHipDestroyEngine(eng); return 2; }
  ZraHipRecordIndex info;
  st = ZraHipIndexRecords(eng, dArc, arc.size(), delimiter, 0, UINT64_MAX, 0, nullptr, 0, &info);
  if (st.zra == OutputBufferTooSmall) {
    if (hipMalloc(&dIndex, info.frames * 8) != hipSuccess) { dIndex = nullptr; st.zra = ZStdError; st.zstd = 64; }
    else st = ZraHipIndexRecords(eng, dArc, arc.size(), delimiter, 0, UINT64_MAX, 0, (uint64_t*)dIndex, info.frames, &info);
  }
  std::string text;
  uint64_t got = 0;
  if (st.zra == Success && read && first < info.records) {
    got = std::min<uint64_t>(count, info.records - first);
    std::vector<uint64_t> numbers(got);
    for (uint64_t i = 0; i < got; i++) numbers[i] = first + i;
    uint64_t bytes = 0;
    st = ZraHipReadRecords(eng, dArc, arc.size(), &info, (const uint64_t*)dIndex, info.frames, numbers.data(), numbers.size(), 0, nullptr, nullptr, 0, &bytes);
    if (st.zra == OutputBufferTooSmall) {
      text.resize(bytes);
      if (hipMalloc(&dData, bytes) != hipSuccess) { dData = nullptr; st.zra = ZStdError; st.zstd = 64; }
      else {
        st = ZraHipReadRecords(eng, dArc, arc.size(), &info, (const uint64_t*)dIndex, info.frames, numbers.data(), numbers.size(), 0, nullptr, dData, bytes, &bytes);
        if (st.zra == Success && hipMemcpy(&text[0], dData, bytes, hipMemcpyDeviceToHost) != hipSuccess) { st.zra = ZStdError; st.zstd = 1; }
      }
    }
  }
  if (dArc) (void)hipFree(dArc);
  if (dIndex) (void)hipFree(dIndex);
  if (dData) (void)hipFree(dData);
  ZraHipDestroyEngine(eng);
  if (st.zra != Success) { std::fprintf(stderr, "%s: cannot %s: %s\n", path, read ? "read records" : "index", ZraGetErrorString(st)); return 2; }
  if (!read) {
    std::printf("%llu frames, %llu delimiters, %llu records\n", (unsigned long long)info.frames, (unsigned long long)info.delimiters, (unsigned long long)info.records);
    return 0;
  }
  if (!got) return 1;
  if (std::fwrite(text.data(), 1, text.size(), stdout) != text.size() || std::fflush(stdout) != 0) { std::fprintf(stderr, "cannot write to stdout\n"); return 2; }
  return 0;
}
}  // namespace

// argv of the reference tool, position by position (zratool.cpp:98-125,213-221):
//   c   {file} {level = 0} {frameSize = 16384} {stream buffer MB = 10}      -> {file}.zra
//   imc {file} {level = 0} {frameSize = 16384}                               -> {file}.zra
//   d   {file} {stream buffer MB = 10}                                       -> {file} without ".zra"
//   imd {file}                                                               -> {file} without ".zra"
//   b   {file} {level} {frameSize} {stream buffer MB} {offset = 0x1000} {size = 0x10000}
// ours: t {file}
//       g {file} {pattern | hex:digits}
//       gm {file} {pattern | hex:digits}...
//       gl {file} {-v} {-d hex byte = 0a} {pattern | hex:digits}...
//       gx {file} {-v} {-d hex byte = 0a} {-o file} {pattern | hex:digits}...
//       gme {file} {-i} {-F} {expression | hex:digits}...
//       gle {file} {-v} {-d hex byte = 0a} {-i} {-F} {expression | hex:digits}...
//       gxe {file} {-v} {-d hex byte = 0a} {-i} {-F} {-o file} {expression | hex:digits}...
//       cut {file} {-v} {-d hex byte = 0a} {-o file} {separator: hex byte} {list} {pattern | hex:digits}...
//       tally {file} {-v} {-d hex byte = 0a} {separator: hex byte} {list} {pattern | hex:digits}...
//       gxw {file} {-v} {-d hex byte = 0a} {-i} {-F} {-o file} -w clause {-w clause}... {expression | hex:digits}...
//       glc {file} {-v} {-d hex byte = 0a} {-i} {-F} {-A records} {-B records} {-C records} {expression | hex:digits}...
//       glr {file} {-i} {-v} {-c} {-d hex byte = 0a} {expression}...
//       gxr {file} {-i} {-v} {-d hex byte = 0a} {-o file} {expression}...
//       glrc {file} {-i} {-v} {-d hex byte = 0a} {-A records} {-B records} {-C records} {expression}...
//       cmp {file A} {file B}
//       diff {file A} {file B} {-g grain}
//       sign {file} {signature file} {-g grain} {-s seed}
//       sigdiff {signature file of A} {file B}
//       ix {file} {-d hex byte = 0a}
//       rr {file} {-d hex byte = 0a} {first record} {count}
int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("%s {mode} {file} ...\n"
                "c {file} {compression level = 3} {frame size = 16384} {stream buffer size = 10MB} - Streaming Compression\n"
                "imc  {file} {compression level = 3} {frame size = 16384} - In-memory Compression\n"
                "d {file} {stream buffer size = 10MB} - Streaming Decompression\n"
                "imd  {file} - In-memory Decompression\n"
                "b  {file} {compression level = 3} {frame size = 16384} {stream buffer size = 10MB} {offset = 0x1000} {size = 0x10000} - Benchmark (Memory Intensive)\n"
                "t  {file} - Test an archive on the device: every faulty frame (exit status 0 clean, 1 faults, 2 cannot verify)\n"
                "g  {file} {pattern | hex:digits} - Search an archive on the device: every offset of the pattern (exit status 0 matches, 1 none, 2 trouble)\n"
                "gm {file} {pattern | hex:digits}... - Search an archive on the device for 1 to 64 patterns in one pass: offset and pattern index of every match (exit status as g)\n"
                "gl {file} {-v} {-d hex byte = 0a} {pattern | hex:digits}... - Grep an archive on the device: offset and size of every record (line) that holds a match, -v: that holds none (exit status 0 some, 1 none, 2 trouble)\n"
                "gx {file} {-v} {-d hex byte = 0a} {-o file} {pattern | hex:digits}... - Extract from an archive on the device: the text of the records gl lists, each with its delimiter, to stdout or to a file (exit status as gl)\n"
                "gme | gle | gxe {file} {options of gm | gl | gx} {-i} {-F} {expression | hex:digits}... - gm, gl and gx with pattern expressions of fixed length: . [set] [^set] \\escape; -i: letters match either case, -F: literal patterns (a refused expression: exit status 2)\n"
                "cut {file} {options of gx} {separator: hex byte} {list} {pattern | hex:digits}... - gx with cut's field selection: of every selected record only the fields of the list (1,3,5-7,9-), cut at the separator; no pattern: every record; output and exit status as gx\n"
                "tally {file} {-v} {-d hex byte = 0a} {separator: hex byte} {list} {pattern | hex:digits}... - cut, counted: one line `count key` per distinct value of cut's output, in order of first appearance (exit status as gl)\n"
                "gxw {file} {options of gxe} {-w clause}... {expression | hex:digits}... - gxe with glw's record predicate: the selected records' bytes, the text grep A | grep B | grep -v C prints; output and exit status as gx\n"
                "glw {file} {options of gle} {-w clause}... {expression | hex:digits}... - gle with a record predicate: a clause is comma-separated +i (pattern i occurs), ?i (one of these occurs), -i (pattern i does not), i counted from 0; a record is selected when some clause holds (a refused clause: exit status 2)\n"
                "glc {file} {options of gle} {-A records} {-B records} {-C records} {expression | hex:digits}... - gle with context: up to 64 records behind (-A), in front of (-B) or around (-C) every selected record; a selected record is marked *, `--` separates groups (exit status as gl)\n"
                "glr {file} {-i} {-v} {-c} {-d hex byte = 0a} {expression}... - gl with regular expressions: POSIX extended expressions over bytes, * + ? {n,m} ( ) | ^ $ on gle's atoms, several expressions are alternatives; -c: only the count (a refused expression: exit status 2)\n"
                "gxr {file} {-i} {-v} {-d hex byte = 0a} {-o file} {expression}... - gx with glr's regular expressions: the text of the records glr lists, each with its delimiter, to stdout or to a file (exit status as glr)\n"
                "glrc {file} {-i} {-v} {-d hex byte = 0a} {-A records} {-B records} {-C records} {expression}... - glr with glc's context: up to 64 records behind (-A), in front of (-B) or around (-C) every record glr selects; output and exit status as glc (a refused expression: exit status 2)\n"
                "cmp {file A} {file B} - Compare the contents of two archives on the device: every differing range (exit status 0 equal, 1 different, 2 trouble)\n"
                "diff {file A} {file B} {-g grain = 1} - The patch that gives archive A the content of archive B, on the device: every write, the tail (exit status 0 empty, 1 not empty, 2 trouble)\n"
                "sign {file} {signature file} {-g grain = 4096} {-s seed = 0} - The content signature of an archive, on the device: per frame one hash of its compressed bytes and one per grain\n"
                "sigdiff {signature file of A} {file B} - diff with archive A given by its signature (output and exit status as diff)\n"
                "ix {file} {-d hex byte = 0a} - Index the records (lines) of an archive on the device: frames, delimiters and records\n"
                "rr {file} {-d hex byte = 0a} {first record} {count} - Read records by their number through the record index: their text, each with its delimiter, to stdout (exit status 0 some, 1 none, 2 trouble)\n",
                argv[0]);
    return 0;
  }
  const std::string mode = argv[1];
  if (mode == "t") return test_archive(argv[2]);
  if (mode == "g") {
    if (argc < 4) { std::fprintf(stderr, "g {file} {pattern | hex:digits}\n"); return 2; }
    return search_archive(argv[2], argv[3]);
  }
  if (mode == "gm") {
    if (argc < 4) { std::fprintf(stderr, "gm {file} {pattern | hex:digits}...\n"); return 2; }
    return search_archive_multi(argv[2], argv + 3, argc - 3, nullptr);
  }
  if (mode == "gme") {
    ExprOpt ex = {false, false};
    int i = 3;
    for (; i < argc; i++) {
      const std::string opt = argv[i];
      if (opt == "-i") ex.fold = true; else if (opt == "-F") ex.fixed = true; else break;
    }
    if (i >= argc) { std::fprintf(stderr, "gme {file} {-i} {-F} {expression | hex:digits}...\n"); return 2; }
    return search_archive_multi(argv[2], argv + i, argc - i, &ex);
  }
  if (mode == "gl" || mode == "gx" || mode == "gle" || mode == "gxe" || mode == "glw" || mode == "gxw" || mode == "cut" || mode == "tally") {
    const bool counted = mode == "tally", fields = mode == "cut" || counted, text = mode[1] == 'x' || fields, expr = mode.size() == 3 && !fields, pred = mode == "glw" || mode == "gxw";
    std::vector<ZraHipRecordClause> where;
    ExprOpt ex = {false, false};
    bool invert = false;
    unsigned long delimiter = 0x0A;
    const char* outPath = nullptr;
    int i = 3;
    for (; i < argc; i++) {
      const std::string opt = argv[i];
      if (opt == "-v") invert = true;
      else if (expr && opt == "-i") ex.fold = true;
      else if (expr && opt == "-F") ex.fixed = true;
      else if (pred && opt == "-w") {
        ZraHipRecordClause c;
        if (++i >= argc || !*argv[i]) { std::fprintf(stderr, "-w takes a clause\n"); return 2; }
        if (!parse_clause(argv[i], &c)) return 2;
        where.push_back(c);
      } else if (text && opt == "-o") {
        if (++i >= argc || !*argv[i]) { std::fprintf(stderr, "-o takes a file name\n"); return 2; }
        outPath = argv[i];
      } else if (opt == "-d") {
        char* end = nullptr;
        if (++i < argc) delimiter = std::strtoul(argv[i], &end, 16);
        if (i >= argc || !*argv[i] || *end || delimiter > 0xFF) { std::fprintf(stderr, "-d takes a byte as hex digits\n"); return 2; }
      } else break;
    }
    if (fields) {
      CutOpt cut = {0, 0};
      char* end = nullptr;
      const unsigned long sep = i < argc ? std::strtoul(argv[i], &end, 16) : 0;
      if (i + 1 >= argc || !*argv[i] || *end || sep > 0xFF || sep == delimiter || ZraHipFieldMask(argv[i + 1], &cut.mask).zra != Success) {
        std::fprintf(stderr, "%s {file} {-v} {-d hex byte = 0a} %s{separator: a byte as hex digits, not the delimiter} {list: 1,3,5-7,9-} {pattern | hex:digits}...\n",
                     mode.c_str(), counted ? "" : "{-o file} ");
        return 2;
      }
      cut.separator = (uint8_t)sep;
      if (counted) return tally_fields(argv[2], invert, (uint8_t)delimiter, cut, argv + i + 2, argc - i - 2);
      return extract_records(argv[2], invert, (uint8_t)delimiter, outPath, argv + i + 2, argc - i - 2, nullptr, nullptr, nullptr, &cut);
    }
    if (i >= argc || (pred && where.empty())) {
      std::fprintf(stderr, "%s {file} {-v} {-d hex byte = 0a} %s%s%s{%s | hex:digits}...\n", mode.c_str(), expr ? "{-i} {-F} " : "", text ? "{-o file} " : "",
                   pred ? "-w clause {-w clause}... " : "", expr ? "expression" : "pattern");
      return 2;
    }
    if (pred && text) return extract_records(argv[2], invert, (uint8_t)delimiter, outPath, argv + i, argc - i, &ex, nullptr, &where);
    if (pred) return grep_archive(argv[2], invert, (uint8_t)delimiter, argv + i, argc - i, &ex, &where);
    if (text) return extract_records(argv[2], invert, (uint8_t)delimiter, outPath, argv + i, argc - i, expr ? &ex : nullptr);
    return grep_archive(argv[2], invert, (uint8_t)delimiter, argv + i, argc - i, expr ? &ex : nullptr);
  }
  if (mode == "glc") {
    ExprOpt ex = {false, false};
    bool invert = false;
    unsigned long delimiter = 0x0A, before = 0, after = 0;
    int i = 3;
    for (; i < argc; i++) {
      const std::string opt = argv[i];
      char* end = nullptr;
      if (opt == "-v") invert = true;
      else if (opt == "-i") ex.fold = true;
      else if (opt == "-F") ex.fixed = true;
      else if (opt == "-A" || opt == "-B" || opt == "-C") {
        unsigned long v = 0;
        if (++i < argc) v = std::strtoul(argv[i], &end, 10);
        if (i >= argc || !*argv[i] || *end || v > ZRA_HIP_GREP_MAX_CONTEXT) { std::fprintf(stderr, "%s takes 0 to %u records\n", opt.c_str(), ZRA_HIP_GREP_MAX_CONTEXT); return 2; }
        if (opt != "-B") after = v;
        if (opt != "-A") before = v;
      } else if (opt == "-d") {
        if (++i < argc) delimiter = std::strtoul(argv[i], &end, 16);
        if (i >= argc || !*argv[i] || *end || delimiter > 0xFF) { std::fprintf(stderr, "-d takes a byte as hex digits\n"); return 2; }
      } else break;
    }
    if (i >= argc) { std::fprintf(stderr, "glc {file} {-v} {-d hex byte = 0a} {-i} {-F} {-A records} {-B records} {-C records} {expression | hex:digits}...\n"); return 2; }
    return grep_archive_context(argv[2], invert, (uint8_t)delimiter, (uint32_t)before, (uint32_t)after, argv + i, argc - i, &ex);
  }
  if (mode == "glrc") {
    bool invert = false, fold = false;
    unsigned long delimiter = 0x0A, before = 0, after = 0;
    int i = 3;
    for (; i < argc; i++) {
      const std::string opt = argv[i];
      char* end = nullptr;
      if (opt == "-v") invert = true;
      else if (opt == "-i") fold = true;
      else if (opt == "-A" || opt == "-B" || opt == "-C") {
        unsigned long v = 0;
        if (++i < argc) v = std::strtoul(argv[i], &end, 10);
        if (i >= argc || !*argv[i] || *end || v > ZRA_HIP_GREP_MAX_CONTEXT) { std::fprintf(stderr, "%s takes 0 to %u records\n", opt.c_str(), ZRA_HIP_GREP_MAX_CONTEXT); return 2; }
        if (opt != "-B") after = v;
        if (opt != "-A") before = v;
      } else if (opt == "-d") {
        if (++i < argc) delimiter = std::strtoul(argv[i], &end, 16);
        if (i >= argc || !*argv[i] || *end || delimiter > 0xFF) { std::fprintf(stderr, "-d takes a byte as hex digits\n"); return 2; }
      } else break;
    }
    if (i >= argc) { std::fprintf(stderr, "glrc {file} {-i} {-v} {-d hex byte = 0a} {-A records} {-B records} {-C records} {expression}...\n"); return 2; }
    return grep_archive_regex_context(argv[2], invert, fold, (uint8_t)delimiter, (uint32_t)before, (uint32_t)after, argv + i, argc - i);
  }
  if (mode == "glr" || mode == "gxr") {
    const bool text = mode == "gxr";
    bool invert = false, fold = false, countOnly = false;
    unsigned long delimiter = 0x0A;
    const char* outPath = nullptr;
    int i = 3;
    for (; i < argc; i++) {
      const std::string opt = argv[i];
      if (opt == "-v") invert = true;
      else if (opt == "-i") fold = true;
      else if (!text && opt == "-c") countOnly = true;
      else if (text && opt == "-o") {
        if (++i >= argc || !*argv[i]) { std::fprintf(stderr, "-o takes a file name\n"); return 2; }
        outPath = argv[i];
      } else if (opt == "-d") {
        char* end = nullptr;
        if (++i < argc) delimiter = std::strtoul(argv[i], &end, 16);
        if (i >= argc || !*argv[i] || *end || delimiter > 0xFF) { std::fprintf(stderr, "-d takes a byte as hex digits\n"); return 2; }
      } else break;
    }
    if (i >= argc) { std::fprintf(stderr, "%s {file} {-i} {-v} %s{-d hex byte = 0a} {expression}...\n", mode.c_str(), text ? "{-o file} " : "{-c} "); return 2; }
    const RegexOpt rx = {fold};
    if (text) return extract_records(argv[2], invert, (uint8_t)delimiter, outPath, argv + i, argc - i, nullptr, &rx);
    return grep_archive_regex(argv[2], invert, fold, countOnly, (uint8_t)delimiter, argv + i, argc - i);
  }
  if (mode == "cmp") {
    if (argc < 4) { std::fprintf(stderr, "cmp {file A} {file B}\n"); return 2; }
    return compare_archives(argv[2], argv[3]);
  }
  if (mode == "diff") {
    if (argc != 4 && !(argc == 6 && std::string(argv[4]) == "-g")) { std::fprintf(stderr, "diff {file A} {file B} {-g grain}\n"); return 2; }
    return diff_archives(argv[2], argv[3], argc == 6 ? (uint32_t)std::strtoul(argv[5], nullptr, 10) : 1u);
  }
  if (mode == "sign") {
    uint32_t grain = 4096; uint64_t seed = 0;
    bool good = argc >= 4 && (argc - 4) % 2 == 0;
    for (int i = 4; good && i + 1 < argc; i += 2) {
      const std::string opt = argv[i];
      char* end = nullptr;
      const unsigned long long v = std::strtoull(argv[i + 1], &end, 0);
      if (!*argv[i + 1] || *end) good = false;
      else if (opt == "-g") grain = v > 0xFFFFFFFFull ? 0u : (uint32_t)v;
      else if (opt == "-s") seed = v;
      else good = false;
    }
    if (!good) { std::fprintf(stderr, "sign {file} {signature file} {-g grain} {-s seed}\n"); return 2; }
    return sign_archive(argv[2], argv[3], grain, seed);
  }
  if (mode == "sigdiff") {
    if (argc != 4) { std::fprintf(stderr, "sigdiff {signature file of A} {file B}\n"); return 2; }
    return diff_signature(argv[2], argv[3]);
  }
  if (mode == "ix" || mode == "rr") {
    const bool read = mode == "rr";
    unsigned long delimiter = 0x0A;
    int i = 3;
    if (i < argc && std::string(argv[i]) == "-d") {
      char* end = nullptr;
      if (++i < argc) delimiter = std::strtoul(argv[i], &end, 16);
      if (i >= argc || !*argv[i] || *end || delimiter > 0xFF) { std::fprintf(stderr, "-d takes a byte as hex digits\n"); return 2; }
      i++;
    }
    unsigned long long first = 0, count = 0;
    bool good = argc - i == (read ? 2 : 0);
    if (good && read) {
      char* e1 = nullptr; char* e2 = nullptr;
      first = std::strtoull(argv[i], &e1, 0); count = std::strtoull(argv[i + 1], &e2, 0);
      good = *argv[i] && !*e1 && *argv[i + 1] && !*e2;
    }
    if (!good) { std::fprintf(stderr, read ? "rr {file} {-d hex byte = 0a} {first record} {count}\n" : "ix {file} {-d hex byte = 0a}\n"); return 2; }
    return index_records(argv[2], (uint8_t)delimiter, read, first, count);
  }
  const bool comp = mode == "c" || mode == "imc" || mode == "b";
  const zra::i8 level = comp && argc > 3 ? (zra::i8)std::atoi(argv[3]) : 0;
  const zra::u32 frameSize = comp && argc > 4 ? (zra::u32)std::strtoul(argv[4], nullptr, 10) : 16384;
  const int bufArg = mode == "d" ? 3 : 5;
  const size_t bufferSize = (mode == "c" || mode == "d" || mode == "b") && argc > bufArg ? (size_t)std::atoi(argv[bufArg]) * 1'000'000 : 10'000'000;
  std::string fileName; size_t fileSize = 0;
  try {
    if (mode == "c") {
      fileName = std::string(argv[2]) + ".zra";
      fileSize = stream_compress(argv[2], fileName.c_str(), level, frameSize, bufferSize);
    } else if (mode == "d") {
      fileName = remove_extension(argv[2]);
      fileSize = stream_decompress(argv[2], fileName.c_str(), bufferSize);
    } else if (mode == "imc") {
      zra::Buffer in = read_file(argv[2]);
      zra::Buffer out = zra::CompressBuffer(in, level, frameSize);
      fileName = std::string(argv[2]) + ".zra"; fileSize = out.size();
      write_file(fileName.c_str(), out.data(), out.size());
    } else if (mode == "imd") {
      zra::Buffer in = read_file(argv[2]);
      zra::Buffer out = zra::DecompressBuffer(in);
      fileName = remove_extension(argv[2]); fileSize = out.size();
      write_file(fileName.c_str(), out.data(), out.size());
    } else if (mode == "b") {
      zra::Buffer in = read_file(argv[2]);
      const std::string arcName = std::string(argv[2]) + ".bench.zra", backName = std::string(argv[2]) + ".bench.out";
      auto t = Clock::now();
      zra::Buffer arc = zra::CompressBuffer(in, level, frameSize);
      double m = ms_since(t);
      std::printf("in-memory compress   : %8.1f ms  %8.1f MB/s  (%zu -> %zu)\n", m, in.size() / 1e3 / m, in.size(), arc.size());
      t = Clock::now();
      zra::Buffer back = zra::DecompressBuffer(arc);
      m = ms_since(t);
      std::printf("in-memory decompress : %8.1f ms  %8.1f MB/s  %s\n", m, in.size() / 1e3 / m, back == in ? "ok" : "MISMATCH");
      t = Clock::now();
      size_t n = stream_compress(argv[2], arcName.c_str(), level, frameSize, bufferSize);
      m = ms_since(t);
      std::printf("streaming compress   : %8.1f ms  %8.1f MB/s  (%zu bytes)\n", m, in.size() / 1e3 / m, n);
      t = Clock::now();
      n = stream_decompress(arcName.c_str(), backName.c_str(), bufferSize);
      m = ms_since(t);
      std::printf("streaming decompress : %8.1f ms  %8.1f MB/s  (%zu bytes)\n", m, in.size() / 1e3 / m, n);
      {
        // steady state of the drop-in C ABI (caller-owned buffers, scratch already allocated): what a long-running host sees
        std::vector<zra::u8> obuf(ZraGetCompressedOutputBufferSize(in.size(), frameSize)), rbuf(in.size());
        for (int rep = 0; rep < 3; rep++) {
          size_t osz = 0;
          t = Clock::now();
          ZraStatus st = ZraCompressBuffer(in.data(), in.size(), obuf.data(), &osz, level, frameSize, true, nullptr, 0);
          const double mc = ms_since(t);
          t = Clock::now();
          ZraStatus sd = ZraDecompressBuffer(obuf.data(), osz, rbuf.data());
          const double md = ms_since(t);
          std::printf("C ABI rep %d: compress %8.1f ms %8.1f MB/s (status %d)   decompress %8.1f ms %8.1f MB/s (status %d, %s)\n", rep, mc,
                      in.size() / 1e3 / mc, (int)st.zra, md, in.size() / 1e3 / md, (int)sd.zra, std::memcmp(rbuf.data(), in.data(), in.size()) == 0 ? "ok" : "MISMATCH");
        }
      }
      {
        // the reference's random-access probe (zratool.cpp:264-279): offset / size from argv, an archive at the DEFAULT frame size
        const size_t off = argc > 6 ? (size_t)std::atoll(argv[6]) : 0x1000, want = argc > 7 ? (size_t)std::atoll(argv[7]) : 0x10000;
        if (in.size() > off + 1) {
          const size_t len = std::min<size_t>(in.size() - off - 1, want);
          zra::Buffer arcDefault = zra::CompressBuffer(in, level);
          t = Clock::now();
          zra::Buffer ra = zra::DecompressRA(arcDefault, off, len);
          m = ms_since(t);
          std::printf("random access %zu B @ %zu (in-memory) : %8.3f ms  %s\n", len, off, m, std::memcmp(ra.data(), in.data() + off, len) == 0 ? "ok" : "MISMATCH");
          zra::Decompressor dec([&arcDefault](size_t o, size_t sz, void* out) { std::memcpy(out, arcDefault.data() + o, sz); });
          t = Clock::now();
          zra::Buffer rs = dec.Decompress(off, len);
          m = ms_since(t);
          std::printf("random access %zu B @ %zu (streaming) : %8.3f ms  %s\n", len, off, m, std::memcmp(rs.data(), in.data() + off, len) == 0 ? "ok" : "MISMATCH");
        }
      }
      zra::Buffer streamed = read_file(arcName.c_str());
      std::printf("streaming archive %s in-memory archive\n", streamed == arc ? "==" : "!=");
      std::remove(arcName.c_str()); std::remove(backName.c_str());
    } else {
      char* again[1] = {argv[0]};
      return main(1, again);
    }
  } catch (const zra::Exception& e) {
    std::fprintf(stderr, "zra error: %s\n", e.what());
    return 3;
  }
  if (fileSize || !fileName.empty()) std::printf("Output Size (%s): %zu bytes\n", fileName.c_str(), fileSize);
  return 0;
}
