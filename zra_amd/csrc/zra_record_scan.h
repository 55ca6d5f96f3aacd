// zra_amd — the one call path of the record scans: ZraHipGrepArchive (zra_grep.hip), ZraHipGrepArchiveWhere (zra_grep_where.hip),
// ZraHipGrepArchiveRegex (zra_grep_regex.hip), ZraHipExtractRecords (zra_extract.hip), ZraHipExtractRecordsRegex
// (zra_extract_regex.hip), ZraHipExtractRecordsWhere (zra_extract_where.hip), ZraHipGrepArchiveContext (zra_grep_context.hip),
// ZraHipGrepArchiveRegexContext (zra_grep_regex_context.hip), ZraHipCutRecords (zra_cut.hip), their ...Expr forms and the same calls
// through an archive handle. They cut a content range into records at a delimiter, select records and return them as a list, the extracts with the
// records' bytes, the two greps with context with the records around the selected ones; they take the arguments of
// one RecordCall (zra_engine.h) and differ in two things only, which record_scan() takes as types:
//  a SELECTOR (three, below, and next to the cut's kernels LiteralSelect wrapped so that no pattern selects every record; host only): what the patterns of the call become. compile(): rule 1 beyond the nulls; M: the longest
//      pattern, which the driver's (carry) and (ownership) run on; nothing(len): a range of len bytes in which no record can be
//      selected; table_bytes() / build(): the table that heads the call's device tables; open(): the carried state of the record that
//      opens at lo, beyond its start.
//  a KERNEL SET (nine, each next to its kernels; ExtractWhereKernels is WhereSelect's second): Sum / Head, the two per-tile entries, kMapBytes more per tile behind them; Totals =
//      {State st[2] (the ping-pong pair of zra_scan.h's (c)), matches, delims}; kData: the call packs bytes; launch(): the three
//      launches of a pass, the third one only when a capacity asks for it.
// record_scan() wraps its steps in ScanImpl::call for the row kData names, so the kernel set alone decides whose counters a call writes.
// Device tables of a call: table | Totals | sums[tilesMax] | heads[tilesMax] | maps[tilesMax * kMapBytes]. The statuses and their
// order are zra_hip.h's; the passes, (contiguity), (carry), (ownership) with trim = 0, (c) and (d) are zra_scan.h's.
#pragma once
#include "zra_patterns.h"
#include "zra_regex.h"
#include "zra_where.h"

namespace {
using zra_eng::RecordCall;

// ---- the selectors
// literal patterns, or with a syntax word expressions of byte classes (zra_patterns.h); mode 1 inverts
struct LiteralSelect {
  PatternSet pset;
  uint32_t inv = 0, M = 0;
  bool compile(const RecordCall& c) {
    inv = c.mode & 1u;
    if (!patterns_ok(c.hPat, c.hSizes, c.nPat, c.syntax, c.delimiter, &pset)) return false;
    M = pset.M;
    return true;
  }
  bool nothing(uint64_t len) const { return !inv && len < pset.mMin; }        // no record could hold a match
  size_t table_bytes() const { return pset.table_bytes() + 64; }
  void build(uint8_t* dst, const RecordCall& c) const { build_pattern_table(dst, pset, c.hPat, c.hSizes, c.nPat); }
  template <class State> void open(State&) const {}
};
// the literal selector's patterns under a record predicate (zra_where.h): the block carries the mode. WhereKernels lists the selected
// records (zra_grep_where.hip), ExtractWhereKernels packs their bytes as well (zra_extract_where.hip)
struct WhereSelect : LiteralSelect {
  zra_where::Block w;
  bool compile(const RecordCall& c) {
    if (!LiteralSelect::compile(c) || !zra_where::clauses_ok((const zra_where::Clause*)c.hClauses, c.nClauses, c.nPat)) return false;
    w = zra_where::make_block((const zra_where::Clause*)c.hClauses, c.nClauses, inv != 0);
    return true;
  }
  bool nothing(uint64_t len) const { return len < pset.mMin && !zra_where::where_selected(w, 0); }   // every set is empty, and the empty set is not selected
};
// regular expressions (zra_regex.h): a position owns its own byte only, and every non-empty range is scanned
struct RegexSelect {
  zra_regex::Table table;
  uint32_t inv = 0, M = 1;
  bool compile(const RecordCall& c) {
    inv = c.mode & 1u;
    zra_regex::Compiled C;
    if (!zra_regex::compile(c.hPat, c.hSizes, c.nPat, c.syntax, c.delimiter, &C)) return false;
    table = C.table;
    return true;
  }
  bool nothing(uint64_t) const { return false; }
  size_t table_bytes() const { return sizeof(table); }
  void build(uint8_t* dst, const RecordCall&) const { std::memcpy(dst, &table, sizeof(table)); }
  template <class State> void open(State& s) const { s.state = table.start; }
};

// what a kernel set's launch() finds of the call's device memory, and the pass in tiles
template <class K>
struct RecordPass {
  const uint8_t* win, * table;
  typename K::Totals* tot;
  typename K::Sum* sums;
  typename K::Head* heads;
  uint8_t* maps;
  Range* list;
  uint64_t listCap, hi;
  uint32_t tiles, groups;
};

// the two extra outputs of a kernel set whose carried state holds a context summary `c` (zra_context.h); nothing for the others
template <class State> auto context_outputs(const State& fin, const RecordCall& c, int) -> decltype((void)fin.c) {
  if (c.nSelected) *c.nSelected = fin.c.sel;
  if (c.nGroups) *c.nGroups = fin.c.groups;
}
template <class State> void context_outputs(const State&, const RecordCall&, long) {}
}  // namespace

namespace zra_eng {

template <class Selector, class K>
Status ScanImpl::record_scan(Engine& E, const RecordCall& c, ScanCacheView* cv) {
  using Totals = typename K::Totals;
  static_assert(sizeof(Totals) % 16 == 0 && sizeof(typename K::Sum) % 16 == 0 && sizeof(typename K::Head) % 16 == 0 && K::kMapBytes % 16 == 0 && sizeof(Range) == 16 &&
                (sizeof(Table) + 64) % 16 == 0 && (sizeof(ClassTable) + 64) % 16 == 0 && sizeof(zra_regex::Table) % 16 == 0, "16-byte entries behind a 16-byte head");
  // the row of counters and milliseconds the call writes, and what it leaves behind on any status (ScanImpl::call): kData decides both
  constexpr int which = K::kData ? kScanExtract : kScanGrep;
  return call(E, which, c.nRecords, K::kData ? c.dataSize : nullptr, [&]() -> Status {
  // ---- 1. arguments, the patterns, and (the calls with data) overlap with the archive and with the arena of the handle the call goes through
  if (!c.nRecords || !c.hPat || !c.hSizes || (!c.dArc && c.arcSize) || (!c.hRecords && c.recordCap) || (c.mode & ~1u)) return zerr(42);
  if (c.before > 64 || c.after > 64) return zerr(42);                        // (ZRA_HIP_GREP_MAX_CONTEXT; 0 for every call but the one with context)
  if (K::kData && (!c.dataSize || (!c.dData && c.dataCap))) return zerr(42);
  Selector sel;
  if (!sel.compile(c)) return zerr(42);
  if (K::kData && c.dataCap) {
    const uintptr_t d = (uintptr_t)c.dData, a = (uintptr_t)c.dArc;
    if (c.arcSize && d < a + c.arcSize && a < d + c.dataCap) return zerr(42);
    if (cv && cv->slots && d < (uintptr_t)cv->arena + (size_t)cv->slots * cv->h.frameSize && (uintptr_t)cv->arena < d + c.dataCap) return zerr(42);
  }
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen, as the search
  ArchiveView arc;
  STCHK(view(E, c.dArc, c.arcSize, cv, &arc));
  // ---- 3. the range [lo, hi)
  uint64_t lo, hi;
  if (!scan_range(arc.U, c.offset, c.size, &lo, &hi)) return {kOutOfBounds, 0};
  uint64_t* const stats = E.callStats_[which];
  if (hi == lo || sel.nothing(hi - lo)) { stats[0] = arc.frames; return ok(); }
  if (arc.fs == 0 || arc.frames == 0) return {kHeaderInvalid, 0};
  // ---- 4. the passes (the last one always owns a position: it holds byte hi - 1)
  const ScanPlan P = scan_plan(arc.U, arc.fs, lo, hi, sel.M, 0, c.stagingBytes);
  const size_t listCap = (size_t)std::min<uint64_t>(c.recordCap, hi - lo);   // (no list is longer: a record per delimiter, or the one open at hi)
  const size_t kTotals = sel.table_bytes(), kHead = kTotals + sizeof(Totals);
  std::vector<uint8_t> head(kHead, 0);                                       // (the totals go up as zeros, the state as "a record opens at lo")
  sel.build(head.data(), c);
  Totals& h = *(Totals*)(head.data() + kTotals);
  h.st[0].start = lo;
  sel.open(h.st[0]);
  uint32_t launches = 0;                                                     // (the driver counts the callbacks in place: inside one, those in front of it)
  STCHK(passes(E, arc, P, &E.callMs_[which], head.data(), kHead, kTotals, sizeof(Totals),
               kHead + P.tilesMax * (sizeof(typename K::Sum) + sizeof(typename K::Head) + K::kMapBytes) + 64, (listCap + c.before) * sizeof(Range) + 64, true, [&](const ScanPass& ps) {
    uint8_t* const tb = E.scan_.tables.as<uint8_t>();
    RecordPass<K> p;
    p.win = window(E); p.table = tb;
    p.tot = (Totals*)(tb + kTotals);
    p.sums = (typename K::Sum*)(tb + kHead);
    p.heads = (typename K::Head*)(p.sums + P.tilesMax);
    p.maps = (uint8_t*)(p.heads + P.tilesMax);
    p.list = E.scan_.list.as<Range>(); p.listCap = listCap; p.hi = hi;
    p.tiles = (uint32_t)((ps.nPos + kTile - 1) / kTile); p.groups = (p.tiles + kGroup - 1) / kGroup;
    K::launch(s, sel, c, ps, p, launches & 1);
  }, &launches, cv));
  // ---- 5. the totals (they came back with the last synchronisation), then the list, once
  const auto& fin = h.st[launches & 1];
  const uint64_t total = fin.sel;
  uint64_t listed = std::min<uint64_t>(total, listCap), word5 = listed;      // a grep clips its list to the capacity
  *c.nRecords = total;
  if constexpr (K::kData) {
    *c.dataSize = word5 = fin.bytes;
    if ((c.recordCap && total > c.recordCap) || fin.bytes > c.dataCap) return {kOutputTooSmall, 0};   // 7: the two words say what the call needs
  }
  if (listed) {
    HIPCHK_CLR(hipMemcpyAsync(c.hRecords, E.scan_.list.p, (size_t)listed * sizeof(Range), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  context_outputs(fin, c, 0);
  const uint64_t st8[8] = {arc.frames, decoded_frames(P, cv), decoded_bytes(P, cv), h.delims + fin.tail, total, word5, P.passes, h.matches};
  std::copy(st8, st8 + 8, stats);
  return ok();
  });
}

}  // namespace zra_eng
