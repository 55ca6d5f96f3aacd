// Host check of (pending) in zra_amd/csrc/zra_context.h: the records that wait in scratch across the passes of a grep
// with context until a later pass selects a record, or never does. Stand-alone: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zra_amd/csrc tools/model/context_pass_check.cpp
// A case: a stream of 0 .. 300 selection bits (no automaton: the algebra starts where a record's bit is known), the last record open
// at the range's end or not, widths before and after in 0 .. 64, the stream cut into 1 .. 6 passes, some of which end no record and
// some exactly one. Every pass does what the kernels of zra_context_tile.h do, with the very pass_end() they call: the old pending
// ranges are moved, kept or dropped, the pass's own pending records go to slot pendBase + npThis - 1 - dist, and the members of O to
// the list at the (true count). After every pass np == min(uncovered tail of the stream so far, before) and the pending entries are
// exactly those records, ascending; no slot index reaches `before`; after the last pass the list is the brute-force O with its
// selected bits, and |S|, |O| and the groups agree. Ends with "context_pass_check: N cases ok".
#include "zra_context.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {
using namespace zra_ctx;
constexpr uint32_t kNone = 0xFFFFFFFFu, kSelected = 1u << 30;

struct Case { std::vector<uint32_t> sel; std::vector<size_t> cuts; uint32_t before, after; bool open; };

int fail(const char* what, unsigned long long n, const Case& c, size_t pass) {
  std::printf("context_pass_check: case %llu FAILED (%s) in pass %zu: before %u after %u open %d bits ", n, what, pass, c.before, c.after, (int)c.open);
  for (uint32_t s : c.sel) std::printf("%u", s);
  std::printf(" passes end behind record");
  for (size_t r : c.cuts) std::printf(" %zu", r);
  std::printf("\n");
  return 1;
}
uint32_t record_look(uint32_t selected) { return selected ? look(true, 0) : look(false, 1); }
}  // namespace

int main(int argc, char** argv) {
  const unsigned long long want = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 200000;
  std::mt19937 rng(20240607);
  unsigned long long done = 0;
  for (; done < want; done++) {
    Case c;
    c.before = (rng() & 3) ? rng() % 5 : rng() % 65;
    c.after = (rng() & 3) ? rng() % 5 : rng() % 65;
    const size_t n = rng() % ((rng() & 3) ? 40 : 301);
    const uint32_t density = 1 + rng() % 40;                                  // a selected record in `density`
    c.sel.resize(n);
    for (auto& s : c.sel) s = rng() % density == 0;
    c.open = n && (rng() & 1);                                                // the last record has no delimiter: the last pass ends it at hi
    const size_t nd = n - (c.open ? 1 : 0), passes = 1 + rng() % 6;
    const uint32_t before = c.before, after = c.after;
    for (size_t p = 0, r = 0; p < passes; p++) {                              // pass p ends the records [cuts[p - 1], cuts[p]) at their delimiters
      const uint32_t how = rng() % 4;
      r = p + 1 == passes ? nd : how == 0 ? r : how == 1 ? std::min(nd, r + 1) : r + rng() % (nd - r + 1);
      c.cuts.push_back(r);
    }
    // ---- the brute-force walk
    const long long R = (long long)n;
    std::vector<uint8_t> inO(n, 0);
    uint64_t nSel = 0, nOut = 0, nGroups = 0;
    for (long long j = 0; j < R; j++)
      if (c.sel[j]) {
        nSel++;
        for (long long k = std::max(0ll, j - (long long)before); k <= std::min(R - 1, j + (long long)after); k++) inO[k] = 1;
      }
    std::vector<uint32_t> wantList;
    for (long long k = 0; k < R; k++) {
      nGroups += inO[k] && (k == 0 || !inO[k - 1]);
      if (inO[k]) wantList.push_back((uint32_t)k | (c.sel[k] ? kSelected : 0));
    }
    nOut = wantList.size();
    // ---- the passes: the carried state, the list and the scratch of `before` pending entries behind it
    std::vector<uint32_t> list(nOut, kNone), pend(before, kNone);
    Ctx carried = Ctx{0, 0, 0, 0, 0};
    uint32_t np = 0;
    size_t r0 = 0;
    for (size_t p = 0; p < passes; p++) {
      const size_t r1 = c.cuts[p];
      const bool lastPass = p + 1 == passes, tailRec = lastPass && c.open;
      const size_t rEnd = r1 + (tailRec ? 1 : 0);
      // the look from every record of the pass on, the record open at hi included; from[rEnd - r0] is the look behind the pass
      std::vector<uint32_t> from(rEnd - r0 + 1, look(false, 0));
      for (size_t k = rEnd; k-- > r0;) from[k - r0] = look_cat(record_look(c.sel[k]), from[k + 1 - r0]);
      // the records that end at a delimiter, forwards: (forward) in front, (look) behind, the (true count)
      Ctx C = carried;
      std::vector<Ctx> front;
      for (size_t k = r0; k < r1; k++) { front.push_back(C); push(C, c.sel[k], before, after); }
      const Ctx atTiles = C;
      if (tailRec) push(C, c.sel[r1], before, after);
      const PassEnd e = pass_end(from[0], carried.out, np, C, lastPass, before, after);
      // the scan kernel's move: read all, then write
      if (e.cnt > np || e.src + e.cnt > before || e.np > before || e.pendBase + e.npThis > before) return fail("a pending index reaches before", done, c, p);
      const std::vector<uint32_t> moved(pend.begin() + e.src, pend.begin() + e.src + e.cnt);
      for (uint32_t i = 0; i < e.cnt; i++) {
        if (!e.toList) { pend[i] = moved[i]; continue; }
        if (e.to + i >= nOut || list[e.to + i] != kNone) return fail("a moved range lands outside its place", done, c, p);
        list[e.to + i] = moved[i];
      }
      auto put = [&](uint64_t at, size_t k) {
        if (at >= nOut || list[at] != kNone) return false;
        list[at] = (uint32_t)k | (c.sel[k] ? kSelected : 0);
        return true;
      };
      // the fill
      for (size_t k = r0; k < r1; k++) {
        const Ctx& F = front[k - r0];
        const uint32_t behind = from[k + 1 - r0];
        const bool member = c.sel[k] || (F.sel && F.tail < after) || (look_has(behind) && look_d(behind) < before);
        if (member) {
          if (!put(F.out + confirmed(uncovered(F, after), from[k - r0], before), k)) return fail("a member of O lands outside its place", done, c, p);
        } else if (!look_has(behind) && look_d(behind) < e.npThis) {
          const uint32_t slot = e.pendBase + e.npThis - 1 - look_d(behind);
          if (slot >= before) return fail("a pending slot reaches before", done, c, p);
          pend[slot] = (uint32_t)k;
        }
      }
      // the record open at hi, by the scan kernel's last lane
      if (tailRec && (c.sel[r1] || (atTiles.sel && atTiles.tail < after)) &&
          !put(atTiles.out + (c.sel[r1] ? umin(uncovered(atTiles, after), before) : 0u), r1))
        return fail("the record open at hi lands outside its place", done, c, p);
      carried = C; np = e.np;
      // ---- after the pass: the stream so far is [0, rEnd)
      size_t tail = 0, anySel = 0;
      for (size_t k = 0; k < rEnd; k++) { anySel |= c.sel[k]; tail = c.sel[k] ? 0 : tail + 1; }
      const size_t unc = anySel ? tail - std::min<size_t>(tail, after) : tail;
      const size_t wantNp = lastPass && rEnd > r0 ? 0 : std::min<size_t>(unc, before);   // (the last pass drops what is pending)
      if (np != wantNp) return fail("np", done, c, p);
      for (size_t i = 0; i < np; i++)
        if (pend[i] != rEnd - np + i) return fail("the pending entries", done, c, p);
      r0 = r1;
    }
    if (list != wantList) return fail("the list", done, c, passes - 1);
    if (carried.sel != nSel || carried.out != nOut || carried.groups != nGroups) return fail("|S|, |O| or the groups", done, c, passes - 1);
  }
  std::printf("context_pass_check: %llu cases ok\n", done);
  return 0;
}
