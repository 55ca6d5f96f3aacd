// The pass geometry of the range scans (zra_amd/csrc/zra_scan_plan.h) walked exhaustively over small shapes: ownership is a partition.
// Every U in 1..30, frame size in {1, 2, 3, 4, 7, 8}, longest pattern M in {1, 2, 3, 5, 9}, 1..3 slots per pass, every range
// 0 <= lo < hi <= U, and trim in {0, M - 1} (the latter only when hi - lo >= M). Per case:
//  1. the owned intervals [passBase + xLo, passBase + xEnd) of the passes that own something, in pass order, abut, start at lo and end
//     at hi - trim: every start position has exactly one owner and the lists ascend across passes;
//  2. a pass reaches no further in front of slot 0 than the carry area holds after the passes before it;
//  3. the byte that decides the owner of a pass's last start q, min(q + M - 1, hi - 1), lies in front of passEnd: every byte any
//     pattern needs at an owned start is decoded;
//  4. passes == ceil(n / passSlots) and nSlots == min(passSlots, n).
// Prints "cases N bad B"; exit status 1 when B != 0. Run by tests/test_scan_plan.py.
#include <cstdio>
#include "zra_scan_plan.h"

using namespace zra_eng;

static bool check(const ScanPlan& P) {
  const uint64_t n = P.f1 - P.f0 + 1;
  if (P.n != n || P.passes != (n + P.passSlots - 1) / P.passSlots || P.nSlots != (n < P.passSlots ? n : P.passSlots)) return false;   // 4
  uint64_t at = P.lo;
  uint32_t carry = 0;
  for (uint64_t p = 0; p < P.passes; p++) {
    const ScanPass s = scan_pass(P, p, carry);
    if (s.xLo < 0 && (uint64_t)-s.xLo > carry) return false;                                                                         // 2
    if (s.xEnd > s.xLo) {
      if (s.passBase + (uint64_t)s.xLo != at || s.nPos != (uint64_t)(s.xEnd - s.xLo) || s.p0 != at) return false;                     // 1
      at += s.nPos;
      const uint64_t q = at - 1, need = q + P.M - 1 < P.hi - 1 ? q + P.M - 1 : P.hi - 1;
      if (need >= s.passEnd) return false;                                                                                           // 3
    }
    carry = s.carry;
  }
  return at == P.hi - P.trim;                                                                                                        // 1
}

int main() {
  const uint64_t sizes[] = {1, 2, 3, 4, 7, 8};
  const uint32_t longest[] = {1, 2, 3, 5, 9};
  unsigned long long cases = 0, bad = 0;
  for (uint64_t U = 1; U <= 30; U++)
    for (uint64_t fs : sizes)
      for (uint32_t M : longest)
        for (uint64_t slots = 1; slots <= 3; slots++)
          for (uint64_t lo = 0; lo < U; lo++)
            for (uint64_t hi = lo + 1; hi <= U; hi++)
              for (int t = 0; t < 2; t++) {
                if (t && hi - lo < M) continue;
                cases++;
                if (!check(scan_plan(U, fs, lo, hi, M, t ? M - 1 : 0, slots * fs))) {
                  if (bad++ < 10) std::printf("bad: U %llu fs %llu M %u slots %llu lo %llu hi %llu trim %u\n", (unsigned long long)U, (unsigned long long)fs, M,
                                              (unsigned long long)slots, (unsigned long long)lo, (unsigned long long)hi, t ? M - 1 : 0);
                }
              }
  std::printf("cases %llu bad %llu\n", cases, bad);
  return bad != 0;
}
