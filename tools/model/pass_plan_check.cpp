// The pass arithmetic of the calls on whole frames (zra_amd/csrc/zra_pass_plan.h) walked exhaustively over small shapes. Every U in
// 0..40, frame size in {1, 2, 3, 4, 7, 16}, staging such that passSlots is 1, 2, 3, 5 or all frames of the archive; every first in
// 0..F + 1 with every count in 0..F + 1 and ~0 (the range rule, ranges that leave the archive among them), and every C <= U (the
// diff's tail). Per case:
//  1. the range rule agrees with a brute-force statement of it: every frame of the range is a frame of the archive;
//  2. the passes of a range tile [first, first + n) in order, without a gap or an overlap; 1 <= nj <= passSlots; there are
//     ceil(n / passSlots) of them and nSlots = min(passSlots, n); the parity is the pass number's;
//  3. the content bytes of the range equal the sum over its passes, and a brute-force count of the content bytes its frames hold;
//  4. the tail's frames are the frames of B that hold a byte of [C, U), and the runs [pLo, pHi) of its passes tile [C, U) in order,
//     each inside the frames of its pass;
//  5. the pair window: a half holds the plan's slots, is a multiple of 16 and wastes fewer than 16 bytes; a pair pass has at most as many
//     slots as a single pass of half the staging.
// Prints "cases N bad B"; exit status 1 when B != 0. Run by tests/test_pass_plan.py.
#include <cstdio>
#include "zra_pass_plan.h"

using namespace zra_eng;

static unsigned long long cases = 0, bad = 0;
static void fail(const char* what, uint64_t U, uint64_t fs, uint32_t slots, uint64_t a, uint64_t b) {
  if (bad++ < 10) std::printf("bad %s: U %llu fs %llu slots %u a %llu b %llu\n", what, (unsigned long long)U, (unsigned long long)fs, slots, (unsigned long long)a,
                              (unsigned long long)b);
}

// 2 and 3 for the frames [first, first + n) of a content of U bytes
static bool passes_tile(uint64_t U, uint64_t fs, uint64_t first, uint64_t n, uint32_t passSlots) {
  const PassPlan P = pass_plan(first, n, passSlots);
  if (P.passes != (n + passSlots - 1) / passSlots || P.nSlots != (n < passSlots ? n : passSlots)) return false;
  uint64_t at = first, bytes = 0;
  for (uint64_t p = 0; p < P.passes; p++) {
    const FramePass s = frame_pass(P, p);
    if (s.p != p || s.first != at || s.nj < 1 || s.nj > passSlots || s.nj > P.nSlots || s.parity != (p & 1)) return false;
    at += s.nj;
    bytes += content_bytes(U, fs, s.first, s.nj);
  }
  if (at != first + n) return false;
  uint64_t brute = 0;
  for (uint64_t x = 0; x < U; x++) brute += x / fs >= first && x / fs < first + n;
  return bytes == brute && content_bytes(U, fs, first, n) == brute;
}

// 4 for the tail [C, U)
static bool tail_tiles(uint64_t C, uint64_t U, uint64_t fs, uint32_t passSlots) {
  const TailPlan T = tail_plan(C, U, fs);
  uint64_t lowest = ~0ull, highest = 0, held = 0;
  for (uint64_t x = C; x < U; x++) { const uint64_t f = x / fs; if (f < lowest) lowest = f; if (f > highest) highest = f; held++; }
  if (held ? (T.fT0 != lowest || T.nTail != highest - lowest + 1) : T.nTail != 0) return false;
  const PassPlan P = pass_plan(T.fT0, T.nTail, passSlots);
  uint64_t at = C;
  for (uint64_t p = 0; p < P.passes; p++) {
    const FramePass s = frame_pass(P, p);
    const TailRun r = tail_run(T, s);
    if (r.pLo != at || r.pHi <= r.pLo || r.len != r.pHi - r.pLo || r.pLo < s.first * fs || r.pHi > (s.first + s.nj) * fs) return false;
    at = r.pHi;
  }
  return at == U;
}

int main() {
  const uint64_t sizes[] = {1, 2, 3, 4, 7, 16};
  const uint32_t slotChoices[] = {1, 2, 3, 5, 0};                              // 0: all frames in one pass
  for (uint64_t U = 0; U <= 40; U++)
    for (uint64_t fs : sizes) {
      const uint64_t F = (U + fs - 1) / fs;
      for (uint32_t choice : slotChoices) {
        const uint64_t staging = (choice ? choice : (F ? F : 1)) * fs;
        const uint32_t passSlots = pass_slots(fs, staging);
        cases++;
        if (passSlots != (choice ? choice : (F ? F : 1))) fail("slots", U, fs, passSlots, staging, 0);
        // 5
        for (uint32_t nSlots = 0; nSlots <= passSlots; nSlots++) {
          const uint64_t half = pair_half(nSlots, fs);
          cases++;
          if (half % 16 || half < (uint64_t)nSlots * fs || half - (uint64_t)nSlots * fs >= 16) fail("half", U, fs, passSlots, nSlots, half);
        }
        cases++;
        if (pair_pass_slots(fs, staging) < 1 || pair_pass_slots(fs, staging) != pass_slots(fs, staging / 2 >= fs ? staging / 2 : 1)) fail("pair", U, fs, passSlots, staging, 0);
        // 1, 2, 3
        for (uint64_t first = 0; first <= F + 1; first++)
          for (uint64_t c = 0; c <= F + 2; c++) {
            const uint64_t count = c == F + 2 ? ~0ull : c;
            uint64_t n = ~0ull;
            const bool okRule = frame_range(F, first, count, &n);
            bool brute = first <= F;
            uint64_t want = 0;
            if (brute) {
              if (count == ~0ull) want = F - first;
              else { want = count; for (uint64_t f = first; f < first + count; f++) brute = brute && f < F; }
            }
            cases++;
            if (okRule != brute || (okRule && n != want)) { fail("range", U, fs, passSlots, first, count); continue; }
            if (okRule && !passes_tile(U, fs, first, n, passSlots)) fail("passes", U, fs, passSlots, first, n);
          }
        // 4
        for (uint64_t C = 0; C <= U; C++) {
          cases++;
          if (!tail_tiles(C, U, fs, passSlots)) fail("tail", U, fs, passSlots, C, 0);
        }
      }
    }
  std::printf("cases %llu bad %llu\n", cases, bad);
  return bad != 0;
}
