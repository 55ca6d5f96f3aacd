// zra_amd — the pass arithmetic of the device-archive calls that work on whole frames (verify, sign, index, compare, diff, signature
// diff): the frame-range rule, the passes of n consecutive frames, the content bytes of a frame range, the diff's tail behind the
// common content and the two-half window of the pair calls. Plain C++17, host only, no HIP types and nothing of the engine:
// tools/model/pass_plan_check.cpp walks it exhaustively on the CPU (tests/test_pass_plan.py). The driver that runs these passes:
// zra_framepass.h. pass_slots is zra_scan_plan.h's.
#pragma once
#include "zra_scan_plan.h"

namespace zra_eng {

// The frame-range rule of verify, sign and index over an archive of F frames: [first, first + count) must lie inside [0, F], count ~0 =
// up to F. *n: the frames of the range (0 is a range). false: OutOfBounds.
inline bool frame_range(uint64_t F, uint64_t first, uint64_t count, uint64_t* n) {
  if (first > F || (count != ~0ull && count > F - first)) return false;
  *n = count == ~0ull ? F - first : count;
  return true;
}

// The passes of the n consecutive frames [first, first + n) at passSlots >= 1 frames a pass: nSlots slots are ever filled.
struct PassPlan {
  uint64_t first, n;
  uint32_t passSlots, nSlots;
  uint64_t passes;
};
inline PassPlan pass_plan(uint64_t first, uint64_t n, uint32_t passSlots) {
  PassPlan P{};
  P.first = first; P.n = n; P.passSlots = passSlots;
  P.nSlots = (uint32_t)(n < passSlots ? n : passSlots);
  P.passes = (n + passSlots - 1) / passSlots;
  return P;
}
// Pass p < passes of a plan: the frames [first, first + nj), frame first + k in slot k. parity = p & 1: the pass reads word `parity`
// of a ping-pong pair (carry, totals) and writes word parity ^ 1.
struct FramePass {
  uint64_t p, first;
  uint32_t nj, parity;
};
inline FramePass frame_pass(const PassPlan& P, uint64_t p) {
  FramePass s{};
  const uint64_t left = P.n - p * P.passSlots;
  s.p = p; s.first = P.first + p * P.passSlots;
  s.nj = (uint32_t)(left < P.passSlots ? left : P.passSlots);
  s.parity = (uint32_t)(p & 1);
  return s;
}

// The content bytes of frames [first, first + n) of a content of U bytes in frames of fs bytes (the range lies inside the archive's
// frames): the last frame of the archive may be short.
inline uint64_t content_bytes(uint64_t U, uint64_t fs, uint64_t first, uint64_t n) {
  const uint64_t end = (first + n) * fs;
  return n ? (end < U ? end : U) - first * fs : 0;
}

// The diff's tail: B's content [C, U) behind the common content, C <= U, held by B's frames [fT0, fT0 + nTail), the first of which
// may start in front of C. No tail (C == U): nTail = 0.
struct TailPlan {
  uint64_t C, U, fs, fT0, nTail;
};
inline TailPlan tail_plan(uint64_t C, uint64_t U, uint64_t fs) {
  TailPlan T{};
  T.C = C; T.U = U; T.fs = fs;
  T.fT0 = C / fs;
  T.nTail = U > C ? (U + fs - 1) / fs - T.fT0 : 0;
  return T;
}
// What a tail pass over the frames [first, first + nj) adds: the content [pLo, pHi), len bytes, which lie pLo - first * fs bytes
// behind slot 0 and go pLo - C bytes behind the dirty bytes.
struct TailRun {
  uint64_t pLo, pHi, len;
};
inline TailRun tail_run(const TailPlan& T, const FramePass& s) {
  TailRun r{};
  r.pLo = T.C > s.first * T.fs ? T.C : s.first * T.fs;
  r.pHi = (s.first + s.nj) * T.fs < T.U ? (s.first + s.nj) * T.fs : T.U;
  r.len = r.pHi - r.pLo;
  return r;
}

// The pair calls (compare, diff) decode both sides of a frame: a slot costs two frames of staging, and the window is [ half A | half
// B ], a half = the plan's slots rounded up to 16 bytes, so the two plaintexts of a frame share their alignment modulo 16.
inline uint32_t pair_pass_slots(uint64_t fs, uint64_t stagingBytes) { return pass_slots(2 * fs, stagingBytes); }
inline uint64_t pair_half(uint32_t nSlots, uint64_t fs) { return ((uint64_t)nSlots * fs + 15) & ~15ull; }

}  // namespace zra_eng
