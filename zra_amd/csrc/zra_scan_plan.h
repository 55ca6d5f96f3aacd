// zra_amd — the pass geometry of the calls that scan a content range of a device-resident archive a staging window at a time
// (zra_search.hip, zra_msearch.hip, zra_grep.hip, zra_extract.hip): the range rule, the plan of a call and the geometry of one pass.
// Plain C++17, host only, no HIP types and nothing of the engine: tools/model/scan_plan_check.cpp walks it exhaustively on the CPU
// (tests/test_scan_plan.py). The conditions (contiguity), (carry) and (ownership) these formulas implement: zra_search.hip.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zra_eng {

// Slots of one staged pass (whole frames, slot s at s * frameSize of the staging window): at most kPassFrames (one internal pass of
// Engine::decode_jobs) and what fits stagingBytes (0: kStageBytes, which 65,536 frames of the headline 64 KiB fill exactly), at least one.
constexpr uint32_t kPassFrames = 1u << 16;
constexpr uint64_t kStageBytes = 4ull << 30;
inline uint32_t pass_slots(uint64_t fs, uint64_t stagingBytes = 0, uint64_t maxFrames = kPassFrames) {
  const uint64_t fit = (stagingBytes ? stagingBytes : kStageBytes) / (fs ? fs : 1);
  return (uint32_t)(fit < 1 ? 1 : fit < maxFrames ? fit : maxFrames);
}

constexpr uint32_t kScanMaxPattern = 256;   // ZRA_HIP_SEARCH_MAX_PATTERN: the carry area in front of slot 0 holds as many bytes
constexpr uint32_t kScanTile = 8192;        // start positions of one workgroup's tile (zra_scan_tile.h)

// The range rule of the four calls: [offset, offset + size) must lie inside the content, bounds included (a scan reaches the last
// byte), size ~0 = to the end. false: OutOfBounds.
inline bool scan_range(uint64_t U, uint64_t offset, uint64_t size, uint64_t* lo, uint64_t* hi) {
  if (offset > U || (size != ~0ull && (offset + size < offset || offset + size > U))) return false;
  *lo = offset; *hi = size == ~0ull ? U : offset + size;
  return true;
}

// The plan of a call over the range [lo, hi), lo < hi <= U, of a content of U bytes in frames of fs > 0 bytes. M: the longest pattern
// (1 .. kScanMaxPattern). trim: the start positions in front of hi the last pass leaves out: M - 1 for a call that tests only the
// starts p with p + M <= hi (the single search; it needs hi - lo >= M), 0 for one that owns every position of the range.
struct ScanPlan {
  uint64_t U, fs, lo, hi;
  uint32_t M, trim;
  uint64_t f0, f1, n;          // the frames [f0, f1] of the range, n of them
  uint32_t passSlots, nSlots;  // frames of a full pass; slots the window needs
  uint64_t passes, window;     // window = nSlots * fs bytes behind the carry area
  size_t tilesMax;             // no pass has more tiles: a window's worth of positions and up to M - 1 inside the carry area
};
inline ScanPlan scan_plan(uint64_t U, uint64_t fs, uint64_t lo, uint64_t hi, uint32_t M, uint32_t trim, uint64_t stagingBytes) {
  ScanPlan P{};
  P.U = U; P.fs = fs; P.lo = lo; P.hi = hi; P.M = M; P.trim = trim;
  P.f0 = lo / fs; P.f1 = (hi - 1) / fs; P.n = P.f1 - P.f0 + 1;
  P.passSlots = pass_slots(fs, stagingBytes);
  P.nSlots = (uint32_t)(P.n < P.passSlots ? P.n : P.passSlots);
  P.passes = (P.n + P.passSlots - 1) / P.passSlots;
  P.window = (uint64_t)P.nSlots * fs;
  P.tilesMax = (size_t)((P.window + kScanMaxPattern + kScanTile - 1) / kScanTile);
  return P;
}

// Pass p of a plan: the frames [first, first + nj) are decoded into slots 0 .. nj - 1 and hold the content [passBase, passEnd) as one
// run of L bytes (contiguity). Positions are relative to slot 0: position x is content offset passBase + x, and the carry area holds
// the positions [-carry of the passes before, 0). The pass owns the start positions [xLo, xEnd) (ownership), nPos of them (0: none),
// the first one at content offset p0; xHi is the position of the range's end. carry: the bytes in front of slot 0 AFTER this pass.
struct ScanPass {
  uint64_t first;
  uint32_t nj;
  uint64_t passBase, passEnd, L;
  long long xLo, xHi, xEnd;
  uint64_t nPos, p0;
  bool lastPass;
  uint32_t carry;
};
inline ScanPass scan_pass(const ScanPlan& P, uint64_t p, uint32_t carryBefore) {
  ScanPass s{};
  s.first = P.f0 + p * P.passSlots;
  const uint64_t left = P.n - p * P.passSlots;
  s.nj = (uint32_t)(left < P.passSlots ? left : P.passSlots);
  s.lastPass = p + 1 == P.passes;
  s.passBase = s.first * P.fs;
  s.passEnd = (s.first + s.nj) * P.fs < P.U ? (s.first + s.nj) * P.fs : P.U;
  s.L = s.passEnd - s.passBase;
  // a start in front of slot 0 belongs to this pass when the byte that decides its owner lies here: at most M - 1 positions back
  const uint64_t back = s.passBase > P.lo ? s.passBase - P.lo : 0;
  s.xLo = P.lo > s.passBase ? (long long)(P.lo - s.passBase) : -(long long)(back < P.M - 1 ? back : P.M - 1);
  s.xHi = (long long)(P.hi - s.passBase);
  s.xEnd = s.lastPass ? s.xHi - (long long)P.trim : (long long)s.L - (long long)P.M + 1;
  s.nPos = s.xEnd > s.xLo ? (uint64_t)(s.xEnd - s.xLo) : 0;
  s.p0 = s.passBase + (uint64_t)s.xLo;
  s.carry = (uint32_t)(carryBefore + s.L < P.M - 1 ? carryBefore + s.L : P.M - 1);
  return s;
}

}  // namespace zra_eng
