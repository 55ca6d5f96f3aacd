// zra_amd — the scratch arithmetic of the encode driver (zra_encode.hip): the zstd 1.4.9 parameters of a frame size class and, from
// the parameters of a call's full-size frames and of its short last frame, the per-frame strides of the sequence store, the literal
// buffer and the entropy stage's work area, and the bytes a frame costs a batch. Plain C++17, host only, no HIP types and nothing of
// the engine: tools/model/enc_plan_check.cpp walks it over every level and frame size class on the CPU (tests/test_enc_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include "zra_format.h"
#include "zra_kernels.h"

namespace zra_eng {

// ---- zstd 1.4.9 parameter rows (dumped there from the dependency): [wlog clog hlog slog mml tlen strat]
inline const uint16_t kCP16[23][7] = {{14,14,15,2,4,0,2},{14,14,15,1,5,0,1},{14,14,15,1,4,0,1},{14,14,15,2,4,0,2},{14,14,14,4,4,2,3},{14,14,14,3,4,4,4},
  {14,14,14,4,4,8,5},{14,14,14,6,4,8,5},{14,14,14,8,4,8,5},{14,15,14,5,4,8,6},{14,15,14,9,4,8,6},{14,15,14,3,4,12,7},{14,15,14,4,3,24,7},
  {14,15,14,5,3,32,8},{14,15,15,6,3,64,8},{14,15,15,7,3,256,8},{14,15,15,5,3,48,9},{14,15,15,6,3,128,9},{14,15,15,7,3,256,9},{14,15,15,8,3,256,9},{14,15,15,8,3,512,9},{14,15,15,9,3,512,9},{14,15,15,10,3,999,9}};
inline const uint16_t kCP128[23][7] = {{17,15,16,2,5,0,2},{17,12,13,1,6,0,1},{17,13,15,1,5,0,1},{17,15,16,2,5,0,2},{17,17,17,2,4,0,2},{17,16,17,3,4,2,3},
  {17,17,17,3,4,4,4},{17,17,17,3,4,8,5},{17,17,17,4,4,8,5},{17,17,17,5,4,8,5},{17,17,17,6,4,8,5},{17,17,17,5,4,8,6},{17,18,17,7,4,12,6},
  {17,18,17,3,4,12,7},{17,18,17,4,3,32,7},{17,18,17,6,3,256,7},{17,18,17,6,3,128,8},{17,18,17,8,3,256,8},{17,18,17,10,3,512,8},{17,18,17,5,3,256,9},{17,18,17,7,3,512,9},{17,18,17,9,3,512,9},{17,18,17,11,3,999,9}};
inline const uint16_t kCP256[23][7] = {{18,16,16,1,4,0,2},{18,13,14,1,6,0,1},{18,14,14,1,5,0,2},{18,16,16,1,4,0,2},{18,16,17,2,5,2,3},{18,18,18,3,5,2,3},
  {18,18,19,3,5,4,4},{18,18,19,4,4,4,4},{18,18,19,4,4,8,5},{18,18,19,5,4,8,5},{18,18,19,6,4,8,5},{18,18,19,5,4,12,6},{18,19,19,7,4,12,6},
  {18,18,19,4,4,16,7},{18,18,19,4,3,32,7},{18,18,19,6,3,128,7},{18,19,19,6,3,128,8},{18,19,19,8,3,256,8},{18,19,19,6,3,128,9},{18,19,19,8,3,256,9},{18,19,19,10,3,512,9},{18,19,19,12,3,512,9},{18,19,19,13,3,999,9}};

// row 0 of ZSTD_getCParams_internal's level tables, "base for negative levels": strategy fast, the level becomes the acceleration
// (targetLength = -level), and literals are then stored raw (ZSTD_compressLiterals' disableLiteralCompression)
inline const uint16_t kCPNeg16[7] = {14, 12, 13, 1, 5, 1, 1}, kCPNeg128[7] = {17, 12, 12, 1, 5, 1, 1}, kCPNeg256[7] = {18, 12, 13, 1, 5, 1, 1};

// the "default" table (srcSize > 256 KB), levels 0..15 (13-15: btlazy2)
inline const uint16_t kCPDef[23][7] = {{21,16,17,1,5,0,2},{19,13,14,1,7,0,1},{20,15,16,1,6,0,1},{21,16,17,1,5,0,2},{21,18,18,1,5,0,2},{21,18,19,2,5,2,3},
  {21,19,19,3,5,4,3},{21,19,19,3,5,8,4},{21,19,19,3,5,16,5},{21,19,20,4,5,16,5},{22,20,21,4,5,16,5},{22,21,22,4,5,16,5},{22,21,22,5,5,16,5},
  {22,21,22,5,5,32,6},{22,22,23,5,5,32,6},{22,23,23,6,5,32,6},
  {22,22,22,5,5,48,7},{23,23,22,5,4,64,7},{23,23,22,6,3,64,8},{23,24,22,7,3,256,9},{25,25,23,7,3,256,9},{26,26,24,7,3,512,9},{27,27,25,9,3,999,9}};
inline const uint16_t kCPNegDef[7] = {19, 12, 13, 1, 6, 1, 1};

// parameters of ZSTD_getCParams(level, S) for every level (-128..22); false only for S == 0
inline bool get_params(int level, size_t S, ZraEncParams* p) {
  if (level == 0) level = 3;
  if (S == 0) return false;
  if (level > 22) level = 22;                                                       // ZSTD_maxCLevel
  const uint16_t* r = level < 0 ? (S <= (16u << 10) ? kCPNeg16 : S <= (128u << 10) ? kCPNeg128 : S <= (256u << 10) ? kCPNeg256 : kCPNegDef)
                               : (S <= (16u << 10) ? kCP16[level] : S <= (128u << 10) ? kCP128[level] : S <= (256u << 10) ? kCP256[level] : kCPDef[level]);
  // (a frame larger than 2^windowLog is parsed by the serial finders with the sliding-window rules: compress_impl_body, serialAll)
  p->windowLog = r[0]; p->chainLog = r[1]; p->hashLog = r[2]; p->searchLog = r[3]; p->minMatch = r[4];
  p->targetLength = level < 0 ? (uint32_t)(-level) : r[5]; p->strategy = r[6];
  const uint32_t srcLog = S < 64 ? 6 : (31u - (uint32_t)__builtin_clz((uint32_t)S - 1)) + 1;
  if (p->windowLog > srcLog) p->windowLog = srcLog;
  if (p->hashLog > p->windowLog + 1) p->hashLog = p->windowLog + 1;
  const uint32_t cycleLog = p->chainLog - (p->strategy >= 6);
  if (cycleLog > p->windowLog) p->chainLog -= cycleLog - p->windowLog;
  if (p->windowLog < 10) p->windowLog = 10;
  p->blockSize = std::min<uint32_t>(128u << 10, 1u << p->windowLog);
  return true;
}

// The sequences a block of these parameters can hold: every sequence carries a match of at least minMatch bytes, and zstd's finders
// take minMatch 3 for what it is only with the optimal parsers; every other finder's shortest match is 4 bytes whatever the table says
// (ZSTD_resetCCtx_internal sizes its store the same way: blockSize / (minMatch == 3 ? 3 : 4)).
inline uint64_t enc_max_seqs(const ZraEncParams& q) { return q.blockSize / (q.minMatch == 3 ? 3u : 4u); }

// Per-frame scratch of a call whose full-size frames take `full` and whose short last frame takes `tail` (a call without one of the
// two passes the other twice).
struct EncPlan {
  uint64_t tableWords;     // u32 words of the frame's table slot: hash table + chain table / tree (+ the optimal parsers' 3-byte hash table and state), 16-byte slots
  uint32_t maxBlock;       // the larger of the two block sizes
  uint64_t seqStride;      // packed sequences (8 bytes each) per frame: what the block with the most sequences holds, + 16, a multiple of 8 (the
                           // entropy stage's u16 chain output sits behind 3 * seqStride code bytes, and the chain kernel moves 8 bytes at a time)
  uint64_t litStride;      // literal bytes per entropy-stage workgroup
  uint64_t entWorkStride;  // entropy stage's work area: codes [3][seqStride] u8 + chain output [3][seqStride] u16, 256-byte aligned
  uint64_t slotStride;     // the encoded frame's slot
  uint64_t perFrame;       // bytes a frame of the batch path costs its context (what the batch size is cut from)
};
inline uint64_t enc_slot_words(const ZraEncParams& q) {
  uint64_t w = (1ull << q.hashLog) + (1ull << q.chainLog);
  if (q.strategy >= 3 && q.strategy <= 5) w += 3ull << q.chainLog;   // the wave-cooperative hash-chain finder keeps four links per slot
  if (q.strategy >= 7) w += (q.minMatch == 3 ? 1ull << std::min(17u, q.windowLog) : 0) + (sizeof(ZraOptState) + 3) / 4 + 16;
  return w;
}
inline EncPlan enc_plan(const ZraEncParams& full, const ZraEncParams& tail, uint32_t frameSize, uint32_t maxBlocksPerFrame) {
  EncPlan P{};
  P.tableWords = (std::max(enc_slot_words(full), enc_slot_words(tail)) + 3) & ~3ull;
  P.maxBlock = std::max(full.blockSize, tail.blockSize);
  P.seqStride = (std::max(enc_max_seqs(full), enc_max_seqs(tail)) + 16 + 7) & ~7ull;
  P.litStride = ((uint64_t)P.maxBlock + 64 + 15) & ~15ull;
  P.entWorkStride = (9 * P.seqStride + 255) & ~255ull;
  P.slotStride = (zra_fmt::compress_bound(frameSize) + 1024 + 4 * (uint64_t)maxBlocksPerFrame + 15) & ~15ull;
  P.perFrame = P.tableWords * 4 + P.seqStride * 8 + P.litStride + P.slotStride + sizeof(ZraEncFrameState) + sizeof(ZraEncBlockOut) + 64;
  return P;
}

}  // namespace zra_eng
