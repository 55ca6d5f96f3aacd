// The scratch arithmetic of the encode driver (zra_amd/csrc/zra_enc_plan.h) walked over every level -128..22, the frame sizes 1, 7,
// 1024, 4096, 16384, 65536, 100000, 131072, 262144 and 2 MiB, and a call without a short last frame and with one of 1 byte, a third of
// the frame, and the frame less one byte (where the frame is that long). Per case:
//  1. the sequence store of a frame holds what a block can produce: seqStride >= blockSize / minMatch for both parameter sets (every
//     sequence carries a match of at least minMatch bytes), and it is a multiple of 8 (the chain kernel moves 8 bytes at a time);
//  2. where both parameter sets have minMatch >= 4 every stride is what the driver computed before the plan moved here:
//     seqStride = (maxBlock / 4 + 16 + 7) & ~7, litStride = (maxBlock + 64 + 15) & ~15, entWorkStride = (9 * seqStride + 255) & ~255,
//     the slot is compressBound(frameSize) + 1024 + 4 per block rounded to 16, and perFrame is the same sum;
//  3. the work area of the entropy stage holds its [3][seqStride] code bytes and [3][seqStride] u16 behind them, the literal buffer a
//     block and the 64 bytes the gather reads past it.
// Prints "cases N bad B"; exit status 1 when B != 0.
// `enc_plan_check stride LEVEL FRAMESIZE INSIZE` prints the seqStride of that call instead (tests/test_enc_plan.py holds the
// oracle's sequence counts of dense inputs against it). Run by tests/test_enc_plan.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "zra_enc_plan.h"

using namespace zra_eng;

static unsigned long long cases = 0, bad = 0;
static void fail(const char* what, int level, uint64_t fs, uint64_t tailSize, uint64_t a, uint64_t b) {
  if (bad++ < 10) std::printf("bad %s: level %d fs %llu tail %llu a %llu b %llu\n", what, level, (unsigned long long)fs, (unsigned long long)tailSize,
                              (unsigned long long)a, (unsigned long long)b);
}

// the two parameter sets of a call of inSize bytes in frames of fs, as the driver picks them
static bool call_params(int level, uint64_t fs, uint64_t inSize, ZraEncParams* full, ZraEncParams* tail, uint32_t* maxBlocksPerFrame) {
  const uint64_t nFrames = (inSize + fs - 1) / fs, tailSize = inSize % fs;
  const bool hasFull = nFrames > 1 || !tailSize;
  if (hasFull && !get_params(level, fs, full)) return false;
  if (tailSize && !get_params(level, tailSize, tail)) return false;
  if (!hasFull) *full = *tail;
  if (!tailSize) *tail = *full;
  const uint64_t fullFrame = fs < inSize ? fs : inSize;
  const uint64_t bf = hasFull ? (fullFrame + full->blockSize - 1) / full->blockSize : 0, bt = tailSize ? (tailSize + tail->blockSize - 1) / tail->blockSize : 0;
  *maxBlocksPerFrame = (uint32_t)(bf > bt ? bf : bt);
  return true;
}

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "stride")) {
    ZraEncParams full{}, tail{}; uint32_t mb = 0;
    const uint64_t fs = std::strtoull(argv[3], nullptr, 10), inSize = std::strtoull(argv[4], nullptr, 10);
    if (!fs || !inSize || !call_params(std::atoi(argv[2]), fs, inSize, &full, &tail, &mb)) return 2;
    const EncPlan P = enc_plan(full, tail, (uint32_t)fs, mb);
    std::printf("seqStride %llu minMatch %u %u blockSize %u %u\n", (unsigned long long)P.seqStride, full.minMatch, tail.minMatch, full.blockSize, tail.blockSize);
    return 0;
  }
  const uint64_t sizes[] = {1, 7, 1024, 4096, 16384, 65536, 100000, 131072, 262144, 2u << 20};
  for (int level = -128; level <= 22; level++)
    for (uint64_t fs : sizes) {
      const uint64_t tails[] = {0, 1, fs / 3, fs - 1};
      for (int t = 0; t < 4; t++) {
        const uint64_t tailSize = tails[t];
        if (t && (tailSize == 0 || tailSize >= fs || (t > 1 && tailSize == tails[t - 1]))) continue;
        // three full frames and the tail; and the tail alone (a call shorter than a frame)
        for (int alone = 0; alone <= (tailSize ? 1 : 0); alone++) {
          ZraEncParams full{}, tail{}; uint32_t mb = 0;
          cases++;
          if (!call_params(level, fs, alone ? tailSize : 3 * fs + tailSize, &full, &tail, &mb)) { fail("params", level, fs, tailSize, 0, 0); continue; }
          const EncPlan P = enc_plan(full, tail, (uint32_t)fs, mb);
          // 1
          if (P.seqStride < full.blockSize / full.minMatch) fail("seqs full", level, fs, tailSize, P.seqStride, full.blockSize / full.minMatch);
          if (P.seqStride < tail.blockSize / tail.minMatch) fail("seqs tail", level, fs, tailSize, P.seqStride, tail.blockSize / tail.minMatch);
          if (P.seqStride % 8) fail("seqs % 8", level, fs, tailSize, P.seqStride, 0);
          // 2
          const uint64_t maxBlock = full.blockSize > tail.blockSize ? full.blockSize : tail.blockSize;
          const uint64_t oldSeq = (maxBlock / 4 + 16 + 7) & ~7ull, oldLit = (maxBlock + 64 + 15) & ~15ull;
          if (P.maxBlock != maxBlock || P.litStride != oldLit) fail("lits", level, fs, tailSize, P.litStride, oldLit);
          if (P.entWorkStride != ((9 * P.seqStride + 255) & ~255ull)) fail("work", level, fs, tailSize, P.entWorkStride, P.seqStride);
          if (P.slotStride != ((zra_fmt::compress_bound(fs) + 1024 + 4 * (uint64_t)mb + 15) & ~15ull)) fail("slot", level, fs, tailSize, P.slotStride, mb);
          if (full.minMatch >= 4 && tail.minMatch >= 4) {
            if (P.seqStride != oldSeq) fail("seqs changed", level, fs, tailSize, P.seqStride, oldSeq);
            const uint64_t oldPer = P.tableWords * 4 + oldSeq * 8 + oldLit + P.slotStride + sizeof(ZraEncFrameState) + sizeof(ZraEncBlockOut) + 64;
            if (P.perFrame != oldPer) fail("perFrame changed", level, fs, tailSize, P.perFrame, oldPer);
          } else if (P.seqStride < oldSeq) fail("seqs shrank", level, fs, tailSize, P.seqStride, oldSeq);
          if (P.perFrame != P.tableWords * 4 + P.seqStride * 8 + P.litStride + P.slotStride + sizeof(ZraEncFrameState) + sizeof(ZraEncBlockOut) + 64)
            fail("perFrame", level, fs, tailSize, P.perFrame, 0);
          // 3
          if (P.entWorkStride < 9 * P.seqStride || P.entWorkStride % 256) fail("work holds", level, fs, tailSize, P.entWorkStride, P.seqStride);
          if (P.litStride < maxBlock + 64 || P.litStride % 16 || P.tableWords % 4 || P.slotStride % 16) fail("align", level, fs, tailSize, P.litStride, P.tableWords);
        }
      }
    }
  std::printf("cases %llu bad %llu\n", cases, bad);
  return bad != 0;
}
