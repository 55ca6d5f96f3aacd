// zra_amd — content signatures of a device-resident archive (zra_hip.h: ZraHipSignArchive) and the diff of an archive against the
// signature of a replica that lies elsewhere (ZraHipDiffSignature). A signature is a record of 1 + gpf XXH64 words per frame, gpf =
// ceil(frameSize / grain): word 0 over the frame's compressed span, word 1 + g over grain g of its plaintext, grains cut as the diff
// cuts them (zra_compare.hip). Updates overwrite in place and append, so aligned grains are enough: no rolling hash.
//
// Sign, per pass of at most passSlots consecutive frames of the range:
//   1. the seek-table span of every frame is hashed as it lies, four lanes per frame -> word 0 of its record     zra_sig_spans_kernel
//   2. the frames become decode jobs, slot = frame - first frame of the pass                                      search_launch_jobs
//   3. the pass is decoded whole, checksums verified, into the staging window                                     Engine::staged_pass
//   4. every grain of the window is hashed, four lanes per grain -> words 1 .. gpf of the records                 zra_sig_grains_kernel
// Signature diff, per pass over the frames of [0, C), C = A's content size:
//   1. B's span of every frame is hashed and compared with A's frame word: one flag per slot, equal or decode     zra_sig_spans_kernel
//   2. the decode-flagged frames, in frame order, become decode jobs, each into its own slot                       zra_sig_jobs_kernel
//   3. they are decoded whole; none flagged: the decoder is not launched                                           Engine::staged_pass
//   4. every grain of the pass is hashed and compared with A's word: one dirty flag per grain, 0 for the grains
//      of a frame that was not decoded and for grains without a byte                                               zra_sig_grains_kernel
//   5. starts, ends and dirty bytes per item of 256 grains                                                         zra_sig_count_kernel
//   6. the item counts become list positions and places in the packed data (the diff's three-column scan)         diff_launch_scan
//   7. items that hold a listed start or end, or a byte in front of dataCapacity, redo their count, write the
//      positions and copy B's bytes of their dirty grains                                                          zra_sig_fill_kernel
// then B's frames from the one that holds C on, as the diff takes them (search_launch_jobs, staged_pass, diff_launch_tail), and the
// counts and lists come to the host, once.
//
// The passes of both calls run through the one frame-pass driver (zra_framepass.h: the sign's plain, the signature diff's flagged, the
// tail's plain again): their order on the stream, the timed span and which failing frame ends the call are stated there. What the
// kernels of this file rely on:
//  (slots) slot = frame - first frame of the pass whether the frame is decoded or not, slot s at s * frameSize of the window. Grain
//      i = s * gpf + g of a pass is the bytes [g * grain, min((g + 1) * grain, frameSize)) of slot s, clipped to C by arithmetic. A
//      decoded frame regenerates its share of B's content (anything else is a failing frame and ends the call), which covers its share
//      of [0, C) because UB >= UA. The slot of a frame that was not decoded is plaintext of earlier passes and is never read: its flag
//      is looked at first.
//  (runs) the grains of a pass in the order of i are consecutive in content: the last grain of slot s ends where grain 0 of slot s + 1
//      starts. With D(i) = "grain i is dirty", a start is D(i) && !D(i - 1) at the grain's first byte, an end (exclusive) is
//      !D(i) && D(i - 1) at min(first byte of grain i, C) (a grain without a byte lies behind C). D(-1) of a pass is the carry: the
//      count launch leaves D of the pass's last grain in a word (pass k reads word k & 1 and writes word (k + 1) & 1). Behind the last
//      pass the carry is a run that ends at C: the one end no item holds, added by the host.
//  (order) starts, ends and dirty bytes are counted per item, scanned (three 64-bit totals ping-pong between passes) and filled
//      independently; start i and end i belong together. A list position and a byte's place in dData are sums of counts and prefixes,
//      never the result of an atomic, and no workgroup waits for another one. (The dirty-grain and span-byte totals are sums that no
//      position depends on; they are added up with atomics.)
//  (d) the lists stay on the device until the last pass is done; dData alone is written while the passes run, never at or behind
//      dataCapacity. A sign call writes the words of the range's records only, and none at or behind sigCapacityWords.
#include "zra_framepass.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include <algorithm>

using namespace zra_dev;

namespace {
constexpr u32 kItem = 256;                   // grains of one workgroup of the count and fill launches
// the table words in front of the per-item entries (bytes): dirty grains | compressed bytes hashed | carry x 2 (u32) | decode jobs of the
// pass (u32) | totals {starts, ends, dirty bytes} x 2 at kOffTot
constexpr u32 kHdrBytes = 128, kOffGrains = 0, kOffSpan = 8, kOffCarry = 16, kOffJobs = 24, kOffTot = 64;

struct GrainArgs {
  const u8* win; const u8* flags;            // slot 0; slot -> 1 decoded, 0 not (nullptr: every slot is decoded)
  u64 fs, first, C, total;                   // total = slots of the pass x gpf
  u32 gpf, grain;
};
// grain i of a pass: its first content position, and its bytes after the clip to its frame and to C
__device__ __forceinline__ u64 grain_pos(const GrainArgs& G, u64 i) { return (G.first + i / G.gpf) * G.fs + (i % G.gpf) * (u64)G.grain; }
__device__ __forceinline__ u32 grain_len(const GrainArgs& G, u64 i) {
  const u64 f = G.first + i / G.gpf, lo = f * G.fs + (i % G.gpf) * (u64)G.grain, hi = min(min(lo + G.grain, (f + 1) * G.fs), G.C);
  return hi > lo ? (u32)(hi - lo) : 0u;
}
__device__ __forceinline__ const u8* grain_src(const GrainArgs& G, u64 i) { return G.win + (i / G.gpf) * G.fs + (i % G.gpf) * (u64)G.grain; }

// What one item (grains [256 b, 256 b + 256) of a pass, a lane per grain) found: this lane's start, end and dirty bytes, and the
// workgroup's sums per wave in sRed (starts at w, ends at 4 + w, bytes at 8 + w, dirty grains at 12 + w).
struct ItemOut { bool st, en; u32 bytes; u64 i; };
__device__ __forceinline__ void run_item(const GrainArgs& G, const u8* dirty, const u32* carryIn, u32* sRed, ItemOut& o) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  o.i = (u64)blockIdx.x * kItem + tid;
  const bool in = o.i < G.total;
  const bool d = in && dirty[o.i] != 0;
  const bool prev = in && (o.i ? dirty[o.i - 1] != 0 : *carryIn != 0);
  o.st = d && !prev; o.en = in && !d && prev;
  o.bytes = d ? grain_len(G, o.i) : 0u;
  const u32 wS = (u32)__popcll(__ballot(o.st)), wE = (u32)__popcll(__ballot(o.en)), wB = wave_sum(o.bytes), wG = (u32)__popcll(__ballot(d));
  if (lane == 0) { sRed[wave] = wS; sRed[4 + wave] = wE; sRed[8 + wave] = wB; sRed[12 + wave] = wG; }
  __syncthreads();
}
}  // namespace

// Four lanes per frame of a pass: XXH64 with `seed` of the seek-table span of frame first + q, read as it lies (8-byte loads at any
// alignment, only bytes of the span). A span that is not well formed (the decoder's convention: a <= b <= body size) is not read.
// sigOut != nullptr (sign): the word goes to word 0 of the frame's record and the span's length is added to *spanBytes; a frame whose
// span is not well formed is skipped: its decode fails the call.
// sigA != nullptr (signature diff): flags[q] = 0 when the span is well formed and its word equals A's frame word, 1 otherwise: decode.
extern "C" __global__ void __launch_bounds__(256) zra_sig_spans_kernel(const u8* table, const u8* body, u64 bodyBytes, u64 first, u32 nj, u64 seed, u32 stride,
                                                                       u64* sigOut, u64* spanBytes, const u64* sigA, u8* flags) {
  const u32 q = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int j = (int)(threadIdx.x & 3);
  const bool in = q < nj;
  const u64 f = first + (in ? q : 0);
  const u64 a = seek_entry(table, f), b = seek_entry(table, f + 1);
  const bool well = in && a <= b && b <= bodyBytes;
  const u64 h = zra_xxh64_quad_seed(body + (well ? a : 0), well ? b - a : 0, j, seed);   // (every lane of the wave: the group's shuffles)
  if (j != 0 || !in) return;
  if (sigOut) {
    if (well) { sigOut[f * stride] = h; atomicAdd((unsigned long long*)spanBytes, (unsigned long long)(b - a)); }
  } else {
    flags[q] = well && h == sigA[f * stride] ? 0 : 1;
  }
}

// One workgroup walks the slots of the pass, 1024 at a time: the decode-flagged ones, in order, become jobs 0 .. nDec - 1 of archive B
// (zra_joblist.h: block_rank, emit_job), each into the frame's OWN slot. *nJobs: the job count for the host.
extern "C" __global__ void __launch_bounds__(1024) zra_sig_jobs_kernel(const u8* flags, u32 nj, const u8* table, u64 U, u64 fs, u64 first, u64* frameOff, u64* outOff,
                                                                       u32* expect, u32* nJobs) {
  u32 jobBase = 0;
  for (u32 base = 0; base < nj; base += 1024) {
    const u32 s = base + threadIdx.x;
    const bool p[1] = {s < nj && flags[s] != 0};
    u32 rank[1], total[1];
    block_rank<1>(p, rank, total);
    if (p[0]) emit_job(table, first + s, fs, U, jobBase + rank[0], s, frameOff, outOff, expect);
    jobBase += total[0];
  }
  if (threadIdx.x == 0) *nJobs = jobBase;
}

// Four lanes per grain of a pass: XXH64 with `seed` of the grain's bytes in its slot, clipped (grain_len). The slots are not 8-byte
// aligned when the frame size is not: the loads are the hardware's unaligned ones, and only bytes of the grain are read. A wave's 16
// grains are neighbours in the window, so at grain 64 its loads cover 1 KiB in one run; at larger grains a group's four lanes read
// one 32-byte stripe per load, eight loads in flight (zra_xxh64_quad_seed).
// sigOut != nullptr (sign): word 1 + g of the frame's record = the grain's hash, 0 for a grain without a byte.
// sigA != nullptr (signature diff): dirty[i] = 1 when the frame was decoded, the grain has a byte and its hash differs from A's word.
extern "C" __global__ void __launch_bounds__(256) zra_sig_grains_kernel(GrainArgs G, u64 seed, u32 stride, u64* sigOut, const u64* sigA, u8* dirty) {
  const u64 i = (u64)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int j = (int)(threadIdx.x & 3);
  const bool in = i < G.total;
  const u64 ii = in ? i : 0;
  const bool decoded = in && (!G.flags || G.flags[ii / G.gpf] != 0);
  const u32 len = grain_len(G, ii);
  const u64 h = zra_xxh64_quad_seed(grain_src(G, ii), decoded ? len : 0, j, seed);        // (every lane of the wave: the group's shuffles)
  if (j != 0 || !in) return;
  const u64 w = (G.first + ii / G.gpf) * stride + 1 + ii % G.gpf;
  if (sigOut) sigOut[w] = len ? h : 0;
  else dirty[i] = decoded && len && h != sigA[w] ? 1 : 0;
}

// Workgroup b: item b of the pass. tab[3 b] = its starts, tab[3 b + 1] = its ends, tab[3 b + 2] = its dirty bytes. The dirty grains
// are summed into one word (a sum, not a position); the lane of the pass's last grain leaves the carry.
extern "C" __global__ void __launch_bounds__(256) zra_sig_count_kernel(GrainArgs G, const u8* dirty, const u32* carryIn, u64* tab, u64* grains, u32* carryOut) {
  __shared__ u32 sRed[16];
  ItemOut o;
  run_item(G, dirty, carryIn, sRed, o);
  if (o.i + 1 == G.total) *carryOut = dirty[o.i] != 0;
  if (threadIdx.x == 0) {
    u64* const e = tab + 3 * (size_t)blockIdx.x;
    u32 t[4] = {0, 0, 0, 0};
    for (u32 w = 0; w < 4; w++) { t[0] += sRed[w]; t[1] += sRed[4 + w]; t[2] += sRed[8 + w]; t[3] += sRed[12 + w]; }
    e[0] = t[0]; e[1] = t[1]; e[2] = t[2];
    if (t[3]) atomicAdd((unsigned long long*)grains, (unsigned long long)t[3]);
  }
}

// Workgroup b redoes item b's count when it holds a listed start or end, or a dirty byte with a place in front of dataCap (an item
// without any leaves at once). A start's place is the item's base, plus the starts of the waves in front of its own, plus those of
// the lanes in front of its own; an end's and a dirty grain's place in dData likewise. Then the gather copy: every wave packs its 64
// grains, L = min(64, grain / 16) lanes per grain and 64 / L grains at a time, 16 bytes per lane and trip. A 16-byte piece whose
// place is 16-byte aligned and lies in front of dataCap as a whole leaves as one 16-byte store (every piece when the frame size is a
// multiple of the grain and dData is aligned); anything else byte by byte, each byte checked against dataCap.
extern "C" __global__ void __launch_bounds__(256) zra_sig_fill_kernel(GrainArgs G, const u8* dirty, const u32* carryIn, const u64* tab, u64* starts, u64* ends, u64 cap,
                                                                      u8* dData, u64 dataCap) {
  __shared__ u32 sRed[16], sLen[kItem];
  __shared__ u64 sAt[kItem];
  const u64* const e = tab + 3 * (size_t)blockIdx.x;
  const u64 baseS = e[0], baseE = e[1], baseB = e[2];
  const u64 cntS = e[3] - baseS, cntE = e[4] - baseE, cntB = e[5] - baseB;
  if ((cntS == 0 || baseS >= cap) && (cntE == 0 || baseE >= cap) && (cntB == 0 || baseB >= dataCap)) return;   // (uniform in the workgroup)
  ItemOut o;
  run_item(G, dirty, carryIn, sRed, o);
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  u64 atS = baseS + (u32)__popcll(__ballot(o.st) & below), atE = baseE + (u32)__popcll(__ballot(o.en) & below);
  u64 atB = baseB + wave_incl_scan(o.bytes) - o.bytes;
  for (u32 w = 0; w < wave; w++) { atS += sRed[w]; atE += sRed[4 + w]; atB += sRed[8 + w]; }
  if (o.st && atS < cap) starts[atS] = grain_pos(G, o.i);
  if (o.en && atE < cap) ends[atE] = min(grain_pos(G, o.i), G.C);
  sLen[tid] = o.bytes; sAt[tid] = atB;
  __syncthreads();
  if (cntB == 0 || baseB >= dataCap) return;                                  // (uniform in the workgroup)
  const u32 L = min(64u, G.grain / 16), per = 64 / L, sub = lane % L;
  for (u32 r = 0; r < 64; r += per) {
    const u32 gi = wave * 64 + r + lane / L;
    const u32 len = sLen[gi];
    if (!len) continue;
    const u64 at = sAt[gi];
    const u8* const src = grain_src(G, (u64)blockIdx.x * kItem + gi);
    for (u32 x = sub * 16; x < len; x += L * 16) {
      const u64 p = at + x;
      if (x + 16 <= len && p + 16 <= dataCap && (((size_t)dData + p) & 15) == 0) {
        const u128_u v = *(const u128_u*)(src + x);
        *(uint4*)(dData + p) = make_uint4(v.a, v.b, v.c, v.d);
      } else {
        for (u32 k = 0; k < 16 && x + k < len; k++) if (p + k < dataCap) dData[p + k] = src[x + k];
      }
    }
  }
}

// =================================================================================================
namespace zra_eng {

namespace {
constexpr uint32_t kMinGrain = 64, kMaxGrain = 8192;                          // ZRA_HIP_SIGN_MIN_GRAIN, ZRA_HIP_SIGN_MAX_GRAIN
bool grain_ok(uint64_t g) { return g >= kMinGrain && g <= kMaxGrain && (g & (g - 1)) == 0; }
bool ranges_overlap(const void* p, uint64_t n, const void* q, uint64_t m) {
  return n && m && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}
// the grains of a pass: nj slots of gpf grains each, clipped to C
GrainArgs grain_args(const uint8_t* win, const uint8_t* flags, uint64_t fs, uint64_t C, uint32_t gpf, uint32_t grain, const FramePass& ps) {
  GrainArgs G;
  G.win = win; G.flags = flags; G.fs = fs; G.first = ps.first; G.C = C; G.total = (uint64_t)ps.nj * gpf; G.gpf = gpf; G.grain = grain;
  return G;
}

Status sign_run(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count,
                size_t stagingBytes, uint64_t* dSig, size_t sigCap, uint64_t info6[6]) {
  // ---- 1. arguments, 2. overlap
  if (!info6 || (!dArc && arcSize) || (!dSig && sigCap) || !grain_ok(grain)) return zerr(42);
  if (sigCap > (~(size_t)0) / 8 || ranges_overlap(dSig, 8 * (uint64_t)sigCap, dArc, arcSize)) return zerr(42);
  FramePasses F(E, ms);
  STCHK(F.start());
  // ---- 3. header: the statuses of ZraHipArchiveOpen. (The header's CRC-32 is not looked at: that is the verifier's job.)
  ArchiveView arc;
  STCHK(E.archive_view(dArc, arcSize, &arc));
  if (arc.fs == 0) return {kHeaderInvalid, 0};
  const uint64_t fs = arc.fs, U = arc.U;
  const uint64_t Fr = (U + fs - 1) / fs;                                      // (ra_header ties the table's frames to U when there is content)
  const uint32_t gpf = (uint32_t)((fs + grain - 1) / grain), stride = 1 + gpf;
  const uint64_t words = Fr * stride;
  // ---- 4. the range, as the verifier's
  uint64_t n;
  if (!frame_range(Fr, first, count, &n)) return {kOutOfBounds, 0};
  const uint64_t info[6] = {U, fs, grain, seed, Fr, words};
  for (int i = 0; i < 6; i++) info6[i] = info[i];
  if (!n) { stats[0] = Fr; return ok(); }
  // ---- 5. capacity: header arithmetic alone
  if (sigCap < words) return {kOutputTooSmall, 0};
  // ---- 6. scratch
  const PassPlan P = pass_plan(first, n, pass_slots(fs, stagingBytes));
  STCHK(F.open({(size_t)((uint64_t)P.nSlots * fs) + 64, 0, 0, kHdrBytes, 0, P.nSlots, P.nSlots}));
  uint8_t* const hdr = F.tables;
  // ---- passes: plain, one side. The spans of a pass are hashed in front of its decode, its grains behind it
  STCHK(F.begin(hdr, kHdrBytes));
  STCHK(F.run(P, FramePasses::Side{&arc, 0, F.win}, nullptr, nullptr, nullptr,
      [&](const FramePass& ps) {
        hipLaunchKernelGGL(zra_sig_spans_kernel, dim3((ps.nj + 63) / 64), dim3(256), 0, F.s, arc.table, arc.body, (u64)arc.bodyBytes, (u64)ps.first, ps.nj, (u64)seed, stride,
                           (u64*)dSig, (u64*)(hdr + kOffSpan), (const u64*)nullptr, (u8*)nullptr);
        return ok();
      },
      [&](const FramePass& ps, uint32_t) {
        const GrainArgs G = grain_args(F.win, nullptr, fs, U, gpf, grain, ps);
        hipLaunchKernelGGL(zra_sig_grains_kernel, dim3((unsigned)((G.total + 63) / 64)), dim3(256), 0, F.s, G, (u64)seed, stride, (u64*)dSig, (const u64*)nullptr, (u8*)nullptr);
        return ok();
      }));
  uint64_t spanBytes = 0;
  STCHK(F.finish(&spanBytes, hdr + kOffSpan, 8));
  const uint64_t full = first + n == Fr && U % fs ? n - 1 : n;                // frames of the range that hold frameSize bytes
  const uint64_t grains = full * gpf + (full < n ? (U % fs + grain - 1) / grain : 0);
  const uint64_t st8[8] = {Fr, n, grains, content_bytes(U, fs, first, n), spanBytes, P.passes, 0, 0};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  return ok();
}

Status sigdiff_run(Engine& E, uint64_t (&stats)[8], double* ms, const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB,
                   uint32_t mode, size_t stagingBytes, const PatchOut& out) {
  constexpr uint32_t kDecodeAll = 1u;                                         // ZRA_HIP_SIGDIFF_DECODE_ALL
  // ---- 1. arguments, the signature's own consistency among them, 2. overlap
  if (!out.args_ok() || !sig6 || (!dSigA && sigWords) || (!dB && sizeB) || (mode & ~kDecodeAll)) return zerr(42);
  const uint64_t C = sig6[0], fs = sig6[1], grain = sig6[2], seed = sig6[3], n = sig6[4], words = sig6[5];
  if (!grain_ok(grain) || fs == 0 || fs > 0xFFFFFFFFull) return zerr(42);
  const uint32_t gpf = (uint32_t)((fs + grain - 1) / grain), stride = 1 + gpf;
  if (n != C / fs + (C % fs != 0) || n > 0xFFFFFFFFull || words != n * stride || sigWords < words) return zerr(42);
  if (sigWords > (~(size_t)0) / 8 || out.data_overlaps(dB, sizeB) || out.data_overlaps(dSigA, 8 * (uint64_t)sigWords)) return zerr(42);
  FramePasses F(E, ms);
  STCHK(F.start());
  // ---- 3. B's header, 4. one frame size, 5. an update cannot shorten content
  ArchiveView B;
  STCHK(E.archive_view(dB, sizeB, &B));
  if (B.fs == 0) return {kHeaderInvalid, 0};
  if (B.fs != fs) return zerr(40);
  if (B.U < C) return zerr(40);
  const TailPlan tail = tail_plan(C, B.U, fs);                                 // B's frames that hold content behind C
  const uint64_t tailBytes = B.U - C;
  // ---- 6. scratch. Only B is decoded: the window is not halved, and the tail's passes are as long as the others
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const PassPlan P = pass_plan(0, n, passSlots), PT = pass_plan(tail.fT0, tail.nTail, passSlots);
  const uint64_t grainsMax = (uint64_t)P.nSlots * gpf;
  const size_t itemsMax = (size_t)((grainsMax + kItem - 1) / kItem);
  const size_t listCap = (size_t)std::min<uint64_t>(out.writeCap, (n * gpf + 1) / 2);   // (writes are at least one grain long and one grain apart)
  const size_t slotsMax = std::max<size_t>(P.nSlots, PT.nSlots);
  if (itemsMax > 0xFFFFFFFEull) return zerr(64);
  STCHK(F.open({(size_t)(slotsMax * fs) + 64, (size_t)P.nSlots + 64, (size_t)grainsMax + 64, kHdrBytes + (itemsMax + 1) * 24 + 64, listCap * 16 + 64, slotsMax, slotsMax}));
  uint8_t* const hdr = F.tables;
  uint64_t* const tot = (uint64_t*)(hdr + kOffTot);
  uint32_t* const carry = (uint32_t*)(hdr + kOffCarry);
  uint64_t* const tab = (uint64_t*)(hdr + kHdrBytes);
  uint64_t* const starts = F.list;
  uint64_t* const ends = starts + listCap;
  uint8_t* const dData = out.dData;
  const uint64_t dataCap = out.dataCap;
  // ---- passes over [0, C): flagged, one side
  uint64_t decoded = 0;
  STCHK(F.begin(hdr, kHdrBytes));
  STCHK(F.run(P, FramePasses::Side{&B, 0, F.win}, nullptr, (const uint32_t*)(hdr + kOffJobs), &decoded,
      [&](const FramePass& ps) {
        if (mode & kDecodeAll) HIPCHK_CLR(hipMemsetAsync(F.flags, 1, ps.nj, F.s));
        else
          hipLaunchKernelGGL(zra_sig_spans_kernel, dim3((ps.nj + 63) / 64), dim3(256), 0, F.s, B.table, B.body, (u64)B.bodyBytes, (u64)ps.first, ps.nj, (u64)seed, stride,
                             (u64*)nullptr, (u64*)nullptr, (const u64*)dSigA, F.flags);
        hipLaunchKernelGGL(zra_sig_jobs_kernel, dim3(1), dim3(1024), 0, F.s, F.flags, ps.nj, B.table, (u64)B.U, (u64)fs, (u64)ps.first, F.frameOff, F.outOff, F.expect,
                           (u32*)(hdr + kOffJobs));
        return ok();
      },
      [&](const FramePass& ps, uint32_t) {
        const GrainArgs G = grain_args(F.win, F.flags, fs, C, gpf, (uint32_t)grain, ps);
        const uint32_t items = (uint32_t)((G.total + kItem - 1) / kItem);
        uint32_t* const cIn = carry + ps.parity; uint32_t* const cOut = carry + (ps.parity ^ 1);
        hipLaunchKernelGGL(zra_sig_grains_kernel, dim3((unsigned)((G.total + 63) / 64)), dim3(256), 0, F.s, G, (u64)seed, stride, (u64*)nullptr, (const u64*)dSigA, F.dirty);
        hipLaunchKernelGGL(zra_sig_count_kernel, dim3(items), dim3(256), 0, F.s, G, F.dirty, cIn, tab, (u64*)(hdr + kOffGrains), cOut);
        diff_launch_scan(F.s, tab, items, tot + 3 * ps.parity, tot + 3 * (ps.parity ^ 1));
        if (listCap || dataCap)
          hipLaunchKernelGGL(zra_sig_fill_kernel, dim3(items), dim3(256), 0, F.s, G, F.dirty, cIn, tab, starts, ends, (u64)listCap, dData, (u64)dataCap);
        return ok();
      }));
  // ---- tail passes: B's frames from the one that holds C on, decoded on their own; their bytes behind C follow the dirty bytes
  const uint64_t* const totEnd = tot + 3 * (P.passes & 1);                     // {writes, ends, dirty bytes} behind the last pass over [0, C)
  STCHK(F.run(PT, FramePasses::Side{&B, 0, F.win}, nullptr, nullptr, nullptr, nullptr, [&](const FramePass& ps, uint32_t) {
      const TailRun r = tail_run(tail, ps);
      if (dataCap) diff_launch_tail(F.s, F.win + (r.pLo - ps.first * fs), r.len, totEnd + 2, r.pLo - C, dData, dataCap);
      return ok();
    }));
  // ---- the counts, then the lists, once
  uint64_t h16[kHdrBytes / 8] = {0};
  STCHK(F.finish(h16, hdr, kHdrBytes));
  const uint64_t* const t3 = h16 + kOffTot / 8 + 3 * (P.passes & 1);
  const uint64_t total = t3[0], dirtyBytes = t3[2];
  const bool open = ((const uint32_t*)((const uint8_t*)h16 + kOffCarry))[P.passes & 1] != 0;   // (runs) the last run ends at C
  if (t3[1] + (open ? 1 : 0) != total) return zerr(1);                        // (cannot happen: every write has one start and one end)
  STCHK(F.patch(out, starts, ends, total, t3[1], C, dirtyBytes, tailBytes));
  const uint64_t st8[8] = {n, n - decoded, decoded, tail.nTail, total, dirtyBytes, P.passes + PT.passes, h16[kOffGrains / 8]};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  return ok();
}
}  // namespace

Status Engine::sign_archive(const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count, size_t stagingBytes,
                            uint64_t* dSig, size_t sigCapWords, uint64_t info6[6]) {
  // (rule 5, OutputTooSmall, leaves the six words: they say how many words the signature needs)
  return entry_call(callStats_[kCallSign], &callMs_[kCallSign], {{info6, 6}}, true, [&] {
    return sign_run(*this, callStats_[kCallSign], &callMs_[kCallSign], dArc, arcSize, grain, seed, first, count, stagingBytes, dSig, sigCapWords, info6);
  });
}

Status Engine::diff_signature(const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
                              uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap,
                              uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize) {
  const PatchOut out{hOff, hSize, hDataOff, writeCap, nWrites, dData, dataCap, dataSize, appendOffset, appendSize};
  // (rule 8, OutputTooSmall, alone leaves what is needed in the four words)
  return entry_call(callStats_[kCallSigDiff], &callMs_[kCallSigDiff], {{nWrites, 1}, {dataSize, 1}, {appendOffset, 1}, {appendSize, 1}}, true, [&] {
    return sigdiff_run(*this, callStats_[kCallSigDiff], &callMs_[kCallSigDiff], sig6, dSigA, sigWords, dB, sizeB, mode, stagingBytes, out);
  });
}

}  // namespace zra_eng
