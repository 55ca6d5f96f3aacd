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
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
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
#include "zra_host.h"
#include "zra_dev.h"
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

// One workgroup: the decode-flagged slots of the pass, in order, become jobs 0 .. nDec - 1 of archive B; a job decodes its frame's
// seek-table span, whatever it says (the decoder refuses a span that runs backwards or leaves the body), into the frame's OWN slot,
// and has to regenerate that frame's share of B's content. *nJobs: the job count for the host.
extern "C" __global__ void __launch_bounds__(1024) zra_sig_jobs_kernel(const u8* flags, u32 nj, const u8* table, u64 U, u64 fs, u64 first, u64* frameOff, u64* outOff,
                                                                       u32* expect, u32* nJobs) {
  __shared__ u32 sS[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nj + 1023) / 1024;
  const u32 s0 = min(nj, tid * per), s1 = min(nj, s0 + per);
  u32 own = 0;
  for (u32 s = s0; s < s1; s++) own += flags[s] != 0;
  sS[tid] = own;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {                     // Hillis-Steele inclusive scan of the 1024 partials
    const u32 x = tid >= d ? sS[tid - d] : 0;
    __syncthreads();
    sS[tid] += x;
    __syncthreads();
  }
  u32 k = sS[tid] - own;
  for (u32 s = s0; s < s1; s++) {
    if (!flags[s]) continue;
    const u64 f = first + s;
    frameOff[2 * (size_t)k] = seek_entry(table, f); frameOff[2 * (size_t)k + 1] = seek_entry(table, f + 1);
    expect[k] = (u32)frame_expect(f, fs, U);
    outOff[k] = (u64)s * fs;
    k++;
  }
  if (tid == 1023) *nJobs = sS[1023];
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

struct SignImpl {
  static Status sign(Engine& E, const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count, size_t stagingBytes,
                     uint64_t* dSig, size_t sigCap, uint64_t info6[6]);
  static Status diff(Engine& E, const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
                     uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap, uint64_t* dataSize,
                     uint64_t* appendOffset, uint64_t* appendSize);
};

namespace {
constexpr uint32_t kMinGrain = 64, kMaxGrain = 8192;                          // ZRA_HIP_SIGN_MIN_GRAIN, ZRA_HIP_SIGN_MAX_GRAIN
bool grain_ok(uint64_t g) { return g >= kMinGrain && g <= kMaxGrain && (g & (g - 1)) == 0; }
bool ranges_overlap(const void* p, uint64_t n, const void* q, uint64_t m) {
  return n && m && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}
}  // namespace

Status Engine::sign_archive(const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count, size_t stagingBytes,
                            uint64_t* dSig, size_t sigCapWords, uint64_t info6[6]) {
  for (auto& v : gstats_) v = 0;
  signMs_ = 0;
  if (info6) for (int i = 0; i < 6; i++) info6[i] = 0;
  const Status st = SignImpl::sign(*this, dArc, arcSize, grain, seed, first, count, stagingBytes, dSig, sigCapWords, info6);
  if (st.zra) {
    signMs_ = 0;
    for (auto& v : gstats_) v = 0;
    if (st.zra != kOutputTooSmall && info6) for (int i = 0; i < 6; i++) info6[i] = 0;
  }
  return st;
}

Status SignImpl::sign(Engine& E, const uint8_t* dArc, size_t arcSize, uint32_t grain, uint64_t seed, uint64_t first, uint64_t count, size_t stagingBytes,
                      uint64_t* dSig, size_t sigCap, uint64_t info6[6]) {
  // ---- 1. arguments, 2. overlap
  if (!info6 || (!dArc && arcSize) || (!dSig && sigCap) || !grain_ok(grain)) return zerr(42);
  if (sigCap > (~(size_t)0) / 8 || ranges_overlap(dSig, 8 * (uint64_t)sigCap, dArc, arcSize)) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 3. header: the statuses of ZraHipArchiveOpen. (The header's CRC-32 is not looked at: that is the verifier's job.)
  ArchiveView arc;
  { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  if (arc.fs == 0) return {kHeaderInvalid, 0};
  const uint64_t fs = arc.fs, U = arc.U;
  const uint64_t F = (U + fs - 1) / fs;                                       // (ra_header ties the table's frames to U when there is content)
  const uint32_t gpf = (uint32_t)((fs + grain - 1) / grain), stride = 1 + gpf;
  const uint64_t words = F * stride;
  // ---- 4. the range, as the verifier's
  if (first > F || (count != ~0ull && count > F - first)) return {kOutOfBounds, 0};
  const uint64_t n = count == ~0ull ? F - first : count;
  const uint64_t info[6] = {U, fs, grain, seed, F, words};
  if (!n) { for (int i = 0; i < 6; i++) info6[i] = info[i]; E.gstats_[0] = F; return ok(); }
  // ---- 5. capacity: header arithmetic alone
  for (int i = 0; i < 6; i++) info6[i] = info[i];
  if (sigCap < words) return {kOutputTooSmall, 0};
  // ---- 6. scratch
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, n);
  const uint64_t passes = (n + passSlots - 1) / passSlots;
  if (!E.stage_.reserve((size_t)((uint64_t)nSlots * fs) + 64) || !E.sig_.tables.reserve(kHdrBytes) || !E.frameOff_.reserve(((size_t)nSlots + 1) * 16) ||
      !E.outOff_.reserve(((size_t)nSlots + 1) * 8) || !E.expect_.reserve(((size_t)nSlots + 1) * 4))
    return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>();
  uint8_t* const hdr = E.sig_.tables.as<uint8_t>();
  HIPCHK_CLR(hipMemsetAsync(hdr, 0, kHdrBytes, s));
  // ---- passes. evCall_[0] .. evCall_[1] spans the call's own launches between two decodes: the grains of a pass and the spans of the
  // next one follow each other on the stream. Taken behind a synchronisation of the stream.
  auto take_time = [&]() { E.signMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]); };
  HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
  for (uint64_t p = 0; p < passes; p++) {
    const uint64_t f0 = first + p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, n - p * passSlots);
    hipLaunchKernelGGL(zra_sig_spans_kernel, dim3((nj + 63) / 64), dim3(256), 0, s, arc.table, arc.body, (u64)arc.bodyBytes, (u64)f0, nj, (u64)seed, stride, (u64*)dSig,
                       (u64*)(hdr + kOffSpan), (const u64*)nullptr, (u8*)nullptr);
    search_launch_jobs(s, arc.table, fs, U, f0, nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    unsigned long long firstError;
    { Status st = E.staged_pass(arc, 0, nj, win, &firstError); if (st.zra) return st; }
    take_time();
    if (firstError != ~0ull) return zerr(reported_code(firstError));          // the lowest failing frame of the first failing pass
    GrainArgs G;
    G.win = win; G.flags = nullptr; G.fs = fs; G.first = f0; G.C = U; G.total = (uint64_t)nj * gpf; G.gpf = gpf; G.grain = grain;
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    hipLaunchKernelGGL(zra_sig_grains_kernel, dim3((unsigned)((G.total + 63) / 64)), dim3(256), 0, s, G, (u64)seed, stride, (u64*)dSig, (const u64*)nullptr, (u8*)nullptr);
  }
  uint64_t spanBytes = 0;
  HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
  HIPCHK_CLR(hipMemcpyAsync(&spanBytes, hdr + kOffSpan, 8, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const uint64_t end = first + n, bytes = std::min<uint64_t>(U, end * fs) - first * fs;
  const uint64_t full = end == F && U % fs ? n - 1 : n;                       // frames of the range that hold frameSize bytes
  const uint64_t grains = full * gpf + (full < n ? (U % fs + grain - 1) / grain : 0);
  const uint64_t st8[8] = {F, n, grains, bytes, spanBytes, passes, 0, 0};
  for (int i = 0; i < 8; i++) E.gstats_[i] = st8[i];
  return ok();
}

Status Engine::diff_signature(const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
                              uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap,
                              uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize) {
  for (auto& v : hstats_) v = 0;
  sigDiffMs_ = 0;
  for (uint64_t* w : {nWrites, dataSize, appendOffset, appendSize}) if (w) *w = 0;
  const Status st = SignImpl::diff(*this, sig6, dSigA, sigWords, dB, sizeB, mode, stagingBytes, hOff, hSize, hDataOff, writeCap, nWrites, dData, dataCap, dataSize,
                                   appendOffset, appendSize);
  if (st.zra) {
    sigDiffMs_ = 0;
    if (st.zra != kOutputTooSmall) for (uint64_t* w : {nWrites, dataSize, appendOffset, appendSize}) if (w) *w = 0;   // (rule 8 alone leaves what is needed)
  }
  return st;
}

Status SignImpl::diff(Engine& E, const uint64_t sig6[6], const uint64_t* dSigA, size_t sigWords, const uint8_t* dB, size_t sizeB, uint32_t mode, size_t stagingBytes,
                      uint64_t* hOff, uint64_t* hSize, uint64_t* hDataOff, size_t writeCap, uint64_t* nWrites, uint8_t* dData, size_t dataCap, uint64_t* dataSize,
                      uint64_t* appendOffset, uint64_t* appendSize) {
  constexpr uint32_t kDecodeAll = 1u;                                         // ZRA_HIP_SIGDIFF_DECODE_ALL
  // ---- 1. arguments, the signature's own consistency among them, 2. overlap
  if (!nWrites || !dataSize || !appendOffset || !appendSize || !sig6 || (!dSigA && sigWords) || (!dB && sizeB) || (writeCap && (!hOff || !hSize || !hDataOff)) ||
      (!dData && dataCap) || (mode & ~kDecodeAll))
    return zerr(42);
  const uint64_t C = sig6[0], fs = sig6[1], grain = sig6[2], seed = sig6[3], n = sig6[4], words = sig6[5];
  if (!grain_ok(grain) || fs == 0 || fs > 0xFFFFFFFFull) return zerr(42);
  const uint32_t gpf = (uint32_t)((fs + grain - 1) / grain), stride = 1 + gpf;
  if (n != C / fs + (C % fs != 0) || n > 0xFFFFFFFFull || words != n * stride || sigWords < words) return zerr(42);
  if (sigWords > (~(size_t)0) / 8 || ranges_overlap(dData, dataCap, dB, sizeB) || ranges_overlap(dData, dataCap, dSigA, 8 * (uint64_t)sigWords)) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 3. B's header, 4. one frame size, 5. an update cannot shorten content
  ArchiveView B;
  { Status st = E.archive_view(dB, sizeB, &B); if (st.zra) return st; }
  if (B.fs == 0) return {kHeaderInvalid, 0};
  if (B.fs != fs) return zerr(40);
  if (B.U < C) return zerr(40);
  const uint64_t tailBytes = B.U - C;
  const uint64_t fT0 = C / fs, nTail = tailBytes ? (B.U + fs - 1) / fs - fT0 : 0;   // B's frames that hold content behind C
  // ---- 6. scratch. Only B is decoded: the window is not halved
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, n), nTSlots = (uint32_t)std::min<uint64_t>(passSlots, nTail);
  const uint64_t passes = (n + passSlots - 1) / passSlots, tailPasses = (nTail + passSlots - 1) / passSlots;
  const uint64_t grainsMax = (uint64_t)nSlots * gpf;
  const size_t itemsMax = (size_t)((grainsMax + kItem - 1) / kItem);
  const size_t listCap = (size_t)std::min<uint64_t>(writeCap, (n * gpf + 1) / 2);   // (writes are at least one grain long and one grain apart)
  const size_t slotsMax = std::max<size_t>(nSlots, nTSlots);
  if (itemsMax > 0xFFFFFFFEull) return zerr(64);
  if (!E.stage_.reserve((size_t)(slotsMax * fs) + 64) || !E.sig_.flags.reserve((size_t)nSlots + 64) || !E.sig_.dirty.reserve((size_t)grainsMax + 64) ||
      !E.sig_.tables.reserve(kHdrBytes + (itemsMax + 1) * 24 + 64) || !E.sig_.list.reserve(listCap * 16 + 64) || !E.frameOff_.reserve((slotsMax + 1) * 16) ||
      !E.outOff_.reserve((slotsMax + 1) * 8) || !E.expect_.reserve((slotsMax + 1) * 4))
    return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>();
  uint8_t* const flags = E.sig_.flags.as<uint8_t>();
  uint8_t* const dirty = E.sig_.dirty.as<uint8_t>();
  uint8_t* const hdr = E.sig_.tables.as<uint8_t>();
  uint64_t* const tot = (uint64_t*)(hdr + kOffTot);
  uint32_t* const carry = (uint32_t*)(hdr + kOffCarry);
  uint64_t* const tab = (uint64_t*)(hdr + kHdrBytes);
  uint64_t* const starts = E.sig_.list.as<uint64_t>();
  uint64_t* const ends = starts + listCap;
  HIPCHK_CLR(hipMemsetAsync(hdr, 0, kHdrBytes, s));
  // ---- passes over [0, C). evCall_[0] .. evCall_[1] spans the call's own launches between two decodes, as in the diff
  uint64_t decoded = 0;
  auto take_time = [&]() { E.sigDiffMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]); };
  HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
  for (uint64_t p = 0; p < passes; p++) {
    const uint64_t first = p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, n - p * passSlots);
    if (mode & kDecodeAll) HIPCHK_CLR(hipMemsetAsync(flags, 1, nj, s));
    else
      hipLaunchKernelGGL(zra_sig_spans_kernel, dim3((nj + 63) / 64), dim3(256), 0, s, B.table, B.body, (u64)B.bodyBytes, (u64)first, nj, (u64)seed, stride, (u64*)nullptr,
                         (u64*)nullptr, (const u64*)dSigA, flags);
    hipLaunchKernelGGL(zra_sig_jobs_kernel, dim3(1), dim3(1024), 0, s, flags, nj, B.table, (u64)B.U, (u64)fs, (u64)first, E.frameOff_.as<uint64_t>(),
                       E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>(), (u32*)(hdr + kOffJobs));
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    uint32_t nDec = 0;
    HIPCHK_CLR(hipMemcpyAsync(&nDec, hdr + kOffJobs, 4, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    HIPCHK_CLR(hipGetLastError());
    take_time();
    if (nDec > nj) return zerr(1);                                            // (cannot happen)
    if (nDec) {
      unsigned long long errB;
      { Status st = E.staged_pass(B, 0, nDec, win, &errB); if (st.zra) return st; }
      if (errB != ~0ull) return zerr(reported_code(errB));                    // the lowest failing frame of the first failing pass
      decoded += nDec;
    }
    GrainArgs G;
    G.win = win; G.flags = flags; G.fs = fs; G.first = first; G.C = C; G.total = (uint64_t)nj * gpf; G.gpf = gpf; G.grain = (uint32_t)grain;
    const uint32_t items = (uint32_t)((G.total + kItem - 1) / kItem);
    uint32_t* const cIn = carry + (p & 1); uint32_t* const cOut = carry + ((p + 1) & 1);
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    hipLaunchKernelGGL(zra_sig_grains_kernel, dim3((unsigned)((G.total + 63) / 64)), dim3(256), 0, s, G, (u64)seed, stride, (u64*)nullptr, (const u64*)dSigA, dirty);
    hipLaunchKernelGGL(zra_sig_count_kernel, dim3(items), dim3(256), 0, s, G, dirty, cIn, tab, (u64*)(hdr + kOffGrains), cOut);
    diff_launch_scan(s, tab, items, tot + 3 * (p & 1), tot + 3 * ((p + 1) & 1));
    if (listCap || dataCap)
      hipLaunchKernelGGL(zra_sig_fill_kernel, dim3(items), dim3(256), 0, s, G, dirty, cIn, tab, starts, ends, (u64)listCap, dData, (u64)dataCap);
  }
  // ---- tail passes: B's frames from the one that holds C on, decoded on their own; their bytes behind C follow the dirty bytes
  const uint64_t* const totEnd = tot + 3 * (passes & 1);                       // {writes, ends, dirty bytes} behind the last pass over [0, C)
  for (uint64_t p = 0; p < tailPasses; p++) {
    const uint64_t first = fT0 + p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, nTail - p * passSlots);
    search_launch_jobs(s, B.table, fs, B.U, first, nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    unsigned long long errB;
    { Status st = E.staged_pass(B, 0, nj, win, &errB); if (st.zra) return st; }
    take_time();
    if (errB != ~0ull) return zerr(reported_code(errB));
    const uint64_t pLo = std::max<uint64_t>(C, first * fs), pHi = std::min<uint64_t>(B.U, (first + nj) * fs), len = pHi - pLo;
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    if (dataCap) diff_launch_tail(s, win + (pLo - first * fs), len, totEnd + 2, pLo - C, dData, dataCap);
  }
  // ---- the counts, then the lists, once
  uint64_t h16[kHdrBytes / 8] = {0};
  HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
  HIPCHK_CLR(hipMemcpyAsync(h16, hdr, kHdrBytes, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const uint64_t* const t3 = h16 + kOffTot / 8 + 3 * (passes & 1);
  const uint64_t total = t3[0], dirtyBytes = t3[2];
  const bool open = ((const uint32_t*)((const uint8_t*)h16 + kOffCarry))[passes & 1] != 0;   // (runs) the last run ends at C
  if (t3[1] + (open ? 1 : 0) != total) return zerr(1);                        // (cannot happen: every write has one start and one end)
  *nWrites = total; *dataSize = dirtyBytes + tailBytes; *appendOffset = dirtyBytes; *appendSize = tailBytes;
  if (total > writeCap || dirtyBytes + tailBytes > dataCap) return {kOutputTooSmall, 0};
  if (total) {
    std::vector<uint64_t> se(2 * (size_t)total);
    HIPCHK_CLR(hipMemcpyAsync(se.data(), starts, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    if (t3[1]) HIPCHK_CLR(hipMemcpyAsync(se.data() + total, ends, (size_t)t3[1] * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    if (open) se[2 * (size_t)total - 1] = C;
    uint64_t at = 0;
    for (size_t i = 0; i < total; i++) { hOff[i] = se[i]; hSize[i] = se[total + i] - se[i]; hDataOff[i] = at; at += hSize[i]; }
  }
  const uint64_t st8[8] = {n, n - decoded, decoded, nTail, total, dirtyBytes, passes + tailPasses, h16[kOffGrains / 8]};
  for (int i = 0; i < 8; i++) E.hstats_[i] = st8[i];
  return ok();
}

}  // namespace zra_eng
