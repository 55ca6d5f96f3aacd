// zra_amd — verification of a device-resident archive (zra_hip.h: ZraHipVerifyArchive): every faulty frame of a frame range reported,
// in frame order, without an output buffer.
//
//   1. the header comes to the host once (5 bytes per frame) and its CRC-32 is checked                  zra_fmt::header_hash
//   2. structure: a lane per frame walks the frame's table entries, frame header and block headers       zra_vfy_structure_kernel
//   3. content only: the structurally sound frames become decode jobs, in frame order                    zra_vfy_jobs_kernel
//   4. content only: passes of at most passSlots jobs are decoded whole into the staging window          Engine::staged_pass
//   5. the faults of the frames a pass covers are appended to the device fault list, in frame order      zra_vfy_collect_kernel
//   6. the fault count and the first faultCapacity entries come to the host, once
// Everything is indexed by i = frame - firstFrame: the tables cost 28 bytes per frame of the RANGE, not of the archive.
//
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
//  (a) jobs are ranks among the sound frames in frame order, so pass p decodes the sound frames of the index span
//      [passFirst[p], passFirst[p + 1]) and no others; the collection behind pass p covers exactly that span (the first one starts at 0,
//      the last one ends at the range's end), so the spans tile the range and the fault list is ascending across passes.
//  (b) a structurally faulty frame has no job: the collection takes its code from the structure stage alone.
//  (c) the collection launches are chained by a counter that ping-pongs between two words: launch k reads word k & 1 and its last
//      workgroup writes word (k + 1) & 1, so no workgroup reads a word another one of the same launch writes.
//  (d) nothing goes to the caller's fault array before the last pass is done: a call that fails midway writes nothing.
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include "zra_format.h"
#include <algorithm>
#include <vector>

using namespace zra_dev;

namespace {
constexpr u32 kNoJob = 0xFFFFFFFFu;       // jobOf: the frame is structurally faulty, nothing decodes it
constexpr u32 kCollectSpan = 1u << 16;    // frames of one collection launch: 256 workgroups of 256 lanes
constexpr u32 kStageStructure = 1u, kStageContent = 2u;   // ZRA_HIP_VERIFY_*

// ZraHipFrameFault (zra_hip.h), restated: the device list is copied to the caller's array as it is
struct Fault { u64 frame; u32 code; u32 stage; };

// The structure rules of one frame (the table in zra_hip.h, in its order); 0 = sound. Reads the frame's two table entries, its header
// and three bytes per block; every read lies inside [body + a, body + b), which the first rule puts inside the body.
__device__ __forceinline__ u32 structure_code(const u8* table, u32 nFrames, const u8* body, u64 bodyBytes, u64 fs, u64 total, u32 f) {
  const u64 a = seek_entry(table, f), b = seek_entry(table, (u64)f + 1);
  if (b < a || b > bodyBytes) return ZE_SRCSIZE_WRONG;
  if (f + 1 == nFrames && b != bodyBytes) return ZE_SRCSIZE_WRONG;
  const u64 n = b - a;
  if (n < 9 || n > 0xFFFFFFFFull) return ZE_SRCSIZE_WRONG;            // (the decoder's frame cursor is 32 bits wide)
  const u8* const p = body + a;
  const u32 fhd = p[4], did = fhd & 3, ss = (fhd >> 5) & 1, fcs = fhd >> 6;
  const u32 didSize = did == 3 ? 4u : did, fcsSize = fcs == 0 ? ss : fcs == 1 ? 2u : fcs == 2 ? 4u : 8u;
  const u32 hs = 5 + !ss + didSize + fcsSize;
  if (n < hs + 3) return ZE_SRCSIZE_WRONG;
  if (ld32(p) != 0xFD2FB528u) return ZE_PREFIX_UNKNOWN;
  if (fhd & 8) return ZE_FRAMEPARAM_UNSUPPORTED;
  if (!ss && 10 + (p[5] >> 3) > 31) return ZE_WINDOW_TOO_LARGE;
  const u8* q = p + 5 + !ss;
  const u32 dict = did == 0 ? 0u : did == 1 ? (u32)q[0] : did == 2 ? ld16(q) : ld32(q);
  if (dict) return ZE_DICT_WRONG;
  q += didSize;
  if (fcsSize) {
    const u64 v = fcsSize == 1 ? (u64)q[0] : fcsSize == 2 ? (u64)ld16(q) + 256 : fcsSize == 4 ? (u64)ld32(q) : ld64(q);
    const u64 expect = frame_expect(f, fs, total);
    if (v > expect) return ZE_DSTSIZE_TOOSMALL;
    if (v < expect) return ZE_CORRUPTION;
  }
  u64 pos = hs;
  for (;;) {                                                          // (ends: every step consumes at least the 3 header bytes)
    if (n - pos < 3) return ZE_SRCSIZE_WRONG;
    const u32 bh = ld24(p + pos);
    pos += 3;
    const u32 type = (bh >> 1) & 3, payload = type == 1 ? 1u : bh >> 3;
    if (type == 3) return ZE_CORRUPTION;
    if (payload > n - pos) return ZE_SRCSIZE_WRONG;
    pos += payload;
    if (bh & 1) break;
  }
  if (fhd & 4) pos += 4;
  return pos == n ? 0u : (u32)ZE_SRCSIZE_WRONG;
}

// the fault of range index i, as code | stage << 8; 0: none. status == nullptr: structure codes alone.
__device__ __forceinline__ u32 fault_word(const u32* sstat, const u32* jobOf, const u32* status, u32 jobBase, u32 nJobs, u32 i) {
  const u32 s = sstat[i];
  if (s) return s | (kStageStructure << 8);
  if (!status) return 0;
  const u32 j = jobOf[i] - jobBase;                                   // (condition (a): inside the pass; anything else reads nothing)
  if (j >= nJobs) return 0;
  u32 c = status[j] & 0xFF;
  c = (u32)zra_eng::reported_code(c);
  return c ? c | (kStageContent << 8) : 0u;
}
}  // namespace

// Lane per frame of the range: each frame is one short dependent walk. sstat[i] = the code of frame first + i, 0 if it is sound.
extern "C" __global__ void __launch_bounds__(256) zra_vfy_structure_kernel(const u8* table, u32 nFrames, const u8* body, u64 bodyBytes, u64 fs, u64 total,
                                                                         u32 first, u32 count, u32* sstat) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  sstat[i] = structure_code(table, nFrames, body, bodyBytes, fs, total, first + i);
}

// One workgroup walks the range, 1024 frames at a time: a sound frame's job is its rank among the sound frames (zra_joblist.h:
// block_rank, emit_job); the job gets the frame's compressed span and the size it has to regenerate.
// passFirst[p] = range index of the first frame of pass p (jobs [p * passSlots, ...)), passFirst[passes] = count.
// outOff[s] = where slot s of the staging window starts: every pass uses the same nSlots entries. totals[0] = jobs.
extern "C" __global__ void __launch_bounds__(1024) zra_vfy_jobs_kernel(const u32* sstat, u32 first, u32 count, const u8* table, u64 fs, u64 total, u32 passSlots,
                                                                     u32 nSlots, u32* jobOf, u64* frameOff, u64* outOff, u32* expect, u32* passFirst, u32* totals) {
  for (u32 s = threadIdx.x; s < nSlots; s += 1024) outOff[s] = (u64)s * fs;
  u32 jobBase = 0;
  for (u32 base = 0; base < count; base += 1024) {
    const u32 i = base + threadIdx.x;
    const bool in = i < count, p[1] = {in && sstat[i] == 0};
    u32 rank[1], all[1];
    block_rank<1>(p, rank, all);
    const u32 job = jobBase + rank[0];
    if (in) jobOf[i] = p[0] ? job : kNoJob;
    if (p[0]) {
      emit_job(table, (u64)first + i, fs, total, job, 0, frameOff, nullptr, expect);
      if (job % passSlots == 0) passFirst[job / passSlots] = i;
    }
    jobBase += all[0];
  }
  if (threadIdx.x == 0) { passFirst[(jobBase + passSlots - 1) / passSlots] = count; totals[0] = jobBase; }
}

// Ordered compaction of the faults of range indices [i0, i0 + n) into the fault list, behind the *cntIn entries counted so far.
// Workgroup b takes indices i0 + 256 b + tid. Its base is the number of faults in front of it in this launch: every wave counts the
// fault words of the indices before the workgroup's own with ballots (at most kCollectSpan words, resident in L2; no workgroup waits
// for another one), the four wave counts are added up; inside the workgroup a fault's place is its wave's offset plus the prefix count
// of its ballot. Entries beyond `cap` are counted, not written. The last workgroup hands the new count on (condition (c)).
// produced != nullptr: the bytes the pass's jobs regenerated are summed into *bytes (a wave sum, one atomic per wave).
extern "C" __global__ void __launch_bounds__(256) zra_vfy_collect_kernel(const u32* sstat, const u32* jobOf, const u32* status, const u32* produced, u32 jobBase,
                                                                       u32 nJobs, u32 i0, u32 n, u64 first, Fault* faults, u64 cap, const u32* cntIn,
                                                                       u32* cntOut, unsigned long long* bytes) {
  __shared__ u32 sPrior[4], sOwn[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u32 prior = 0;
  for (u32 k = tid; k < blockIdx.x * 256; k += 256)                    // (the same trip count for every lane)
    prior += (u32)__popcll(__ballot(fault_word(sstat, jobOf, status, jobBase, nJobs, i0 + k) != 0));
  const u32 k = blockIdx.x * 256 + tid;
  const bool in = k < n;
  const u32 w = in ? fault_word(sstat, jobOf, status, jobBase, nJobs, i0 + k) : 0u;
  const u64 m = __ballot(w != 0);
  if (lane == 0) { sPrior[wave] = prior; sOwn[wave] = (u32)__popcll(m); }
  if (produced) {
    const u32 j = in && sstat[i0 + k] == 0 ? jobOf[i0 + k] - jobBase : kNoJob;
    u64 got = j < nJobs ? (u64)produced[j] : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) got += __shfl_xor(got, d, 64);
    if (lane == 0 && got) atomicAdd(bytes, (unsigned long long)got);
  }
  __syncthreads();
  u32 at = *cntIn, own = 0;
  for (u32 x = 0; x < 4; x++) { at += sPrior[x]; own += sOwn[x]; at += x < wave ? sOwn[x] : 0u; }
  at += (u32)__popcll(m & ((1ull << lane) - 1));
  if (w && at < cap) { Fault e; e.frame = first + i0 + k; e.code = w & 0xFF; e.stage = w >> 8; faults[at] = e; }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *cntOut = *cntIn + sPrior[0] + sPrior[1] + sPrior[2] + sPrior[3] + own;
}

// =================================================================================================
namespace zra_eng {

struct VerifyImpl {
  static Status run(Engine& E, uint64_t (&stats)[8], const uint8_t* dArc, size_t arcSize, uint32_t mode, uint64_t first, uint64_t count, size_t stagingBytes,
                    void* hFaults, size_t faultCap, size_t* nFaults);
};

Status Engine::verify_archive(const uint8_t* dArc, size_t arcSize, uint32_t mode, uint64_t first, uint64_t count, size_t stagingBytes,
                              void* hFaults, size_t faultCap, size_t* nFaults) {
  static_assert(sizeof(size_t) == sizeof(uint64_t), "the fault count is one output word");
  // (the verify has no milliseconds, and no status that keeps the count: faultCapacity cuts the list, it refuses nothing)
  return entry_call(callStats_[kCallVerify], nullptr, {{reinterpret_cast<uint64_t*>(nFaults), 1}}, false, [&] {
    return VerifyImpl::run(*this, callStats_[kCallVerify], dArc, arcSize, mode, first, count, stagingBytes, hFaults, faultCap, nFaults);
  });
}

Status VerifyImpl::run(Engine& E, uint64_t (&stats)[8], const uint8_t* dArc, size_t arcSize, uint32_t mode, uint64_t first, uint64_t count, size_t stagingBytes,
                       void* hFaults, size_t faultCap, size_t* nFaults) {
  // ---- 1. arguments
  if (!nFaults || (!dArc && arcSize) || (!hFaults && faultCap) || !mode || (mode & ~(kStageStructure | kStageContent))) return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen
  ArchiveView arc;
  { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  // ---- 3. the CRC-32 over the header as it lies on the device (ra_header: 38 <= arc.h.size <= arcSize)
  {
    std::vector<uint8_t> hdr(arc.h.size);
    HIPCHK_CLR(hipMemcpyAsync(hdr.data(), dArc, arc.h.size, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    if (zra_fmt::header_hash(hdr.data(), hdr.data() + zra_fmt::kFixedSize) != zra_fmt::rd32(hdr.data() + 14)) return {kHeaderInvalid, 0};
  }
  // ---- 4. the range
  const uint32_t F = arc.frames;
  const uint64_t fs = arc.fs, U = arc.U;
  uint64_t n64;
  if (!frame_range(F, first, count, &n64)) return {kOutOfBounds, 0};
  const uint32_t f0 = (uint32_t)first, n = (uint32_t)n64;
  if (!n) { stats[0] = F; return ok(); }
  // ---- 5. scratch
  const bool content = (mode & kStageContent) != 0;
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = std::min(passSlots, n);
  const size_t passesMax = (size_t)n / passSlots + 2;
  const size_t listCap = (size_t)std::min<uint64_t>(faultCap, n);
  const size_t planWords = 2 * (size_t)n + 16 + passesMax + 1;            // sstat[n] | jobOf[n] | totals[16] | passFirst[passes + 1]
  if (!E.vfy_.plan.reserve(planWords * 4 + 64) || !E.vfy_.faults.reserve(listCap * sizeof(Fault) + 64)) return zerr(64);
  if (content && (!E.frameOff_.reserve(((size_t)n + 1) * 16) || !E.outOff_.reserve(((size_t)nSlots + 1) * 8) || !E.expect_.reserve(((size_t)n + 1) * 4)))
    return zerr(64);
  uint32_t* sstat = E.vfy_.plan.as<uint32_t>(), *jobOf = sstat + n, *totals = jobOf + n, *passFirst = totals + 16;
  uint32_t* cnt = totals + 4;                                              // the ping-pong fault count (condition (c))
  unsigned long long* bytes = (unsigned long long*)(totals + 8);
  Fault* faults = (Fault*)E.vfy_.faults.p;
  HIPCHK_CLR(hipMemsetAsync(totals, 0, 64, s));
  // ---- structure
  hipLaunchKernelGGL(zra_vfy_structure_kernel, dim3((n + 255) / 256), dim3(256), 0, s, arc.table, F, arc.body, (u64)arc.bodyBytes, (u64)fs, (u64)U, f0, n, sstat);
  uint32_t launches = 0;
  // faults of range indices [i0, i1) -> the list; status: the status words of the pass that decoded the sound frames among them
  auto collect = [&](uint32_t i0, uint32_t i1, const uint32_t* status, const uint32_t* produced, uint32_t jobBase, uint32_t nJobs) {
    for (uint32_t a = i0; a < i1;) {
      const uint32_t m = std::min(kCollectSpan, i1 - a);
      hipLaunchKernelGGL(zra_vfy_collect_kernel, dim3((m + 255) / 256), dim3(256), 0, s, sstat, content ? jobOf : nullptr, status, produced, jobBase, nJobs, a, m,
                         (u64)f0, faults, (u64)listCap, cnt + (launches & 1), cnt + ((launches + 1) & 1), bytes);
      launches++; a += m;
    }
  };
  uint32_t jobs = 0, passes = 0;
  if (!content) collect(0, n, nullptr, nullptr, 0, 0);
  else {
    // ---- content: jobs, then passes of decode + collection
    hipLaunchKernelGGL(zra_vfy_jobs_kernel, dim3(1), dim3(1024), 0, s, sstat, f0, n, arc.table, (u64)fs, (u64)U, passSlots, nSlots, jobOf, E.frameOff_.as<uint64_t>(),
                       E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>(), passFirst, totals);
    HIPCHK_CLR(hipMemcpyAsync(&jobs, totals, 4, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    HIPCHK_CLR(hipGetLastError());
    passes = (jobs + passSlots - 1) / passSlots;
    if (!passes) collect(0, n, nullptr, nullptr, 0, 0);
    else {
      std::vector<uint32_t> pf(passes + 1);
      HIPCHK_CLR(hipMemcpyAsync(pf.data(), passFirst, ((size_t)passes + 1) * 4, hipMemcpyDeviceToHost, s));
      HIPCHK_CLR(hipStreamSynchronize(s));
      pf[0] = 0;                                                           // (faulty frames in front of the first sound one)
      if (!E.stage_.reserve((size_t)std::min(jobs, passSlots) * fs + 64)) return zerr(64);
      for (uint32_t p = 0; p < passes; p++) {
        const uint32_t j0 = p * passSlots, nj = std::min(passSlots, jobs - j0);
        unsigned long long firstError;                                     // (the pass's reduction: not what a scrubber wants)
        Status st = E.staged_pass(arc, j0, nj, E.stage_.as<uint8_t>(), &firstError);
        if (st.zra) return st;
        collect(pf[p], pf[p + 1], E.status_.as<uint32_t>(), E.produced_.as<uint32_t>(), j0, nj);
      }
    }
  }
  // ---- the count, then the list, once
  uint32_t nf = 0; unsigned long long regenerated = 0;
  HIPCHK_CLR(hipMemcpyAsync(&nf, cnt + (launches & 1), 4, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipMemcpyAsync(&regenerated, bytes, 8, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  const size_t nOut = std::min<size_t>(nf, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hFaults, faults, nOut * sizeof(Fault), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  *nFaults = nf;
  const uint64_t structural = content ? (uint64_t)n - jobs : nf;
  const uint64_t st8[8] = {F, n, structural, nf - structural, jobs, regenerated, passes, 0};
  for (int i = 0; i < 8; i++) stats[i] = st8[i];
  return ok();
}

}  // namespace zra_eng
