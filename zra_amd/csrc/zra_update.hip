// zra_amd — update of a device-resident archive (zra_hip.h: ZraHipUpdateArchive): byte ranges of the content overwritten, bytes
// appended, without decoding or encoding the frames that do not change.
//
// Every frame is an independent zstd frame and the seek table alone ties them together, so an update
//   1. plans, per frame, whether new bytes land in it (touched), how many, and its staging slot        zra_upd_mark / zra_upd_plan
//   2. decodes the touched frames that keep some old bytes, whole and with their checksum              Engine::decode_jobs
//      (through an archive handle: those of them that are resident are copied out of its arena instead   zra_upd_stage_cached)
//   3. copies the new bytes over them in the staging buffer                                            zra_upd_patch
//   4. encodes the staged frames like ZraHipCompressBuffer encodes frames of that content              Engine::compress_frames
//   5. sizes every frame (new size if touched, old table difference if not), scans, writes the table   zra_upd_sizes / _scan / _offsets
//   6. copies every frame to its new place: the bandwidth step                                         zra_upd_gather
// Steps 2-4 run in passes over the slots of the engine's staging window (pass_slots); the encoded frames stay packed in scratch until step 6.
//
// Ordering conditions (all launches on the engine's stream, decode_jobs and compress_frames return synchronised):
//  (a) slots are ranks among the touched frames in frame order: only the archive's last frame can be short and it is the last slot of
//      the last pass (what compress_frames expects of its input), decode jobs are in frame order (the first failing job is the
//      lowest failing frame), and the packed encoded frames are in frame order (one scan gives their places).
//  (b) the patch kernel of a pass runs behind the pass's decode and before its encode: new bytes win over decoded ones.
//  (c) nothing is written to dOut before every size is known and every check has passed: a refused update leaves dOut alone.
// Through an archive handle (UpdCacheView) two more:
//  (d) a pass's copies out of the arena write other staging slots than its decode jobs and run before its patch kernel; copies and
//      jobs are each ranked in frame order, so (a) holds for the jobs: the first failing job is the lowest failing DECODED frame.
//  (e) the arena is only read before the last check; the new bytes are laid over the resident frames beside the gather: a REFUSED
//      update changes nothing (a HIP runtime error behind that point leaves dOut and those frames undefined).
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_joblist.h"
#include "zra_format.h"
#include <algorithm>
#include <vector>

using namespace zra_dev;

namespace {
constexpr u32 kNone = 0xFFFFFFFFu;        // slotOf: the frame is not touched
constexpr u32 kGatherChunk = 32u << 10;   // output bytes one wave of the gather copies per step
constexpr u32 kGatherGrid = 2048;         // workgroups of the gather at most (4 waves each; 8 per CU on 256 CUs)

// one wave copies n bytes: 16-byte loads aligned on the source, four in flight per lane; the stores fall as they may
// (zra_gather_frames_kernel's choice)
__device__ __forceinline__ void copy_span(u8* dst, const u8* src, u64 n, u32 lane) {
  const u32 head = (u32)min<u64>((16u - ((uintptr_t)src & 15u)) & 15u, n);
  if (lane < head) dst[lane] = src[lane];
  const u32 n16 = (u32)((n - head) >> 4);
  const uint4* s4 = (const uint4*)(src + head);
  u8* d16 = dst + head;
  u32 i = lane;
  for (; i + 192 < n16; i += 256) {
    const uint4 v0 = s4[i], v1 = s4[i + 64], v2 = s4[i + 128], v3 = s4[i + 192];
    st128(d16 + 16 * (size_t)i, v0.x, v0.y, v0.z, v0.w); st128(d16 + 16 * (size_t)(i + 64), v1.x, v1.y, v1.z, v1.w);
    st128(d16 + 16 * (size_t)(i + 128), v2.x, v2.y, v2.z, v2.w); st128(d16 + 16 * (size_t)(i + 192), v3.x, v3.y, v3.z, v3.w);
  }
  for (; i < n16; i += 64) { const uint4 v = s4[i]; st128(d16 + 16 * (size_t)i, v.x, v.y, v.z, v.w); }
  for (u64 k = head + ((u64)n16 << 4) + lane; k < n; k += 64) dst[k] = src[k];
}
}  // namespace

// Thread per slice: the bytes the slice replaces are counted into its frame. Writes do not overlap and the append lies behind all
// of them, so cover[f] is exactly the number of bytes of frame f that the update supplies.
extern "C" __global__ void __launch_bounds__(256) zra_upd_mark_kernel(const u64* q, u32 nq, u64 nSlices, u64 fs, u32* cover) {
  const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
  if (s >= nSlices) return;
  const Slice c = slice_of(q, nq, s, fs);
  atomicAdd(&cover[c.frame], c.len);
}

// One workgroup walks the frames of the result, 1024 at a time. A frame is touched when cover != 0; its staging slot is its rank among
// the touched frames (zra_joblist.h, block_rank: four predicates ranked at once, the running bases kept here). A touched frame that
// keeps old bytes (cover < its new length) gets a decode job, ranked the same way (emit_job): compressed span from the old seek table,
// destination = its slot of the pass, expected size = its old length.
// passJob[p] = jobs in front of pass p (slots [p * passSlots, ...)), passJob[passes] = all.
// An untouched frame is carried over by its table entries: they must not run backwards nor end beyond the body (flag).
// With a handle's cache (cacheSlotOf != nullptr, readable for nNew frames) a frame that keeps old bytes and is resident gets no job but
// a copy entry {staging slot, arena slot, old length, frame}, ranked in frame order like the jobs, passCopy[] like passJob[]; and
// every touched resident frame is counted: its arena slot is to hold the new content.
// totals = {touched, jobs, flag, copies, touched resident frames}.
extern "C" __global__ void __launch_bounds__(1024) zra_upd_plan_kernel(const u32* cover, u32 nNew, u32 nOld, const u8* table, u64 bodyBytes, u64 fs,
                                                                    u64 oldTotal, u64 newTotal, u32 passSlots, const u32* cacheSlotOf, u32* slotOf,
                                                                    u64* frameOff, u64* outOff, u32* expect, u32* passJob, u32* copies,
                                                                    u32* passCopy, u32* totals) {
  __shared__ u32 sFlag;
  const u32 tid = threadIdx.x;
  if (tid == 0) sFlag = 0;
  u32 slotBase = 0, jobBase = 0, copyBase = 0, fresh = 0;
  for (u32 base = 0; base < nNew; base += 1024) {
    const u32 f = base + tid;
    const bool in = f < nNew;
    const u32 c = in ? cover[f] : 0u;
    const u64 o = (u64)f * fs;
    const u32 newLen = in ? (u32)min<u64>(fs, newTotal - o) : 0u;
    const bool touched = c != 0;
    const u32 cs = touched && cacheSlotOf ? cacheSlotOf[f] : kNone;
    const bool keeps = touched && c != newLen, cpy = keeps && cs != kNone, dec = keeps && !cpy;
    const bool p[4] = {touched, dec, cpy, cs != kNone};
    u32 rank[4], total[4];
    block_rank<4>(p, rank, total);
    const u32 slot = slotBase + rank[0], job = jobBase + rank[1], copy = copyBase + rank[2];
    if (in) slotOf[f] = touched ? slot : kNone;
    if (touched && slot % passSlots == 0) { passJob[slot / passSlots] = job; passCopy[slot / passSlots] = copy; }
    if (cpy) {
      u32* e = copies + 4 * (size_t)copy;
      e[0] = slot; e[1] = cs; e[2] = (u32)min<u64>(fs, oldTotal - o); e[3] = f;
    }
    // (dec implies f < nOld: a frame behind the old content is supplied whole by the append)
    if (dec) emit_job(table, f, fs, oldTotal, job, slot % passSlots, frameOff, outOff, expect);
    if (in && !touched && f < nOld) {
      const u64 a = seek_entry(table, f), b = seek_entry(table, (u64)f + 1);
      if (b < a || b > bodyBytes) atomicOr(&sFlag, 1u);
    }
    slotBase += total[0]; jobBase += total[1]; copyBase += total[2]; fresh += total[3];
  }
  __syncthreads();                                                    // (sFlag)
  if (tid == 0) {
    passJob[(slotBase + passSlots - 1) / passSlots] = jobBase; passCopy[(slotBase + passSlots - 1) / passSlots] = copyBase;
    totals[0] = slotBase; totals[1] = jobBase; totals[2] = sFlag; totals[3] = copyBase; totals[4] = fresh;
  }
}

// The cache's bandwidth kernel: copy entries [0, n) of a pass (zra_upd_plan_kernel), a wave per kGatherChunk bytes of a frame (one wave
// for a frame of up to 32 KiB, 64 for one of 2 MiB), a capped grid striding over them. The frame's old length goes from its arena slot
// to its staging slot of the pass that starts at slot s0; both sides are fs-strided, so with a frame size that is no multiple of 16
// they are not co-aligned (copy_span: loads aligned, stores as they fall).
extern "C" __global__ void __launch_bounds__(256) zra_upd_stage_cached_kernel(const u32* copies, u32 n, u32 s0, u64 fs, const u8* arena, u8* stage) {
  const u32 lane = threadIdx.x & 63;
  const u32 perFrame = (u32)((fs + kGatherChunk - 1) / kGatherChunk);
  const u64 nWork = (u64)n * perFrame;
  for (u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); w < nWork; w += (u64)gridDim.x * 4) {
    const u32 k = (u32)(w / perFrame);
    const u64 x = (w - (u64)k * perFrame) * kGatherChunk;
    const u32* e = copies + 4 * (size_t)k;
    const u32 slot = e[0], cs = e[1], len = e[2];
    if (x >= len) continue;
    copy_span(stage + (u64)(slot - s0) * fs + x, arena + (u64)cs * fs + x, min<u64>(kGatherChunk, len - x), lane);
  }
}

// Wave per slice, for the slices whose frame has a slot in the pass [s0, s0 + n): the new bytes go over the staged frame. Tuples below
// nData take their bytes from data, the one behind them (the append) from app.
extern "C" __global__ void __launch_bounds__(256) zra_upd_patch_kernel(const u64* q, u32 nq, u32 nData, u64 nSlices, u64 fs, const u32* slotOf, u32 s0, u32 n,
                                                                     const u8* data, const u8* app, u8* stage) {
  const int lane = (int)(threadIdx.x & 63);
  for (u64 s = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); s < nSlices; s += (u64)gridDim.x * 4) {
    const Slice c = slice_of(q, nq, s, fs);
    const u32 slot = slotOf[c.frame];
    if (slot < s0 || slot - s0 >= n) continue;
    copy_slice(stage + (u64)(slot - s0) * fs + c.inFrame, (c.tuple < nData ? data : app) + c.user, c.len, lane);
  }
}

namespace {
// compressed size of frame f in the result, and that size again if it was newly encoded (0 if carried over); f == nNew: the end entry
__device__ __forceinline__ void upd_frame_size(u32 f, u32 nNew, const u32* slotOf, const u64* encSizes, const u8* table, u64* sz, u64* tsz) {
  *sz = 0; *tsz = 0;
  if (f >= nNew) return;
  const u32 slot = slotOf[f];
  if (slot != kNone) { *sz = *tsz = encSizes[slot]; return; }
  *sz = seek_entry(table, (u64)f + 1) - seek_entry(table, f);               // (not backwards: the plan kernel has checked the untouched frames)
}
}  // namespace

// Workgroup b sums the sizes of frames [1024 b, 1024 b + 1024): sums[2b] all, sums[2b + 1] the newly encoded ones.
extern "C" __global__ void __launch_bounds__(1024) zra_upd_sizes_kernel(u32 nNew, const u32* slotOf, const u64* encSizes, const u8* table, u64* sums) {
  u64 v[2], tot[2];
  upd_frame_size(blockIdx.x * 1024 + threadIdx.x, nNew, slotOf, encSizes, table, &v[0], &v[1]);
  block_excl_scan<2>(v, tot);
  if (threadIdx.x == 0) { sums[2 * (size_t)blockIdx.x] = tot[0]; sums[2 * (size_t)blockIdx.x + 1] = tot[1]; }
}

// One workgroup: the workgroup sums become exclusive prefixes in place; sums[2 nBlocks], [2 nBlocks + 1] = the totals
// (zra_joblist.h, scan_in_place).
extern "C" __global__ void __launch_bounds__(1024) zra_upd_scan_kernel(u64* sums, u32 nBlocks) { scan_in_place<2>(sums, nBlocks, nullptr, nullptr); }

// Thread per frame (and one for the end entry): newOff[f] = where the frame starts in the new body, its 5-byte entry of the new seek
// table, and disp[f] = the address of its compressed bytes minus newOff[f] — in the old body for a frame carried over, in the packed
// buffer for a newly encoded one. Neighbours that stay neighbours have the same displacement: the gather copies them as one span.
extern "C" __global__ void __launch_bounds__(1024) zra_upd_offsets_kernel(u32 nNew, const u32* slotOf, const u64* encSizes, const u8* table, const u64* sums,
                                                                       const u8* oldBody, const u8* packed, u64* newOff, u64* disp, u8* entries) {
  const u32 f = blockIdx.x * 1024 + threadIdx.x;
  u64 v[2], tot[2];
  upd_frame_size(f, nNew, slotOf, encSizes, table, &v[0], &v[1]);
  const bool enc = v[1] != 0 || (f < nNew && slotOf[f] != kNone);
  block_excl_scan<2>(v, tot);
  if (f > nNew) return;
  const u64 off = sums[2 * (size_t)blockIdx.x] + v[0], toff = sums[2 * (size_t)blockIdx.x + 1] + v[1];
  newOff[f] = off;
  u8* e = entries + (size_t)f * 5;
  e[0] = (u8)off; e[1] = (u8)(off >> 8); e[2] = (u8)(off >> 16); e[3] = (u8)(off >> 24); e[4] = (u8)(off >> 32);
  if (f == nNew) disp[f] = ~0ull;
  else disp[f] = (enc ? (u64)(uintptr_t)packed + toff : (u64)(uintptr_t)oldBody + seek_entry(table, f)) - off;
}

// The bandwidth kernel. The new body is cut into chunks of kGatherChunk bytes, a capped grid strides over them, one wave per chunk.
// The wave finds the frame its chunk starts in by binary search over newOff, then copies span after span: a span ends where the
// displacement changes (ballot over the next 64 frames at a time) or the chunk does (copy_span).
extern "C" __global__ void __launch_bounds__(256) zra_upd_gather_kernel(const u64* newOff, const u64* disp, u32 nNew, u64 total, u8* body) {
  const u32 lane = threadIdx.x & 63;
  const u64 nChunks = (total + kGatherChunk - 1) / kGatherChunk;
  for (u64 c = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); c < nChunks; c += (u64)gridDim.x * 4) {
    u64 x = c * kGatherChunk;
    const u64 x1 = min<u64>(x + kGatherChunk, total);
    u32 lo = 0, hi = nNew - 1;                                        // the last frame that starts at or before x
    while (lo < hi) {
      const u32 mid = lo + (hi - lo + 1) / 2;
      if (newOff[mid] <= x) lo = mid; else hi = mid - 1;
    }
    u32 f = lo;
    while (x < x1 && f < nNew) {
      const u64 d = disp[f];
      u32 g = f + 1;
      for (;;) {                                                      // (ends: disp[nNew] is no frame's displacement)
        const u32 i = g + lane;
        const bool brk = i > nNew || newOff[min(i, nNew)] >= x1 || disp[min(i, nNew)] != d;
        const u64 m = __ballot(brk);
        if (m) { g += (u32)__builtin_ctzll(m); break; }
        g += 64;
      }
      g = min(g, nNew);
      const u64 end = min<u64>(x1, newOff[g]);
      if (end > x) {
        copy_span(body + x, (const u8*)(uintptr_t)(d + x), end - x, lane);
        x = end;
      }
      f = g;
    }
  }
}

// =================================================================================================
namespace zra_eng {

// the stage-from-cache launch of a pass: the update's own, and the one a range scan through a handle makes (zra_engine.h, zra_scan.h)
void upd_launch_stage_cached(hipStream_t s, const uint32_t* copies, uint32_t n, uint32_t s0, uint64_t fs, const uint8_t* arena, uint8_t* stage) {
  const uint64_t nWork = (uint64_t)n * ((fs + kGatherChunk - 1) / kGatherChunk);
  hipLaunchKernelGGL(zra_upd_stage_cached_kernel, dim3((uint32_t)std::min<uint64_t>((nWork + 3) / 4, kGatherGrid)), dim3(256), 0, s, copies, n, s0, (u64)fs,
                     arena, stage);
}

struct UpdateImpl {
  static Status run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize,
                    const uint64_t* hDataOff, size_t nw, const uint8_t* dAppend, size_t appendSize, uint8_t* dOut, size_t outCap,
                    size_t* outSize, int level, bool checksum, UpdCacheView* cache);
};

Status Engine::update_archive(const uint8_t* dArc, size_t arcSize, const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize,
                              const uint64_t* hDataOff, size_t nw, const uint8_t* dAppend, size_t appendSize, uint8_t* dOut, size_t outCap,
                              size_t* outSize, int level, bool checksum, UpdCacheView* cache) {
  for (auto& v : ustats_) v = 0;
  return UpdateImpl::run(*this, dArc, arcSize, dData, hOff, hSize, hDataOff, nw, dAppend, appendSize, dOut, outCap, outSize, level, checksum, cache);
}

Status UpdateImpl::run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* dData, const uint64_t* hOff, const uint64_t* hSize,
                       const uint64_t* hDataOff, size_t nw, const uint8_t* dAppend, size_t appendSize, uint8_t* dOut, size_t outCap,
                       size_t* outSize, int level, bool checksum, UpdCacheView* cache) {
  // ---- 1. arguments, 2. overlap (with the archive, and with the arena of the handle the update goes through)
  if (!outSize || !dOut || (!dArc && arcSize) || (nw && (!hOff || !hSize || !hDataOff)) || (!dAppend && appendSize)) return zerr(42);
  if (!dData) for (size_t i = 0; i < nw; i++) if (hSize[i]) return zerr(42);
  if (outCap && arcSize && (uintptr_t)dOut < (uintptr_t)dArc + arcSize && (uintptr_t)dArc < (uintptr_t)dOut + outCap) return zerr(42);
  const bool cached = cache && cache->slots;
  if (cached && outCap && (uintptr_t)dOut < (uintptr_t)cache->arena + (size_t)cache->slots * cache->h.frameSize &&
      (uintptr_t)cache->arena < (uintptr_t)dOut + outCap)
    return zerr(42);
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  // ---- 3. header: the statuses of ZraHipArchiveOpen; beyond them a frame size of 0 and a table that does not cover the content
  // (an open handle refuses every read of such an archive; here there is no frame to put a byte in)
  // (a handle holds a checked header: it is not read from the device again)
  ArchiveView arc;
  if (cache) arc = ArchiveView::over(cache->h, dArc, arcSize);
  else { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  const uint64_t fs = arc.fs, U = arc.U;
  const uint32_t F = arc.frames;
  if (fs == 0 || (U + fs - 1) / fs != F) return {kHeaderInvalid, 0};
  // ---- 4. writes. The bound is inclusive: offset + size == uncompressedSize is the write that reaches the last byte. (The reference's
  // ">=" (zra.cpp:260) is a quirk of its reads, kept there for compatibility; a write that could never touch the last byte of the
  // content would be a defect.) Empty writes are ignored wherever they point.
  std::vector<size_t> idx;
  uint64_t written = appendSize, maxEnd = 0;
  for (size_t i = 0; i < nw; i++) {
    const uint64_t o = hOff[i], z = hSize[i];
    if (!z) continue;
    if (o > U || z > U - o) return {kOutOfBounds, 0};
    idx.push_back(i); written += z; maxEnd = std::max(maxEnd, o + z);
  }
  // two writes that share a byte: refused — no "last one wins" between slices that are copied side by side
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return hOff[a] < hOff[b]; });
  for (size_t k = 1; k < idx.size(); k++) if (hOff[idx[k - 1]] + hSize[idx[k - 1]] > hOff[idx[k]]) return zerr(42);
  if (appendSize > ~0ull - U) return {kCompressedTooLarge, 0};
  const uint64_t U2 = U + appendSize, F2wide = U2 / fs + (U2 % fs ? 1 : 0);
  if (F2wide > 0xFFFFFFF0ull) return {kCompressedTooLarge, 0};
  const uint32_t F2 = (uint32_t)F2wide;
  const size_t nData = idx.size(), nT = nData + (appendSize ? 1 : 0);
  if (nT > 0xFFFFFFF0ull) return zerr(64);
  // the handle's frame table over the frames of the result (behind the host-side checks: a refused call allocates nothing)
  const uint32_t* const cacheSlotOf = cached ? cache->table(cache->ctx, F2) : nullptr;
  if (cached && !cacheSlotOf) return zerr(64);
  E.updStageMs_ = 0;
  if (cached && !E.call_events()) return zerr(1);
  // the tuples, sorted by offset, in page-locked memory and from there to the device in chunks
  uint64_t nSlices = 0;
  if (nT) {
    uint64_t* const hq = E.pinned_tuples(nT);
    if (!hq || !E.qmeta_.reserve(4 * nT * 8 + 64)) return zerr(64);
    for (size_t q0 = 0; q0 < nT; q0 += Engine::kTupleChunk) {
      const size_t q1 = std::min(nT, q0 + Engine::kTupleChunk);
      for (size_t q = q0; q < q1; q++) {
        const uint64_t o = q < nData ? hOff[idx[q]] : U, z = q < nData ? hSize[idx[q]] : appendSize;
        hq[4 * q] = o; hq[4 * q + 1] = z; hq[4 * q + 2] = q < nData ? hDataOff[idx[q]] : 0; hq[4 * q + 3] = nSlices;
        nSlices += (o + z - 1) / fs - o / fs + 1;
      }
      { Status st = E.upload_tuples(q0, q1); if (st.zra) return st; }
    }
  }
  const uint64_t* dq = E.qmeta_.as<uint64_t>();
  // ---- plan
  const uint32_t passSlots = pass_slots(fs);
  const uint64_t touchedMax = std::min<uint64_t>(F2, nSlices), jobsMax = std::min<uint64_t>(F, nSlices);
  const size_t passesMax = (size_t)((touchedMax + passSlots - 1) / passSlots);
  // cover[F2] | slotOf[F2] | totals[16] | passJob[passes + 1] | passCopy[passes + 1]
  const size_t planWords = 2 * (size_t)F2 + 16 + 2 * (passesMax + 1);
  const uint32_t nBlocks = F2 / 1024 + 1;                                  // (F2 + 1 entries: the frames and the end)
  if (!E.upd_.plan.reserve(planWords * 4 + 64) || !E.upd_.frames.reserve((2 * ((size_t)F2 + 1) + 2 * ((size_t)nBlocks + 1)) * 8 + 64) ||
      !E.upd_.table.reserve(((size_t)F2 + 1) * 5 + 64) || !E.frameOff_.reserve((jobsMax + 1) * 16) || !E.outOff_.reserve((jobsMax + 1) * 8) ||
      !E.expect_.reserve((jobsMax + 1) * 4) || (cacheSlotOf && !E.upd_.copies.reserve((jobsMax + 1) * 16)))
    return zerr(64);
  uint32_t* cover = E.upd_.plan.as<uint32_t>(), *slotOf = cover + F2, *totals = slotOf + F2, *passJob = totals + 16;
  uint32_t* const passCopy = passJob + passesMax + 1, * const copies = cacheSlotOf ? E.upd_.copies.as<uint32_t>() : nullptr;
  uint64_t* newOff = E.upd_.frames.as<uint64_t>(), *disp = newOff + F2 + 1, *sums = disp + F2 + 1;
  HIPCHK_CLR(hipMemsetAsync(cover, 0, planWords * 4, s));
  if (nSlices)
    hipLaunchKernelGGL(zra_upd_mark_kernel, dim3((uint32_t)((nSlices + 255) / 256)), dim3(256), 0, s, dq, (u32)nT, (u64)nSlices, (u64)fs, cover);
  uint32_t hTotals[5] = {0, 0, 0, 0, 0};
  if (F2) {
    hipLaunchKernelGGL(zra_upd_plan_kernel, dim3(1), dim3(1024), 0, s, cover, F2, F, arc.table, (u64)arc.bodyBytes, (u64)fs, (u64)U, (u64)U2, passSlots,
                       cacheSlotOf, slotOf, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>(), passJob, copies, passCopy,
                       totals);
    HIPCHK_CLR(hipMemcpyAsync(hTotals, totals, sizeof(hTotals), hipMemcpyDeviceToHost, s));
  }
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  // ---- 5. the old seek table over the frames carried over
  if (hTotals[2]) return zerr(20);
  const uint32_t touched = hTotals[0], jobs = hTotals[1], staged = hTotals[3], refreshed = hTotals[4];
  const uint32_t passes = (touched + passSlots - 1) / passSlots;
  // ---- 6. passes: decode the frames that keep old bytes, lay the new bytes over them, encode
  uint64_t encoded = 0;
  if (touched) {
    std::vector<uint32_t> hPassJob(passes + 1), hPassCopy(passes + 1, 0u);
    HIPCHK_CLR(hipMemcpyAsync(hPassJob.data(), passJob, ((size_t)passes + 1) * 4, hipMemcpyDeviceToHost, s));
    if (staged) HIPCHK_CLR(hipMemcpyAsync(hPassCopy.data(), passCopy, ((size_t)passes + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    const uint64_t bound = zra_fmt::compress_bound(fs);
    if (!E.stage_.reserve((size_t)std::min<uint64_t>(touched, passSlots) * fs + 64) || !E.upd_.packed.reserve((size_t)touched * bound + 64) ||
        !E.upd_.encSizes.reserve((size_t)touched * 8 + 64))
      return zerr(64);
    uint8_t* const stage = E.stage_.as<uint8_t>();
    // only the last frame of the result can be short, and only if new bytes reach it is it staged (then as the last slot of all)
    const bool lastStaged = F2 && (appendSize || maxEnd > (uint64_t)(F2 - 1) * fs);
    const uint64_t lastLen = F2 ? U2 - (uint64_t)(F2 - 1) * fs : 0;
    const uint32_t patchGrid = (uint32_t)std::min<uint64_t>((nSlices + 3) / 4, 1u << 20);
    for (uint32_t p = 0; p < passes; p++) {
      const uint32_t s0 = p * passSlots, n = std::min(passSlots, touched - s0);
      const uint32_t j0 = hPassJob[p], j1 = hPassJob[p + 1], c0 = hPassCopy[p], c1 = hPassCopy[p + 1];
      if (c1 > c0) {                                                  // (other staging slots than the decode jobs': no order between the two)
        HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
        upd_launch_stage_cached(s, copies + 4 * (size_t)c0, c1 - c0, s0, fs, cache->arena, stage);
        HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
      }
      if (j1 > j0) {
        Status st = E.decode_jobs(arc.body, arc.bodyBytes, E.frameOff_.as<uint64_t>() + 2 * (size_t)j0, stage, E.outOff_.as<uint64_t>() + j0,
                                  E.expect_.as<uint32_t>() + j0, j1 - j0, (uint32_t)std::min<uint64_t>(fs, 0xFFFFFFFFu), 2);
        if (st.zra) return st;
      }
      hipLaunchKernelGGL(zra_upd_patch_kernel, dim3(patchGrid), dim3(256), 0, s, dq, (u32)nT, (u32)nData, (u64)nSlices, (u64)fs, slotOf, s0, n,
                         dData, dAppend, stage);
      const size_t inSize = (size_t)(n - 1) * fs + (size_t)(p + 1 == passes && lastStaged ? lastLen : fs);
      size_t bsz = 0;
      Status st = E.compress_frames(stage, inSize, E.upd_.packed.as<uint8_t>() + encoded, E.upd_.encSizes.as<uint64_t>() + s0, &bsz, level, (uint32_t)fs, checksum);
      if (st.zra) return st;
      encoded += bsz;
      // (compress_frames returned synchronised: the pass's events have completed)
      if (c1 > c0) E.updStageMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
    }
  }
  // ---- sizes, offsets, table
  uint64_t hTot[2] = {0, 0};
  hipLaunchKernelGGL(zra_upd_sizes_kernel, dim3(nBlocks), dim3(1024), 0, s, F2, slotOf, E.upd_.encSizes.as<uint64_t>(), arc.table, sums);
  hipLaunchKernelGGL(zra_upd_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nBlocks);
  hipLaunchKernelGGL(zra_upd_offsets_kernel, dim3(nBlocks), dim3(1024), 0, s, F2, slotOf, E.upd_.encSizes.as<uint64_t>(), arc.table, sums, arc.body,
                     E.upd_.packed.as<uint8_t>(), newOff, disp, E.upd_.table.as<uint8_t>());
  // the header on the host (5 bytes per frame, as compress_device does): fixed part rewritten, meta section copied, new table, CRC-32
  const size_t metaSize = arc.h.metaSize, tableBytes = ((size_t)F2 + 1) * 5;
  const uint64_t headerSize = zra_fmt::kFixedSize + (uint64_t)metaSize + tableBytes;
  if (headerSize > 0xFFFFFFFFull) return {kCompressedTooLarge, 0};
  std::vector<uint8_t> hdr((size_t)headerSize);
  HIPCHK_CLR(hipMemcpyAsync(hTot, sums + 2 * (size_t)nBlocks, 16, hipMemcpyDeviceToHost, s));
  if (metaSize) HIPCHK_CLR(hipMemcpyAsync(hdr.data() + zra_fmt::kFixedSize, dArc + zra_fmt::kFixedSize, metaSize, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipMemcpyAsync(hdr.data() + zra_fmt::kFixedSize + metaSize, E.upd_.table.p, tableBytes, hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  const uint64_t body = hTot[0];
  // ---- 7. size limit (compress_device's rule, zra.cpp:227), 8. capacity
  if (headerSize + body >= zra_fmt::kMaxCompressedSize) return {kCompressedTooLarge, 0};
  *outSize = (size_t)(headerSize + body);
  if (outCap < headerSize + body) return {kOutputTooSmall, 0};
  zra_fmt::write_fixed(hdr.data(), U2, F2 + 1, (uint32_t)fs, (uint32_t)metaSize);
  zra_fmt::wr32(hdr.data() + 14, zra_fmt::header_hash(hdr.data(), hdr.data() + zra_fmt::kFixedSize));
  // ---- the handle's resident frames: the same slices over their arena slots (the patch is idempotent, and a staging window of an
  // earlier pass is long overwritten). A wholly replaced frame and the old last frame grown by the append are among them. Launched
  // whenever there is a cache and a slice: coherence does not hang on the counter.
  if (cached && nSlices)
    hipLaunchKernelGGL(zra_upd_patch_kernel, dim3((uint32_t)std::min<uint64_t>((nSlices + 3) / 4, 1u << 20)), dim3(256), 0, s, dq, (u32)nT, (u32)nData,
                       (u64)nSlices, (u64)fs, cacheSlotOf, 0u, cache->slots, dData, dAppend, cache->arena);
  // ---- gather
  HIPCHK_CLR(hipMemcpyAsync(dOut, hdr.data(), (size_t)headerSize, hipMemcpyHostToDevice, s));
  // (ZraHipLastKernelMs after an update: the gather, the call's bandwidth kernel)
  E.lastKernelMs_ = 0;
  const bool gather = body && F2;
  if (gather) {
    const uint64_t nChunks = (body + kGatherChunk - 1) / kGatherChunk;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nChunks + 3) / 4, kGatherGrid);
    HIPCHK_CLR(hipEventRecord(E.ev0_, s));
    hipLaunchKernelGGL(zra_upd_gather_kernel, dim3(grid), dim3(256), 0, s, newOff, disp, F2, (u64)body, dOut + headerSize);
    HIPCHK_CLR(hipEventRecord(E.ev1_, s));
  }
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  if (gather) E.lastKernelMs_ = Engine::elapsed_ms(E.ev0_, E.ev1_);
  const uint64_t st8[8] = {F2, touched, jobs, touched, body - encoded, encoded, written, passes};
  for (int i = 0; i < 8; i++) E.ustats_[i] = st8[i];
  if (cache) {
    if (parse_fixed_header(hdr.data(), &cache->newHeader)) return zerr(1);   // (cannot happen: the fixed part was written above)
    cache->staged = staged; cache->refreshed = refreshed;
  }
  return ok();
}

}  // namespace zra_eng
