// zra_amd — batched random access: the planner that turns a batch of queries into decode jobs and slice lists on the device, and
// the entry points that run it (the archive handle, zra_archive.hip, drives the same planner over the frames its cache misses).
#include "zra_host.h"
#include "zra_dev.h"
#include <algorithm>

using namespace zra_dev;

namespace {

// whole-frame jobs carry no limit. A limit of `expect` would stop the decoder as soon as that many bytes exist: before the frame end of
// a frame whose last block does not say it is the last, and before the frame-end checks (a stopped frame has none). The frame's room
// is its capacity, outCap.
constexpr u32 kNoLimit = 0xFFFFFFFFu;

// the jobs are built from the query arrays and the archive's own seek table (zra.cpp:265-269 per query: first frame, frames touched, head skip, tail length)
// pass 1: every query marks the frames it touches
__global__ void zra_ra_count_kernel(const u64* q, u32 nq, u64 fs, RaPlan P) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const u64 off = q[4 * (size_t)i], size = q[4 * (size_t)i + 1];
  if (!size) return;
  const u64 f0 = off / fs, f1 = (off + size - 1) / fs;
  for (u64 f = f0; f <= f1; f++) {
    atomicAdd(&P.cnt[f], 1u);
    const u32 end = f == f1 ? (u32)((off + size - 1) % fs) + 1 : (u32)fs;
    atomicMax(&P.need[f], end);
  }
}
// pass 2 (one workgroup): exclusive scans over the frames -> dense slots + slice-list bases, and the decode job of every touched
// frame: compressed span from the 5-byte seek-table entries, destination slot inside the pass-sized scratch window, bytes to produce
// compressed span of frame f from the 5-byte entries, relative to the body bytes this device holds ([bodyBase, ...) of the archive's
// body: a shard of a distributed archive holds its own frames only); a span that starts before them comes out inverted (refused as
// srcSize_wrong by the decoder, like any span outside the buffer)
__device__ __forceinline__ void ra_frame_span(const u8* table, u64 f, u64 bodyBase, u64* so, u64* se) {
  const u64 a = seek_entry(table, f), b = seek_entry(table, f + 1);
  if (a < bodyBase || b < bodyBase) { *so = 1; *se = 0; }
  else { *so = a - bodyBase; *se = b - bodyBase; }
}
__global__ void __launch_bounds__(1024) zra_ra_plan_kernel(RaPlan P, u32 nFrames, const u8* table, u64 bodyBase, u64 fs, u64 total, u32 passSlots, u32 fullFrames,
                                                           u64* frameOff, u64* outOff, u32* outCap, u32* limit, u32* pieceBase, const u32* victim) {
  __shared__ u32 sT[1024], sP[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nFrames + 1023) / 1024;
  const u32 b0 = tid * per, b1 = min(nFrames, b0 + per);
  u32 t = 0, p = 0;
  for (u32 f = b0; f < b1; f++) { const u32 c = P.cnt[f]; t += c != 0; p += c; }
  sT[tid] = t; sP[tid] = p;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {                     // Hillis-Steele inclusive scan of the 1024 partials
    const u32 xt = tid >= d ? sT[tid - d] : 0, xp = tid >= d ? sP[tid - d] : 0;
    __syncthreads();
    sT[tid] += xt; sP[tid] += xp;
    __syncthreads();
  }
  u32 st = sT[tid] - t, sp = sP[tid] - p;                  // exclusive
  for (u32 f = b0; f < b1; f++) {
    const u32 c = P.cnt[f];
    if (!c) continue;
    P.slot[f] = st;
    ra_frame_span(table, f, bodyBase, &frameOff[2 * (size_t)st], &frameOff[2 * (size_t)st + 1]);
    const u32 expect = (u32)frame_expect(f, fs, total);
    // (victim: the archive handle's arena slots, zra_archive.hip — job st of a pass decodes into slot victim[st % passSlots])
    outOff[st] = (u64)(victim ? victim[st % passSlots] : st % passSlots) * fs;
    outCap[st] = expect;
    limit[st] = fullFrames ? kNoLimit : min(P.need[f], expect);
    pieceBase[st] = sp;
    st++; sp += c;
  }
  if (tid == 1023) { P.totals[0] = sT[1023]; P.totals[1] = sP[1023]; pieceBase[sT[1023]] = sP[1023]; }
}
// pass 3: every query writes its slices into the lists of the frames it touches
__global__ void zra_ra_fill_kernel(const u64* q, u32 nq, u64 fs, RaPlan P, const u32* pieceBase, ZraRaPiece* pieces) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const u64 off = q[4 * (size_t)i], size = q[4 * (size_t)i + 1], dst = q[4 * (size_t)i + 2];
  if (!size) return;
  const u64 f0 = off / fs, f1 = (off + size - 1) / fs;
  u64 done = 0;
  for (u64 f = f0; f <= f1; f++) {
    const u32 srcOff = f == f0 ? (u32)(off % fs) : 0u;
    const u64 len = min<u64>(fs - srcOff, size - done);
    // a frame with no count has no job: the archive handle counts only the frames its lookup missed (a hit's slice has been copied
    // already); that count is the only test — P.slot of such a frame is not set
    if (P.cnt[f]) {
      const u32 at = pieceBase[P.slot[f]] + atomicAdd(&P.cursor[f], 1u);
      ZraRaPiece pc; pc.dstOff = dst + done; pc.srcOff = srcOff; pc.len = (u32)len;
      pieces[at] = pc;
    }
    done += len;
  }
}

// small batches (far fewer slices than the archive has frames): one decode job per slice, built from the query alone — no pass over
// the frames of the archive, no count/scan, nothing read back. A frame two slices share is decoded once per slice.
__global__ void zra_ra_direct_kernel(const u64* q, u32 nq, u32 nPieces, u64 fs, u64 total, const u8* table, u64 bodyBase, u32 fullFrames, u64* frameOff, u64* outOff,
                                     u32* outCap, u32* limit, u32* pieceBase, ZraRaPiece* pieces) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) pieceBase[nPieces] = nPieces;
  if (i >= nq) return;
  const u64 off = q[4 * (size_t)i], size = q[4 * (size_t)i + 1], dst = q[4 * (size_t)i + 2];
  if (!size) return;
  const u64 f0 = off / fs, f1 = (off + size - 1) / fs;
  u32 st = (u32)q[4 * (size_t)i + 3];
  u64 done = 0;
  for (u64 f = f0; f <= f1; f++, st++) {
    ra_frame_span(table, f, bodyBase, &frameOff[2 * (size_t)st], &frameOff[2 * (size_t)st + 1]);
    const u32 expect = (u32)frame_expect(f, fs, total);
    const u32 srcOff = f == f0 ? (u32)(off % fs) : 0u;
    const u64 len = min<u64>(fs - srcOff, size - done);
    outOff[st] = (u64)st * fs;
    outCap[st] = expect;
    limit[st] = fullFrames ? kNoLimit : min((u32)(srcOff + len), expect);
    pieceBase[st] = st;
    ZraRaPiece pc; pc.dstOff = dst + done; pc.srcOff = srcOff; pc.len = (u32)len;
    pieces[st] = pc;
    done += len;
  }
}

}  // namespace

// =================================================================================================
namespace zra_eng {

// the fixed header of a device-resident archive, read back and checked: the statuses of ZraHipDecompressRABatch (the archive handle
// opens with the same ones, zra_archive.hip)
Status Engine::ra_header(const uint8_t* dArc, size_t arcSize, HeaderInfo* h) {
  { Status st = read_fixed_header(dArc, arcSize, h); if (st.zra) return st; }
  const uint32_t nFrames = h->frames();
  const uint64_t fs = h->frameSize, U = h->uncompressedSize;
  // the reference indexes the table with offset / frameSize without looking at tableSize (zra.cpp:265-268); a header whose fields
  // disagree (size beyond what the table covers, table outside the header) would send it out of bounds — here it is HeaderInvalid
  if ((uint64_t)h->seekTableOffset + h->seekTableSize > h->size) return {kHeaderInvalid, 0};
  if (fs && U && (U + fs - 1) / fs != nFrames) return {kHeaderInvalid, 0};
  return ok();
}

uint64_t* Engine::pinned_tuples(size_t nTuples) {
  if (pinQCap_ >= 4 * nTuples) return pinQ_;
  if (pinQ_) (void)hipHostFree(pinQ_);
  pinQ_ = nullptr; pinQCap_ = 0;
  const size_t cap = std::max<size_t>(4 * nTuples, 4096);
  if (hipHostMalloc((void**)&pinQ_, cap * 8 + 64, hipHostMallocDefault) != hipSuccess) { pinQ_ = nullptr; (void)hipGetLastError(); return nullptr; }
  pinQCap_ = cap;
  return pinQ_;
}

// one walk over the queries: the reference's bound (offset + size >= uncompressedSize is refused: the ">=" quirk, zra.cpp:260;
// overflow-safe), the slices (one per frame a query touches) and the (offset, size, destination, first slice) tuples the device
// kernels read — written straight into page-locked memory, so that their copy (into qmeta_) runs at bus speed beside the launches that
// follow. *maxPieces = the slices; 0 when there is nothing to decode (the copies may still be in flight: the caller synchronises).
Status Engine::ra_walk_queries(const ArchiveView& a, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, uint64_t* maxPieces,
                               bool endInclusive) {
  const uint32_t nFrames = a.frames;
  const uint64_t fs = a.fs, U = a.U;
  *maxPieces = 0;
  if (nq > 0xFFFFFFF0ull) return zerr(64);
  uint64_t* const hq = pinned_tuples(nq);
  if (!hq) return zerr(64);
  uint64_t pieces = 0;
  const uint64_t slack = endInclusive ? 1 : 0;                  // (the record read: offset + size == U is inside)
  const bool pow2 = fs && !(fs & (fs - 1));
  const unsigned fsLog = pow2 ? (unsigned)__builtin_ctzll(fs) : 0u;
  if (fs == 0 || nFrames == 0) {
    for (size_t q = 0; q < nq; q++) if (hSize[q] >= U + slack || hOff[q] >= U - hSize[q] + slack) return {kOutOfBounds, 0};
    return ok();
  }
  if (!qmeta_.reserve(4 * nq * 8 + 64)) return zerr(64);
  for (size_t q0 = 0; q0 < nq; q0 += kTupleChunk) {     // tuples go to the device while the next ones are being written
    const size_t q1 = std::min(nq, q0 + kTupleChunk);
    for (size_t q = q0; q < q1; q++) {
      const uint64_t o = hOff[q], z = hSize[q];
      if (z >= U + slack || o >= U - z + slack) { (void)hipStreamSynchronize(stream_); return {kOutOfBounds, 0}; }
      hq[4 * q] = o; hq[4 * q + 1] = z; hq[4 * q + 2] = hOutOff[q]; hq[4 * q + 3] = pieces;
      if (z) pieces += pow2 ? ((o + z - 1) >> fsLog) - (o >> fsLog) + 1 : (o + z - 1) / fs - o / fs + 1;
    }
    { Status st = upload_tuples(q0, q1); if (st.zra) return st; }
  }
  *maxPieces = pieces;
  return ok();
}

// dense job numbers, decode jobs and piece lists of the frames counted in plan (a RaPlan's scratch) from the query tuples in qmeta_;
// totals = {jobs, pieces}. victim: see zra_ra_plan_kernel (nullptr: scratch window).
Status Engine::ra_plan_fill(uint32_t* plan, size_t nq, const ArchiveView& a, uint32_t passSlots, bool fullFrames, const uint32_t* victim, uint32_t totals[2]) {
  const RaPlan P = RaPlan::over(plan, a.frames);
  hipLaunchKernelGGL(zra_ra_plan_kernel, dim3(1), dim3(1024), 0, stream_, P, a.frames, a.table, (u64)a.bodyBase, (u64)a.fs, (u64)a.U, passSlots,
                     fullFrames ? 1u : 0u, frameOff_.as<uint64_t>(), outOff_.as<uint64_t>(), expect_.as<uint32_t>(), raLimit_.as<uint32_t>(),
                     raPieceBase_.as<uint32_t>(), victim);
  hipLaunchKernelGGL(zra_ra_fill_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, stream_, qmeta_.as<uint64_t>(), (u32)nq, (u64)a.fs, P,
                     raPieceBase_.as<uint32_t>(), raPieces_.as<ZraRaPiece>());
  totals[0] = totals[1] = 0;
  HIPCHK(hipMemcpyAsync(totals, P.totals, 8, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipGetLastError());
  return ok();
}

// dBody == nullptr: a whole archive at dArc (header, table, body). Otherwise dArc holds header + table only and dBody the bytes
// [bodyBase, bodyBase + bodyBytes) of the archive's body — the frames one rank of a distributed archive owns (zra_comm.hip).
Status Engine::decompress_ra_batch_shard(const uint8_t* dArc, size_t arcSize, const uint8_t* dBody, uint64_t bodyBytes, uint64_t bodyBase, uint8_t* dOut,
                                         const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq) {
  HIPCHK(hipSetDevice(device_));
  reset_decode_stats();
  ArchiveView a;
  { Status st = archive_view(dArc, arcSize, &a); if (st.zra) return st; }
  if (dBody) { a.body = dBody; a.bodyBytes = bodyBytes; a.bodyBase = bodyBase; }
  return ra_batch_body(a, dOut, hOff, hSize, hOutOff, nq);
}

// the batch behind a header that has been read and checked (ra_header): the archive handle without slots comes here directly
Status Engine::ra_batch_body(const ArchiveView& a, uint8_t* dOut, const uint64_t* hOff, const uint64_t* hSize, const uint64_t* hOutOff, size_t nq, bool endInclusive,
                             uint32_t* jobsOut) {
  if (jobsOut) *jobsOut = 0;
  RaTrace trace{"  ra", 14};
  HIPCHK(hipSetDevice(device_));
  reset_decode_stats();
  trace.mark("header read");
  const uint32_t nFrames = a.frames;
  const uint64_t fs = a.fs, U = a.U;
  if (nq == 0) return ok();
  uint64_t maxPieces = 0;
  { Status st = ra_walk_queries(a, hOff, hSize, hOutOff, nq, &maxPieces, endInclusive); if (st.zra) return st; }
  if (fs == 0 || nFrames == 0) return ok();
  if (maxPieces == 0) { HIPCHK(hipStreamSynchronize(stream_)); return ok(); }
  trace.mark("queries");
  const uint32_t passSlots = pass_slots(fs, 16ull << 30, nFrames);    // (the batch's own bounds: 16 GiB, every frame of the archive)
  const bool direct = maxPieces * 8 <= nFrames && maxPieces <= passSlots;
  const size_t nJobsMax = direct ? (size_t)maxPieces : (size_t)nFrames;
  if (!frameOff_.reserve((nJobsMax + 1) * 16) || !outOff_.reserve(nJobsMax * 8) || !expect_.reserve(nJobsMax * 4) ||
      !raLimit_.reserve(nJobsMax * 4) || !raPieceBase_.reserve((nJobsMax + 1) * 4) || !raPieces_.reserve((size_t)maxPieces * sizeof(ZraRaPiece) + 64))
    return zerr(64);
  uint32_t touched = 0;
  if (direct) {
    hipLaunchKernelGGL(zra_ra_direct_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, stream_, qmeta_.as<uint64_t>(), (u32)nq, (u32)maxPieces, (u64)fs,
                       (u64)U, a.table, (u64)a.bodyBase, raVerifyWholeFrames_ ? 1u : 0u, frameOff_.as<uint64_t>(), outOff_.as<uint64_t>(),
                       expect_.as<uint32_t>(), raLimit_.as<uint32_t>(), raPieceBase_.as<uint32_t>(), raPieces_.as<ZraRaPiece>());
    touched = (uint32_t)maxPieces;
    trace.mark("jobs queued");
  } else {
    if (!raPlan_.reserve(RaPlan::words(nFrames) * 4)) return zerr(64);
    HIPCHK(hipMemsetAsync(raPlan_.p, 0, RaPlan::words(nFrames) * 4, stream_));
    hipLaunchKernelGGL(zra_ra_count_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, stream_, qmeta_.as<uint64_t>(), (u32)nq, (u64)fs,
                       RaPlan::over(raPlan_.as<uint32_t>(), nFrames));
    uint32_t totals[2];
    Status st = ra_plan_fill(raPlan_.as<uint32_t>(), nq, a, passSlots, raVerifyWholeFrames_, nullptr, totals);
    if (st.zra) return st;
    touched = totals[0];
    trace.mark("plan");
  }
  if (jobsOut) *jobsOut = touched;
  if (!touched) return ok();
  // decode the touched frames, a scratch window of passSlots frames at a time (only frames that are decoded in full — or larger
  // than what the decoder needs as its match window — actually write there); slices leave for dOut as each frame finishes
  if (!stage_.reserve((size_t)std::min<uint64_t>(touched, passSlots) * fs + 64)) return zerr(64);
  ZraDecodeArgs ra{};
  ra.pieces = raPieces_.as<ZraRaPiece>(); ra.raOut = dOut;
  for (uint32_t s0 = 0; s0 < touched; s0 += passSlots) {
    const uint32_t n = std::min(passSlots, touched - s0);
    ra.limit = raLimit_.as<uint32_t>() + s0; ra.pieceBase = raPieceBase_.as<uint32_t>() + s0;
    Status st = decode_jobs(a.body, a.bodyBytes, frameOff_.as<uint64_t>() + 2 * (size_t)s0, stage_.as<uint8_t>(), outOff_.as<uint64_t>() + s0,
                            expect_.as<uint32_t>() + s0, n, (uint32_t)std::min<uint64_t>(fs, 0xFFFFFFFFu), 2, 0, &ra);
    if (st.zra) return st;
  }
  trace.mark("decode");
  return ok();
}

}  // namespace zra_eng
