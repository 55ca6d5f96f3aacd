// zra_amd — host engine implementation: CRC-32, engine lifetime and scratch, the decode driver and the whole-archive entry points.
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_format.h"
#include <algorithm>
#include <atomic>

extern "C" __global__ void zra_dec_parse_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_huf_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_chain_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_chain_lds_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_exec_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_parse_all_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_dec_exec_all_kernel(ZraDecodeArgs a);
extern "C" __global__ void zra_ra_small_kernel(ZraDecodeArgs a, uint32_t* bail, const uint32_t* expect, uint32_t jobBase, unsigned long long* result);

using namespace zra_dev;

namespace zra_fmt {
uint32_t crc32(uint32_t crc, const void* data, size_t n) {
  static uint32_t T[8][256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
      T[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; i++)
      for (int t = 1; t < 8; t++) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
    init = true;
  }
  const uint8_t* p = (const uint8_t*)data;
  crc = ~crc;
  while (n >= 8) {
    uint32_t a = rd32(p) ^ crc, b = rd32(p + 4);
    crc = T[7][a & 0xFF] ^ T[6][(a >> 8) & 0xFF] ^ T[5][(a >> 16) & 0xFF] ^ T[4][a >> 24] ^
          T[3][b & 0xFF] ^ T[2][(b >> 8) & 0xFF] ^ T[1][(b >> 16) & 0xFF] ^ T[0][b >> 24];
    p += 8; n -= 8;
  }
  while (n--) crc = T[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
  return ~crc;
}
}  // namespace zra_fmt

// ---- utility kernels
namespace {

// seek table (5-byte entries inside the archive) -> u64 frame offsets + trivial output layout
__global__ void zra_jobs_from_seektable_kernel(const u8* table, u32 nFrames, u32 frameSize, u64 total,
                                               u64* frameOff, u64* outOff, u32* expect) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nFrames) frameOff[i] = seek_entry(table, i);
  if (i < nFrames) {
    // a frame whose slot starts at or beyond the declared size gets no room at all (an inflated tableSize or a shrunk
    // uncompressedSize in a crafted header): the decoder then reports dstSize_tooSmall for it, like the reference's single
    // multi-frame call running out of destination (zra.cpp:249), and nothing is written past `total`
    u64 o = (u64)i * frameSize;
    outOff[i] = o < total ? o : total;
    expect[i] = (u32)frame_expect(i, frameSize, total);
  }
}

// content-checksum verification of decoded frames: 4 lanes per frame (16 frames per wave)
// Frame end, in the order of ZSTD_decompressFrame: content checksum over the bytes the frame actually regenerated, then (ours, the
// frames being decoded side by side into fixed slots) the regenerated size against the slot: ZE_SIZE_MISMATCH is not a zstd code —
// the caller either re-decodes sequentially from that frame (whole-archive decode: one multi-frame zstd call in the reference packs
// frames back to back whatever they regenerate) or reports corruption_detected.
constexpr u32 ZE_SIZE_MISMATCH = 255;
__global__ void zra_xxh64_verify_kernel(const u8* out, const u64* outOff, const u32* expect, const u32* produced, const u32* frameMeta,
                                        u32* status, u32 nFrames) {
  const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 f = gid >> 2; const int j = gid & 3;
  const bool live = f < nFrames && status[f] == 0 && frameMeta[2 * (size_t)f] != 2;   // 2: stopped early (random access), nothing to check
  const bool active = live && frameMeta[2 * (size_t)f] == 1;
  const u8* p = active ? out + outOff[f] : out;
  const u32 n = active ? produced[f] : 0;
  const u64 h = zra_xxh64_quad(p, n, j);
  if (live && j == 0) {
    if (active && (u32)h != frameMeta[2 * (size_t)f + 1]) status[f] = ZE_CHECKSUM_WRONG;
    else if (expect && produced[f] != expect[f]) status[f] = ZE_SIZE_MISMATCH;
  }
}

// result[0] = min over failing frames of (frame << 8 | code); ~0 when all succeeded
__global__ void zra_first_error_kernel(const u32* status, u32 nFrames, u32 jobBase, unsigned long long* result) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nFrames && status[i]) atomicMin(result, ((unsigned long long)(jobBase + i) << 8) | (status[i] & 0xFF));
}

}  // namespace

// =================================================================================================
namespace zra_eng {

// bytes of device scratch all engines of the process hold (what the engine pool's cap looks at)
static std::atomic<uint64_t> g_scratchBytes{0};
uint64_t scratch_bytes_in_use() { return g_scratchBytes.load(); }

bool DevBuf::reserve(size_t n) {
  if (n <= cap) return true;
  if (p) { (void)hipFree(p); g_scratchBytes -= cap; p = nullptr; cap = 0; }
  size_t want = n + n / 8 + 256;
  // test hook: ZRA_ALLOC_LIMIT_MIB makes any single reservation above the limit fail (memory_allocation paths without a full device)
  static const uint64_t limit = zra_env::env_set("ZRA_ALLOC_LIMIT_MIB") ? (uint64_t)zra_env::env_i64("ZRA_ALLOC_LIMIT_MIB", 0) << 20 : ~0ull;
  const hipError_t ea = want > limit ? hipErrorOutOfMemory : hipMalloc(&p, want);
  if (ea != hipSuccess) { p = nullptr; cap = 0; (void)hipGetLastError(); return false; }
  cap = want; g_scratchBytes += cap;
  return true;
}
void DevBuf::release() { if (p) { (void)hipFree(p); g_scratchBytes -= cap; } p = nullptr; cap = 0; }

int parse_fixed_header(const uint8_t* b, HeaderInfo* h) {
  using namespace zra_fmt;
  if (rd32(b + 8) != kZraMagic || rd16(b + 12) > kVersion) return kHeaderInvalid;   // zra.cpp:144-145
  h->version = rd16(b + 12);
  h->size = rd32(b + 4) + 8;
  h->uncompressedSize = rd64(b + 18);
  h->frameSize = rd32(b + 30);
  h->metaOffset = (uint32_t)kFixedSize;
  h->metaSize = rd32(b + 34);
  h->seekTableOffset = h->metaOffset + h->metaSize;
  h->seekTableSize = rd32(b + 26) * (uint32_t)kEntrySize;
  if (h->version != 1) return kVersionLow;                                           // zra.cpp:156-162
  return 0;
}

Status Engine::create(Engine** out, int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return zerr(1);
  HIPCHK(hipSetDevice(device));
  Engine* e = new Engine();
  e->device_ = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete e; return zerr(1); }
  e->numCUs_ = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&e->stream_, hipStreamNonBlocking) != hipSuccess) { delete e; return zerr(1); }
  {
    // Stream B carries the persistent entropy stage (which also scans and gathers) beside the persistent match finder of stream A.
    // The runtime multiplexes streams onto a handful of hardware queues per priority class, and two streams that land on one queue run
    // their kernels one after the other — two persistent kernels that wait for each other must not: B gets the highest priority class,
    // a queue that stream A (normal priority) is never put on.
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo) {
      if (hipStreamCreateWithPriority(&e->stream2_, hipStreamNonBlocking, hi) != hipSuccess) { delete e; return zerr(1); }
    } else if (hipStreamCreateWithFlags(&e->stream2_, hipStreamNonBlocking) != hipSuccess) { delete e; return zerr(1); }
  }
  if (hipEventCreate(&e->ev0_) != hipSuccess || hipEventCreate(&e->ev1_) != hipSuccess ||
      hipEventCreateWithFlags(&e->evWait_, hipEventDisableTiming) != hipSuccess) { delete e; return zerr(1); }
  for (auto& ev : e->evR_) if (hipEventCreate(&ev) != hipSuccess) { delete e; return zerr(1); }
  *out = e;
  return ok();
}

void Engine::free_scratch() {
  for (DevBuf* b : {&raPlan_, &raLimit_, &raPieceBase_, &raPieces_, &decFrames_, &decTables_, &decLists_, &decCounters_, &decLits_, &decSeqs_, &roundN_, &status_,
                    &produced_, &frameMeta_, &frameOff_, &outOff_, &expect_, &result_, &stage_, &qmeta_, &encScan_, &hostIn_, &hostOut_, &seqScratch_, &mfFlags_, &decBlkRecs_, &decBlkTables_, &decBlkLists_})
    b->release();
  for (auto& x : encCtx_) for (DevBuf* b : {&x.tables, &x.seqs, &x.lits, &x.work, &x.slots, &x.misc, &x.ck, &x.sizes, &x.rec}) b->release();
  for (DevBuf* b : {&upd_.plan, &upd_.packed, &upd_.encSizes, &upd_.frames, &upd_.table, &upd_.copies}) b->release();
  for (DevBuf* b : {&vfy_.plan, &vfy_.faults, &scan_.tables, &scan_.list, &fp_.flags, &fp_.dirty, &fp_.tables, &fp_.list, &rec_.tables, &rec_.ranges, &tally_.hdr, &tally_.tables, &tally_.entries}) b->release();
}

Status Engine::release_scratch() {
  HIPCHK(hipSetDevice(device_));
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipStreamSynchronize(stream2_));
  free_scratch();
  mfTeleDev_ = nullptr;                                // (lived inside encScan_)
  dbgB_ = 0;                                           // (debug_read_seqs: the batch it would read lived in encCtx_[0])
  decCountersClean_ = false;
  return ok();
}

Engine::~Engine() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  free_scratch();
  for (auto ev : evPool_) (void)hipEventDestroy(ev);
  for (auto ev : stageEv_) (void)hipEventDestroy(ev);
  if (stream2_) { (void)hipStreamSynchronize(stream2_); (void)hipStreamDestroy(stream2_); }
  for (auto st : pipeStreams_) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  if (pinQ_) (void)hipHostFree(pinQ_);
  if (pinSmall_) (void)hipHostFree(pinSmall_);
  for (auto& ev : evR_) if (ev) (void)hipEventDestroy(ev);
  for (auto ev : evCall_) if (ev) (void)hipEventDestroy(ev);
  if (ev0_) (void)hipEventDestroy(ev0_);
  if (ev1_) (void)hipEventDestroy(ev1_);
  if (evWait_) (void)hipEventDestroy(evWait_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

Status Engine::sync() { HIPCHK(hipSetDevice(device_)); HIPCHK(hipStreamSynchronize(stream_)); HIPCHK(hipStreamSynchronize(stream2_)); return ok(); }

Status Engine::wait_stream(hipStream_t producer) {
  HIPCHK(hipSetDevice(device_));
  HIPCHK(hipEventRecord(evWait_, producer));
  HIPCHK(hipStreamWaitEvent(stream_, evWait_, 0));
  HIPCHK(hipStreamWaitEvent(stream2_, evWait_, 0));
  return ok();
}

// scratch of one decode pass over a.nFrames jobs (decode records, table slots, stage lists, literal / sequence scratch, result words)
Status Engine::decode_scratch(ZraDecodeArgs& a, uint32_t maxFrameBytes) {
  const uint32_t n = a.nFrames;
  // scratch of a round: Huffman-decoded literals and decoded sequences of one block per frame, bump-allocated on the device
  const uint64_t perFrame = std::min<uint64_t>((uint64_t)maxFrameBytes + 16, (128u << 10) + 16);
  // sized for what data needs, not for the worst case (a frame whose allocation does not fit simply takes the next round):
  // Huffman-coded literals rarely exceed half of the output, sequences (8 bytes each) three quarters of it
  const uint64_t litCap = std::max<uint64_t>((uint64_t)n * perFrame / 2, 1u << 20);
  const uint64_t seqCap = std::max<uint64_t>((uint64_t)n * perFrame * 3 / 32, 1u << 20);               // entries of 8 bytes
  if (!decFrames_.reserve((size_t)n * sizeof(ZraDecFrame)) || !decTables_.reserve((size_t)n * ZRA_DEC_TBL_WORDS * 4) ||
      !decLists_.reserve((size_t)n * 16 + 64) || !decCounters_.reserve(ZRA_DC_WORDS * 4 + 64) || !decLits_.reserve(litCap + 64) ||
      !decSeqs_.reserve(seqCap * 8 + 64) || !status_.reserve((size_t)n * 4) || !produced_.reserve((size_t)n * 4) ||
      !frameMeta_.reserve((size_t)n * 8) || !result_.reserve(64))
    return zerr(64 /* memory_allocation */);
  uint32_t* listA = decLists_.as<uint32_t>();
  a.pending = listA + 2 * (size_t)n; a.hufJobs = listA + 3 * (size_t)n;
  a.counters = decCounters_.as<uint32_t>();
  a.frames = decFrames_.as<ZraDecFrame>(); a.tables = decTables_.as<uint32_t>();
  a.lits = decLits_.as<uint8_t>(); a.litCap = litCap; a.seqs = decSeqs_.as<uint64_t>(); a.seqCap = seqCap;
  a.status = status_.as<uint32_t>(); a.produced = produced_.as<uint32_t>(); a.frameMeta = frameMeta_.as<uint32_t>();
  return ok();
}

// Small batches (random access): every job in ONE launch of zra_ra_small_kernel, frame-end checks behind it, one synchronisation.
// *bailed: jobs the kernel handed back (damaged or unusual frames): the caller takes the batch through decode_launch.
Status Engine::decode_small(const ZraDecodeArgs& a0, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* hResult, uint32_t* bailed) {
  ZraDecodeArgs a = a0;
  const uint32_t n = a.nFrames;
  RaTrace trace{"    small", 12};
  { Status st = decode_scratch(a, maxFrameBytes); if (st.zra) return st; }
  trace.mark("scratch");
  a.active = nullptr; a.nActive = n; a.round = 0; a.nextActive = decLists_.as<uint32_t>();
  // the round counters are zero whenever this path finds them (zeroed behind the previous use, off the caller's wait); the result
  // word and the kernel's bail counter (counting down) were preset together by decode_jobs' one memset; frame-end checks and the
  // first-error reduction happen inside the kernel: one launch, one copy back, one synchronisation
  if (!decCountersClean_) HIPCHK(hipMemsetAsync(a.counters, 0, ZRA_DC_WORDS * 4, stream_));
  decCountersClean_ = false;
  uint32_t* dBail = (uint32_t*)(result_.as<uint8_t>() + 8);
  HIPCHK(hipEventRecord(ev0_, stream_));
  hipLaunchKernelGGL(zra_ra_small_kernel, dim3(n), dim3(192), 0, stream_, a, dBail, dExpect, jobBase, result_.as<unsigned long long>());
  HIPCHK(hipEventRecord(ev1_, stream_));
  trace.mark("launched");
  unsigned long long two[2] = {~0ull, ~0ull};
  HIPCHK(hipMemcpyAsync(two, result_.p, 16, hipMemcpyDeviceToHost, stream_));
  trace.mark("queued rest");
  HIPCHK(hipStreamSynchronize(stream_));
  trace.mark("sync");
  HIPCHK(hipGetLastError());
  if (hipMemsetAsync(a.counters, 0, ZRA_DC_WORDS * 4, stream_) == hipSuccess) decCountersClean_ = true;     // (for the next call; nobody waits for it)
  two[1] = 0xFFFFFFFFull - (two[1] & 0xFFFFFFFFull);
  *bailed = (uint32_t)two[1];
  if (!*bailed) *hResult = two[0];
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) { lastKernelMs_ = ms; kstats_[4] += ms; kstats_[5] += 1; dstats_[5] += ms; dstats_[6] += 1; }
  return ok();
}

hipEvent_t Engine::stage_event() {
  if (stageEvNext_ == stageEv_.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; stageEv_.push_back(e); }
  return stageEv_[stageEvNext_++];
}

// The chain stage over nJobs jobs, on stream_ behind `after` (the event recorded behind the Huffman stage).
Status Engine::launch_chain(uint64_t nJobs, const ZraDecodeArgs& mid, hipEvent_t after) {
  // (resident waves per CU of the chain kernel — lane = frame, 64 frames' tables per wave: fewer frames in flight keep more of their table cells in the caches; A/B on one box, round 3,
  // 8 GiB decode, chain stage 2 / 3 / 4 / 6 / 8 waves per CU -> 26.0 / 26.6 / 30.1 / 35.2 / 32.9 ms; 16 GiB, 1 / 1.5 / 2 / 2.5: 74.1 / 58.2 / 51.9 / 53.0 ms)
  constexpr uint32_t chainWaves = 2;
  // (ZRA_DEC_CHAIN_LDS_MIN: jobs from which the LDS-table chain kernel runs beside the other one; the tests set it to 1)
  static const uint32_t chainLdsMin = (uint32_t)zra_env::env_int("ZRA_DEC_CHAIN_LDS_MIN", numCUs_ * 96);
  static const int chainLdsMode = zra_env::env_int("ZRA_DEC_CHAIN_LDS", 1);   // 0: without the LDS-table kernel; 2 (test hook): that kernel alone
  const uint32_t gridChain = (uint32_t)std::min<uint64_t>((nJobs + 63) / 64, (uint64_t)numCUs_ * chainWaves);
  // beside the lane-per-frame chain kernel (tables in HBM scratch, two waves per CU) one workgroup per CU with its frames' tables in
  // LDS, on another stream, pulling from the same queue
  if (chainLdsMode != 0 && nJobs >= chainLdsMin) {
    if (!pipeStreams_[1]) { if (hipStreamCreateWithFlags(&pipeStreams_[1], hipStreamNonBlocking) != hipSuccess) { pipeStreams_[1] = nullptr; (void)hipGetLastError(); } }
    const size_t ldsBytes = (128 + (size_t)ZRA_CHAIN_LDS_FRAMES * (ZRA_DEC_TBL_WORDS / 2 + ZRA_CHAIN_RING_WORDS)) * 4;   // two-byte cells + a 144-byte bitstream ring per frame
    if (pipeStreams_[1] && !chainLdsAttr_) {
      if (hipFuncSetAttribute((const void*)zra_dec_chain_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes) == hipSuccess) chainLdsAttr_ = 1;
      else { chainLdsAttr_ = -1; (void)hipGetLastError(); }
    }
    if (pipeStreams_[1] && chainLdsAttr_ > 0) {
      hipEvent_t eJoin = stage_event(); if (!eJoin) return zerr(1);
      HIPCHK(hipStreamWaitEvent(pipeStreams_[1], after, 0));
      hipLaunchKernelGGL(zra_dec_chain_lds_kernel, dim3((uint32_t)numCUs_), dim3(64), ldsBytes, pipeStreams_[1], mid);
      HIPCHK(hipEventRecord(eJoin, pipeStreams_[1]));
      if (chainLdsMode != 2) hipLaunchKernelGGL(zra_dec_chain_kernel, dim3(gridChain), dim3(64), 0, stream_, mid);
      HIPCHK(hipStreamWaitEvent(stream_, eJoin, 0));
      return ok();
    }
  }
  hipLaunchKernelGGL(zra_dec_chain_kernel, dim3(gridChain), dim3(64), 0, stream_, mid);
  return ok();
}

Status Engine::launch_stages(uint64_t nJobs, const ZraDecodeArgs& a, const ZraDecodeArgs& mid, uint32_t nFrames, bool blockPass, hipEvent_t se[5]) {
  for (int k = 0; k < 5; k++) { se[k] = stage_event(); if (!se[k]) return zerr(1); }
  const uint32_t gridParse = (uint32_t)std::min<uint64_t>(nFrames, (uint64_t)numCUs_ * decOccParse_);
  const uint32_t gridHuf = (uint32_t)std::min<uint64_t>((nJobs + ZRA_HUF_FRAMES - 1) / ZRA_HUF_FRAMES, (uint64_t)numCUs_ * decOccHuf_);
  const uint32_t gridExec = (uint32_t)std::min<uint64_t>(nFrames, (uint64_t)numCUs_ * decOccExec_);
  HIPCHK(hipEventRecord(se[0], stream_));
  hipLaunchKernelGGL(blockPass ? zra_dec_parse_all_kernel : zra_dec_parse_kernel, dim3(gridParse), dim3(64), 0, stream_, a);
  HIPCHK(hipEventRecord(se[1], stream_));
  hipLaunchKernelGGL(zra_dec_huf_kernel, dim3(gridHuf), dim3(64), 0, stream_, mid);
  HIPCHK(hipEventRecord(se[2], stream_));
  { Status st = launch_chain(nJobs, mid, se[2]); if (st.zra) return st; }
  HIPCHK(hipEventRecord(se[3], stream_));
  hipLaunchKernelGGL(blockPass ? zra_dec_exec_all_kernel : zra_dec_exec_kernel, dim3(gridExec), dim3(64), 0, stream_, a);
  HIPCHK(hipEventRecord(se[4], stream_));
  return ok();
}

// One pass of the decoder over the jobs of `a0`: rounds of parse -> chain -> execute (a round = one compressed block of every
// unfinished frame) until no frame is left, then the content checksums and the first-error reduction.
Status Engine::decode_launch(const ZraDecodeArgs& a0, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* hResult) {
  ZraDecodeArgs a = a0;
  const uint32_t n = a.nFrames;
  { Status st = decode_scratch(a, maxFrameBytes); if (st.zra) return st; }
  decCountersClean_ = false;
  // ZRA_DEC_FRONT=0: every block with Huffman-coded literals goes through the Huffman kernel (the two kernels as they were); default:
  // the parse wave of the rounds below decodes the literals of a block with a new tree itself, the Huffman launch takes the rest
  static const int decFront = zra_env::env_int("ZRA_DEC_FRONT", 1);
  a.decFront = decFront != 0;
  uint32_t* listA = decLists_.as<uint32_t>(); uint32_t* listB = listA + n;
  if (!decOccParse_) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&decOccParse_, zra_dec_parse_kernel, 64, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&decOccExec_, zra_dec_exec_kernel, 64, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&decOccHuf_, zra_dec_huf_kernel, 64, 0));
    decOccParse_ = std::max(1, decOccParse_); decOccExec_ = std::max(1, decOccExec_); decOccHuf_ = std::max(1, decOccHuf_);
  }
  HIPCHK(hipEventRecord(ev0_, stream_));
  constexpr uint32_t aheadCap = 16;                     // rounds of one burst, at most (the rounds below)
  if (!roundN_.reserve(4 * (aheadCap + 2) + 64)) return zerr(64);
  // ---- Block-parallel pass (round 6) for frames of several blocks. The rounds below take one block of every frame per round, and their
  // chain stage runs one LANE per frame: at 256 KiB frames a pass of 8 GiB has 32 Ki lanes walking a 128 KiB block each, twice in a row (47 of
  // 76 ms), at 2 MiB frames 4 Ki lanes, sixteen times (168 of 208 ms). Here every compressed block of every frame is a job of the Huffman
  // and chain stages at once — one parse launch that walks all blocks of a frame, one Huffman launch, one chain launch over the blocks
  // (their initial repeat offsets as markers), one execute launch that walks a frame's blocks in order and puts the markers' values in.
  // A frame that is not a clean frame of zstd's own making (an error anywhere, a compressed block that regenerates something else than
  // 128 KiB, the long-offset mode) comes back on a list and takes the rounds below, where every status of the reference is reproduced.
  // ZRA_DEC_FMB=0 turns the pass off.
  static const int fmbEnv = zra_env::env_int("ZRA_DEC_FMB", 1);
  static const uint32_t fmbMin = (uint32_t)zra_env::env_int("ZRA_DEC_FMB_MIN", 64);
  const uint32_t bpf = (uint32_t)(((uint64_t)maxFrameBytes + ZRA_FMB_BLOCK - 1) / ZRA_FMB_BLOCK);
  bool fmb = fmbEnv != 0 && bpf >= 2 && maxFrameBytes <= (64u << 20) && n >= fmbMin && (uint64_t)n * bpf < (1ull << 30);
  uint32_t nRest = n;
  if (fmb) {
    const uint64_t nb = (uint64_t)n * bpf;
    // scratch for every block of every frame at once (the rounds size theirs for one block per frame)
    const uint64_t litAll = std::max<uint64_t>((uint64_t)n * ((uint64_t)maxFrameBytes + 16) / 2, 1u << 20);
    const uint64_t seqAll = std::max<uint64_t>((uint64_t)n * ((uint64_t)maxFrameBytes + 16) * 3 / 32, 1u << 20);
    if (!decBlkRecs_.reserve((size_t)nb * sizeof(ZraDecFrame)) || !decBlkTables_.reserve((size_t)nb * ZRA_DEC_TBL_WORDS * 4) ||
        !decBlkLists_.reserve((size_t)(2 * nb + n) * 4 + 64) || !decLits_.reserve(litAll + 64) || !decSeqs_.reserve(seqAll * 8 + 64)) {
      (void)hipGetLastError();
      fmb = false;                                      // (no memory for it: the rounds)
      // a failed reserve leaves its buffer EMPTY (zra_engine.h), and the one before it may have moved: the rounds' scratch is sized again,
      // so that a.lits / a.litCap / a.seqs / a.seqCap describe live buffers (they fitted a moment ago; if they do not now, a status)
      { Status st = decode_scratch(a, maxFrameBytes); if (st.zra) return st; }
    } else { a.lits = decLits_.as<uint8_t>(); a.seqs = decSeqs_.as<uint64_t>(); }       // (the buffers may have moved)
    if (fmb) {
      ZraDecodeArgs x = a;
      x.bpf = bpf; x.blkRecs = decBlkRecs_.as<ZraDecFrame>(); x.blkTables = decBlkTables_.as<uint32_t>();
      uint32_t* bl = decBlkLists_.as<uint32_t>();
      x.pending = bl; x.hufJobs = bl + nb; x.execList = bl + 2 * nb;
      x.litCap = litAll; x.seqCap = seqAll;
      x.active = nullptr; x.nActive = n; x.round = 0; x.nActivePtr = nullptr; x.nextActive = listA;
      HIPCHK(hipMemsetAsync(x.counters, 0, ZRA_DC_WORDS * 4, stream_));
      ZraDecodeArgs y = x; y.frames = x.blkRecs; y.tables = x.blkTables;      // the Huffman and chain stages: jobs are blocks
      hipEvent_t se[5];
      { Status st = launch_stages(nb, x, y, n, true, se); if (st.zra) return st; }
      uint32_t back = 0;
      HIPCHK(hipMemcpyAsync(&back, x.counters + ZRA_DC_NNEXT, 4, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      HIPCHK(hipGetLastError());
      for (int k = 0; k < 4; k++) { float m = 0; if (hipEventElapsedTime(&m, se[k], se[k + 1]) == hipSuccess) dstats_[k] += m; }
      dstats_[4] += 1;
      stageEvNext_ = 0;
      nRest = back;
    }
  }
  // ---- The rounds of one set of jobs, one stage after the other on the engine's stream.
  // Rounds are enqueued `ahead` at a time without a host synchronisation in between (round 4): a frame of B blocks needs B rounds, and the
  // job count of round r+1 is round r's counter — copied aside on the device and read by the parse kernel (the other stages always
  // counted on the device). Grids are sized by the previous burst's job count (an upper bound: jobs only drop out). One copy back and
  // one synchronisation per burst; frames that still go on afterwards (foreign archives with more, smaller blocks; scratch deferrals)
  // take further bursts of one round.
  auto run_rounds = [&](ZraDecodeArgs& x, uint32_t nActive, const uint32_t* active, uint32_t round, uint32_t* lA, uint32_t* lB, uint32_t ahead) -> Status {
    uint32_t* const dN = roundN_.as<uint32_t>();
    while (nActive) {
      const uint32_t burst = std::max(1u, std::min(ahead, aheadCap));
      hipEvent_t se[aheadCap][5];
      for (uint32_t bi = 0; bi < burst; bi++) {
        HIPCHK(hipMemsetAsync(x.counters, 0, ZRA_DC_WORDS * 4, stream_));
        x.active = active; x.nActive = nActive; x.round = round + bi;
        x.nActivePtr = bi ? dN + bi : nullptr;
        x.nextActive = (active == lA) ? lB : lA;
        { Status st = launch_stages(nActive, x, x, nActive, false, se[bi]); if (st.zra) return st; }
        // the next round's job count stays on the device (the counters are cleared before it starts)
        HIPCHK(hipMemcpyAsync(dN + bi + 1, x.counters + ZRA_DC_NNEXT, 4, hipMemcpyDeviceToDevice, stream_));
        active = x.nextActive;
      }
      uint32_t next = 0;
      HIPCHK(hipMemcpyAsync(&next, dN + burst, 4, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      HIPCHK(hipGetLastError());
      for (uint32_t bi = 0; bi < burst; bi++)
        for (int k = 0; k < 4; k++) { float m = 0; if (hipEventElapsedTime(&m, se[bi][k], se[bi][k + 1]) == hipSuccess) dstats_[k] += m; }
      dstats_[4] += burst;
      stageEvNext_ = 0;
      x.nActivePtr = nullptr;
      nActive = next; round += burst; ahead = 1;
      if (round > (1u << 20)) return zerr(1);          // cannot happen: every round finishes at least one block of some frame
    }
    return ok();
  };
  Status st = fmb ? run_rounds(a, nRest, listA, 0, listA, listB, 1)
                  : run_rounds(a, n, nullptr, 0, listA, listB, (maxFrameBytes + (128u << 10) - 1) / (128u << 10));
  if (st.zra) return st;
  // ---- frame-end checks
  HIPCHK(hipEventRecord(ev1_, stream_));
  const uint32_t tb = 256;
  hipLaunchKernelGGL(zra_xxh64_verify_kernel, dim3((n * 4 + tb - 1) / tb), dim3(tb), 0, stream_, a.out, a.outOff, dExpect,
                     produced_.as<uint32_t>(), frameMeta_.as<uint32_t>(), status_.as<uint32_t>(), n);
  hipLaunchKernelGGL(zra_first_error_kernel, dim3((n + tb - 1) / tb), dim3(tb), 0, stream_, status_.as<uint32_t>(), n, jobBase,
                     result_.as<unsigned long long>());
  HIPCHK(hipMemcpyAsync(hResult, result_.p, 8, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipGetLastError());
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) { lastKernelMs_ = ms; kstats_[4] += ms; kstats_[5] += 1; }
  return ok();
}

// One pass of decode_jobs. Few jobs: the one-launch kernel (latency path); a job it hands back (damaged / unusual frame) sends the pass
// through the four-kernel pipeline, where every status of the reference is reproduced.
Status Engine::decode_pass(const ZraDecodeArgs& b, const uint32_t* dExpect, uint32_t maxFrameBytes, uint32_t jobBase, unsigned long long* res) {
  static const uint32_t smallMax = (uint32_t)zra_env::env_int("ZRA_DEC_SMALL_MAX", 1024);
  if (b.nFrames <= smallMax) {
    uint32_t bailed = 0;
    unsigned long long r2 = *res;
    Status st = decode_small(b, dExpect, maxFrameBytes, jobBase, &r2, &bailed);
    if (st.zra) return st;
    if (!bailed) { *res = r2; return ok(); }
    if (*res == ~0ull) HIPCHK(hipMemsetAsync(result_.p, 0xFF, 64, stream_));   // (what the handed-back pass left in the result word)
    else { unsigned long long keep = *res; HIPCHK(hipMemsetAsync(result_.p, 0xFF, 64, stream_)); HIPCHK(hipMemcpyAsync(result_.p, &keep, 8, hipMemcpyHostToDevice, stream_)); HIPCHK(hipStreamSynchronize(stream_)); }
  }
  return decode_launch(b, dExpect, maxFrameBytes, jobBase, res);
}

Status Engine::staged_pass(const ArchiveView& a, uint32_t j0, uint32_t n, uint8_t* window, unsigned long long* firstError) {
  lastProducedTotal_ = ~0ull;
  if (!result_.reserve(64)) return zerr(64);
  HIPCHK_CLR(hipMemsetAsync(result_.p, 0xFF, 64, stream_));
  ZraDecodeArgs b{};
  b.body = a.body; b.bodySize = a.bodyBytes; b.out = window; b.offStride = 2; b.nFrames = n;
  b.frameOff = frameOff_.as<uint64_t>() + 2 * (size_t)j0; b.outOff = outOff_.as<uint64_t>(); b.outCap = expect_.as<uint32_t>() + j0;
  *firstError = ~0ull;
  return decode_pass(b, b.outCap, (uint32_t)std::min<uint64_t>(a.fs, 0xFFFFFFFFu), 0, firstError);
}

// seqTotal == 0: every frame owns its slot (random access: the reference decodes the touched frames into frameSize buffers).
// seqTotal != 0: whole-archive semantics of ONE multi-frame zstd call over `seqTotal` bytes of destination (zra.cpp:249): frames are
// decoded side by side into their nominal slots; if one regenerates another size than its slot (only possible for a corrupted or
// foreign archive) everything from that frame on is re-decoded one frame at a time, packed back to back, exactly as the reference
// would — first error in frame order, dstSize_tooSmall against the whole destination.
Status Engine::decode_jobs(const uint8_t* dBody, uint64_t bodySize, const uint64_t* dFrameOff, uint8_t* dOut,
                           const uint64_t* dOutOff, const uint32_t* dExpect, uint32_t nFrames, uint32_t maxFrameBytes, uint32_t offStride,
                           uint64_t seqTotal, const ZraDecodeArgs* ra) {
  lastProducedTotal_ = ~0ull;
  if (nFrames == 0) return ok();
  HIPCHK(hipSetDevice(device_));
  if (!result_.reserve(64)) return zerr(64);
  HIPCHK(hipMemsetAsync(result_.p, 0xFF, 64, stream_));
  ZraDecodeArgs a{};
  if (ra) a = *ra;
  a.body = dBody; a.bodySize = bodySize; a.out = dOut; a.offStride = offStride;
  // passes: the chain kernel runs one LANE per frame, so a pass wants hundreds of thousands of frames; its per-round scratch
  // (literals + sequences of one block per frame, ~1.25 bytes per output byte) is what bounds it — 16 GiB of output per pass
  const uint64_t perFrame = std::min<uint64_t>((uint64_t)maxFrameBytes + 16, (128u << 10) + 16);
  constexpr uint64_t passBytes = 16ull << 30;
  // equal passes (a remainder pass of a few frames would cost a whole latency-bound round)
  const uint64_t inFlight = std::max<uint64_t>(1, passBytes / perFrame);
  const uint32_t nPass = (uint32_t)((nFrames + inFlight - 1) / inFlight);
  const uint32_t passFrames = (nFrames + nPass - 1) / nPass;
  // (Measured and dropped: two passes in flight on the engine's two streams, each driven by its own host thread, with full or with
  // halved grids — 52.1 vs 53.0 ms per 4 GiB. The four stages do not hide each other: they queue on the same L2 / fabric request path.)
  unsigned long long res = ~0ull;
  for (uint32_t p0 = 0; p0 < nFrames; p0 += passFrames) {
    ZraDecodeArgs b = a;
    b.nFrames = std::min(passFrames, nFrames - p0);
    b.frameOff = dFrameOff + (size_t)p0 * offStride; b.outOff = dOutOff + p0; b.outCap = dExpect + p0;
    if (ra) { if (ra->limit) b.limit = ra->limit + p0; if (ra->pieceBase) b.pieceBase = ra->pieceBase + p0; }
    Status st = decode_pass(b, dExpect + p0, maxFrameBytes, p0, &res);
    if (st.zra) return st;
  }
  if (res == ~0ull) return ok();
  const uint32_t code = (uint32_t)(res & 0xFF), first = (uint32_t)(res >> 8);
  const bool resize = code == 255 /* ZE_SIZE_MISMATCH */ || code == 70;
  if (!seqTotal || !resize) return zerr(reported_code(res));
  return decode_sequential_tail(a, dFrameOff, offStride, dOutOff, first, nFrames, maxFrameBytes, seqTotal);
}

// The sequential tail of decode_jobs (seqTotal != 0) from frame `first`, the first one that regenerated another size than its slot.
Status Engine::decode_sequential_tail(const ZraDecodeArgs& a, const uint64_t* dFrameOff, uint32_t offStride, const uint64_t* dOutOff, uint32_t first,
                                      uint32_t nFrames, uint32_t maxFrameBytes, uint64_t seqTotal) {
  unsigned long long res = ~0ull;
  uint64_t cur = 0;
  HIPCHK(hipMemcpyAsync(&cur, dOutOff + first, 8, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  // One frame at a time is what the reference's multi-frame call does, and what decides a frame's status (its room is what the frames
  // before it left) — but an archive whose frames simply regenerate another size than the header says (a damaged or foreign frameSize)
  // would take one four-kernel pass per frame that way: hundreds of thousands of them. So after a frame has regenerated `got` bytes
  // the frames behind it are decoded side by side, on the guess that they regenerate the same (each at its guessed place, with exactly
  // that room); the longest run for which the guess held — no status, that size — stands as decoded; the first frame that deviates is
  // decoded again alone with its true room, which decides what it reports, and gives the next guess.
  constexpr uint32_t kSpec = 1u << 16;
  if (!seqScratch_.reserve(64 + (size_t)kSpec * 12)) return zerr(64);
  uint64_t* dCur = seqScratch_.as<uint64_t>(); uint32_t* dCap = (uint32_t*)(seqScratch_.as<uint8_t>() + 16);
  uint64_t* dSpecOff = (uint64_t*)(seqScratch_.as<uint8_t>() + 64); uint32_t* dSpecCap = (uint32_t*)(seqScratch_.as<uint8_t>() + 64 + (size_t)kSpec * 8);
  std::vector<uint64_t> hOff; std::vector<uint32_t> hCap, hProduced, hStatus;
  uint32_t guess = 0;
  // the side-by-side batch grows geometrically while the guess holds and starts small again after a miss: an archive whose frame sizes
  // alternate would otherwise decode up to 64 Ki frames to advance by one (quadratic work an untrusted archive could ask for)
  uint32_t specB = 16;
  for (uint32_t f = first; f < nFrames;) {
    if (guess && nFrames - f >= 2 && seqTotal > cur) {
      const uint32_t B = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(nFrames - f, kSpec), specB), (seqTotal - cur) / guess);
      if (B >= 2) {
        hOff.resize(B); hCap.assign(B, guess); hProduced.resize(B); hStatus.resize(B);
        for (uint32_t i = 0; i < B; i++) hOff[i] = cur + (uint64_t)i * guess;
        HIPCHK(hipMemcpyAsync(dSpecOff, hOff.data(), (size_t)B * 8, hipMemcpyHostToDevice, stream_));
        HIPCHK(hipMemcpyAsync(dSpecCap, hCap.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream_));
        HIPCHK(hipMemsetAsync(result_.p, 0xFF, 64, stream_));
        ZraDecodeArgs b = a;
        b.frameOff = dFrameOff + (size_t)f * offStride; b.outOff = dSpecOff; b.outCap = dSpecCap; b.nFrames = B;
        b.limit = nullptr; b.pieceBase = nullptr; b.pieces = nullptr;
        unsigned long long r2 = ~0ull;
        // (scratch sized for real frames, not for a tiny guess in front of full-size ones: a block is at most 128 KiB)
        Status st = decode_launch(b, nullptr, std::max<uint32_t>(guess, std::min<uint32_t>(maxFrameBytes ? maxFrameBytes : (128u << 10), 128u << 10)), f, &r2);
        if (st.zra) return st;
        HIPCHK(hipMemcpyAsync(hProduced.data(), produced_.p, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipMemcpyAsync(hStatus.data(), status_.p, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        uint32_t k = 0;
        while (k < B && hStatus[k] == 0 && hProduced[k] == guess) k++;
        cur += (uint64_t)k * guess; f += k;
        specB = k == B ? (uint32_t)std::min<uint64_t>((uint64_t)specB * 4, kSpec) : 16u;
        if (f >= nFrames) break;
      }
    }
    const uint32_t cap = (uint32_t)std::min<uint64_t>(seqTotal > cur ? seqTotal - cur : 0, 0xFFFFFF00u);
    HIPCHK(hipMemcpyAsync(dCur, &cur, 8, hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemcpyAsync(dCap, &cap, 4, hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemsetAsync(result_.p, 0xFF, 64, stream_));
    ZraDecodeArgs b = a;
    b.frameOff = dFrameOff + (size_t)f * offStride; b.outOff = dCur; b.outCap = dCap; b.nFrames = 1;
    b.limit = nullptr; b.pieceBase = nullptr; b.pieces = nullptr;
    Status st = decode_launch(b, nullptr, (uint32_t)std::min<uint64_t>(cap, 0x7FFFFFFFu), f, &res);
    if (st.zra) return st;
    uint32_t got = 0;
    HIPCHK(hipMemcpyAsync(&got, produced_.p, 4, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (res != ~0ull) return zerr((int)(res & 0xFF));
    cur += got; guess = got; f++;
  }
  lastProducedTotal_ = cur;
  return ok();
}

Status Engine::read_fixed_header(const uint8_t* dArc, size_t arcSize, HeaderInfo* h) {
  if (arcSize <= zra_fmt::kFixedSize) return {kOutOfBounds, 0};          // BufferView reader quirk, zra.cpp:166
  uint8_t fixed[zra_fmt::kFixedSize];
  HIPCHK(hipMemcpyAsync(fixed, dArc, sizeof(fixed), hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  if (int e = parse_fixed_header(fixed, h)) return {e, 0};
  if (arcSize < h->size) return {kOutOfBounds, 0};                         // zra.cpp:169-170
  return ok();
}

Status Engine::decompress_device(const uint8_t* dArc, size_t arcSize, uint8_t* dOut, size_t outCap) {
  HIPCHK(hipSetDevice(device_));
  reset_decode_stats();
  HeaderInfo h;
  { Status st = read_fixed_header(dArc, arcSize, &h); if (st.zra) return st; }
  if (outCap < h.uncompressedSize) return {kOutputTooSmall, 0};            // zra.cpp:245-246
  const uint32_t nFrames = h.frames();
  if (nFrames == 0 || h.frameSize == 0) return ok();
  if ((uint64_t)h.seekTableOffset + h.seekTableSize > h.size) return {kHeaderInvalid, 0};
  // Frames beyond the declared size get a zero-capacity slot in the job kernel (dstSize_tooSmall, like the reference's
  // sequential call running out of destination); nothing can be written at or beyond dOut + uncompressedSize <= dOut + outCap.
  if (!frameOff_.reserve(((size_t)nFrames + 1) * 8) || !outOff_.reserve((size_t)nFrames * 8) || !expect_.reserve((size_t)nFrames * 4))
    return zerr(64);
  hipLaunchKernelGGL(zra_jobs_from_seektable_kernel, dim3((nFrames + 256) / 256), dim3(256), 0, stream_, dArc + h.seekTableOffset,
                     nFrames, h.frameSize, h.uncompressedSize, frameOff_.as<uint64_t>(), outOff_.as<uint64_t>(), expect_.as<uint32_t>());
  return decode_jobs(dArc + h.size, arcSize - h.size, frameOff_.as<uint64_t>(), dOut, outOff_.as<uint64_t>(), expect_.as<uint32_t>(), nFrames, h.frameSize, 1, outCap);
}

Status Engine::upload_jobs(const std::vector<uint64_t>& frameOff, const std::vector<uint64_t>& outOff, const std::vector<uint32_t>& expect) {
  if (!frameOff_.reserve(frameOff.size() * 8) || !outOff_.reserve(outOff.size() * 8) || !expect_.reserve(expect.size() * 4)) return zerr(64);
  HIPCHK(hipMemcpyAsync(frameOff_.p, frameOff.data(), frameOff.size() * 8, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipMemcpyAsync(outOff_.p, outOff.data(), outOff.size() * 8, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipMemcpyAsync(expect_.p, expect.data(), expect.size() * 4, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipStreamSynchronize(stream_));   // host vectors go out of scope
  return ok();
}

Status Engine::decompress_frames_host_list(const uint8_t* dBody, uint64_t bodySize, const std::vector<uint64_t>& hFrameOff,
                                           uint8_t* dOut, uint64_t total, uint32_t frameSize) {
  HIPCHK(hipSetDevice(device_));
  const uint32_t nFrames = (uint32_t)(hFrameOff.size() - 1);
  if (nFrames == 0) return ok();
  std::vector<uint64_t> oo(nFrames); std::vector<uint32_t> ex(nFrames);
  for (uint32_t i = 0; i < nFrames; i++) {
    oo[i] = (uint64_t)i * frameSize;
    ex[i] = (uint32_t)frame_expect(i, frameSize, total);
  }
  { Status st = upload_jobs(hFrameOff, oo, ex); if (st.zra) return st; }
  return decode_jobs(dBody, bodySize, frameOff_.as<uint64_t>(), dOut, outOff_.as<uint64_t>(), expect_.as<uint32_t>(), nFrames, frameSize);
}

}  // namespace zra_eng
