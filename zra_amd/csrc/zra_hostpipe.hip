// zra_amd — host-pointer calls with the PCIe copies running beside the kernels.
//
// The reference's in-memory calls hand over host buffers (zra.cpp:194-256, C ABI zra.cpp:508-533). Large inputs are cut into chunks of
// whole frames; three threads work on neighbouring chunks at once:
//     uploader:   host -> device copy of chunk k+1 (and k+2)
//     this thread: kernels of chunk k (the engine's ordinary device-pointer calls)
//     downloader: device -> host copy of the result of chunk k-1
// Plain pageable memory is enough: on this platform a blocking hipMemcpy of pageable memory runs at the link rate (55 GB/s per
// direction measured, tools/pcie_probe.cpp) and only blocks the thread that issued it, so nothing is staged or registered.
// Frames are independent (zra.cpp:216-225), so the chunked result is byte-identical to the one-piece result.
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_format.h"
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace zra_eng {

namespace {

// progress counters of the three stages (chunks finished by each)
struct Pipe {
  std::mutex m;
  std::condition_variable cv;
  size_t uploaded = 0, computed = 0, downloaded = 0;
  bool failed = false;
  void bump(size_t& c) { { std::lock_guard<std::mutex> g(m); c++; } cv.notify_all(); }
  void fail() { { std::lock_guard<std::mutex> g(m); failed = true; } cv.notify_all(); }
  // waits until `c` >= want; false when another stage failed
  bool wait(const size_t& c, size_t want) {
    std::unique_lock<std::mutex> g(m);
    cv.wait(g, [&] { return failed || c >= want; });
    return !failed;
  }
};

}  // namespace

size_t host_chunk_bytes() {
  const size_t mib = (size_t)zra_env::env_i64("ZRA_HOST_CHUNK_MIB", 1024);   // read per call: tests shrink it to reach the chunked path with small inputs
  return std::max<size_t>(1, mib) << 20;
}

// ------------------------------------------------------------------------------------------------
// CompressBuffer on host memory. Small inputs: one piece. Otherwise chunks of ~1 GiB of whole frames through compress_frames();
// the seek table and the fixed header are put together on the host from the per-frame sizes (they are 5 bytes per frame).
Status Engine::compress_host(const uint8_t* hIn, size_t n, uint8_t* hOut, size_t* outSize, int level, uint32_t frameSize, bool checksum) {
  HIPCHK(hipSetDevice(device_));
  if (frameSize == 0) return zerr(42);
  const uint32_t tableSize = zra_fmt::table_size(n, frameSize);
  const size_t nFrames = tableSize - 1;
  const size_t headerSize = zra_fmt::kFixedSize + (size_t)tableSize * zra_fmt::kEntrySize;
  const size_t chunkFrames = std::max<size_t>(1, host_chunk_bytes() / frameSize);
  if (nFrames < 2 * chunkFrames) {
    const size_t cap = headerSize + zra_fmt::compress_bound(frameSize) * nFrames;
    if (!hostIn_.reserve(n + 64) || !hostOut_.reserve(cap + 64)) return zerr(64);
    if (n) HIPCHK(hipMemcpyAsync(hostIn_.p, hIn, n, hipMemcpyHostToDevice, stream_));
    Status s = compress_device(hostIn_.as<uint8_t>(), n, hostOut_.as<uint8_t>(), outSize, level, frameSize, checksum);
    if (s.zra) { (void)hipStreamSynchronize(stream_); return s; }
    HIPCHK(hipMemcpyAsync(hOut, hostOut_.p, *outSize, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    return ok();
  }
  const size_t chunkBytes = chunkFrames * frameSize;
  const size_t nChunks = (n + chunkBytes - 1) / chunkBytes;
  const size_t bodyCap = zra_fmt::compress_bound(frameSize) * chunkFrames;
  const size_t sizesOff = (bodyCap + 63) & ~(size_t)63;
  const size_t outSlot = sizesOff + chunkFrames * 8 + 64;
  // three input slots (one being filled, one queued, one being compressed), two output slots (one being written, one on its way back)
  if (!hostIn_.reserve(3 * chunkBytes + 64) || !hostOut_.reserve(2 * outSlot + 64)) return zerr(64);
  uint8_t* const dIn = hostIn_.as<uint8_t>();
  uint8_t* const dOut = hostOut_.as<uint8_t>();
  std::vector<uint64_t> sizes(nFrames);
  std::vector<uint64_t> bodyOff(nChunks + 1, 0);          // where a chunk's frames start inside the archive body
  std::vector<size_t> bodyLen(nChunks, 0);
  Pipe P;
  const int dev = device_;
  std::thread up([&] {
    if (hipSetDevice(dev) != hipSuccess) { P.fail(); return; }
    for (size_t k = 0; k < nChunks; k++) {
      if (k >= 3 && !P.wait(P.computed, k - 2)) return;                     // slot k%3 was chunk k-3's
      const size_t o = k * chunkBytes, len = std::min(chunkBytes, n - o);
      if (hipMemcpy(dIn + (k % 3) * chunkBytes, hIn + o, len, hipMemcpyHostToDevice) != hipSuccess) { P.fail(); return; }
      P.bump(P.uploaded);
    }
  });
  std::thread down([&] {
    if (hipSetDevice(dev) != hipSuccess) { P.fail(); return; }
    for (size_t k = 0; k < nChunks; k++) {
      if (!P.wait(P.computed, k + 1)) return;
      const uint8_t* slot = dOut + (k % 2) * outSlot;
      const size_t f0 = k * chunkFrames, nf = std::min(chunkFrames, nFrames - f0);
      if ((bodyLen[k] && hipMemcpy(hOut + headerSize + bodyOff[k], slot, bodyLen[k], hipMemcpyDeviceToHost) != hipSuccess) ||
          hipMemcpy(sizes.data() + f0, slot + sizesOff, nf * 8, hipMemcpyDeviceToHost) != hipSuccess) { P.fail(); return; }
      P.bump(P.downloaded);
    }
  });
  Status st = ok();
  for (size_t k = 0; k < nChunks; k++) {
    if (!P.wait(P.uploaded, k + 1) || (k >= 2 && !P.wait(P.downloaded, k - 1))) { st = zerr(1); break; }
    const size_t o = k * chunkBytes, len = std::min(chunkBytes, n - o);
    uint8_t* slot = dOut + (k % 2) * outSlot;
    size_t body = 0;
    st = compress_frames(dIn + (k % 3) * chunkBytes, len, slot, (uint64_t*)(slot + sizesOff), &body, level, frameSize, checksum);
    if (st.zra) { P.fail(); break; }
    bodyLen[k] = body; bodyOff[k + 1] = bodyOff[k] + body;
    P.bump(P.computed);
  }
  up.join(); down.join();
  if (!st.zra && P.failed) st = zerr(1);
  if (st.zra) { (void)hipDeviceSynchronize(); return st; }
  const uint64_t bodySize = bodyOff[nChunks];
  if (headerSize + bodySize >= zra_fmt::kMaxCompressedSize) return {kCompressedTooLarge, 0};   // zra.cpp:227
  zra_fmt::write_fixed(hOut, n, tableSize, frameSize, 0);
  uint8_t* e = hOut + zra_fmt::kFixedSize;
  uint64_t run = 0;
  for (size_t f = 0; f < nFrames; f++) { zra_fmt::entry_put(e + f * 5, run); run += sizes[f]; }
  zra_fmt::entry_put(e + nFrames * 5, run);
  if (run != bodySize) return zerr(1);
  zra_fmt::wr32(hOut + 14, zra_fmt::header_hash(hOut, hOut + zra_fmt::kFixedSize));
  *outSize = headerSize + bodySize;
  return ok();
}

// ------------------------------------------------------------------------------------------------
// DecompressBuffer on host memory (frames walked on the host, zra_capi.cpp). Chunks of whole frames: compressed span up, decoded
// frames down. The chunked path only ever finishes a clean archive; at the first frame that fails (or regenerates another size than
// its slot) the caller is told to take the one-piece path, which reproduces the reference's error and partial-output behaviour.
Status Engine::decode_host_pipelined(const uint8_t* hSpan, const std::vector<uint64_t>& starts, const std::vector<uint64_t>& ends,
                                     uint32_t frameSize, uint64_t total, uint8_t* hOut, bool* fallBack) {
  *fallBack = false;
  HIPCHK(hipSetDevice(device_));
  const size_t nFrames = starts.size();
  const size_t chunkFrames = std::max<size_t>(1, host_chunk_bytes() / frameSize);
  const size_t nChunks = (nFrames + chunkFrames - 1) / chunkFrames;
  size_t maxSpan = 0;
  for (size_t k = 0; k < nChunks; k++) {
    const size_t f0 = k * chunkFrames, f1 = std::min(nFrames, f0 + chunkFrames);
    if (ends[f1 - 1] < starts[f0]) { *fallBack = true; return ok(); }
    maxSpan = std::max<size_t>(maxSpan, ends[f1 - 1] - starts[f0]);
  }
  if (maxSpan > (4ull << 30)) { *fallBack = true; return ok(); }
  const size_t inSlot = (maxSpan + 64 + 63) & ~(size_t)63, outSlot = chunkFrames * (size_t)frameSize;
  std::vector<uint64_t> se(nFrames * 2), oo(nFrames);
  std::vector<uint32_t> ex(nFrames);
  for (size_t i = 0; i < nFrames; i++) {
    const size_t f0 = i / chunkFrames * chunkFrames;
    if (ends[i] < starts[i] || starts[i] < starts[f0]) { *fallBack = true; return ok(); }
    se[2 * i] = starts[i] - starts[f0]; se[2 * i + 1] = ends[i] - starts[f0];
    oo[i] = (uint64_t)(i - f0) * frameSize;
    ex[i] = (uint32_t)zra_dev::frame_expect(i, frameSize, total);
  }
  if (!hostIn_.reserve(3 * inSlot + 64) || !hostOut_.reserve(2 * outSlot + 64)) return zerr(64);
  { Status st = upload_jobs(se, oo, ex); if (st.zra) return st; }
  uint8_t* const dIn = hostIn_.as<uint8_t>();
  uint8_t* const dOut = hostOut_.as<uint8_t>();
  Pipe P;
  const int dev = device_;
  std::thread up([&] {
    if (hipSetDevice(dev) != hipSuccess) { P.fail(); return; }
    for (size_t k = 0; k < nChunks; k++) {
      if (k >= 3 && !P.wait(P.computed, k - 2)) return;
      const size_t f0 = k * chunkFrames, f1 = std::min(nFrames, f0 + chunkFrames);
      const size_t len = ends[f1 - 1] - starts[f0];
      if (len && hipMemcpy(dIn + (k % 3) * inSlot, hSpan + starts[f0], len, hipMemcpyHostToDevice) != hipSuccess) { P.fail(); return; }
      P.bump(P.uploaded);
    }
  });
  std::thread down([&] {
    if (hipSetDevice(dev) != hipSuccess) { P.fail(); return; }
    for (size_t k = 0; k < nChunks; k++) {
      if (!P.wait(P.computed, k + 1)) return;
      const uint64_t o = (uint64_t)k * outSlot;
      const size_t len = (size_t)std::min<uint64_t>(outSlot, total - std::min(total, o));   // the part of the chunk inside the declared size
      if (len && hipMemcpy(hOut + o, dOut + (k % 2) * outSlot, len, hipMemcpyDeviceToHost) != hipSuccess) { P.fail(); return; }
      P.bump(P.downloaded);
    }
  });
  Status st = ok();
  for (size_t k = 0; k < nChunks; k++) {
    if (!P.wait(P.uploaded, k + 1) || (k >= 2 && !P.wait(P.downloaded, k - 1))) { st = zerr(1); break; }
    const size_t f0 = k * chunkFrames, f1 = std::min(nFrames, f0 + chunkFrames);
    st = decode_jobs(dIn + (k % 3) * inSlot, ends[f1 - 1] - starts[f0], frameOff_.as<uint64_t>() + 2 * f0, dOut + (k % 2) * outSlot,
                     outOff_.as<uint64_t>() + f0, expect_.as<uint32_t>() + f0, (uint32_t)(f1 - f0), frameSize, 2, 0);
    if (st.zra) { P.fail(); break; }
    P.bump(P.computed);
  }
  up.join(); down.join();
  if (st.zra == kZStdError && st.zstd != 1 && st.zstd != 64) { *fallBack = true; return ok(); }   // a frame failed: the one-piece path reports it
  if (!st.zra && P.failed) st = zerr(1);
  if (st.zra) (void)hipDeviceSynchronize();
  return st;
}

// ------------------------------------------------------------------------------------------------
// The one-piece path behind DecompressBuffer and DecompressRA: frames walked on the host, compressed span and answer in host memory.
Status Engine::decode_host(const uint8_t* hSpan, size_t spanSize, const std::vector<uint64_t>& starts, const std::vector<uint64_t>& ends,
                           uint32_t frameSize, uint64_t total, uint8_t* hOut, size_t skip, size_t size, bool wholeArchive) {
  HIPCHK(hipSetDevice(device_));
  const uint32_t nFrames = (uint32_t)starts.size();
  if (nFrames == 0) return ok();
  std::vector<uint64_t> se((size_t)nFrames * 2), oo(nFrames);
  std::vector<uint32_t> ex(nFrames);
  for (uint32_t i = 0; i < nFrames; i++) {
    se[2 * (size_t)i] = starts[i]; se[2 * (size_t)i + 1] = ends[i];
    const uint64_t o = (uint64_t)i * frameSize;
    oo[i] = wholeArchive ? std::min<uint64_t>(o, total) : o;        // a slot past the declared size has no room and no address of its own
    ex[i] = (uint32_t)zra_dev::frame_expect(i, frameSize, total);
  }
  if (wholeArchive && skip == 0 && frameSize && (size_t)nFrames >= 2 * std::max<size_t>(1, host_chunk_bytes() / frameSize) && size == std::min<uint64_t>(total, (uint64_t)nFrames * frameSize)) {
    bool fallBack = false;
    Status s = decode_host_pipelined(hSpan, starts, ends, frameSize, total, hOut, &fallBack);
    if (!fallBack) return s;
  }
  // ---- small calls (round 6; the reference's own calling convention, one query of a few KiB through ZraDecompressRA): the four pageable
  // host-to-device copies (each staged and waited for by the runtime), the synchronisation behind them and the pageable copy back were
  // ~40 % of such a call. Here the job arrays and the compressed span travel in ONE copy from page-locked memory, the kernel is queued
  // straight behind it, and the answer comes back through page-locked memory: one copy in, one launch, one copy out, one wait.
  constexpr size_t kSmallSpan = 768u << 10, kSmallOut = 1u << 20, kSmallJobs = 16;
  if (!wholeArchive && nFrames <= kSmallJobs && spanSize <= kSmallSpan && size <= kSmallOut && (uint64_t)nFrames * frameSize <= (64ull << 20)) {
    const size_t metaBytes = (size_t)kSmallJobs * (16 + 8 + 4 + 4);                   // frameOff pairs, outOff, expect (padded)
    const size_t inBytes = metaBytes + ((spanSize + 63) & ~(size_t)63);
    if (!pinSmall_) {
      void* pq = nullptr;
      if (hipHostMalloc(&pq, metaBytes + kSmallSpan + 64 + kSmallOut + 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pq = nullptr; }
      pinSmall_ = (uint8_t*)pq;
    }
    if (pinSmall_ && hostIn_.reserve(metaBytes + kSmallSpan + 128) && hostOut_.reserve((size_t)nFrames * frameSize + 64)) {
      uint8_t* const hp = pinSmall_;
      std::memcpy(hp, se.data(), se.size() * 8);
      std::memcpy(hp + kSmallJobs * 16, oo.data(), (size_t)nFrames * 8);
      std::memcpy(hp + kSmallJobs * 24, ex.data(), (size_t)nFrames * 4);
      std::memcpy(hp + metaBytes, hSpan, spanSize);
      uint8_t* const dIn = hostIn_.as<uint8_t>();
      HIPCHK(hipMemcpyAsync(dIn, hp, inBytes, hipMemcpyHostToDevice, stream_));
      Status s = decode_jobs(dIn + metaBytes, spanSize, (const uint64_t*)dIn, hostOut_.as<uint8_t>(), (const uint64_t*)(dIn + kSmallJobs * 16),
                             (const uint32_t*)(dIn + kSmallJobs * 24), nFrames, frameSize, 2, 0);
      if (s.zra) return s;
      if (skip + size > (uint64_t)nFrames * frameSize) return {kOutOfBounds, 0};
      if (size) {
        uint8_t* const ho = pinSmall_ + metaBytes + kSmallSpan + 64;
        HIPCHK(hipMemcpyAsync(ho, hostOut_.as<uint8_t>() + skip, size, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        std::memcpy(hOut, ho, size);
      }
      return ok();
    }
  }
  // whole-archive mode never writes at or beyond `total` (slots past it have no room), whatever the header's frameSize claims
  if (!hostIn_.reserve(spanSize + 64) || !hostOut_.reserve((wholeArchive ? (size_t)total : (size_t)nFrames * frameSize) + 64) || !frameOff_.reserve(se.size() * 8) ||
      !outOff_.reserve((size_t)nFrames * 8) || !expect_.reserve((size_t)nFrames * 4))   // (all five before the first copy is queued)
    return zerr(64);
  HIPCHK(hipMemcpyAsync(hostIn_.p, hSpan, spanSize, hipMemcpyHostToDevice, stream_));
  { Status st = upload_jobs(se, oo, ex); if (st.zra) return st; }
  Status s = decode_jobs(hostIn_.as<uint8_t>(), spanSize, frameOff_.as<uint64_t>(), hostOut_.as<uint8_t>(), outOff_.as<uint64_t>(),
                         expect_.as<uint32_t>(), nFrames, frameSize, 2, wholeArchive ? total : 0);
  if (s.zra) return s;
  if (wholeArchive && lastProducedTotal_ != ~0ull) {
    // frames that regenerated another size than the header's frameSize (corrupted or foreign archive): the sequential tail has packed
    // them back to back like the reference's one multi-frame call (zra.cpp:249) — what it wrote, less or MORE than the nominal slots
    // add up to (a frameSize field damaged downwards), is what reaches the caller; never more than the declared size
    const uint64_t have = std::min<uint64_t>(total, lastProducedTotal_);
    size = have > skip ? (size_t)(have - skip) : 0;
  } else if (skip + size > (uint64_t)nFrames * frameSize) return {kOutOfBounds, 0};
  if (size) HIPCHK(hipMemcpyAsync(hOut, hostOut_.as<uint8_t>() + skip, size, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  return ok();
}

}  // namespace zra_eng
