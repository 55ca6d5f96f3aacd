// zra_amd — the drop-in boundary: C++ API (include/zra.hpp) and the 29-symbol C ABI (include/zra.h)
// implemented on the HIP engine. Host-pointer semantics, status codes, exceptions and the documented quirks
// follow the reference (source/zra.cpp); the per-frame codec work is never done on the CPU here.
#include "zra.hpp"
#include "zra.h"
#include "zra_hip.h"
#include "zra_engine.h"
#include "zra_archive.h"
#include "zra_scan.h"
#include "zra_format.h"
#include "zra_env.h"
#include "zra_pattern_expr.h"
#include "zra_where.h"
#include "zra_regex.h"

#include <functional>
#include <atomic>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <vector>

using zra_eng::Engine;
using zra_eng::kRecGrep, zra_eng::kRecGrepWhere, zra_eng::kRecGrepRegex, zra_eng::kRecExtract, zra_eng::kRecExtractRegex;   // the record scans' entry points fill a RecordCall
namespace fmt = zra_fmt;

namespace {
// The reference's free functions are re-entrant (a fresh zstd context per call, zra.cpp:209,248,271). Here a call needs an
// engine (device streams + scratch), so the free functions and the streaming classes borrow one from a small pool: concurrent
// callers get different engines (up to ZRA_ENGINES, default 4, created on demand) and only wait when all of them are busy.
class EnginePool {
 public:
  class Lease {
   public:
    Lease(EnginePool& p, Engine* e) : pool_(p), e_(e) {}
    ~Lease() { pool_.give_back(e_); }
    Lease(const Lease&) = delete; Lease& operator=(const Lease&) = delete;
    Engine* operator->() const { return e_; }
   private:
    EnginePool& pool_; Engine* e_;
  };
  Engine* take() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      if (!idle_.empty()) { Engine* e = idle_.back(); idle_.pop_back(); return e; }
      if (created_ < limit()) {
        created_++;
        lk.unlock();
        const int dev = zra_env::env_int("ZRA_DEVICE", 0);
        Engine* e = nullptr;
        zra_eng::Status st = Engine::create(&e, dev);
        if (st.zra) {
          lk.lock(); created_--; cv_.notify_one();
          throw zra::Exception(zra::StatusCode::ZStdError, st.zstd ? st.zstd : 1);   // no GPU: fail loudly, no CPU fallback
        }
        return e;
      }
      cv_.wait(lk);
    }
  }
  // Scratch is grow-only per engine (a level-9 compression can leave tens of GiB behind); the pool as a whole keeps at most
  // ZRA_SCRATCH_CAP_GIB (default 48) of it between calls: an engine that comes back while the process is above the cap hands its
  // scratch to the device again, and so do the idle ones until the total fits.
  void give_back(Engine* e) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (zra_eng::scratch_bytes_in_use() > cap()) {
        (void)e->release_scratch();
        for (Engine* i : idle_) { if (zra_eng::scratch_bytes_in_use() <= cap()) break; (void)i->release_scratch(); }
      }
      idle_.push_back(e);
    }
    cv_.notify_one();
  }
 private:
  static int limit() {
    static const int n = [] { const int v = zra_env::env_int("ZRA_ENGINES", 4); return v < 1 ? 1 : v > 64 ? 64 : v; }();
    return n;
  }
  static uint64_t cap() {
    static const uint64_t c = [] { const long long v = zra_env::env_i64("ZRA_SCRATCH_CAP_GIB", 48); return (uint64_t)(v < 1 ? 1 : v) << 30; }();
    return c;
  }
  std::mutex mu_; std::condition_variable cv_;
  std::vector<Engine*> idle_; int created_ = 0;
};
EnginePool g_pool;
#define LEASE_ENGINE(name) EnginePool::Lease name(g_pool, g_pool.take())

void check(zra_eng::Status s) { if (s.zra) throw zra::Exception(static_cast<zra::StatusCode>(s.zra), s.zstd); }

const char* zstd_error_string(int code) {   // ZSTD_getErrorString of zstd 1.4.9, every code of its ZSTD_ErrorCode enum (pinned by tests/test_boundary.py)
  switch (code) {
    case 0: return "No error detected";
    case 1: return "Error (generic)";
    case 10: return "Unknown frame descriptor";
    case 12: return "Version not supported";
    case 14: return "Unsupported frame parameter";
    case 16: return "Frame requires too much memory for decoding";
    case 20: return "Corrupted block detected";
    case 22: return "Restored data doesn't match checksum";
    case 30: return "Dictionary is corrupted";
    case 32: return "Dictionary mismatch";
    case 34: return "Cannot create Dictionary from provided samples";
    case 40: return "Unsupported parameter";
    case 42: return "Parameter is out of bound";
    case 44: return "tableLog requires too much memory : unsupported";
    case 46: return "Unsupported max Symbol Value : too large";
    case 48: return "Specified maxSymbolValue is too small";
    case 60: return "Operation not authorized at current processing stage";
    case 62: return "Context should be init first";
    case 64: return "Allocation error : not enough memory";
    case 66: return "workSpace buffer is not large enough";
    case 70: return "Destination buffer is too small";
    case 72: return "Src size is incorrect";
    case 74: return "Operation on NULL destination buffer";
    case 100: return "Frame index is too large";
    case 102: return "An I/O error occurred when reading/seeking";
    case 104: return "Destination buffer is wrong";
    case 105: return "Source buffer is wrong";
    default: return "Unspecified error code";
  }
}

// Walk the zstd frames of a body on the host (block headers only), the way one ZSTD_decompressDCtx call over the
// whole body does (zra.cpp:249): skippable frames are skipped, the seek table is NOT consulted.
// offs receives frame boundaries (n+1 entries for n data frames, contiguous runs only: a skippable frame in the
// middle is reported through `gaps`). Returns 0 or the zstd error code of the walk.
// *brokenAt: start of the frame inside which a header/block walk error occurred (its magic was fine), else ~0: the sequential
// reference would still decode that frame's leading blocks before it reaches the broken part, so the caller hands the device the
// span [brokenAt, n) as a last job and lets the decoder report whichever error comes first in block order.
int walk_frames(const zra::u8* body, size_t n, std::vector<uint64_t>& starts, std::vector<uint64_t>& ends, uint64_t* brokenAt) {
  size_t pos = 0; bool more = false;
  *brokenAt = ~0ull;
  while (n - pos >= 5) {
    uint32_t magic = fmt::rd32(body + pos);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
      if (n - pos < 8) return 72;
      size_t skip = (size_t)fmt::rd32(body + pos + 4) + 8;
      if (skip > n - pos) return 72;
      pos += skip; continue;
    }
    // ZSTD_decompressFrame + ZSTD_getFrameHeader_advanced of 1.4.9, in their order: the size checks come before the magic number
    const size_t f0 = pos;
    if (n - pos < 6 + 3) return 72;
    unsigned fhd = body[pos + 4], did = fhd & 3, ss = (fhd >> 5) & 1, fcs = fhd >> 6;
    size_t hs = 5 + !ss + (did == 3 ? 4 : did) + (fcs == 0 ? ss : fcs == 1 ? 2 : fcs == 2 ? 4 : 8);
    if (n - pos < hs + 3) return 72;
    if (magic != 0xFD2FB528u) return more ? 72 : 10;
    // the header checks made before any block is looked at (same order as the device decoder)
    if (fhd & 8) { *brokenAt = f0; return 14; }
    if (!ss) {
      unsigned b = body[pos + 5], wl = 10 + (b >> 3);
      if (wl > 31) { *brokenAt = f0; return 16; }
    }
    {
      const zra::u8* q = body + pos + 5 + !ss;
      uint32_t dict = did == 0 ? 0u : did == 1 ? (uint32_t)q[0] : did == 2 ? (uint32_t)(q[0] | (q[1] << 8)) : fmt::rd32(q);
      if (dict) { *brokenAt = f0; return 32; }
    }
    pos += hs;
    for (;;) {
      if (n - pos < 3) { *brokenAt = f0; return 72; }
      uint32_t bh = (uint32_t)body[pos] | ((uint32_t)body[pos + 1] << 8) | ((uint32_t)body[pos + 2] << 16);
      pos += 3;
      unsigned type = (bh >> 1) & 3; size_t bs = type == 1 ? 1 : (bh >> 3);
      if (type == 3) { *brokenAt = f0; return 20; }
      if (bs > n - pos) { *brokenAt = f0; return 72; }
      pos += bs;
      if (bh & 1) break;
    }
    if (fhd & 4) { if (n - pos < 4) { *brokenAt = f0; return 22; } pos += 4; }
    starts.push_back(f0); ends.push_back(pos);
    more = true;
  }
  return pos == n ? 0 : 72;
}
}  // namespace

namespace {
// Opt-in integrity options (default 0 = reference-compatible, quirks included). Set through ZraHipSetOptions.
std::atomic<uint32_t> g_options{0};
enum : uint32_t { kOptVerifyHeaderCrc = 1, kOptInclusiveRaBound = 2, kOptStoreMetaInMemory = 4, kOptRaWholeFrames = 8 };
}  // namespace

namespace zra {
  // ------------------------------------------------------------------ errors (zra.cpp:46-86)
  Exception::Exception(StatusCode code, i32 zstdCode) : code(code), zstdCode(zstdCode) {}

  const char* Exception::GetExceptionString(StatusCode code) {
    static const char* const text[] = {
        "The operation was successful",
        "An error was returned by ZStandard",
        "This archive was compressed using a newer version of ZRA",
        "The header in the supplied buffer was invalid",
        "The header hasn't been fully written before being accessed",
        "The specified offset and size are past the data contained within the buffer",
        "The output buffer is too small to contain the output",
        "The compressed output's size exceeds the maximum limit",
        "The input size is not divisible by the frame size and nor is it the final frame",
    };
    auto i = static_cast<unsigned>(code);
    return i < sizeof(text) / sizeof(text[0]) ? text[i] : "An unknown error has occurred";
  }

  const char* Exception::what() const noexcept {
    if (code != StatusCode::ZStdError) return GetExceptionString(code);
    static thread_local std::string reason;
    reason = std::string(GetExceptionString(code)) + ": " + zstd_error_string(zstdCode);
    return reason.c_str();
  }

  u16 GetVersion() { return fmt::kVersion; }

  // ------------------------------------------------------------------ Header (zra.cpp:141-187)
  Header::Header(const std::function<void(size_t, size_t, void*)>& rf) : readFunction(rf) {
    u8 fixed[fmt::kFixedSize];
    readFunction(0, sizeof(fixed), fixed);
    zra_eng::HeaderInfo h{};
    int e = zra_eng::parse_fixed_header(fixed, &h);
    if (e == zra_eng::kHeaderInvalid) throw Exception(StatusCode::HeaderInvalid);
    version = h.version; size = h.size; uncompressedSize = h.uncompressedSize; frameSize = h.frameSize;
    metaOffset = h.metaOffset; metaSize = h.metaSize; seekTableOffset = h.seekTableOffset; seekTableSize = h.seekTableSize;
    if (e) throw Exception(static_cast<StatusCode>(e));
    if (g_options.load() & kOptVerifyHeaderCrc) {
      // the reference writes the CRC-32 (zra.cpp:128-133,231,346) and never checks it; opt-in check on open
      if (size < fmt::kFixedSize) throw Exception(StatusCode::HeaderInvalid);
      Buffer rest(size - fmt::kFixedSize);
      if (!rest.empty()) readFunction(fmt::kFixedSize, rest.size(), rest.data());
      if (fmt::header_hash(fixed, rest.data()) != fmt::rd32(fixed + 14)) throw Exception(StatusCode::HeaderInvalid);
    }
  }

  // The reference captures the view by reference (dangling for temporaries, zra.cpp:165); we keep a copy of the
  // (pointer, size) pair instead — same behaviour whenever the reference's is defined.
  Header::Header(const BufferView& buffer)
      : Header([buffer](size_t offset, size_t readSize, void* out) {
          if ((offset + readSize) >= buffer.size) throw Exception(StatusCode::OutOfBoundsAccess);   // ">=" as in zra.cpp:166
          std::memcpy(out, buffer.data + offset, readSize);
        }) {
    if (buffer.size < size) throw Exception(StatusCode::OutOfBoundsAccess);
  }

  Buffer Header::GetSeekTable() const { Buffer t(seekTableSize); readFunction(seekTableOffset, seekTableSize, t.data()); return t; }
  void Header::GetMetadata(const BufferView& buffer) const { readFunction(metaOffset, metaSize, buffer.data); }
  Buffer Header::GetMetadata() const { Buffer m(metaSize); GetMetadata(m); return m; }

  // ------------------------------------------------------------------ in-memory calls (zra.cpp:189-302)
  size_t GetOutputBufferSize(size_t inputSize, u32 frameSize, u32 metaSize) {
    u32 tableSize = fmt::table_size(inputSize, frameSize);
    return fmt::kFixedSize + metaSize + (size_t)tableSize * fmt::kEntrySize + fmt::compress_bound(frameSize) * (size_t)(tableSize - 1);
  }

  size_t CompressBuffer(const BufferView& input, const BufferView& output, i8 level, u32 frameSize, bool checksum, const BufferView& meta) {
    u32 tableSize = fmt::table_size(input.size, frameSize);
    size_t need = fmt::kFixedSize + (size_t)tableSize * fmt::kEntrySize + fmt::compress_bound(frameSize) * (size_t)(tableSize - 1);
    const bool storeMeta = meta.size && (g_options.load() & kOptStoreMetaInMemory);
    if (storeMeta) need += meta.size;
    if (output.size < need) throw Exception(StatusCode::OutputBufferTooSmall);   // meta not counted, zra.cpp:196
    LEASE_ENGINE(eng);
    size_t outSize = 0;
    check(eng->compress_host(input.data, input.size, output.data, &outSize, level, frameSize, checksum));
    if (storeMeta) {
      // opt-in fix of the quirk below: the archive the streaming Compressor would write (meta stored, table behind it)
      std::memmove(output.data + fmt::kFixedSize + meta.size, output.data + fmt::kFixedSize, outSize - fmt::kFixedSize);
      std::memcpy(output.data + fmt::kFixedSize, meta.data, meta.size);
      fmt::write_fixed(output.data, input.size, tableSize, frameSize, (u32)meta.size);
      fmt::wr32(output.data + 14, fmt::header_hash(output.data, output.data + fmt::kFixedSize));
      outSize += meta.size;
    } else if (meta.size) {
      // reference quirk (zra.cpp:202-205,231): meta is counted in headerSize/metaSize but never stored, the table stays at
      // +38, and the CRC then runs meta.size bytes into the body. Reproduced bit-for-bit.
      fmt::write_fixed(output.data, input.size, tableSize, frameSize, (u32)meta.size);
      fmt::wr32(output.data + 14, fmt::header_hash(output.data, output.data + fmt::kFixedSize));
    }
    return outSize;
  }

  Buffer CompressBuffer(const BufferView& buffer, i8 level, u32 frameSize, bool checksum, const BufferView& meta) {
    Buffer output(GetOutputBufferSize(buffer.size, frameSize, (g_options.load() & kOptStoreMetaInMemory) ? (u32)meta.size : 0));   // meta not counted, zra.cpp:237
    output.resize(CompressBuffer(buffer, output, level, frameSize, checksum, meta));
    output.shrink_to_fit();
    return output;
  }

  void DecompressBuffer(const BufferView& input, const BufferView& output) {
    Header header(input);
    if (output.size < header.uncompressedSize) throw Exception(StatusCode::OutputBufferTooSmall);
    // one multi-frame zstd call over the whole body in the reference (zra.cpp:249): walk the frames on the host,
    // decode them all in parallel on the device.
    const u8* body = input.data + header.size; const size_t bodySize = input.size - header.size;
    std::vector<uint64_t> starts, ends;
    uint64_t brokenAt = ~0ull;
    int walkErr = walk_frames(body, bodySize, starts, ends, &brokenAt);
    if (walkErr && brokenAt != ~0ull) { starts.push_back(brokenAt); ends.push_back(bodySize); }
    LEASE_ENGINE(eng);
    // frames complete before a walk error are still decoded (their errors come first, as in the sequential reference)
    const u64 avail = std::min<u64>(header.uncompressedSize, (u64)starts.size() * header.frameSize);
    zra_eng::Status s = eng->decode_host(body, bodySize, starts, ends, header.frameSize, header.uncompressedSize, output.data, 0, (size_t)avail, true);
    check(s);
    if (walkErr) throw Exception(StatusCode::ZStdError, walkErr);
  }

  Buffer DecompressBuffer(const BufferView& buffer) {
    Buffer output(fmt::rd64(buffer.data + 18));   // read before validation, as zra.cpp:253
    DecompressBuffer(buffer, output);
    return output;
  }

  namespace {
    // frames [first, last) of the seek table -> decode -> copy [skip, skip+size) into out (the 3 phases of zra.cpp:279-295
    // collapse to this on a device that decodes all touched frames at once)
    void ra_decode(const u8* table, size_t tableBytes, const u8* span, u64 spanAvail, u64 spanBase, u64 firstIdx, u64 count, const Header& header,
                   u8* out, size_t skip, size_t size) {
      // an inconsistent header (uncompressedSize beyond what the seek table covers) would index past the table: the reference reads
      // whatever lies there (zra.cpp:267-268); here it is a HeaderInvalid. Entries that run backwards or past the bytes the caller
      // handed over are what zstd reports as srcSize_wrong.
      if ((firstIdx + count + 1) * fmt::kEntrySize > tableBytes) throw Exception(StatusCode::HeaderInvalid);
      std::vector<uint64_t> starts(count), ends(count);
      for (u64 i = 0; i < count; i++) {
        const u64 a = fmt::entry_get(table + (firstIdx + i) * 5), b = fmt::entry_get(table + (firstIdx + i + 1) * 5);
        if (a < spanBase || b < a || b - spanBase > spanAvail) throw Exception(StatusCode::ZStdError, 72);
        starts[i] = a - spanBase; ends[i] = b - spanBase;
      }
      const u64 spanSize = count ? ends[count - 1] : 0;
      // every touched frame but possibly the archive's last regenerates frameSize bytes
      const u64 firstByte = firstIdx * (u64)header.frameSize;
      const u64 total = std::min<u64>(count * (u64)header.frameSize, header.uncompressedSize > firstByte ? header.uncompressedSize - firstByte : 0);
      LEASE_ENGINE(eng);
      check(eng->decode_host(span, spanSize, starts, ends, header.frameSize, total, out, skip, size));
    }
  }

  namespace {
    // One ZSTD_decompressDCtx call of the reference over `n` source bytes into `cap` bytes of destination, with libzstd's multi-frame
    // semantics (zero, one or several concatenated frames packed back to back, skippable frames skipped, errors in frame order,
    // dstSize_tooSmall against the whole destination) — the machinery of DecompressBuffer on a piece of the body. Returns the bytes
    // regenerated.
    size_t multiframe_call(const u8* src, size_t n, u8* dst, size_t cap, u32 slotSize) {
      std::vector<uint64_t> starts, ends;
      uint64_t brokenAt = ~0ull;
      const int walkErr = walk_frames(src, n, starts, ends, &brokenAt);
      if (walkErr && brokenAt != ~0ull) { starts.push_back(brokenAt); ends.push_back(n); }
      size_t produced = 0;
      if (!starts.empty()) {
        LEASE_ENGINE(eng);
        const u64 avail = std::min<u64>(cap, (u64)starts.size() * slotSize);
        check(eng->decode_host(src, n, starts, ends, slotSize, cap, dst, 0, (size_t)avail, true));
        const uint64_t packed = eng->last_produced_total();
        produced = packed == ~0ull ? (size_t)avail : (size_t)std::min<u64>(cap, packed);
      }
      if (walkErr) throw Exception(StatusCode::ZStdError, walkErr);
      return produced;
    }

    // The three zstd calls of the reference's random access, literally (zra.cpp:279-295 and :400-414): taken when the one-pass device
    // decode of the touched frames reports anything but success — a seek table, frameSize or uncompressedSize that does not describe
    // the frames (damaged or foreign archive). What the reference then returns depends on what each of ITS calls sees: a span with two
    // frames in it overflows the frameSize buffer (dstSize_tooSmall), one that starts inside a frame has no magic number
    // (prefix_unknown), a frame shorter than frameSize is simply copied from a zero-filled buffer. `span` = the body bytes from
    // the caller holds (the whole body for the in-memory call, the bytes read from entry[q] on for the streaming class); entries
    // that run backwards or leave those bytes are srcSize_wrong here (the reference reads out of bounds).
    void ra_exact(const u8* table, u64 q, u64 rem, u64 quot2, u64 rem2, const u8* span, u64 spanAvail, u64 spanBase, const Header& header, u8* out, size_t outSize, size_t size) {
      const u64 last = quot2 + (rem2 ? 1 : 0);
      auto rel = [&](u64 i) -> u64 {                      // entry -> position inside `span` (whose first byte is body offset spanBase)
        const u64 e = fmt::entry_get(table + (q + i) * 5);
        if (e < spanBase || e - spanBase > spanAvail) throw Exception(StatusCode::ZStdError, 72);
        return e - spanBase;
      };
      auto piece = [&](u64 a, u64 b) -> std::pair<const u8*, size_t> {
        const u64 ra = rel(a), rb = rel(b);
        if (rb < ra) throw Exception(StatusCode::ZStdError, 72);
        return {span + ra, (size_t)(rb - ra)};
      };
      std::vector<u8> frameBuffer;
      if (rem || rem2) frameBuffer.assign(header.frameSize, 0);
      size_t done = 0; u64 first = 0;
      if (rem) {
        auto p = piece(0, 1);
        multiframe_call(p.first, p.second, frameBuffer.data(), frameBuffer.size(), header.frameSize);
        const size_t minSize = std::min<size_t>(size, (size_t)(header.frameSize - rem));
        std::memcpy(out, frameBuffer.data() + rem, minSize);
        done += minSize; first = 1;
      }
      if (done < size) {
        auto p = piece(first, rem2 ? last - 1 : last);
        done += multiframe_call(p.first, p.second, out + done, outSize - done, header.frameSize);
      }
      if (done < size && rem2) {
        auto p = piece(last - 1, last);
        multiframe_call(p.first, p.second, frameBuffer.data(), frameBuffer.size(), header.frameSize);
        // frames that regenerate less than the header's frameSize (damaged frames, an inflated frameSize / uncompressedSize) leave more
        // than one frame buffer to fill here: the reference copies past its buffer and reports success (zra.cpp:293; the bytes are
        // whatever its heap held). Same status here, the bytes behind the buffer's end defined: zero.
        const size_t want = size - done, have = std::min(want, frameBuffer.size());
        std::memcpy(out + done, frameBuffer.data(), have);
        std::memset(out + done + have, 0, want - have);
      }
    }
    // infrastructure failures (allocation, launch) are not statuses of the archive: they are not retried
    bool archive_status(const Exception& e) { return e.code == StatusCode::ZStdError && e.zstdCode != 1 && e.zstdCode != 64; }
  }

  void DecompressRA(const BufferView& input, const BufferView& output, size_t offset, size_t size) {
    Header header(input);
    const bool inclusive = g_options.load() & kOptInclusiveRaBound;      // opt-in: the last byte becomes reachable, as in Decompressor
    if (inclusive ? offset + size > header.uncompressedSize : offset + size >= header.uncompressedSize)
      throw Exception(StatusCode::OutOfBoundsAccess);   // ">=", zra.cpp:260
    if (output.size < size) throw Exception(StatusCode::OutputBufferTooSmall);
    const u64 q = offset / header.frameSize, r = offset % header.frameSize;
    const u64 n = (r + size) / header.frameSize, t = (r + size) % header.frameSize;
    const u64 count = n + (t ? 1 : 0);
    if (size == 0 || count == 0) return;
    if ((u64)header.seekTableOffset + header.seekTableSize > header.size) throw Exception(StatusCode::HeaderInvalid);
    const u8* table = input.data + header.seekTableOffset;
    if ((q + count + 1) * fmt::kEntrySize > header.seekTableSize) throw Exception(StatusCode::HeaderInvalid);
    const u64 base = fmt::entry_get(table + q * 5);
    const u64 bodyAvail = input.size - header.size;
    if (base > bodyAvail) throw Exception(StatusCode::ZStdError, 72);
    try {
      ra_decode(table, header.seekTableSize, input.data + header.size + base, bodyAvail - base, base, q, count, header, output.data, r, size);
    } catch (const Exception& e) {
      if (!archive_status(e)) throw;
      ra_exact(table, q, r, n, t, input.data + header.size, bodyAvail, 0, header, output.data, output.size, size);
    }
  }

  Buffer DecompressRA(const BufferView& buffer, size_t offset, size_t size) {
    Buffer output(size);
    DecompressRA(buffer, output, offset, size);
    return output;
  }

  // ------------------------------------------------------------------ Compressor (zra.cpp:304-365)
  struct Compressor::Impl {
    i8 level; bool checksum;
    u32 frameSize, tableSize;
    Buffer header;
    size_t entryIndex{0}, metaSize{0};
    u64 outputOffset{0};
    u8* entry(size_t i) { return header.data() + fmt::kFixedSize + metaSize + i * fmt::kEntrySize; }
  };

  Compressor::Compressor(size_t size, i8 level, u32 frameSize, bool checksum, const BufferView& meta) : impl(std::make_shared<Impl>()) {
    impl->level = level; impl->checksum = checksum; impl->frameSize = frameSize;
    impl->tableSize = fmt::table_size(size, frameSize);
    impl->metaSize = meta.size;
    impl->header.resize(fmt::kFixedSize + meta.size + (size_t)impl->tableSize * fmt::kEntrySize);
    fmt::write_fixed(impl->header.data(), size, impl->tableSize, frameSize, (u32)meta.size);
    if (meta.data) std::memcpy(impl->header.data() + fmt::kFixedSize, meta.data, meta.size);
  }

  size_t Compressor::GetOutputBufferSize(size_t inputSize) const {
    return fmt::compress_bound(impl->frameSize) * ((inputSize / impl->frameSize) + ((inputSize % impl->frameSize) ? 1 : 0));
  }

  size_t Compressor::Compress(const BufferView& input, const BufferView& output) {
    Impl& m = *impl;
    if (output.size < GetOutputBufferSize(input.size)) throw Exception(StatusCode::OutputBufferTooSmall);
    // the reference measures the entry index from +38 even with metadata present (zra.cpp:324); kept
    const size_t refIndex = m.entryIndex + m.metaSize / fmt::kEntrySize;
    if (input.size % m.frameSize && (refIndex + (input.size / m.frameSize) + 2) < m.tableSize) throw Exception(StatusCode::InputFrameSizeMismatch);
    size_t bodySize = 0;
    std::vector<uint64_t> sizes;
    if (input.size) {
      LEASE_ENGINE(eng);
      check(eng->compress_frames_host(input.data, input.size, output.data, sizes, &bodySize, m.level, m.frameSize, m.checksum));
    }
    for (uint64_t c : sizes) {
      fmt::entry_put(m.entry(m.entryIndex++), m.outputOffset);
      m.outputOffset += c;
    }
    if (input.size % m.frameSize) m.frameSize = (u32)(input.size % m.frameSize);   // member shrinks on the short last frame, zra.cpp:330
    if (m.outputOffset >= fmt::kMaxCompressedSize) throw Exception(StatusCode::CompressedSizeTooLarge);
    if (m.entryIndex == (size_t)m.tableSize - 1) {
      fmt::entry_put(m.entry(m.entryIndex++), m.outputOffset);
      fmt::wr32(m.header.data() + 14, fmt::header_hash(m.header.data(), m.header.data() + fmt::kFixedSize));
    }
    return bodySize;
  }

  void Compressor::Compress(const BufferView& input, Buffer& output) {
    output.resize(GetOutputBufferSize(input.size));
    output.resize(Compress(input, BufferView(output)));
  }

  const Buffer& Compressor::GetHeader() {
    if (impl->entryIndex == impl->tableSize) return impl->header;
    throw Exception(StatusCode::HeaderIncomplete);
  }
  size_t Compressor::GetHeaderSize() { return impl->header.size(); }

  // ------------------------------------------------------------------ Decompressor (zra.cpp:367-424)
  Decompressor::Decompressor(const std::function<void(size_t, size_t, void*)>& rf, size_t maxCacheSize)
      : readFunction(rf), header(rf), seekTable(header.GetSeekTable()), maxCacheSize(maxCacheSize) {}

  void Decompressor::Decompress(size_t offset, size_t size, const BufferView& output) {
    if (offset + size > header.uncompressedSize) throw Exception(StatusCode::OutOfBoundsAccess);   // ">" here, zra.cpp:370
    if (output.size < size) throw Exception(StatusCode::OutputBufferTooSmall);
    const u64 q = offset / header.frameSize, r = offset % header.frameSize;
    const u64 n = (r + size) / header.frameSize, t = (r + size) % header.frameSize;
    const u64 count = n + (t ? 1 : 0);
    const u8* table = seekTable.data();
    if ((q + count + 1) * fmt::kEntrySize > seekTable.size()) throw Exception(StatusCode::HeaderInvalid);
    const u64 base = fmt::entry_get(table + q * 5);
    if (fmt::entry_get(table + (q + count) * 5) < base) throw Exception(StatusCode::ZStdError, 72);
    const u64 compressedSize = fmt::entry_get(table + (q + count) * 5) - base;
    Buffer own;
    Buffer& in = compressedSize > maxCacheSize ? own : cache;
    in.resize(compressedSize);
    readFunction(header.size + base, compressedSize, in.data());
    if (size == 0 || count == 0) return;
    try {
      ra_decode(table, seekTable.size(), in.data(), in.size(), base, q, count, header, output.data, r, size);
    } catch (const Exception& e) {
      if (!archive_status(e)) throw;
      ra_exact(table, q, r, n, t, in.data(), in.size(), base, header, output.data, output.size, size);
    }
  }
  void Decompressor::Decompress(size_t offset, size_t size, Buffer& output) { output.resize(size); Decompress(offset, size, BufferView(output)); }
  Buffer Decompressor::Decompress(size_t offset, size_t size) { Buffer b; Decompress(offset, size, b); return b; }

  // ------------------------------------------------------------------ FullDecompressor (zra.cpp:426-436)
  FullDecompressor::FullDecompressor(const std::function<void(size_t, size_t, void*)>& rf)
      : readFunction(rf), header(rf), seekTable(header.GetSeekTable()) {}

  // Frames decoded ahead of the caller. The reference reads and decodes exactly the frames one call returns (zra.cpp:428-435); with the
  // tool's 10 MB buffers that is a 160-frame device batch per call. Here a call that finds nothing decoded fetches and decodes a
  // window of ZRA_STREAM_AHEAD_MIB (default 256) in one go and the following calls are served from it. Same bytes, fewer and larger
  // readFunction calls. If anything in the window fails, the window is dropped and the call decodes exactly its own frames, so an
  // error surfaces at the call where the reference raises it.
  struct FullDecompressor::Ahead {
    Buffer data;                 // decoded frames [first, last) of the seek table
    size_t first{0}, last{0};
    bool disabled{false};
  };

  size_t FullDecompressor::Decompress(const BufferView& output) {
    if (output.size < header.frameSize) throw Exception(StatusCode::OutputBufferTooSmall);
    const size_t lastIndex = seekTable.size() / fmt::kEntrySize - 1;
    const size_t stop = std::min(lastIndex, entryIndex + output.size / header.frameSize);
    const u8* table = seekTable.data();
    const size_t first = entryIndex, count = stop - entryIndex;
    const u64 firstByte = (u64)first * header.frameSize;
    const size_t produced = count ? (size_t)std::min<u64>((u64)count * header.frameSize, header.uncompressedSize > firstByte ? header.uncompressedSize - firstByte : 0) : 0;
    const size_t aheadBytes = (size_t)zra_env::env_i64("ZRA_STREAM_AHEAD_MIB", 256) << 20;   // (read per call: tests change it)
    if (!ahead) ahead = std::make_shared<Ahead>();
    Ahead& A = *ahead;
    if (count && aheadBytes && !A.disabled && header.frameSize) {
      if (!(first >= A.first && stop <= A.last)) {
        // decode a window that starts at this call's first frame
        const size_t want = std::max<size_t>(count, aheadBytes / header.frameSize);
        const size_t wStop = std::min(lastIndex, first + want);
        bool good = false;
        try {
          const u64 base = fmt::entry_get(table + first * 5), end = fmt::entry_get(table + wStop * 5);
          if (end >= base && wStop > stop) {
            cache.resize(end - base);
            readFunction(header.size + base, cache.size(), cache.data());
            const size_t bytes = (size_t)std::min<u64>((u64)(wStop - first) * header.frameSize, header.uncompressedSize > firstByte ? header.uncompressedSize - firstByte : 0);
            A.data.resize(bytes);
            ra_decode(table, seekTable.size(), cache.data(), cache.size(), base, first, wStop - first, header, A.data.data(), 0, bytes);
            A.first = first; A.last = wStop;
            good = true;
          }
        } catch (const Exception&) { A.disabled = true; }          // the exact path below decides what this call reports
        if (!good) { A.first = A.last = 0; A.data.clear(); }
      }
      if (first >= A.first && stop <= A.last) {
        std::memcpy(output.data, A.data.data() + (first - A.first) * (size_t)header.frameSize, produced);
        entryIndex = stop;
        if (stop == A.last) { A.data.clear(); A.data.shrink_to_fit(); A.first = A.last = 0; }
        return produced;
      }
    }
    const u64 base = fmt::entry_get(table + entryIndex * 5);
    if (fmt::entry_get(table + stop * 5) < base) throw Exception(StatusCode::ZStdError, 72);
    cache.resize(fmt::entry_get(table + stop * 5) - base);
    readFunction(header.size + base, cache.size(), cache.data());
    entryIndex = stop;
    if (!count) return 0;
    try {
      ra_decode(table, seekTable.size(), cache.data(), cache.size(), base, first, count, header, output.data, 0, produced);
    } catch (const Exception& e) {
      // frames that do not fill frameSize-sized slots (damaged or foreign header): the reference's single zstd call over the span
      // packs whatever the frames regenerate into the caller's buffer and returns that size (zra.cpp:435)
      if (!archive_status(e)) throw;
      return multiframe_call(cache.data(), cache.size(), output.data, output.size, header.frameSize);
    }
    return produced;
  }
}  // namespace zra

// ====================================================================================== C ABI (zra.cpp:439-626)
namespace {
ZraStatus mk(ZraStatusCode z, int zstd = 0) { return ZraStatus{z, (int)(int8_t)zstd}; }
ZraStatus mk(const zra::Exception& e) { return mk(static_cast<ZraStatusCode>(e.code), e.zstdCode); }
ZraStatus mk(zra_eng::Status s) { return ZraStatus{static_cast<ZraStatusCode>(s.zra), s.zstd}; }
template <typename F> ZraStatus guarded(F&& f) {
  try { f(); return mk(Success); } catch (const zra::Exception& e) { return mk(e); }
}
}  // namespace

extern "C" {
uint16_t ZraGetVersion(void) { return zra::GetVersion(); }
const char* ZraGetErrorString(ZraStatus status) {
  static thread_local std::string s;
  s = zra::Exception(static_cast<zra::StatusCode>(status.zra), status.zstd).what();
  return s.c_str();
}

ZraStatus ZraCreateHeader(ZraHeader** header, ZraReadFunction* rf) {
  return guarded([&] { *header = reinterpret_cast<ZraHeader*>(new zra::Header(std::function<void(size_t, size_t, void*)>(rf))); });
}
ZraStatus ZraCreateHeader2(ZraHeader** header, void* buffer, size_t size) {
  return guarded([&] { *header = reinterpret_cast<ZraHeader*>(new zra::Header(zra::BufferView(buffer, size))); });
}
void ZraDeleteHeader(ZraHeader* h) { delete reinterpret_cast<zra::Header*>(h); }
size_t ZraGetVersionWithHeader(ZraHeader* h) { return reinterpret_cast<zra::Header*>(h)->version; }
size_t ZraGetHeaderSizeWithHeader(ZraHeader* h) { return reinterpret_cast<zra::Header*>(h)->size; }
size_t ZraGetUncompressedSizeWithHeader(ZraHeader* h) { return reinterpret_cast<zra::Header*>(h)->uncompressedSize; }
size_t ZraGetFrameSizeWithHeader(ZraHeader* h) { return reinterpret_cast<zra::Header*>(h)->frameSize; }
size_t ZraGetMetadataSize(ZraHeader* h) { return reinterpret_cast<zra::Header*>(h)->metaSize; }
void ZraGetMetadata(ZraHeader* h, void* buffer) {
  auto* o = reinterpret_cast<zra::Header*>(h);
  o->GetMetadata(zra::BufferView(buffer, o->metaSize));
}

size_t ZraGetCompressedOutputBufferSize(size_t inputSize, size_t frameSize) { return zra::GetOutputBufferSize(inputSize, (uint32_t)frameSize); }

ZraStatus ZraCompressBuffer(void* in, size_t inSize, void* out, size_t* outSize, int8_t level, uint32_t frameSize, bool checksum, void* meta, size_t metaSize) {
  return guarded([&] {
    // the wrapper assumes `out` holds ZraGetCompressedOutputBufferSize(inSize, frameSize) bytes (zra.cpp:510) — plus metaSize when the
    // opt-in meta storage is on (the caller then sizes the buffer with the metaSize argument of that function)
    const size_t cap = zra::GetOutputBufferSize(inSize, frameSize, (g_options.load() & kOptStoreMetaInMemory) ? (zra::u32)metaSize : 0);
    *outSize = zra::CompressBuffer(zra::BufferView(in, inSize), zra::BufferView(out, cap), level, frameSize,
                                   checksum, zra::BufferView(meta, metaSize));
  });
}
ZraStatus ZraDecompressBuffer(void* in, size_t inSize, void* out) {
  return guarded([&] {
    // capacity is read from the raw header before validation, like the wrapper at zra.cpp:519
    uint64_t cap = inSize >= 26 ? zra_fmt::rd64(static_cast<uint8_t*>(in) + 18) : 0;
    zra::DecompressBuffer(zra::BufferView(in, inSize), zra::BufferView(out, cap));
  });
}
ZraStatus ZraDecompressRA(void* in, size_t inSize, void* out, size_t offset, size_t size) {
  return guarded([&] { zra::DecompressRA(zra::BufferView(in, inSize), zra::BufferView(out, size), offset, size); });
}

ZraStatus ZraCreateCompressor(ZraCompressor** c, size_t size, int8_t level, uint32_t frameSize, bool checksum, void* meta, size_t metaSize) {
  return guarded([&] { *c = reinterpret_cast<ZraCompressor*>(new zra::Compressor(size, level, frameSize, checksum, zra::BufferView(meta, metaSize))); });
}
void ZraDeleteCompressor(ZraCompressor* c) { delete reinterpret_cast<zra::Compressor*>(c); }
size_t ZraGetOutputBufferSizeWithCompressor(ZraCompressor* c, size_t inputSize) { return reinterpret_cast<zra::Compressor*>(c)->GetOutputBufferSize(inputSize); }
ZraStatus ZraCompressWithCompressor(ZraCompressor* c, void* in, size_t inSize, void* out, size_t* outSize) {
  return guarded([&] {
    auto* o = reinterpret_cast<zra::Compressor*>(c);
    *outSize = o->Compress(zra::BufferView(in, inSize), zra::BufferView(out, o->GetOutputBufferSize(inSize)));
  });
}
size_t ZraGetHeaderSizeWithCompressor(ZraCompressor* c) { return reinterpret_cast<zra::Compressor*>(c)->GetHeaderSize(); }
ZraStatus ZraGetHeaderWithCompressor(ZraCompressor* c, void* out) {
  return guarded([&] { const zra::Buffer& h = reinterpret_cast<zra::Compressor*>(c)->GetHeader(); std::memcpy(out, h.data(), h.size()); });
}

ZraStatus ZraCreateDecompressor(ZraDecompressor** d, ZraReadFunction* rf, size_t maxCacheSize) {
  return guarded([&] { *d = reinterpret_cast<ZraDecompressor*>(new zra::Decompressor(std::function<void(size_t, size_t, void*)>(rf), maxCacheSize)); });
}
void ZraDeleteDecompressor(ZraDecompressor* d) { delete reinterpret_cast<zra::Decompressor*>(d); }
ZraHeader* ZraGetHeaderWithDecompressor(ZraDecompressor* d) { return reinterpret_cast<ZraHeader*>(&reinterpret_cast<zra::Decompressor*>(d)->header); }
ZraStatus ZraDecompressWithDecompressor(ZraDecompressor* d, size_t offset, size_t size, void* out) {
  return guarded([&] { reinterpret_cast<zra::Decompressor*>(d)->Decompress(offset, size, zra::BufferView(out, size)); });
}

ZraStatus ZraCreateFullDecompressor(ZraFullDecompressor** d, ZraReadFunction* rf, size_t /*maxCacheSize: ignored, zra.cpp:602-604*/) {
  return guarded([&] { *d = reinterpret_cast<ZraFullDecompressor*>(new zra::FullDecompressor(std::function<void(size_t, size_t, void*)>(rf))); });
}
void ZraDeleteFullDecompressor(ZraFullDecompressor* d) { delete reinterpret_cast<zra::FullDecompressor*>(d); }
ZraHeader* ZraGetHeaderWithFullDecompressor(ZraFullDecompressor* d) { return reinterpret_cast<ZraHeader*>(&reinterpret_cast<zra::FullDecompressor*>(d)->header); }
ZraStatus ZraDecompressWithFullDecompressor(ZraFullDecompressor* d, void* out, size_t cap, size_t* outSize) {
  return guarded([&] { *outSize = reinterpret_cast<zra::FullDecompressor*>(d)->Decompress(zra::BufferView(out, cap)); });
}

// ---------------------------------------------------------------------------- device-side additions (zra_hip.h)
struct ZraHipEngine { Engine* e; };

int ZraHipDeviceCount(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
ZraStatus ZraHipCreateEngine(ZraHipEngine** engine, int device) {
  Engine* e = nullptr;
  zra_eng::Status s = Engine::create(&e, device);
  if (s.zra) return mk(s);
  *engine = new ZraHipEngine{e};
  return mk(Success);
}
void ZraHipDestroyEngine(ZraHipEngine* engine) { if (engine) { delete engine->e; delete engine; } }
ZraStatus ZraHipSynchronize(ZraHipEngine* engine) { return mk(engine->e->sync()); }
ZraStatus ZraHipReleaseScratch(ZraHipEngine* engine) { return mk(engine->e->release_scratch()); }
ZraStatus ZraHipWaitStream(ZraHipEngine* engine, void* producerStream) { return mk(engine->e->wait_stream((hipStream_t)producerStream)); }
void* ZraHipGetStream(ZraHipEngine* engine) { return (void*)engine->e->stream(); }
double ZraHipLastKernelMs(ZraHipEngine* engine) { return engine->e->last_kernel_ms(); }
void ZraHipSetOptions(uint32_t mask) { g_options.store(mask); }
uint32_t ZraHipGetOptions(void) { return g_options.load(); }
void ZraHipGetKernelStats(ZraHipEngine* engine, double* out6) { engine->e->kernel_stats(out6); }
void ZraHipGetDecodeStageStats(ZraHipEngine* engine, double* out8) { engine->e->decode_stage_stats(out8); }
size_t ZraHipGetLaunchTelemetry(ZraHipEngine* engine, uint64_t* out, size_t capWords) { return engine->e->launch_telemetry(out, capWords); }
uint32_t ZraHipDebugReadSeqs(ZraHipEngine* engine, uint32_t frame, uint64_t* out, uint32_t cap, uint32_t* meta3) { return engine->e->debug_read_seqs(frame, out, cap, meta3); }

ZraStatus ZraHipCompressBuffer(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut, size_t* outSize, int8_t level, uint32_t frameSize, bool checksum) {
  return mk(engine->e->compress_device((const uint8_t*)dIn, inSize, (uint8_t*)dOut, outSize, level, frameSize, checksum));
}
ZraStatus ZraHipDecompressBuffer(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut, size_t outCapacity) {
  return mk(engine->e->decompress_device((const uint8_t*)dIn, inSize, (uint8_t*)dOut, outCapacity));
}
ZraStatus ZraHipDecompressRABatch(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dOut, const uint64_t* hOffsets, const uint64_t* hSizes,
                                  const uint64_t* hOutOffsets, size_t nQueries) {
  engine->e->set_ra_verify_whole_frames((g_options.load() & kOptRaWholeFrames) != 0);
  return mk(engine->e->decompress_ra_batch((const uint8_t*)dIn, inSize, (uint8_t*)dOut, hOffsets, hSizes, hOutOffsets, nQueries));
}

struct ZraHipArchive { zra_eng::ArchiveCache* c; };
ZraStatus ZraHipArchiveOpen(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, size_t cacheBytes, ZraHipArchive** archive) {
  if (!engine || !archive || (!dArchive && archiveSize)) return mk(ZStdError, 42);
  zra_eng::ArchiveCache* c = nullptr;
  const zra_eng::Status s = zra_eng::ArchiveCache::open(engine->e, (const uint8_t*)dArchive, archiveSize, cacheBytes, &c);
  if (s.zra) return mk(s);
  *archive = new ZraHipArchive{c};
  return mk(Success);
}
void ZraHipArchiveClose(ZraHipArchive* archive) { if (archive) { delete archive->c; delete archive; } }
ZraStatus ZraHipArchiveRead(ZraHipArchive* archive, void* dOut, const uint64_t* hOffsets, const uint64_t* hSizes, const uint64_t* hOutOffsets, size_t nQueries) {
  if (!archive || (nQueries && (!hOffsets || !hSizes || !hOutOffsets))) return mk(ZStdError, 42);
  return mk(archive->c->read((uint8_t*)dOut, hOffsets, hSizes, hOutOffsets, nQueries, (g_options.load() & kOptRaWholeFrames) != 0));
}
ZraStatus ZraHipArchiveDropCache(ZraHipArchive* archive) { return archive ? mk(archive->c->drop()) : mk(ZStdError, 42); }
void ZraHipArchiveGetStats(const ZraHipArchive* archive, uint64_t* out8) {
  if (!out8) return;
  if (archive) archive->c->stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
ZraStatus ZraHipArchiveUpdate(ZraHipArchive* archive, const void* dData, const uint64_t* hOffsets, const uint64_t* hSizes, const uint64_t* hDataOffsets,
                              size_t nWrites, const void* dAppend, size_t appendSize, void* dOut, size_t outCapacity, size_t* outSize, int8_t level,
                              bool checksum) {
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->update((const uint8_t*)dData, hOffsets, hSizes, hDataOffsets, nWrites, (const uint8_t*)dAppend, appendSize, (uint8_t*)dOut,
                               outCapacity, outSize, level, checksum));
}
void ZraHipArchiveGetUpdateStats(const ZraHipArchive* archive, uint64_t* out8) {
  if (!out8) return;
  if (archive) archive->c->update_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
ZraStatus ZraHipArchiveSearch(ZraHipArchive* archive, const void* hPattern, size_t patternSize, uint64_t offset, uint64_t size, size_t stagingBytes,
                              uint64_t* hMatches, size_t matchCapacity, uint64_t* nMatches) {
  if (nMatches) *nMatches = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->search(hPattern, patternSize, offset, size, stagingBytes, hMatches, matchCapacity, nMatches));
}
ZraStatus ZraHipArchiveSearchMulti(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint64_t offset, uint64_t size,
                                   size_t stagingBytes, ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern) {
  if (nMatches) *nMatches = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->search_multi(hPatterns, hPatternSizes, nPatterns, 0, offset, size, stagingBytes, hMatches, matchCapacity, nMatches, hPerPattern));
}
ZraStatus ZraHipArchiveGrep(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint8_t delimiter, uint32_t mode,
                            uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecGrep, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, 0, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
ZraStatus ZraHipArchiveExtractRecords(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint8_t delimiter,
                                      uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity,
                                      uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecExtract, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, 0, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
void ZraHipArchiveGetScanStats(const ZraHipArchive* archive, uint64_t* out8) {
  if (!out8) return;
  if (archive) archive->c->scan_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugArchiveScanStageMs(const ZraHipArchive* archive) { return archive ? archive->c->scan_stage_ms() : 0.0; }
void ZraHipDebugArchiveArena(const ZraHipArchive* archive, const void** base, size_t* bytes) {
  if (!base || !bytes) return;
  *base = nullptr; *bytes = 0;
  if (archive) archive->c->arena_range(base, bytes);
}
ZraStatus ZraHipArchiveIndexRecords(ZraHipArchive* archive, uint32_t delimiter, uint64_t firstFrame, uint64_t frameCount, size_t stagingBytes, uint64_t* dIndex,
                                    size_t indexCapacityWords, ZraHipRecordIndex* info) {
  if (info) *info = ZraHipRecordIndex{0, 0, 0, 0, 0, 0};
  if (!archive || !info) return mk(ZStdError, 42);
  uint64_t w[6] = {0, 0, 0, 0, 0, 0};
  const ZraStatus st = mk(archive->c->index_records(delimiter, firstFrame, frameCount, stagingBytes, dIndex, indexCapacityWords, w));
  *info = ZraHipRecordIndex{w[0], (uint32_t)w[1], (uint32_t)w[2], w[3], w[4], w[5]};
  return st;
}
ZraStatus ZraHipArchiveLocateRecords(ZraHipArchive* archive, const ZraHipRecordIndex* info, const uint64_t* dIndex, size_t indexWords, const uint64_t* hRecordNumbers,
                                     size_t nRecords, size_t stagingBytes, ZraHipContentRange* hRanges) {
  if (!archive || !info) return mk(ZStdError, 42);
  const uint64_t w[6] = {info->contentSize, info->frameSize, info->delimiter, info->frames, info->delimiters, info->records};
  return mk(archive->c->locate_records(w, dIndex, indexWords, hRecordNumbers, nRecords, stagingBytes, (uint64_t*)hRanges));
}
ZraStatus ZraHipArchiveReadRecords(ZraHipArchive* archive, const ZraHipRecordIndex* info, const uint64_t* dIndex, size_t indexWords, const uint64_t* hRecordNumbers,
                                   size_t nRecords, size_t stagingBytes, ZraHipContentRange* hRanges, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (dataSize) *dataSize = 0;
  if (!archive || !info) return mk(ZStdError, 42);
  const uint64_t w[6] = {info->contentSize, info->frameSize, info->delimiter, info->frames, info->delimiters, info->records};
  return mk(archive->c->read_records(w, dIndex, indexWords, hRecordNumbers, nRecords, stagingBytes, (uint64_t*)hRanges, (uint8_t*)dData, dataCapacity, dataSize));
}
void ZraHipArchiveGetRecordStats(const ZraHipArchive* archive, uint64_t* out8) {
  if (!out8) return;
  if (archive) archive->c->record_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugArchiveRecordStageMs(const ZraHipArchive* archive) { return archive ? archive->c->record_stage_ms() : 0.0; }
ZraStatus ZraHipUpdateArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* dData, const uint64_t* hOffsets,
                              const uint64_t* hSizes, const uint64_t* hDataOffsets, size_t nWrites, const void* dAppend, size_t appendSize, void* dOut,
                              size_t outCapacity, size_t* outSize, int8_t level, bool checksum) {
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->update_archive((const uint8_t*)dArchive, archiveSize, (const uint8_t*)dData, hOffsets, hSizes, hDataOffsets, nWrites,
                                      (const uint8_t*)dAppend, appendSize, (uint8_t*)dOut, outCapacity, outSize, level, checksum));
}
double ZraHipDebugUpdateStageMs(ZraHipEngine* engine) { return engine ? engine->e->update_stage_ms() : 0.0; }
void ZraHipGetUpdateStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->update_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
ZraStatus ZraHipVerifyArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t mode, uint64_t firstFrame, uint64_t frameCount,
                              size_t stagingBytes, ZraHipFrameFault* hFaults, size_t faultCapacity, size_t* nFaults) {
  if (nFaults) *nFaults = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->verify_archive((const uint8_t*)dArchive, archiveSize, mode, firstFrame, frameCount, stagingBytes, hFaults, faultCapacity, nFaults));
}
void ZraHipGetVerifyStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->verify_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
ZraStatus ZraHipSearchArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPattern, size_t patternSize, uint64_t offset,
                              uint64_t size, size_t stagingBytes, uint64_t* hMatches, size_t matchCapacity, uint64_t* nMatches) {
  if (nMatches) *nMatches = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->search_archive((const uint8_t*)dArchive, archiveSize, hPattern, patternSize, offset, size, stagingBytes, hMatches, matchCapacity,
                                      nMatches));
}
void ZraHipGetSearchStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->search_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugSearchScanMs(ZraHipEngine* engine) { return engine ? engine->e->search_scan_ms() : 0.0; }
ZraStatus ZraHipSearchArchiveMulti(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes,
                                   size_t nPatterns, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipPatternMatch* hMatches, size_t matchCapacity,
                                   uint64_t* nMatches, uint64_t* hPerPattern) {
  static_assert(sizeof(ZraHipPatternMatch) == 16, "a 64-bit offset and two 32-bit words per match");
  if (nMatches) *nMatches = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->search_archive_multi((const uint8_t*)dArchive, archiveSize, hPatterns, hPatternSizes, nPatterns, 0, offset, size, stagingBytes, hMatches,
                                            matchCapacity, nMatches, hPerPattern));
}
void ZraHipGetSearchMultiStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->search_multi_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugSearchMultiScanMs(ZraHipEngine* engine) { return engine ? engine->e->search_multi_scan_ms() : 0.0; }
ZraStatus ZraHipGrepArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                            uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                            size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecGrep, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, 0, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
void ZraHipGetGrepStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->grep_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugGrepScanMs(ZraHipEngine* engine) { return engine ? engine->e->grep_scan_ms() : 0.0; }
ZraStatus ZraHipExtractRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes,
                               size_t nPatterns, uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes,
                               ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecExtract, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, 0, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
void ZraHipGetExtractStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->extract_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugExtractMs(ZraHipEngine* engine) { return engine ? engine->e->extract_ms() : 0.0; }

// ---- the scans with a pattern syntax word: the literal calls above through the same ScanImpl functions, `syntax` behind
// nPatterns. They write their literal twins' stats rows and millisecond words.
ZraStatus ZraHipCheckPatternExpr(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, int delimiter, uint32_t* hLengths,
                                 uint32_t* nSets) {
  zra_expr::Compiled C;
  if (!zra_expr::compile((const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, &C)) return mk(ZStdError, 42);
  if (hLengths) for (size_t i = 0; i < nPatterns; i++) hLengths[i] = C.len[i];
  if (nSets) *nSets = (uint32_t)C.sets.size();
  return mk(Success, 0);
}
ZraStatus ZraHipSearchArchiveMultiExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes,
                                       size_t nPatterns, uint32_t syntax, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipPatternMatch* hMatches,
                                       size_t matchCapacity, uint64_t* nMatches, uint64_t* hPerPattern) {
  if (nMatches) *nMatches = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->search_archive_multi((const uint8_t*)dArchive, archiveSize, hPatterns, hPatternSizes, nPatterns, syntax, offset, size, stagingBytes, hMatches,
                                            matchCapacity, nMatches, hPerPattern));
}
ZraStatus ZraHipGrepArchiveExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                uint32_t syntax, uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecGrep, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
ZraStatus ZraHipExtractRecordsExpr(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes,
                                   size_t nPatterns, uint32_t syntax, uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes,
                                   ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecExtract, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
ZraStatus ZraHipArchiveSearchMultiExpr(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint64_t offset,
                                       uint64_t size, size_t stagingBytes, ZraHipPatternMatch* hMatches, size_t matchCapacity, uint64_t* nMatches,
                                       uint64_t* hPerPattern) {
  if (nMatches) *nMatches = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->search_multi(hPatterns, hPatternSizes, nPatterns, syntax, offset, size, stagingBytes, hMatches, matchCapacity, nMatches, hPerPattern));
}
ZraStatus ZraHipArchiveGrepExpr(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity,
                                uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecGrep, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
ZraStatus ZraHipArchiveExtractRecordsExpr(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
                                          uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                          size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecExtract, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
// ---- the grep with context records: kernels of its own (zra_grep_context.hip), the grep's stats row and milliseconds
ZraStatus ZraHipGrepArchiveContext(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                   uint32_t syntax, uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after, uint64_t offset, uint64_t size, size_t stagingBytes,
                                   ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, uint64_t* nSelected, uint64_t* nGroups) {
  static_assert(ZRA_HIP_GREP_MAX_CONTEXT == 64 && ZRA_HIP_CONTEXT_SELECTED == 1ull << 63, "a wave's width; the bit above a content size");
  if (nRecords) *nRecords = 0;
  if (nSelected) *nSelected = 0;
  if (nGroups) *nGroups = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({zra_eng::kRecGrepContext, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode,
                                    offset, size, stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, nullptr, 0, before, after, nSelected,
                                    nGroups}));
}
ZraStatus ZraHipArchiveGrepContext(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                   uint32_t mode, uint32_t before, uint32_t after, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                   size_t recordCapacity, uint64_t* nRecords, uint64_t* nSelected, uint64_t* nGroups) {
  if (nRecords) *nRecords = 0;
  if (nSelected) *nSelected = 0;
  if (nGroups) *nGroups = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({zra_eng::kRecGrepContext, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size,
                                     stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, nullptr, 0, before, after, nSelected, nGroups}));
}
// ---- the regex grep with context records: kernels of its own (zra_grep_regex_context.hip), the grep's stats row and milliseconds
ZraStatus ZraHipGrepArchiveRegexContext(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                        uint32_t syntax, uint8_t delimiter, uint32_t mode, uint32_t before, uint32_t after, uint64_t offset, uint64_t size,
                                        size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, uint64_t* nSelected,
                                        uint64_t* nGroups) {
  if (nRecords) *nRecords = 0;
  if (nSelected) *nSelected = 0;
  if (nGroups) *nGroups = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({zra_eng::kRecGrepRegexContext, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter,
                                    mode, offset, size, stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, nullptr, 0, before, after, nSelected,
                                    nGroups}));
}
ZraStatus ZraHipArchiveGrepRegexContext(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                        uint32_t mode, uint32_t before, uint32_t after, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                        size_t recordCapacity, uint64_t* nRecords, uint64_t* nSelected, uint64_t* nGroups) {
  if (nRecords) *nRecords = 0;
  if (nSelected) *nSelected = 0;
  if (nGroups) *nGroups = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({zra_eng::kRecGrepRegexContext, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size,
                                     stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, nullptr, 0, before, after, nSelected, nGroups}));
}
// ---- the grep with a record predicate: kernels of its own (zra_grep_where.hip), the grep's stats row and milliseconds
ZraStatus ZraHipCheckRecordClauses(const ZraHipRecordClause* hClauses, size_t nClauses, size_t nPatterns) {
  static_assert(sizeof(ZraHipRecordClause) == sizeof(zra_where::Clause) && ZRA_HIP_WHERE_MAX_CLAUSES == zra_where::kMaxClauses, "one clause layout");
  return zra_where::clauses_ok((const zra_where::Clause*)hClauses, nClauses, nPatterns) ? mk(Success, 0) : mk(ZStdError, 42);
}
ZraStatus ZraHipGrepArchiveWhere(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                 uint32_t syntax, uint8_t delimiter, uint32_t mode, const ZraHipRecordClause* hClauses, size_t nClauses, uint64_t offset, uint64_t size,
                                 size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecGrepWhere, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, hClauses, nClauses}));
}
ZraStatus ZraHipArchiveGrepWhere(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                 uint32_t mode, const ZraHipRecordClause* hClauses, size_t nClauses, uint64_t offset, uint64_t size, size_t stagingBytes,
                                 ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecGrepWhere, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, nullptr, 0, nullptr, hClauses, nClauses}));
}
// ---- the extract with a record predicate: the predicate grep's selector, kernels of its own (zra_extract_where.hip); the extract's stats row and
// milliseconds
ZraStatus ZraHipExtractRecordsWhere(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                    uint32_t syntax, uint8_t delimiter, uint32_t mode, const ZraHipRecordClause* hClauses, size_t nClauses, uint64_t offset, uint64_t size,
                                    size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity,
                                    uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({zra_eng::kRecExtractWhere, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset,
                                    size, stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize, hClauses, nClauses}));
}
ZraStatus ZraHipArchiveExtractRecordsWhere(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                           uint32_t mode, const ZraHipRecordClause* hClauses, size_t nClauses, uint64_t offset, uint64_t size, size_t stagingBytes,
                                           ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({zra_eng::kRecExtractWhere, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                     (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize, hClauses, nClauses}));
}
// ---- cut records: the extract's selector, where no pattern selects every record, kernels of its own (zra_cut.hip); the extract's stats row and
// milliseconds
ZraStatus ZraHipFieldMask(const char* list, uint64_t* mask) {
  if (mask) *mask = 0;
  if (!list || !mask || !*list) return mk(ZStdError, 42);
  uint64_t m = 0;
  const char* p = list;
  // a number from 1, clamped to 65: everything above 64 is one case
  auto number = [&](uint64_t* v) {
    if (*p < '0' || *p > '9') return false;
    for (*v = 0; *p >= '0' && *p <= '9'; p++) *v = std::min<uint64_t>(*v * 10 + (uint64_t)(*p - '0'), 65);
    return *v != 0;
  };
  for (;;) {
    uint64_t a = 1, b = 0;
    bool range = false;
    if (*p == '-') { range = true; p++; if (!number(&b)) return mk(ZStdError, 42); }   // -M
    else {
      if (!number(&a)) return mk(ZStdError, 42);
      if (*p == '-') { range = true; p++; if (*p == ',' || !*p) b = 65; else if (!number(&b)) return mk(ZStdError, 42); }   // N- | N-M
      else b = a;
    }
    if (b < a || (!range && a > 64)) return mk(ZStdError, 42);
    for (uint64_t j = std::min<uint64_t>(a, 64); j <= std::min<uint64_t>(b, 64); j++) m |= 1ull << (j - 1);
    if (!*p) break;
    if (*p++ != ',') return mk(ZStdError, 42);
  }
  *mask = m;
  return mk(Success, 0);
}
namespace {
const uint32_t kNoPattern = 0;   // what the call path reads in the place of NULL pattern arguments when there is no pattern
}
ZraStatus ZraHipCutRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                           uint32_t syntax, uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask, uint64_t offset, uint64_t size, size_t stagingBytes,
                           ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!engine) return mk(ZStdError, 42);
  if (nPatterns == 0) { hPatterns = &kNoPattern; hPatternSizes = &kNoPattern; }
  zra_eng::RecordCall c = {zra_eng::kRecCut, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset,
                           size, stagingBytes, (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize};
  c.separator = separator; c.fieldMask = fieldMask;
  return mk(engine->e->record_scan(c));
}
ZraStatus ZraHipArchiveCutRecords(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                  uint32_t mode, uint8_t separator, uint64_t fieldMask, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                  size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!archive) return mk(ZStdError, 42);
  if (nPatterns == 0) { hPatterns = &kNoPattern; hPatternSizes = &kNoPattern; }
  zra_eng::RecordCall c = {zra_eng::kRecCut, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                           (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize};
  c.separator = separator; c.fieldMask = fieldMask;
  return mk(archive->c->record_scan(c));
}
// ---- tally records: the primitive is zra_tally.hip's; the composites are the cut above into the caller's workspace and the primitive on what it packed,
// each with its own stats row
ZraStatus ZraHipTallyRecords(ZraHipEngine* engine, const void* dText, size_t textSize, uint8_t delimiter, uint64_t maxDistinct, ZraHipTallyEntry* hEntries,
                             size_t entryCapacity, void* dKeys, size_t keyCapacity, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize) {
  static_assert(sizeof(ZraHipTallyEntry) == 24 && ZRA_HIP_TALLY_MAX_KEY == zra_eng::kTallyMaxKey, "three 64-bit words per entry; the cap the kernels are built with");
  for (uint64_t* w : {nRecords, nDistinct, nSkipped, keySize}) if (w) *w = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->tally_records((const uint8_t*)dText, textSize, delimiter, maxDistinct, (uint64_t*)hEntries, entryCapacity, (uint8_t*)dKeys, keyCapacity, nRecords,
                                     nDistinct, nSkipped, keySize));
}
namespace {
struct TallyOut {
  uint64_t maxDistinct; ZraHipTallyEntry* hEntries; size_t entryCapacity; void* dKeys; size_t keyCapacity; uint64_t* nRecords, * nDistinct, * nSkipped, * keySize;
};
// the composite behind both entry points: rule 1 of the tally, the cut `cut` makes of c, the tally of what it packed. arc / arena: what dKeys may not overlap
ZraStatus tally_fields(Engine* e, zra_eng::RecordCall c, const TallyOut& t, const void* arc, size_t arcBytes, const void* arena, size_t arenaBytes,
                       const std::function<zra_eng::Status(const zra_eng::RecordCall&)>& cut) {
  if (!c.dataSize || !t.nRecords || !t.nDistinct || !t.nSkipped || !t.keySize || (!t.hEntries && t.entryCapacity) || (!t.dKeys && t.keyCapacity)) return mk(ZStdError, 42);
  auto overlaps = [&](const void* p, size_t n) { return t.keyCapacity && n && (uintptr_t)t.dKeys < (uintptr_t)p + n && (uintptr_t)p < (uintptr_t)t.dKeys + t.keyCapacity; };
  if (overlaps(c.dData, c.dataCap) || overlaps(arc, arcBytes) || overlaps(arena, arenaBytes)) return mk(ZStdError, 42);
  uint64_t selected = 0;
  c.nRecords = &selected;
  const zra_eng::Status st = cut(c);
  if (st.zra) { e->tally_clear(); return mk(st); }
  return mk(e->tally_records(c.dData, (size_t)*c.dataSize, c.delimiter, t.maxDistinct, (uint64_t*)t.hEntries, t.entryCapacity, (uint8_t*)t.dKeys, t.keyCapacity, t.nRecords,
                             t.nDistinct, t.nSkipped, t.keySize));
}
}  // namespace
ZraStatus ZraHipTallyFields(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                            uint32_t syntax, uint8_t delimiter, uint32_t mode, uint8_t separator, uint64_t fieldMask, uint64_t offset, uint64_t size, size_t stagingBytes,
                            void* dWork, size_t workCapacity, uint64_t* workSize, uint64_t maxDistinct, ZraHipTallyEntry* hEntries, size_t entryCapacity, void* dKeys,
                            size_t keyCapacity, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize) {
  for (uint64_t* w : {workSize, nRecords, nDistinct, nSkipped, keySize}) if (w) *w = 0;
  if (!engine) return mk(ZStdError, 42);
  if (nPatterns == 0) { hPatterns = &kNoPattern; hPatternSizes = &kNoPattern; }
  zra_eng::RecordCall c = {zra_eng::kRecCut, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset,
                           size, stagingBytes, nullptr, 0, nullptr, (uint8_t*)dWork, workCapacity, workSize};
  c.separator = separator; c.fieldMask = fieldMask;
  Engine* const e = engine->e;
  return tally_fields(e, c, {maxDistinct, hEntries, entryCapacity, dKeys, keyCapacity, nRecords, nDistinct, nSkipped, keySize}, dArchive, archiveSize, nullptr, 0,
                      [&](const zra_eng::RecordCall& rc) { return e->record_scan(rc); });
}
ZraStatus ZraHipArchiveTallyFields(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                   uint32_t mode, uint8_t separator, uint64_t fieldMask, uint64_t offset, uint64_t size, size_t stagingBytes, void* dWork,
                                   size_t workCapacity, uint64_t* workSize, uint64_t maxDistinct, ZraHipTallyEntry* hEntries, size_t entryCapacity, void* dKeys,
                                   size_t keyCapacity, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize) {
  for (uint64_t* w : {workSize, nRecords, nDistinct, nSkipped, keySize}) if (w) *w = 0;
  if (!archive) return mk(ZStdError, 42);
  if (nPatterns == 0) { hPatterns = &kNoPattern; hPatternSizes = &kNoPattern; }
  zra_eng::RecordCall c = {zra_eng::kRecCut, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                           nullptr, 0, nullptr, (uint8_t*)dWork, workCapacity, workSize};
  c.separator = separator; c.fieldMask = fieldMask;
  const void* arc, * arena; size_t arcBytes, arenaBytes;
  archive->c->archive_range(&arc, &arcBytes); archive->c->arena_range(&arena, &arenaBytes);
  return tally_fields(archive->c->engine(), c, {maxDistinct, hEntries, entryCapacity, dKeys, keyCapacity, nRecords, nDistinct, nSkipped, keySize}, arc, arcBytes, arena,
                      arenaBytes, [&](const zra_eng::RecordCall& rc) { return archive->c->record_scan(rc); });
}
void ZraHipGetTallyStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->tally_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugTallyMs(ZraHipEngine* engine) { return engine ? engine->e->tally_ms() : 0.0; }
void ZraHipDebugTallyHashBits(ZraHipEngine* engine, uint32_t bits) {
  if (!engine) return;
  if (bits == 0) engine->e->set_tally_keep(~0ull);
  else if (bits == ZRA_HIP_TALLY_HASH_NONE) engine->e->set_tally_keep(0);
  else if (bits < 64) engine->e->set_tally_keep((1ull << bits) - 1);
}
// ---- the grep with regular expressions: the compiler is zra_regex.h's, the kernels zra_grep_regex.hip's; the grep's stats row and milliseconds
ZraStatus ZraHipCheckRegex(const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, int delimiter, ZraHipRegexInfo* info) {
  static_assert(sizeof(ZraHipRegexInfo) == sizeof(zra_regex::Info) && ZRA_HIP_REGEX_MAX_STATES == zra_regex::kMaxStates &&
                ZRA_HIP_REGEX_MAX_POSITIONS == zra_regex::kMaxPositions, "one info layout");
  zra_regex::Compiled C;
  const bool good = zra_regex::compile((const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, &C);
  if (info) std::memcpy(info, &C.info, sizeof(*info));
  return good ? mk(Success, 0) : mk(ZStdError, 42);
}
ZraStatus ZraHipGrepArchiveRegex(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns,
                                 uint32_t syntax, uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                 size_t recordCapacity, uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecGrepRegex, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
ZraStatus ZraHipArchiveGrepRegex(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax, uint8_t delimiter,
                                 uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords, size_t recordCapacity,
                                 uint64_t* nRecords) {
  if (nRecords) *nRecords = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecGrepRegex, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords}));
}
// ---- the extract with regular expressions: the regex grep's compiler, kernels of its own (zra_extract_regex.hip); the extract's stats row and
// milliseconds
ZraStatus ZraHipExtractRecordsRegex(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const void* hPatterns, const uint32_t* hPatternSizes,
                                    size_t nPatterns, uint32_t syntax, uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes,
                                    ZraHipContentRange* hRecords, size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->record_scan({kRecExtractRegex, (const uint8_t*)dArchive, archiveSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
ZraStatus ZraHipArchiveExtractRecordsRegex(ZraHipArchive* archive, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint32_t syntax,
                                           uint8_t delimiter, uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, ZraHipContentRange* hRecords,
                                           size_t recordCapacity, uint64_t* nRecords, void* dData, size_t dataCapacity, uint64_t* dataSize) {
  if (nRecords) *nRecords = 0;
  if (dataSize) *dataSize = 0;
  if (!archive) return mk(ZStdError, 42);
  return mk(archive->c->record_scan({kRecExtractRegex, nullptr, 0, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, syntax, delimiter, mode, offset, size, stagingBytes,
                                    (uint64_t*)hRecords, recordCapacity, nRecords, (uint8_t*)dData, dataCapacity, dataSize}));
}
ZraStatus ZraHipCompareArchives(ZraHipEngine* engine, const void* dA, size_t sizeA, const void* dB, size_t sizeB, uint32_t mode, uint64_t offset, uint64_t size,
                                size_t stagingBytes, ZraHipContentRange* hRanges, size_t rangeCapacity, uint64_t* nRanges, uint64_t* differingBytes) {
  static_assert(sizeof(ZraHipContentRange) == 16, "two 64-bit words per range");
  if (nRanges) *nRanges = 0;
  if (differingBytes) *differingBytes = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->compare_archives((const uint8_t*)dA, sizeA, (const uint8_t*)dB, sizeB, mode, offset, size, stagingBytes, (uint64_t*)hRanges,
                                        rangeCapacity, nRanges, differingBytes));
}
void ZraHipGetCompareStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->compare_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
void ZraHipGetCompareSizes(ZraHipEngine* engine, uint64_t* out2) {
  if (!out2) return;
  if (engine) engine->e->compare_sizes(out2); else out2[0] = out2[1] = 0;
}
double ZraHipDebugCompareMs(ZraHipEngine* engine) { return engine ? engine->e->compare_ms() : 0.0; }
ZraStatus ZraHipDiffArchives(ZraHipEngine* engine, const void* dA, size_t sizeA, const void* dB, size_t sizeB, uint32_t mode, uint32_t grain, size_t stagingBytes,
                             uint64_t* hOffsets, uint64_t* hSizes, uint64_t* hDataOffsets, size_t writeCapacity, uint64_t* nWrites, void* dData,
                             size_t dataCapacity, uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize) {
  for (uint64_t* w : {nWrites, dataSize, appendOffset, appendSize}) if (w) *w = 0;
  if (!engine) return mk(ZStdError, 42);
  return mk(engine->e->diff_archives((const uint8_t*)dA, sizeA, (const uint8_t*)dB, sizeB, mode, grain, stagingBytes, hOffsets, hSizes, hDataOffsets,
                                     writeCapacity, nWrites, (uint8_t*)dData, dataCapacity, dataSize, appendOffset, appendSize));
}
void ZraHipGetDiffStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->diff_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugDiffMs(ZraHipEngine* engine) { return engine ? engine->e->diff_ms() : 0.0; }
ZraStatus ZraHipSignArchive(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t grain, uint64_t seed, uint64_t firstFrame, uint64_t frameCount,
                            size_t stagingBytes, uint64_t* dSig, size_t sigCapacityWords, ZraHipSignature* info) {
  static_assert(sizeof(ZraHipSignature) == 40, "the signature file's 40-byte head");
  if (info) *info = ZraHipSignature{0, 0, 0, 0, 0, 0};
  if (!engine || !info) return mk(ZStdError, 42);
  uint64_t w[6] = {0, 0, 0, 0, 0, 0};
  const ZraStatus st = mk(engine->e->sign_archive((const uint8_t*)dArchive, archiveSize, grain, seed, firstFrame, frameCount, stagingBytes, dSig, sigCapacityWords, w));
  *info = ZraHipSignature{w[0], (uint32_t)w[1], (uint32_t)w[2], w[3], w[4], w[5]};
  return st;
}
void ZraHipGetSignStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->sign_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugSignMs(ZraHipEngine* engine) { return engine ? engine->e->sign_ms() : 0.0; }
ZraStatus ZraHipDiffSignature(ZraHipEngine* engine, const ZraHipSignature* sigA, const uint64_t* dSigA, size_t sigWords, const void* dB, size_t sizeB, uint32_t mode,
                              size_t stagingBytes, uint64_t* hOffsets, uint64_t* hSizes, uint64_t* hDataOffsets, size_t writeCapacity, uint64_t* nWrites, void* dData,
                              size_t dataCapacity, uint64_t* dataSize, uint64_t* appendOffset, uint64_t* appendSize) {
  for (uint64_t* w : {nWrites, dataSize, appendOffset, appendSize}) if (w) *w = 0;
  if (!engine || !sigA) return mk(ZStdError, 42);
  const uint64_t w[6] = {sigA->contentSize, sigA->frameSize, sigA->grain, sigA->seed, sigA->frames, sigA->words};
  return mk(engine->e->diff_signature(w, dSigA, sigWords, (const uint8_t*)dB, sizeB, mode, stagingBytes, hOffsets, hSizes, hDataOffsets, writeCapacity, nWrites,
                                      (uint8_t*)dData, dataCapacity, dataSize, appendOffset, appendSize));
}
void ZraHipGetDiffSignatureStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->diff_signature_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugDiffSignatureMs(ZraHipEngine* engine) { return engine ? engine->e->diff_signature_ms() : 0.0; }
ZraStatus ZraHipIndexRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, uint32_t delimiter, uint64_t firstFrame, uint64_t frameCount,
                             size_t stagingBytes, uint64_t* dIndex, size_t indexCapacityWords, ZraHipRecordIndex* info) {
  static_assert(sizeof(ZraHipRecordIndex) == 40, "the index file's 40-byte head");
  if (info) *info = ZraHipRecordIndex{0, 0, 0, 0, 0, 0};
  if (!engine || !info) return mk(ZStdError, 42);
  uint64_t w[6] = {0, 0, 0, 0, 0, 0};
  const ZraStatus st = mk(engine->e->index_records((const uint8_t*)dArchive, archiveSize, delimiter, firstFrame, frameCount, stagingBytes, dIndex, indexCapacityWords, w));
  *info = ZraHipRecordIndex{w[0], (uint32_t)w[1], (uint32_t)w[2], w[3], w[4], w[5]};
  return st;
}
void ZraHipGetIndexRecordsStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->index_records_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugIndexRecordsMs(ZraHipEngine* engine) { return engine ? engine->e->index_records_ms() : 0.0; }
ZraStatus ZraHipLocateRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const ZraHipRecordIndex* info, const uint64_t* dIndex, size_t indexWords,
                              const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes, ZraHipContentRange* hRanges) {
  if (!engine || !info) return mk(ZStdError, 42);
  const uint64_t w[6] = {info->contentSize, info->frameSize, info->delimiter, info->frames, info->delimiters, info->records};
  return mk(engine->e->locate_records((const uint8_t*)dArchive, archiveSize, w, dIndex, indexWords, hRecordNumbers, nRecords, stagingBytes, (uint64_t*)hRanges));
}
void ZraHipGetLocateRecordsStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->locate_records_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugLocateRecordsMs(ZraHipEngine* engine) { return engine ? engine->e->locate_records_ms() : 0.0; }
ZraStatus ZraHipReadRecords(ZraHipEngine* engine, const void* dArchive, size_t archiveSize, const ZraHipRecordIndex* info, const uint64_t* dIndex, size_t indexWords,
                            const uint64_t* hRecordNumbers, size_t nRecords, size_t stagingBytes, ZraHipContentRange* hRanges, void* dData, size_t dataCapacity,
                            uint64_t* dataSize) {
  if (dataSize) *dataSize = 0;
  if (!engine || !info) return mk(ZStdError, 42);
  const uint64_t w[6] = {info->contentSize, info->frameSize, info->delimiter, info->frames, info->delimiters, info->records};
  return mk(engine->e->read_records((const uint8_t*)dArchive, archiveSize, w, dIndex, indexWords, hRecordNumbers, nRecords, stagingBytes, (uint64_t*)hRanges,
                                    (uint8_t*)dData, dataCapacity, dataSize));
}
void ZraHipGetReadRecordsStats(ZraHipEngine* engine, uint64_t* out8) {
  if (!out8) return;
  if (engine) engine->e->read_records_stats(out8); else for (int i = 0; i < 8; i++) out8[i] = 0;
}
double ZraHipDebugReadRecordsMs(ZraHipEngine* engine) { return engine ? engine->e->read_records_ms() : 0.0; }
ZraStatus ZraHipCompressFrames(ZraHipEngine* engine, const void* dIn, size_t inSize, void* dBody, uint64_t* dSizes, size_t* bodySize, int8_t level,
                               uint32_t frameSize, bool checksum) {
  return mk(engine->e->compress_frames((const uint8_t*)dIn, inSize, (uint8_t*)dBody, dSizes, bodySize, level, frameSize, checksum));
}
ZraStatus ZraHipStitchHeader(const uint64_t* hFrameSizes, size_t nFramesTotal, uint64_t uncompressedSize, uint32_t frameSize, void* hHeader, size_t* headerSize) {
  uint8_t* h = (uint8_t*)hHeader;
  const uint32_t tableSize = (uint32_t)nFramesTotal + 1;
  zra_fmt::write_fixed(h, uncompressedSize, tableSize, frameSize, 0);
  uint64_t off = 0;
  for (size_t i = 0; i < nFramesTotal; i++) { zra_fmt::entry_put(h + zra_fmt::kFixedSize + i * 5, off); off += hFrameSizes[i]; }
  zra_fmt::entry_put(h + zra_fmt::kFixedSize + nFramesTotal * 5, off);
  if (off + zra_fmt::kFixedSize + (size_t)tableSize * 5 >= zra_fmt::kMaxCompressedSize) return mk(CompressedSizeTooLarge);
  zra_fmt::wr32(h + 14, zra_fmt::header_hash(h, h + zra_fmt::kFixedSize));
  *headerSize = zra_fmt::kFixedSize + (size_t)tableSize * 5;
  return mk(Success);
}
}  // extern "C"

// for zra_comm.hip (the sharded serving path takes the same opt-in as ZraHipDecompressRABatch)
bool zra_ra_whole_frames_option() { return (g_options.load() & kOptRaWholeFrames) != 0; }
