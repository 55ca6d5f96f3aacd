// zra_amd — tally of packed records in device memory (zra_hip.h: ZraHipTallyRecords): the distinct records of a text cut at a
// delimiter byte, in order of first appearance, each with the number of its occurrences: the counts `sort | uniq -c` prints, in the
// order `awk '!seen[$0]++'` prints the keys. The text is what ZraHipExtractRecords* and ZraHipCutRecords write.
//
//  (records) position p of the text starts a record iff p < textSize and (p == 0 or text[p - 1] is the delimiter): a record needs no
//      number and no scan to know where it starts, and the bytes behind the last delimiter form one more record iff there are any.
//      A record ends in front of the next delimiter or at textSize. One longer than kTallyMaxKey is SKIPPED: counted, in no entry.
//  (tile) a workgroup takes kTile consecutive positions and every record that STARTS there; a lane reads 16 of them, the delimiter
//      flags of the tile lie in LDS as kTile / 64 words, and a record that runs over the tile's end is followed in the text itself,
//      for at most kTallyMaxKey + 1 bytes.
//  (table) open addressing with linear probing over `slots` (a power of two) triples {claim, first, count} in engine scratch. A
//      claim word is {offset + 1 of the claimer's record: 40 bits, its length: 13, the hash's top bits: 11}; 0 is an empty slot. A
//      lane claims an empty slot with ONE 64-bit compare-and-swap. A lane that finds a claim with its own length and tag compares its
//      bytes with the TEXT at the claim's offset, which nobody writes during the launch: equality is exact, never the hash's. On
//      equality it adds its count to the slot and lowers the slot's first offset (atomicMin); otherwise it probes on. Slot words are
//      read with agent-scope atomic loads (the XCDs' L2s are not coherent for plain ones). No lane waits for another lane's store: a
//      claim word is complete the moment it exists. Probing is bounded by the slot count, and ends early once the claim counter has
//      passed maxDistinct (every 32 probes one look): rule 4 is then decided.
//  (combining) log fields are skewed: a handful of keys over millions of records would be millions of atomics on a handful of
//      addresses. So the records of a tile first meet in an LDS table of kLdsSlots slots of the same design (claim word: the
//      position in the tile, the length, 32 bits of the hash), at most kLdsProbes probes each; after a barrier one lane per occupied
//      LDS slot inserts {the key's first offset in the tile, its count in the tile} into the table in HBM: one insert per key the
//      workgroup saw. A record that finds no LDS slot within kLdsProbes goes to HBM itself, with count 1.
//  (order) which slot a key gets, and how far it probes, depends on who arrives first. Its count and its first offset do not, and
//      nothing else reaches the outputs: a record is a FIRST OCCURRENCE iff its offset is its slot's first offset. The mark launch
//      sets, per occupied slot, the bit of that offset in a bitmap of the text's positions (starts) and the bits of the key's bytes
//      and its delimiter in a second one (kept). Popcounts per tile and a two-column scan (zra_joblist.h) then give every tile the
//      number of the first key that starts in it and the offset of its bytes in dKeys, in text order: no atomic decides an output
//      position and nothing is sorted. The emit launch (per slot) ranks a key inside its tile by popcounts over the tile's start
//      words; the copy launch (per tile) is a stream compaction of the text by the kept bits, clamped to the capacity. The last
//      record of a text without a final delimiter, when it is a first occurrence, gets its delimiter from the copy launch's lane 0.
//  (launches) zra_tally_count_kernel (the record count sizes the table; one synchronisation), zra_tally_insert_kernel,
//      zra_tally_mark_kernel, zra_tally_sum_kernel, zra_tally_scan_kernel (ONE workgroup; the second synchronisation brings the
//      totals and decides rules 4 and 5), zra_tally_emit_kernel and zra_tally_copy_kernel, each only when its buffer was given.
#include <algorithm>
#include "zra_host.h"
#include "zra_dev.h"
#include "zra_joblist.h"

using namespace zra_dev;

namespace {
constexpr u32 kTile = zra_eng::kTallyTile;
constexpr u32 kMaxKey = zra_eng::kTallyMaxKey;
constexpr u32 kWords = kTile / 64;                                           // the words of a tile in either bitmap
constexpr u32 kLdsSlots = 1024, kLdsProbes = 16;                             // (combining)
constexpr u32 kCountGroup = 8;                                               // consecutive tiles of one workgroup of the count
constexpr u64 kOffMask = (1ull << 40) - 1;                                   // (table) the claim word's offset + 1
static_assert(kTile == 4096 && kMaxKey < (1u << 13) && kTile < (1u << 16), "a lane takes 16 of 4,096 positions; the claim words' length and position fields");
// the call's words on the device
enum : u32 { kHRecords = 0, kHSkipped, kHClaims, kHOverflow, kHProbe, kHInserts, kHDistinct, kHKeyBytes, kHTail, kHWords = 16 };
struct TallyTable { u64* claim; u64* first; u64* count; u64 slots; };
struct __attribute__((aligned(8))) Entry { u64 offset, size, count; };      // ZraHipTallyEntry

__device__ __forceinline__ u64 aload(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hdr_add(u64* p, u64 v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// the delimiter flags of the up to 16 positions from p (bit i: text[p + i]); no byte at or beyond textSize is read
__device__ __forceinline__ u32 delim16(const u8* text, u64 p, u64 textSize, u32 delim) {
  if (p >= textSize) return 0;
  u32 m = 0;
  if (p + 16 <= textSize) {
    const u64 a = ld64(text + p), b = ld64(text + p + 8);
#pragma unroll
    for (u32 i = 0; i < 8; i++) { m |= (u32)(((a >> (8 * i)) & 0xFF) == delim) << i; m |= (u32)(((b >> (8 * i)) & 0xFF) == delim) << (8 + i); }
    return m;
  }
  for (u32 i = 0; i < 16 && p + i < textSize; i++) m |= (u32)(text[p + i] == delim) << i;
  return m;
}

// (table) a function of the key's bytes alone; keep: ZraHipDebugTallyHashBits
__device__ __forceinline__ u64 key_hash(const u8* k, u32 len, u64 keep) {
  u64 h = 0xCBF29CE484222325ull ^ len;
  u32 i = 0;
  for (; i + 8 <= len; i += 8) { h = (h ^ ld64(k + i)) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
  for (; i < len; i++) h = (h ^ k[i]) * 0x100000001B3ull;
  h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
  return h & keep;
}

// len bytes at a and at b, both inside the text
__device__ __forceinline__ bool same_bytes(const u8* a, const u8* b, u32 len) {
  if (a == b) return true;
  u32 i = 0;
  for (; i + 8 <= len; i += 8) if (ld64(a + i) != ld64(b + i)) return false;
  for (; i < len; i++) if (a[i] != b[i]) return false;
  return true;
}

// (table) cnt occurrences of the key of len bytes at text + off, the first of them at off. Returns the slots it looked at, its own
// included.
__device__ __forceinline__ u64 table_insert(const u8* text, const TallyTable& T, u64* hdr, u64 maxDistinct, u64 off, u32 len, u64 hash, u64 cnt) {
  const u64 mine = (off + 1) | (u64)len << 40 | (hash >> 53) << 53;
  u64 slot = hash & (T.slots - 1);
  for (u64 k = 0; k < T.slots; k++) {
    u64 w = aload(T.claim + slot);
    if (w == 0) {
      w = atomicCAS((unsigned long long*)(T.claim + slot), 0ull, (unsigned long long)mine);
      if (w == 0) { hdr_add(hdr + kHClaims, 1); w = mine; }
    }
    if (((w ^ mine) >> 40) == 0 && same_bytes(text + ((w & kOffMask) - 1), text + off, len)) {
      hdr_add(T.count + slot, cnt);
      atomicMin((unsigned long long*)(T.first + slot), (unsigned long long)off);
      return k + 1;
    }
    slot = (slot + 1) & (T.slots - 1);
    if (maxDistinct && (k & 31) == 31 && aload(hdr + kHClaims) > maxDistinct) return k + 1;   // (rule 4 is decided; the key stays out)
  }
  atomicOr((unsigned long long*)(hdr + kHOverflow), 1ull);                   // (every slot holds another key: more keys than the table was sized for)
  return T.slots;
}
}  // namespace

// The records of the text: its delimiters, and one more when bytes lie behind the last. A workgroup takes kCountGroup tiles.
extern "C" __global__ void __launch_bounds__(256) zra_tally_count_kernel(const u8* text, u64 textSize, u32 delim, u64* hdr) {
  const u32 tid = threadIdx.x;
  u32 n = 0;
  for (u32 g = 0; g < kCountGroup; g++) {
    const u64 p = ((u64)blockIdx.x * kCountGroup + g) * kTile + 16 * tid;
    n += (u32)__popc(delim16(text, p, textSize, delim));
  }
  n = wave_sum(n);
  if (blockIdx.x == 0 && tid == 0 && text[textSize - 1] != delim) n++;       // (textSize != 0: the host's rule 2)
  if ((tid & 63) == 0 && n) hdr_add(hdr + kHRecords, n);
}

// (tile), (combining), (table). One workgroup per tile.
extern "C" __global__ void __launch_bounds__(256) zra_tally_insert_kernel(const u8* text, u64 textSize, u32 delim, u64 keep, u64 maxDistinct, TallyTable T, u64* hdr) {
  __shared__ u64 sDelim[kWords];
  __shared__ u16 sList[4][kTile / 4];                                        // per wave: the record starts among its 1,024 positions
  __shared__ u64 sClaim[kLdsSlots], sHash[kLdsSlots];
  __shared__ u32 sFirst[kLdsSlots], sCount[kLdsSlots];
  __shared__ u32 sBail;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const u32 n = (u32)min((u64)kTile, textSize - t0);
  const u32 m16 = delim16(text, t0 + 16 * tid, textSize, delim);
  ((u16*)sDelim)[tid] = (u16)m16;
  for (u32 s = tid; s < kLdsSlots; s += 256) { sClaim[s] = 0; sCount[s] = 0; sFirst[s] = 0xFFFFFFFFu; }
  if (tid == 0) sBail = maxDistinct && aload(hdr + kHClaims) > maxDistinct;
  __syncthreads();
  // (records) the starts among this lane's 16 positions: behind a delimiter, or at the text's head
  u32 prev;
  if (tid) prev = (((const u16*)sDelim)[tid - 1] >> 15) & 1;
  else prev = t0 == 0 ? 1u : (u32)(text[t0 - 1] == delim);
  const u32 valid = 16 * tid >= n ? 0u : (n - 16 * tid >= 16 ? 0xFFFFu : (1u << (n - 16 * tid)) - 1);
  u32 starts = ((m16 << 1) | prev) & valid;
  const u32 c = (u32)__popc(starts), incl = wave_incl_scan(c);
  const u32 mineCnt = lane_value(incl, 63);
  for (u32 at = incl - c; starts; at++) { const u32 b = (u32)__builtin_ctz(starts); starts &= starts - 1; sList[wave][at] = (u16)(16 * tid + b); }
  __syncthreads();
  const bool bail = sBail != 0;
  u32 skipped = 0, inserts = 0;
  u64 probe = 0;
  for (u32 i = lane; i < mineCnt; i += 64) {
    const u32 j = sList[wave][i];
    // the record's end: the next delimiter of the tile, or (tile) the text behind it
    u32 w = j >> 6, len;
    u64 m = sDelim[w] & (~0ull << (j & 63));
    while (m == 0 && ++w < kWords) m = sDelim[w];
    if (m) len = w * 64 + (u32)__builtin_ctzll(m) - j;
    else {
      len = n - j;
      for (u64 q = t0 + n; q < textSize && len <= kMaxKey && text[q] != delim; q++) len++;
    }
    if (len > kMaxKey) { skipped++; continue; }
    if (bail) continue;
    const u8* const key = text + t0 + j;
    const u64 hash = key_hash(key, len, keep);
    const u64 mine = (u64)(j + 1) | (u64)len << 16 | (hash >> 32) << 32;
    u32 s = (u32)hash & (kLdsSlots - 1);
    bool done = false;
    for (u32 k = 0; k < kLdsProbes && !done; k++) {
      u64 v = __hip_atomic_load(&sClaim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (v == 0) {
        v = atomicCAS((unsigned long long*)&sClaim[s], 0ull, (unsigned long long)mine);
        if (v == 0) { sHash[s] = hash; v = mine; }                           // (read behind the barrier below)
      }
      if (((v ^ mine) >> 16) == 0 && same_bytes(text + t0 + ((u32)(v & 0xFFFF) - 1), key, len)) {
        atomicAdd(&sCount[s], 1u); atomicMin(&sFirst[s], j); done = true;
      } else s = (s + 1) & (kLdsSlots - 1);
    }
    if (!done) { probe = max(probe, table_insert(text, T, hdr, maxDistinct, t0 + j, len, hash, 1)); inserts++; }
  }
  __syncthreads();
  for (u32 s = tid; s < kLdsSlots && !bail; s += 256) {
    const u64 v = sClaim[s];
    if (v == 0) continue;
    probe = max(probe, table_insert(text, T, hdr, maxDistinct, t0 + sFirst[s], (u32)(v >> 16) & 0x1FFF, sHash[s], sCount[s]));
    inserts++;
  }
  skipped = wave_sum(skipped); inserts = wave_sum(inserts);
  const u32 far = wave_max((u32)min(probe, (u64)0xFFFFFFFFu));
  if (lane == 0) {
    if (skipped) hdr_add(hdr + kHSkipped, skipped);
    if (inserts) hdr_add(hdr + kHInserts, inserts);
    if (far) atomicMax((unsigned long long*)(hdr + kHProbe), (unsigned long long)far);
  }
}

// (order) per occupied slot: the start bit of the key's first occurrence, the kept bits of its bytes and its delimiter
extern "C" __global__ void __launch_bounds__(256) zra_tally_mark_kernel(TallyTable T, u64 textSize, u64 maxDistinct, u64* startBits, u64* keptBits, u64* hdr) {
  if (hdr[kHOverflow] || (maxDistinct && hdr[kHClaims] > maxDistinct)) return;
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= T.slots) return;
  const u64 w = T.claim[i];
  if (w == 0) return;
  const u32 len = (u32)(w >> 40) & 0x1FFF;
  const u64 f = T.first[i], e = min(f + len + 1, textSize);
  atomicOr((unsigned long long*)(startBits + (f >> 6)), 1ull << (f & 63));
  for (u64 b = f; b < e;) {                                                  // (at most kMaxKey / 64 + 2 words)
    const u32 lo = (u32)(b & 63), k = (u32)min((u64)(64 - lo), e - b);
    atomicOr((unsigned long long*)(keptBits + (b >> 6)), (k == 64 ? ~0ull : (1ull << k) - 1) << lo);
    b += k;
  }
  if (f + len == textSize) hdr[kHTail] = 1;                                  // (one record at most ends there)
}

// the set bits of a tile in either bitmap -> tab[2 t], tab[2 t + 1]; a wave takes a tile
extern "C" __global__ void __launch_bounds__(256) zra_tally_sum_kernel(const u64* startBits, const u64* keptBits, u32 nTiles, u64* tab) {
  const u32 lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= nTiles) return;                                                   // (whole waves; no barrier follows)
  const u32 a = wave_sum((u32)__popcll(startBits[(size_t)t * kWords + lane])), b = wave_sum((u32)__popcll(keptBits[(size_t)t * kWords + lane]));
  if (lane == 0) { tab[2 * (size_t)t] = a; tab[2 * (size_t)t + 1] = b; }
}

// ONE workgroup: the tiles' counts become the number of the first key of each tile and the offset of its bytes in dKeys; the totals
// are the distinct keys and the size of the key text, with the delimiter (order) owes the text's last record
extern "C" __global__ void __launch_bounds__(1024) zra_tally_scan_kernel(u64* tab, u32 nTiles, u64* hdr) {
  scan_in_place<2>(tab, nTiles, nullptr, hdr + kHDistinct);
  if (threadIdx.x == 0 && hdr[kHTail]) hdr[kHKeyBytes] += 1;
}

// per occupied slot: the key's entry, at the tile's base + the keys that start in front of it inside its tile
extern "C" __global__ void __launch_bounds__(256) zra_tally_emit_kernel(TallyTable T, const u64* startBits, const u64* tab, Entry* entries, u64 entryCap) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= T.slots) return;
  const u64 w = T.claim[i];
  if (w == 0) return;
  const u64 f = T.first[i], word = f >> 6, w0 = (f / kTile) * kWords;
  u64 at = tab[2 * (f / kTile)];
  for (u64 x = w0; x < word; x++) at += (u32)__popcll(startBits[x]);         // (fewer than kWords)
  at += (u32)__popcll(startBits[word] & ((1ull << (f & 63)) - 1));
  if (at < entryCap) { Entry e; e.offset = f; e.size = (w >> 40) & 0x1FFF; e.count = T.count[i]; entries[at] = e; }
}

// per tile: the kept bytes of the text, packed behind the tile's base, clamped to the capacity
extern "C" __global__ void __launch_bounds__(256) zra_tally_copy_kernel(const u8* text, const u64* keptBits, const u64* tab, const u64* hdr, u8* dKeys, u64 keyCap, u32 delim) {
  __shared__ u32 sWave[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0 && hdr[kHTail]) { const u64 at = hdr[kHKeyBytes] - 1; if (at < keyCap) dKeys[at] = (u8)delim; }
  const u64 base = tab[2 * (size_t)blockIdx.x + 1];
  if (tab[2 * (size_t)blockIdx.x + 3] == base || base >= keyCap) return;     // (uniform: the table is not written in this launch)
  u32 k16 = ((const u16*)(keptBits + (size_t)blockIdx.x * kWords))[tid];
  const u32 c = (u32)__popc(k16), incl = wave_incl_scan(c);
  if (lane == 63) sWave[wave] = incl;
  __syncthreads();
  u64 at = base + incl - c;
  for (u32 x = 0; x < wave; x++) at += sWave[x];
  const u64 p = (u64)blockIdx.x * kTile + 16 * tid;
  for (; k16; at++) { const u32 b = (u32)__builtin_ctz(k16); k16 &= k16 - 1; if (at < keyCap) dKeys[at] = text[p + b]; }
}

// =================================================================================================
namespace zra_eng {

struct TallyImpl {
  static Status run(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dText, size_t textSize, uint32_t delim, uint64_t maxDistinct, uint64_t* hEntries,
                    size_t entryCap, uint8_t* dKeys, size_t keyCap, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize);
};

Status Engine::tally_records(const uint8_t* dText, size_t textSize, uint32_t delimiter, uint64_t maxDistinct, uint64_t* hEntries, size_t entryCap, uint8_t* dKeys,
                             size_t keyCap, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize) {
  // (rules 4 and 5 keep the words: they say what the call needs)
  return entry_call(callStats_[kCallTally], &callMs_[kCallTally], {{nRecords, 1}, {nDistinct, 1}, {nSkipped, 1}, {keySize, 1}}, true, [&] {
    return TallyImpl::run(*this, callStats_[kCallTally], &callMs_[kCallTally], dText, textSize, delimiter, maxDistinct, hEntries, entryCap, dKeys, keyCap, nRecords,
                          nDistinct, nSkipped, keySize);
  });
}
void Engine::tally_clear() { for (auto& v : callStats_[kCallTally]) v = 0; callMs_[kCallTally] = 0; }

Status TallyImpl::run(Engine& E, uint64_t (&stats)[8], double* ms, const uint8_t* dText, size_t textSize, uint32_t delim, uint64_t maxDistinct, uint64_t* hEntries,
                      size_t entryCap, uint8_t* dKeys, size_t keyCap, uint64_t* nRecords, uint64_t* nDistinct, uint64_t* nSkipped, uint64_t* keySize) {
  static_assert(sizeof(Entry) == 24, "ZraHipTallyEntry");
  // ---- 1. arguments
  if (!nRecords || !nDistinct || !nSkipped || !keySize || (!dText && textSize) || (!hEntries && entryCap) || (!dKeys && keyCap) || delim > 0xFF) return zerr(42);
  if (textSize >= kOffMask) return zerr(42);                                 // ((table): an offset + 1 has 40 bits)
  if (keyCap && textSize) {
    const uintptr_t k = (uintptr_t)dKeys, t = (uintptr_t)dText;
    if (k < t + textSize && t < k + keyCap) return zerr(42);
  }
  // ---- 2. the empty text
  if (textSize == 0) return ok();
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  const bool timed = E.call_events();
  auto begin = [&] { if (timed && hipEventRecord(E.evCall_[0], s) != hipSuccess) (void)hipGetLastError(); };
  auto end = [&]() -> Status {                                               // the launches since begin(): synchronised, their time added
    if (timed && hipEventRecord(E.evCall_[1], s) != hipSuccess) (void)hipGetLastError();
    HIPCHK_CLR(hipStreamSynchronize(s));
    if (timed) *ms += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
    return ok();
  };
  // ---- 3. scratch, in two steps: the record count sizes the table
  const uint64_t nTiles64 = (textSize + kTile - 1) / kTile;
  const uint32_t nTiles = (uint32_t)nTiles64;
  uint64_t h[kHWords] = {};
  if (!E.tally_.hdr.reserve(sizeof h)) return zerr(64);
  uint64_t* const hdr = E.tally_.hdr.as<uint64_t>();
  HIPCHK_CLR(hipMemsetAsync(hdr, 0, sizeof h, s));
  begin();
  hipLaunchKernelGGL(zra_tally_count_kernel, dim3((nTiles + kCountGroup - 1) / kCountGroup), dim3(256), 0, s, dText, (u64)textSize, delim, hdr);
  HIPCHK_CLR(hipGetLastError());
  HIPCHK_CLR(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
  STCHK(end());
  const uint64_t records = h[kHRecords];
  const uint64_t bound = maxDistinct ? std::min(maxDistinct, records) : records;   // (no text has more keys than records)
  uint64_t slots = 64;
  while (slots < bound + bound / 2 + 64) slots <<= 1;
  // tab[2 (tiles + 1)] | start bits | kept bits | claim | count | first: the middle four are zeros, first is all ones
  const size_t tabBytes = 16 * ((size_t)nTiles + 1), mapBytes = (size_t)nTiles * kWords * 8, colBytes = (size_t)slots * 8;
  if (!E.tally_.tables.reserve(tabBytes + 2 * mapBytes + 3 * colBytes)) return zerr(64);
  uint8_t* const tb = E.tally_.tables.as<uint8_t>();
  uint64_t* const tab = (uint64_t*)tb, * const startBits = (uint64_t*)(tb + tabBytes), * const keptBits = (uint64_t*)(tb + tabBytes + mapBytes);
  TallyTable T;
  T.claim = (uint64_t*)(tb + tabBytes + 2 * mapBytes); T.count = T.claim + slots; T.first = T.count + slots; T.slots = slots;
  begin();
  HIPCHK_CLR(hipMemsetAsync(startBits, 0, 2 * mapBytes + 2 * colBytes, s));
  HIPCHK_CLR(hipMemsetAsync(T.first, 0xFF, colBytes, s));
  const uint32_t slotGroups = (uint32_t)((slots + 255) / 256);
  hipLaunchKernelGGL(zra_tally_insert_kernel, dim3(nTiles), dim3(256), 0, s, dText, (u64)textSize, delim, (u64)E.tallyKeep_, (u64)maxDistinct, T, hdr);
  hipLaunchKernelGGL(zra_tally_mark_kernel, dim3(slotGroups), dim3(256), 0, s, T, (u64)textSize, (u64)maxDistinct, startBits, keptBits, hdr);
  hipLaunchKernelGGL(zra_tally_sum_kernel, dim3((nTiles + 3) / 4), dim3(256), 0, s, startBits, keptBits, nTiles, tab);
  hipLaunchKernelGGL(zra_tally_scan_kernel, dim3(1), dim3(1024), 0, s, tab, nTiles, hdr);
  HIPCHK_CLR(hipGetLastError());
  HIPCHK_CLR(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
  STCHK(end());
  *nRecords = records; *nSkipped = h[kHSkipped];
  // ---- 4. more keys than promised
  if (h[kHOverflow] || (maxDistinct && h[kHClaims] > maxDistinct)) { *nDistinct = records - h[kHSkipped]; *keySize = 0; return {kOutputTooSmall, 0}; }
  // ---- 5. the capacities
  const uint64_t distinct = h[kHDistinct], keyBytes = h[kHKeyBytes];
  *nDistinct = distinct; *keySize = keyBytes;
  if ((entryCap && distinct > entryCap) || (keyCap && keyBytes > keyCap)) return {kOutputTooSmall, 0};
  if ((entryCap || keyCap) && distinct) {
    if (entryCap && !E.tally_.entries.reserve((size_t)distinct * sizeof(Entry))) return zerr(64);
    begin();
    if (entryCap) hipLaunchKernelGGL(zra_tally_emit_kernel, dim3(slotGroups), dim3(256), 0, s, T, startBits, tab, E.tally_.entries.as<Entry>(), (u64)distinct);
    if (keyCap) hipLaunchKernelGGL(zra_tally_copy_kernel, dim3(nTiles), dim3(256), 0, s, dText, keptBits, tab, hdr, dKeys, (u64)keyCap, delim);
    HIPCHK_CLR(hipGetLastError());
    if (timed && hipEventRecord(E.evCall_[1], s) != hipSuccess) (void)hipGetLastError();
    if (entryCap) HIPCHK_CLR(hipMemcpyAsync(hEntries, E.tally_.entries.p, (size_t)distinct * sizeof(Entry), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    if (timed) *ms += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
  }
  const uint64_t st8[8] = {records, distinct, h[kHSkipped], keyBytes, slots, h[kHProbe], h[kHInserts], 0};
  std::copy(st8, st8 + 8, stats);
  return ok();
}

}  // namespace zra_eng
