// zra_amd — grep of a device-resident archive (zra_hip.h: ZraHipGrepArchive): the records of a content range, cut at a delimiter byte,
// that hold a match of one of up to 64 byte patterns (or, inverted, none), as ascending {offset, size} pairs, without an output buffer
// for the content. What `grep -F -f patterns -b` (and `-v`, `-c`) is to `zstdgrep`: the lines, not the offsets of the hits.
//
// The passes are those of zra_msearch.hip (header, jobs per pass, Engine::staged_pass, the staging window [ carry area | slot 0 | ... ],
// the carry move; search_launch_jobs and search_launch_carry are used as they are), its conditions (contiguity), (carry) with m = M,
// (ownership) and (filter) hold word for word, and the pattern table and the test of one position are the same code (zra_patterns.h).
// What differs:
//  (stream) the positions of [lo, hi) form one ascending stream, a pass owns the positions the multi search gives it, and a position
//      carries two flags that are both evaluated by its owner: `delimiter` (its byte, read from the carry area as often as from a slot)
//      and `hit` (a match starts here: position_mask != 0). No pattern holds the delimiter, so the two exclude each other and an
//      occurrence lies inside one record.
//  (forward) a record belongs to the delimiter that ENDS it, the last one to hi. What a delimiter needs from in front of it is the
//      position behind the previous delimiter and the OR of the hit flags since then. Nothing is ever patched later: what crosses a
//      trip, a wave, a tile or a pass is the pair (start of the open record, has it matched yet).
//  (summary) a run of positions (a trip's 64, a wave's 2,048, a tile, a lane's run of tiles in the scan) reduces to
//      {has a delimiter, hit in front of the first one, hit behind the last one, position behind the last one, records selected among
//      those that end inside it APART from the first}. Without a delimiter the two hit bits are both "a hit anywhere". Two runs
//      combine associatively (combine() below): the record that the second run's first delimiter ends is selected by
//      (hit behind A's last | hit in front of B's first) ^ invert and joins the sum.
//  (launches) zra_grep_count_kernel: per tile its summary, per call the order-independent totals (matches, delimiters) as atomics.
//      zra_grep_scan_kernel, ONE workgroup: the summaries become per tile {list base, start of the record open at the tile's head, its
//      hit bit}, and the state carried between passes {open record's start, its hit bit, records selected so far} moves on from word
//      k & 1 to word (k + 1) & 1 of a ping-pong pair, the search's condition (c). The last pass's scan ends the open record at hi.
//      zra_grep_fill_kernel: the workgroups redo the tiles that hold a listed record and write the pairs.
//  (order) a list position is a prefix count (the state's count, plus the tiles in front, plus the waves in front, plus the wave's
//      earlier trips, plus the selected lanes below), never the result of an atomic. No workgroup waits for another one: no spin-wait,
//      no look-back; the dependency runs through the launches.
//  (d) nothing goes to the caller's array before the last pass is done: a call that fails midway writes nothing.
#include "zra_patterns.h"

namespace {
// (summary). flags: 1 a delimiter, 2 a hit in front of the first delimiter, 4 a hit behind the last; last: the content offset behind
// the last delimiter
struct __attribute__((aligned(16))) Sum { u64 last; u32 sel, flags; };
// what the scan makes of it for the fill: the list position of the tile's first record, the start of the record open at its head with
// that record's hit bit in bit 63
struct __attribute__((aligned(16))) Head { u64 base, open; };
// the state carried from pass to pass; tail: the last pass ended an open record at hi
struct State { u64 start, hit, sel, tail; };
// The words the launches of a call add up, uploaded with the table: the ping-pong state (c), then the atomics.
struct Totals { State st[2]; u64 matches, delims, pad[6]; };
struct __attribute__((aligned(16))) Range { u64 offset, size; };   // ZraHipContentRange
constexpr u64 kHitBit = 1ull << 63;

// the summary of run A followed by run B. sel is kept wide by the scan: selA + selB + the record B's first delimiter ends
__device__ __forceinline__ void combine(u32& fA, u64& selA, u64& lastA, u32 fB, u64 selB, u64 lastB, u32 inv) {
  if (!(fB & 1)) { if (fB & 2) fA |= (fA & 1) ? 4u : 6u; return; }
  if (!(fA & 1)) { fA = 1 | ((fA | fB) & 2) | (fB & 4); selA = selB; lastA = lastB; return; }
  selA += selB + ((((fA >> 2) | (fB >> 1)) & 1) ^ inv);
  fA = 1 | (fA & 2) | (fB & 4); lastA = lastB;
}

// A wave's walk over its trips. Count: seen = false, and the record that the wave's first delimiter ends is left to whoever combines
// the summaries (hitFirst says whether it matched inside the wave). Fill: seen = true, hit and start come from in front of the wave.
struct Walk { bool seen, hit, hitFirst; u32 sel; u64 start; };

// One trip: dm / hm = the ballots of the two flags, pos = the content offset of lane 0's position. kEmit: the selected records that
// end in the trip go to list[at + ...] while there is room; at moves on.
template <bool kEmit>
__device__ __forceinline__ void walk_trip(Walk& s, u64 dm, u64 hm, u32 lane, u32 inv, u64 pos, u64& at, Range* list, u64 cap) {
  if (dm == 0) { s.hit |= hm != 0; return; }                                 // (uniform in the wave)
  const u32 first = (u32)__builtin_ctzll(dm), last = 63 - (u32)__builtin_clzll(dm);
  const u64 below = (1ull << lane) - 1, dBelow = dm & below;
  const u32 prev = dBelow ? 63 - (u32)__builtin_clzll(dBelow) : 0;           // the delimiter in front of this lane, inside the trip
  const u64 seg = dBelow ? hm & below & ~((2ull << prev) - 1) : hm & below;  // the hits between it (or the trip's head) and this lane
  const bool hit = seg != 0 || (!dBelow && s.hit);
  const bool sel = ((dm >> lane) & 1) && (hit != (bool)inv) && (s.seen || lane != first);
  const u64 sm = __ballot(sel);
  if (kEmit) {
    const u64 idx = at + (u32)__popcll(sm & below);
    if (sel && idx < cap) {
      const u64 start = dBelow ? pos + prev + 1 : s.start;
      Range r; r.offset = start; r.size = pos + lane - start;
      list[idx] = r;
    }
    at += (u32)__popcll(sm);
  }
  s.sel += (u32)__popcll(sm);
  if (!s.seen) { s.hitFirst = s.hit || (hm & ((1ull << first) - 1)) != 0; s.seen = true; }
  s.hit = last < 63 && (hm >> (last + 1)) != 0;
  s.start = pos + last + 1;
}

__device__ __forceinline__ Sum walk_sum(const Walk& s) {
  Sum r;
  r.last = s.start; r.sel = s.sel;
  r.flags = s.seen ? 1u | (s.hitFirst ? 2u : 0u) | (s.hit ? 4u : 0u) : (s.hit ? 6u : 0u);
  return r;
}

// The two ballots of trip t of this wave (tile position j = w0 + 64 t + lane; d = the index of the tile's first byte in sTile; toHi =
// the bytes of the range at and behind the tile's first position), and the lane's matches as (position, pattern) pairs.
__device__ __forceinline__ void trip_flags(const Table* sT, const u32* sTile, u32 d, u32 j, u32 n, long long toHi, u32 delim, u64* dm, u64* hm, u32* pairs) {
  bool isD = false, hit = false;
  if (j < n) {
    isD = (lds_word(sTile, d + j) & 0xFF) == delim;
    bool surv;
    const u64 mask = position_mask(sT, sTile, d + j, (u32)min(toHi - (long long)j, (long long)kMaxPattern), &surv);
    hit = mask != 0;
    *pairs += (u32)__popcll(mask);
  }
  *dm = __ballot(isD);
  *hm = __ballot(hit);
}
}  // namespace

// The run of a pass as the multi search sees it: win = slot 0, position x is the byte win[x]; the positions of the pass are xLo + [0,
// nPos), xHi is the position of the range's end (hi - passBase), M the longest pattern, p0 the content offset of position xLo.
// Workgroup g takes the tiles [g * kGroup, (g + 1) * kGroup): per tile its summary -> sums[tile]; per call the totals.
extern "C" __global__ void __launch_bounds__(256) zra_grep_count_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                        u32 inv, u64 p0, Sum* sums, Totals* tot) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ Table sT;
  __shared__ Sum sW[4];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  stage_table(tbl, &sT);
  u32 pairs = 0, delims = 0;
  for (u32 b = blockIdx.x * kGroup, bEnd = min(tiles, b + kGroup); b < bEnd; b++) {
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();                                                         // (the tile in front is done with)
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    Walk s = {false, false, false, 0, p0 + t0 + w0};
    u64 at = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      trip_flags(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      delims += (u32)__popcll(dm);
      walk_trip<false>(s, dm, hm, lane, inv, p0 + t0 + w0 + t * 64, at, nullptr, 0);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (tid == 0) {
      u32 f = sW[0].flags; u64 sel = sW[0].sel, last = sW[0].last;
      for (u32 w = 1; w < 4; w++) combine(f, sel, last, sW[w].flags, sW[w].sel, sW[w].last, inv);
      Sum r; r.last = last; r.sel = (u32)sel; r.flags = f;
      sums[b] = r;
    }
  }
  pairs = wave_sum(pairs);
  if (lane == 0 && pairs) atomicAdd((unsigned long long*)&tot->matches, (unsigned long long)pairs);
  if (lane == 0 && delims) atomicAdd((unsigned long long*)&tot->delims, (unsigned long long)delims);   // (a ballot's count: the same in every lane)
}

// One workgroup: (launches). Every lane reduces a run of consecutive tiles, the 1024 summaries are scanned in LDS (Hillis-Steele over
// combine()), then the lane walks its run again from the state in front of it: heads[t], and sums[t].sel becomes ALL the selected
// records that end in tile t, the first included (what the fill skips a tile by). lastPass: the record open at hi ends there.
extern "C" __global__ void __launch_bounds__(1024) zra_grep_scan_kernel(Sum* sums, u32 nTiles, Head* heads, const State* in, State* out, u32 inv, u32 lastPass, u64 hi,
                                                                        Range* list, u64 cap) {
  __shared__ u64 sSel[1024], sLast[1024];
  __shared__ u32 sF[1024];
  const u32 tid = threadIdx.x;
  const u32 per = (nTiles + 1023) / 1024;
  const u32 b0 = min(nTiles, tid * per), b1 = min(nTiles, b0 + per);
  u32 f = 0; u64 sel = 0, last = 0;
  for (u32 t = b0; t < b1; t++) { const Sum s = sums[t]; combine(f, sel, last, s.flags, s.sel, s.last, inv); }
  sF[tid] = f; sSel[tid] = sel; sLast[tid] = last;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    u32 fa = 0; u64 sa = 0, la = 0;
    if (tid >= d) { fa = sF[tid - d]; sa = sSel[tid - d]; la = sLast[tid - d]; }
    __syncthreads();
    if (tid >= d) { combine(fa, sa, la, f, sel, last, inv); f = fa; sel = sa; last = la; sF[tid] = f; sSel[tid] = sel; sLast[tid] = last; }
    __syncthreads();
  }
  // the state in front of this lane's run: the carried one, then the lanes in front
  u64 start = in->start, count = in->sel;
  bool hit = in->hit != 0;
  if (tid) {
    const u32 fe = sF[tid - 1];
    if (fe & 1) { count += sSel[tid - 1] + ((u32)(hit || (fe & 2)) ^ inv); hit = (fe & 4) != 0; start = sLast[tid - 1]; }
    else hit |= (fe & 2) != 0;
  }
  for (u32 t = b0; t < b1; t++) {
    const Sum s = sums[t];
    Head h; h.base = count; h.open = start | (hit ? kHitBit : 0);
    heads[t] = h;
    if (s.flags & 1) {
      const u32 all = s.sel + ((u32)(hit || (s.flags & 2)) ^ inv);
      sums[t].sel = all;
      count += all; hit = (s.flags & 4) != 0; start = s.last;
    } else hit |= (s.flags & 2) != 0;
  }
  if (tid == 1023) {                                                         // (its run is the last one, or empty behind the last one)
    u64 tail = 0;
    if (lastPass && start < hi) {
      tail = 1;
      if ((u32)hit != inv) {
        if (count < cap) { Range r; r.offset = start; r.size = hi - start; list[count] = r; }
        count++;
      }
    }
    State o; o.start = start; o.hit = hit; o.sel = count; o.tail = tail;
    *out = o;
  }
}

// The count's workgroups redo the tiles that hold a listed record (a tile without a selected record, or behind the list's capacity, is
// skipped; a workgroup without such a tile leaves at once): the ballots of every trip go to LDS with the waves' summaries, a wave takes
// what lies in front of it from the tile's head and the waves in front, and walks its trips again, writing.
extern "C" __global__ void __launch_bounds__(256) zra_grep_fill_kernel(const u8* win, long long xLo, long long xHi, u64 nPos, u32 M, const Table* tbl, u32 delim,
                                                                       u32 inv, u64 p0, const Sum* sums, const Head* heads, Range* list, u64 cap) {
  __shared__ __attribute__((aligned(16))) u32 sTile[kLdsWords];
  __shared__ Table sT;
  __shared__ Sum sW[4];
  __shared__ u64 sMask[4][kWaveIters][2];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w0 = wave * kWavePos;
  const u32 tiles = (u32)((nPos + kTile - 1) / kTile);
  const u32 bBegin = blockIdx.x * kGroup, bEnd = min(tiles, bBegin + kGroup);
  bool any = false;                                                          // (uniform in the workgroup, like `listed` below)
  for (u32 b = bBegin; b < bEnd; b++) any |= sums[b].sel != 0 && heads[b].base < cap;
  if (!any) return;
  stage_table(tbl, &sT);
  for (u32 b = bBegin; b < bEnd; b++) {
    const Head head = heads[b];
    const bool listed = sums[b].sel != 0 && head.base < cap;
    if (!listed) continue;
    const u64 t0 = (u64)b * kTile;
    const u32 n = (u32)min((u64)kTile, nPos - t0);
    const long long x0 = xLo + (long long)t0, toHi = xHi - x0;
    __syncthreads();
    const u32 d = stage_tile(win + x0, (u32)min((long long)(n + M - 1), toHi), sTile);
    __syncthreads();
    Walk s = {false, false, false, 0, p0 + t0 + w0};
    u64 at = 0;
    u32 pairs = 0;
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++) {
      u64 dm, hm;
      trip_flags(&sT, sTile, d, w0 + t * 64 + lane, n, toHi, delim, &dm, &hm, &pairs);
      if (lane == 0) { sMask[wave][t][0] = dm; sMask[wave][t][1] = hm; }
      walk_trip<false>(s, dm, hm, lane, inv, p0 + t0 + w0 + t * 64, at, nullptr, 0);
    }
    if (lane == 0) sW[wave] = walk_sum(s);
    __syncthreads();
    if (!(sW[wave].flags & 1)) continue;                                     // (uniform in the wave; the barriers are at the loop's head)
    Walk e = {true, (head.open & kHitBit) != 0, false, 0, head.open & ~kHitBit};
    at = head.base;
    for (u32 w = 0; w < wave; w++) {
      const Sum v = sW[w];
      if (v.flags & 1) { at += v.sel + ((u32)(e.hit || (v.flags & 2)) ^ inv); e.hit = (v.flags & 4) != 0; e.start = v.last; }
      else e.hit |= (v.flags & 2) != 0;
    }
    if (at >= cap) continue;
#pragma unroll 1
    for (u32 t = 0; t < kWaveIters && w0 + t * 64 < n; t++)
      walk_trip<true>(e, sMask[wave][t][0], sMask[wave][t][1], lane, inv, p0 + t0 + w0 + t * 64, at, list, cap);
  }
}

// =================================================================================================
namespace zra_eng {

struct GrepImpl {
  static Status run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint8_t delimiter, uint32_t mode,
                    uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap, uint64_t* nRecords);
};

Status Engine::grep_archive(const uint8_t* dArc, size_t arcSize, const void* hPatterns, const uint32_t* hPatternSizes, size_t nPatterns, uint8_t delimiter,
                            uint32_t mode, uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap, uint64_t* nRecords) {
  for (auto& v : rstats_) v = 0;
  grepScanMs_ = 0;
  if (nRecords) *nRecords = 0;
  return GrepImpl::run(*this, dArc, arcSize, (const uint8_t*)hPatterns, hPatternSizes, nPatterns, delimiter, mode, offset, size, stagingBytes, hRecords,
                       recordCap, nRecords);
}

Status GrepImpl::run(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint8_t delimiter, uint32_t mode,
                     uint64_t offset, uint64_t size, size_t stagingBytes, uint64_t* hRecords, size_t recordCap, uint64_t* nRecords) {
  // ---- 1. arguments
  if (!nRecords || !hPat || !hSizes || (!dArc && arcSize) || (!hRecords && recordCap) || (mode & ~1u)) return zerr(42);
  uint32_t M = 0, mMin = kMaxPattern;
  if (!pattern_sizes_ok(hSizes, nPat, &M, &mMin)) return zerr(42);
  {
    size_t bytes = 0;
    for (size_t i = 0; i < nPat; i++) bytes += hSizes[i];
    if (std::memchr(hPat, delimiter, bytes)) return zerr(42);                // (an occurrence lies inside one record)
  }
  const uint32_t inv = mode & 1u;
  HIPCHK_CLR(hipSetDevice(E.device_));
  hipStream_t s = E.stream_;
  E.reset_decode_stats();
  // ---- 2. header: the statuses of ZraHipArchiveOpen, as the search
  ArchiveView arc;
  { Status st = E.archive_view(dArc, arcSize, &arc); if (st.zra) return st; }
  const uint32_t F = arc.frames;
  const uint64_t fs = arc.fs, U = arc.U;
  // ---- 3. the range [lo, hi), inclusive bound
  if (offset > U || (size != ~0ull && (offset + size < offset || offset + size > U))) return {kOutOfBounds, 0};
  const uint64_t lo = offset, hi = size == ~0ull ? U : offset + size;
  if (hi == lo || (!inv && hi - lo < mMin)) { E.rstats_[0] = F; return ok(); }   // no record, or none that could hold a match
  if (fs == 0 || F == 0) return {kHeaderInvalid, 0};
  const uint64_t f0 = lo / fs, f1 = (hi - 1) / fs, n = f1 - f0 + 1;
  // ---- 4. scratch
  const uint32_t passSlots = pass_slots(fs, stagingBytes);
  const uint32_t nSlots = (uint32_t)std::min<uint64_t>(passSlots, n);
  const uint64_t passes = (n + passSlots - 1) / passSlots;
  const uint64_t window = (uint64_t)nSlots * fs;
  // (the last pass owns up to M - 1 positions inside the carry area on top of a window's worth)
  const size_t tilesMax = (size_t)((window + kMaxPattern + kTile - 1) / kTile);
  const size_t listCap = (size_t)std::min<uint64_t>(recordCap, hi - lo);     // (no list is longer: a record per delimiter, or the one open at hi)
  // tables: Table | Totals | sums[tiles] | heads[tiles]
  constexpr size_t kHead = sizeof(Table) + 64 + sizeof(Totals);
  static_assert(kHead % 16 == 0 && sizeof(Sum) == 16 && sizeof(Head) == 16 && sizeof(Range) == 16, "16-byte entries behind a 16-byte head");
  if (!E.stage_.reserve(kMaxPattern + (size_t)window + 64) || !E.grep_.tables.reserve(kHead + tilesMax * (sizeof(Sum) + sizeof(Head)) + 64) ||
      !E.grep_.list.reserve(listCap * sizeof(Range) + 64) || !E.frameOff_.reserve(((size_t)nSlots + 1) * 16) ||
      !E.outOff_.reserve(((size_t)nSlots + 1) * 8) || !E.expect_.reserve(((size_t)nSlots + 1) * 4))
    return zerr(64);
  if (!E.call_events()) return zerr(1);
  uint8_t* const win = E.stage_.as<uint8_t>() + kMaxPattern;                // slot 0; the carry area lies in front of it
  uint8_t* const tb = E.grep_.tables.as<uint8_t>();
  const Table* const tbl = (const Table*)tb;
  Totals* const tot = (Totals*)(tb + sizeof(Table) + 64);
  Sum* const sums = (Sum*)(tb + kHead);
  Head* const heads = (Head*)(sums + tilesMax);
  Range* const list = E.grep_.list.as<Range>();
  {
    std::vector<uint8_t> head(kHead, 0);                                     // (the totals go up as zeros, the state as "a record opens at lo")
    build_table(*(Table*)head.data(), hPat, hSizes, nPat);
    ((Totals*)(head.data() + sizeof(Table) + 64))->st[0].start = lo;
    HIPCHK_CLR(hipMemcpyAsync(tb, head.data(), kHead, hipMemcpyHostToDevice, s));
    HIPCHK_CLR(hipStreamSynchronize(s));                                    // (`head` goes out of scope)
  }
  // ---- passes
  uint32_t launches = 0, carry = 0;
  bool timed = false;
  // (behind a synchronisation of the stream)
  auto take_time = [&]() { if (timed) E.grepScanMs_ += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]); timed = false; };
  for (uint64_t p = 0; p < passes; p++) {
    const uint64_t first = f0 + p * passSlots;
    const uint32_t nj = (uint32_t)std::min<uint64_t>(passSlots, n - p * passSlots);
    search_launch_jobs(s, arc.table, fs, U, first, nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
    unsigned long long firstError;
    Status st = E.staged_pass(arc, 0, nj, win, &firstError);
    take_time();
    if (st.zra) { E.grepScanMs_ = 0; return st; }
    if (firstError != ~0ull) {                                              // the lowest failing frame of the first failing pass
      E.grepScanMs_ = 0;
      return zerr(reported_code(firstError));
    }
    // (contiguity) the run of this pass, and (ownership) the positions it owns, relative to slot 0
    const bool lastPass = p + 1 == passes;
    const uint64_t passBase = first * fs, passEnd = std::min<uint64_t>(U, (first + nj) * fs), L = passEnd - passBase;
    const long long xLo = lo > passBase ? (long long)(lo - passBase) : -(long long)std::min<uint64_t>(M - 1, passBase - lo);
    const long long xHi = (long long)(hi - passBase);
    const long long xEnd = lastPass ? xHi : (long long)L - (long long)M + 1;
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    if (xEnd > xLo) {                                                        // (the last pass always: it holds byte hi - 1)
      const uint64_t nPos = (uint64_t)(xEnd - xLo), p0 = passBase + xLo;
      const uint32_t tiles = (uint32_t)((nPos + kTile - 1) / kTile), groups = (tiles + kGroup - 1) / kGroup;
      hipLaunchKernelGGL(zra_grep_count_kernel, dim3(groups), dim3(256), 0, s, win, xLo, xHi, (u64)nPos, M, tbl, (u32)delimiter, inv, (u64)p0, sums, tot);
      hipLaunchKernelGGL(zra_grep_scan_kernel, dim3(1), dim3(1024), 0, s, sums, tiles, heads, tot->st + (launches & 1), tot->st + ((launches + 1) & 1), inv,
                         (u32)lastPass, (u64)hi, list, (u64)listCap);
      launches++;
      if (listCap)
        hipLaunchKernelGGL(zra_grep_fill_kernel, dim3(groups), dim3(256), 0, s, win, xLo, xHi, (u64)nPos, M, tbl, (u32)delimiter, inv, (u64)p0, sums, heads, list,
                           (u64)listCap);
    }
    if (!lastPass && M > 1) {
      carry = (uint32_t)std::min<uint64_t>(M - 1, carry + L);
      search_launch_carry(s, win, L, carry);
    }
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    timed = true;
  }
  // ---- the totals, then the list, once
  Totals h;
  std::memset(&h, 0, sizeof(h));
  HIPCHK_CLR(hipMemcpyAsync(&h, tot, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHK_CLR(hipStreamSynchronize(s));
  HIPCHK_CLR(hipGetLastError());
  take_time();
  const State& fin = h.st[launches & 1];
  const uint64_t total = fin.sel;
  const size_t nOut = (size_t)std::min<uint64_t>(total, listCap);
  if (nOut) {
    HIPCHK_CLR(hipMemcpyAsync(hRecords, list, nOut * sizeof(Range), hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
  }
  *nRecords = total;
  const uint64_t st8[8] = {F, n, std::min<uint64_t>(U, (f1 + 1) * fs) - f0 * fs, h.delims + fin.tail, total, nOut, passes, h.matches};
  for (int i = 0; i < 8; i++) E.rstats_[i] = st8[i];
  return ok();
}

}  // namespace zra_eng
