// zra_amd — the host driver of the range scans: ZraHipSearchArchive (zra_search.hip), ZraHipSearchArchiveMulti (zra_msearch.hip), and
// the five record scans, which reach it through one call path (zra_record_scan.h): ZraHipGrepArchive (zra_grep.hip), its forms with a
// record predicate (zra_grep_where.hip) and with regular expressions (zra_grep_regex.hip), ZraHipExtractRecords (zra_extract.hip) and
// its form with regular expressions (zra_extract_regex.hip). The seven calls decode the frames of a content range a staging window at
// a time and scan the window's plaintext with kernels of their own; what they share is written once, here:
//
//   1. the fixed header comes to the host (Engine::archive_view); the range becomes frames [f0, f1]       scan_range, scan_plan
//   2. per pass of at most passSlots consecutive frames: the frames become decode jobs                   zra_search_jobs_kernel
//   3. the pass is decoded whole, checksums verified, into the staging window                            Engine::staged_pass
//   4. the call's own launches over the start positions the pass owns                                    the per-pass callback
//   5. the last M - 1 bytes seen so far move in front of slot 0 for the next pass                         zra_search_carry_kernel
//   6. the call's totals come to the host with the last synchronisation; the call reads its list, once
// Through an archive handle with a cache (ScanCacheView) steps 2 and 3 of a pass become
//   2'. the frames are split by residency, one launch: the missing ones become decode jobs, compacted in frame order,   zra_scan_split_kernel
//       the resident ones copy entries; the two counts come to the host through a pinned word (the pass's one read-back)
//   2". the resident frames are copied from their arena slots into their window slots, when there are any          zra_upd_stage_cached_kernel
//   3'. the missing frames are decoded whole, checksums verified, when there are any                              Engine::staged_pass
// on the engine's stream, in that order. Copies and jobs write different slots, each frame its own; a resident frame was decoded whole
// with status 0, a verified checksum and its exact size, so (contiguity) holds as before and the scan kernels see the same window.
// The jobs are in frame order: the first failing job is the lowest failing frame, which is by construction a missing one. The driver
// only reads the arena and the handle's table: a scan is not a read.
// The staging window (Engine::stage_, reserved kScanMaxPattern bytes larger) is  [ carry area | slot 0 | slot 1 | ... ]: slot s lies at
// s * frameSize behind the carry area. The arithmetic of a pass is zra_scan_plan.h's (host only, checked exhaustively on the CPU).
//
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
//  (contiguity) the frames of a pass are consecutive and all but the archive's last regenerate frameSize bytes (anything else is a
//      failing frame and ends the call), so the slots hold the content [passBase, passEnd) as one run, passEnd = min(U, (last frame of
//      the pass + 1) * frameSize). The scan's bounds come from that arithmetic alone: what lies behind a short last frame, and in slots a
//      smaller last pass does not fill, is plaintext of earlier passes and is never compared.
//  (carry) after pass k the carry area holds, right-aligned against slot 0, the last min(M - 1, bytes decoded so far) bytes of the
//      content decoded so far, M the longest pattern. A pass can be shorter than M - 1 bytes, so source and destination of the move
//      overlap: one workgroup reads all of its bytes, synchronises, then writes.
//  (ownership) a start position p belongs to the pass that holds content byte min(p + M - 1, hi - 1): one rule for all patterns,
//      monotone in p, so every position of [lo, hi) has one owner and a list ascends across passes whatever the pattern lengths are.
//      A pass that is not the range's last owns only p with p + M - 1 < passEnd < hi: every byte any pattern needs is there; its
//      starts begin up to M - 1 bytes inside the carry. The last pass owns every remaining start up to hi - 1 - trim: trim = 0 for a
//      call that tests pattern i only where p + m_i <= hi, trim = M - 1 for the single search, which tests only p + M <= hi.
//  (c) the launches of a call are chained by a state that ping-pongs between two words: the k-th pass whose callback runs reads word
//      k & 1 and writes word (k + 1) & 1. A list position is a prefix count, never the result of an atomic, and no workgroup waits for
//      another one. The driver returns the number of callbacks that ran: the parity of the final word.
//  (d) nothing goes to the caller's arrays before the last pass is done: a call that fails midway writes nothing.
#pragma once
#include "zra_host.h"
#include <algorithm>

namespace zra_eng {

struct ScanImpl {
  // the two searches behind Engine's entry points, each in its own file. syntax: the pattern syntax word of the ...Expr entry points
  // (zra_pattern_expr.h), 0 for the literal ones
  static Status search(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, size_t m, uint64_t offset, uint64_t size, size_t stagingBytes,
                       uint64_t* hMatches, size_t matchCap, uint64_t* nMatches, ScanCacheView* cv = nullptr);
  static Status msearch(Engine& E, const uint8_t* dArc, size_t arcSize, const uint8_t* hPat, const uint32_t* hSizes, size_t nPat, uint32_t syntax, uint64_t offset,
                        uint64_t size, size_t stagingBytes, void* hMatches, size_t matchCap, uint64_t* nMatches, uint64_t* hPerPattern, ScanCacheView* cv = nullptr);
  // the five record scans: zra_record_scan.h's one call path, instantiated with the selector and the kernel set of the file named;
  // Engine::record_scan (below) picks one by RecordCall::kind. record_scan() itself goes through call(), for the row its kernel set names
  template <class Selector, class Kernels>
  static Status record_scan(Engine& E, const RecordCall& c, ScanCacheView* cv);
  static Status grep(Engine& E, const RecordCall& c, ScanCacheView* cv);            // zra_grep.hip
  static Status grep_where(Engine& E, const RecordCall& c, ScanCacheView* cv);      // zra_grep_where.hip
  static Status grep_regex(Engine& E, const RecordCall& c, ScanCacheView* cv);      // zra_grep_regex.hip
  static Status extract(Engine& E, const RecordCall& c, ScanCacheView* cv);         // zra_extract.hip
  static Status extract_regex(Engine& E, const RecordCall& c, ScanCacheView* cv);   // zra_extract_regex.hip
  static Status grep_context(Engine& E, const RecordCall& c, ScanCacheView* cv);    // zra_grep_context.hip
  static Status grep_regex_context(Engine& E, const RecordCall& c, ScanCacheView* cv);   // zra_grep_regex_context.hip
  static Status extract_where(Engine& E, const RecordCall& c, ScanCacheView* cv);   // zra_extract_where.hip
  static Status cut(Engine& E, const RecordCall& c, ScanCacheView* cv);             // zra_cut.hip

  // What a call of the family leaves behind: entry_call's rule (zra_host.h). `which`: kScanSearch .. kScanExtract; out0 / out1: the
  // call's output words (either may be nullptr), kept on OutputTooSmall (the extract's rule 7, whose two words say what the call needs).
  template <class Run>
  static Status call(Engine& E, int which, uint64_t* out0, uint64_t* out1, Run&& run) {
    return entry_call(E.callStats_[which], &E.callMs_[which], {{out0, 1}, {out1, 1}}, true, run);
  }

  static uint8_t* window(Engine& E) { return E.stage_.as<uint8_t>() + kScanMaxPattern; }   // slot 0; the carry area lies in front of it

  // The passes of plan P over the archive `arc`. tableBytes / listBytes size the scratch pair Engine::scan_, whose `tables` begins
  // with the headBytes bytes at `head`: uploaded before the first launch (then the stream is synchronised), and its bytes [backOff,
  // backOff + backBytes), the words the call's launches add up, are copied back into `head` behind the last pass, in front of the
  // final synchronisation. perPass(const ScanPass&) launches the call's own kernels on the engine's stream, for every pass, or,
  // ownedOnly, for the passes that own a start position; *ran counts its invocations, (c). *ms gains the HIP-event time from in
  // front of a pass's callback to behind its carry move. Returns synchronised; a frame that does not decode ends the call with the
  // lowest failing frame's code of the first failing pass.
  // cv (a call through an archive handle): with slots, a pass takes its plaintext from two places (through a handle, above); without,
  // the passes are the plain call's. Either way cv's counters say what the passes did, as far as they came.
  template <class PerPass>
  static Status passes(Engine& E, const ArchiveView& arc, const ScanPlan& P, double* ms, void* head, size_t headBytes, size_t backOff, size_t backBytes,
                       size_t tableBytes, size_t listBytes, bool ownedOnly, PerPass&& perPass, uint32_t* ran, ScanCacheView* cv = nullptr) {
    const size_t jobs = (size_t)P.nSlots + 1;
    const bool cached = cv && cv->slots;
    if (!E.stage_.reserve(kScanMaxPattern + (size_t)P.window + 64) || !E.scan_.tables.reserve(tableBytes) || !E.scan_.list.reserve(listBytes) ||
        !E.frameOff_.reserve(jobs * 16) || !E.outOff_.reserve(jobs * 8) || !E.expect_.reserve(jobs * 4) || (cached && !E.upd_.copies.reserve(jobs * 16)))
      return zerr(64);
    if (!E.call_events()) return zerr(1);
    hipStream_t s = E.stream_;
    HIPCHK_CLR(hipMemcpyAsync(E.scan_.tables.p, head, headBytes, hipMemcpyHostToDevice, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    uint8_t* const win = window(E);
    // (through a handle) the pass's count words, then its copy entries, 4 words each: jobs * 16 bytes
    uint32_t* const counts = cached ? E.upd_.copies.as<uint32_t>() : nullptr, * const copies = cached ? counts + 4 : nullptr;
    uint32_t carry = 0;
    bool timed = false, stageTimed = false;
    // (behind a synchronisation of the stream)
    auto take_time = [&]() {
      if (timed) *ms += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
      if (stageTimed) cv->stageMs += Engine::elapsed_ms(E.evCall_[4], E.evCall_[5]);
      timed = stageTimed = false;
    };
    *ran = 0;
    for (uint64_t p = 0; p < P.passes; p++) {
      const ScanPass ps = scan_pass(P, p, carry);
      uint32_t nDec = ps.nj;
      uint64_t decBytes = ps.L;
      if (cached) {
        HIPCHK_CLR(hipEventRecord(E.evCall_[2], s));
        scan_launch_split(s, cv->slotOf, cv->frames, arc.table, P.fs, P.U, ps.first, ps.nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(),
                          E.expect_.as<uint32_t>(), copies, counts);
        HIPCHK_CLR(hipEventRecord(E.evCall_[3], s));
        HIPCHK_CLR(hipMemcpyAsync(cv->pin, counts, 16, hipMemcpyDeviceToHost, s));
        HIPCHK_CLR(hipStreamSynchronize(s));
        HIPCHK_CLR(hipGetLastError());
        take_time();
        cv->stageMs += Engine::elapsed_ms(E.evCall_[2], E.evCall_[3]);
        nDec = cv->pin[0];
        const uint32_t nCopy = cv->pin[1];
        decBytes = (uint64_t)cv->pin[2] | (uint64_t)cv->pin[3] << 32;
        if (nCopy) {
          HIPCHK_CLR(hipEventRecord(E.evCall_[4], s));
          upd_launch_stage_cached(s, copies, nCopy, 0, P.fs, cv->arena, win);
          HIPCHK_CLR(hipEventRecord(E.evCall_[5], s));
          stageTimed = true;
          cv->staged += nCopy;
        }
      }
      if (nDec) {                                                      // (always, without a handle's cache: a pass has a frame)
        if (!cached)
          search_launch_jobs(s, arc.table, P.fs, P.U, ps.first, ps.nj, E.frameOff_.as<uint64_t>(), E.outOff_.as<uint64_t>(), E.expect_.as<uint32_t>());
        unsigned long long firstError;
        const Status st = E.staged_pass(arc, 0, nDec, win, &firstError);
        take_time();
        if (st.zra) return st;
        if (firstError != ~0ull) return zerr(reported_code(firstError));
      }
      if (cv) { cv->decoded += nDec; cv->decodedBytes += decBytes; cv->passes++; }
      HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
      if (!ownedOnly || ps.nPos) { perPass(ps); ++*ran; }
      if (!ps.lastPass && P.M > 1) search_launch_carry(s, win, ps.L, ps.carry);
      carry = ps.carry;
      HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
      timed = true;
    }
    HIPCHK_CLR(hipMemcpyAsync((uint8_t*)head + backOff, E.scan_.tables.as<uint8_t>() + backOff, backBytes, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    HIPCHK_CLR(hipGetLastError());
    take_time();
    return ok();
  }

  // words [1] and [2] of a call's counters: the decode jobs and the bytes they regenerated. Without a handle every frame of the
  // range is one; through a handle the frames staged from its arena are left out
  static uint64_t decoded_frames(const ScanPlan& P, const ScanCacheView* cv) { return cv ? cv->decoded : P.n; }
  static uint64_t decoded_bytes(const ScanPlan& P, const ScanCacheView* cv) {
    return cv ? cv->decodedBytes : std::min<uint64_t>(P.U, (P.f1 + 1) * P.fs) - P.f0 * P.fs;
  }
  // the header step of a call: read and checked (the statuses of ZraHipArchiveOpen), or, through a handle, the one it checked at open
  static Status view(Engine& E, const uint8_t* dArc, size_t arcSize, const ScanCacheView* cv, ArchiveView* arc) {
    if (cv) { *arc = ArchiveView::over(cv->h, dArc, arcSize); return ok(); }
    return E.archive_view(dArc, arcSize, arc);
  }
};

// the one entry of the five record scans
inline Status Engine::record_scan(const RecordCall& c, ScanCacheView* cv) {
  switch (c.kind) {
    case kRecGrep: return ScanImpl::grep(*this, c, cv);
    case kRecGrepWhere: return ScanImpl::grep_where(*this, c, cv);
    case kRecGrepRegex: return ScanImpl::grep_regex(*this, c, cv);
    case kRecExtract: return ScanImpl::extract(*this, c, cv);
    case kRecExtractRegex: return ScanImpl::extract_regex(*this, c, cv);
    case kRecGrepContext: return ScanImpl::grep_context(*this, c, cv);
    case kRecGrepRegexContext: return ScanImpl::grep_regex_context(*this, c, cv);
    case kRecExtractWhere: return ScanImpl::extract_where(*this, c, cv);
    case kRecCut: return ScanImpl::cut(*this, c, cv);
  }
  return zerr(42);
}

}  // namespace zra_eng
