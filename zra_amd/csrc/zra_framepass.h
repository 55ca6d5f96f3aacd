// zra_amd — the host driver of the device-archive calls that decode whole frames a staging window at a time and run launches of their
// own over the window: ZraHipCompareArchives and ZraHipDiffArchives (zra_compare.hip), ZraHipSignArchive and ZraHipDiffSignature
// (zra_sign.hip), ZraHipIndexRecords (zra_records.hip). What their passes share is written once, here; the arithmetic of a pass is
// zra_pass_plan.h's (host only, checked exhaustively on the CPU). Not here: the range scans (zra_scan.h, with a carry area and a
// handle's cache), the verify's passes (they read every job's own status word) and the locate sweep (zra_records.hip says why).
//
// A pass of a plan (FramePasses::run), on the engine's stream, in this order:
//   1. the caller's `before` launches: the sign call's span hash, the flags and jobs of a flagged pass
//   2. (plain pass) the frames [first, first + nj) become decode jobs 0 .. nj - 1, frame first + k into slot k      search_launch_jobs
//   3. evCall_[1] is recorded
//   4. (flagged pass) the job count comes to the host: a 4-byte copy, a synchronisation, the time is taken
//   5. the jobs are decoded whole, checksums verified, for each side into its window                               Engine::staged_pass
//      (flagged pass, no job: the decoder is not launched); (plain pass) the time is taken
//   6. evCall_[0] is recorded
//   7. the caller's `after` launches, over the window(s)
// and behind the last pass (FramePasses::finish): evCall_[1] is recorded, the call's header words come to the host, the stream is
// synchronised, the time is taken.
// Through an archive handle with a cache (Side::cv with slots, the index alone; zra_scan.h has the same steps as 2', 2", 3') step 2 of
// a PLAIN pass becomes
//   2a. evCall_[1] is recorded; the frames [first, first + nj) are split by residency, one launch: the missing ones become decode jobs,
//       compacted in frame order, frame first + k still into slot k, the resident ones copy entries               scan_launch_split
//   2b. the pass's four count words come to the host through the handle's pinned words: a 16-byte copy, a synchronisation, the time is taken
//   2c. the resident frames are copied from their arena slots into their window slots, when there are any         upd_launch_stage_cached
// and step 5 decodes the missing frames only (none: the decoder is not launched). Copies and jobs write different slots, each frame its
// own, so `after` sees the window of the plain pass. The driver only reads the arena and the handle's table: a pass is not a read.
// A view on a flagged pass, or on a second side, is refused ({ZStdError, 1}): the flags of a flagged pass would have to be split too.
// A PLAIN pass decodes every frame of the pass; the host knows the job count, so the pass has no read-back and no synchronisation but
// staged_pass's own. A FLAGGED pass decodes the frames its `before` flagged, compacted in frame order into jobs by a kernel that
// leaves their count in a device word (jobCount): one read-back per pass. A pass has one SIDE (sign, signature diff, index, the
// tails) or two (compare, diff: archives A and B, B's jobs at jobBase = the plan's slots, the same job k -> slot on both sides).
//
// Ordering conditions (all launches on the engine's stream, staged_pass returns synchronised):
//  (time) evCall_[0] .. evCall_[1] spans the call's own launches between two decodes: `after` of a pass and `before` (and the job
//      build) of the next one follow each other on the stream, the decoder's launches lie outside. The span is read behind the next
//      synchronisation of the stream: the read-back's, else staged_pass's, else finish's. begin() records the first evCall_[0], so
//      the `before` of pass 0 is inside; a second plan of the same call (the diff's tail) continues the first one's last span.
//      The synchronisation of 2b falls under this condition: it is a read-back's, as the flagged pass's of step 4, and the span it reads
//      was closed in 2a, in front of the split. The split (evCall_[2] .. [3]) and the stage kernel (evCall_[4] .. [5]) lie outside the
//      span, like the decoder's launches, and go to the view's stageMs; the stage kernel's pair is read behind the next synchronisation.
//  (error) jobs are in frame order, the same on both sides, so a side's error word is its lowest failing frame. Both sides are decoded
//      before either word is looked at; the lower frame wins, A wins a tie; the call ends with that frame's code, at the first
//      failing pass. Nothing of `after` runs for that pass. Through a handle the jobs are the missing frames, still in frame order: a
//      resident frame was decoded whole with status 0, a verified checksum and its exact size, so the lowest failing frame is a job.
//  (ping-pong) pass p reads word p & 1 of a carry or totals pair and writes word (p + 1) & 1 (FramePass::parity): launches are chained
//      by prefix counts, never by an atomic's result, and no workgroup waits for another one. Behind P passes the result is in word P & 1.
//  (d) nothing goes to the caller's host arrays before the last pass is done: a call that fails midway writes none of them.
#pragma once
#include "zra_host.h"
#include <type_traits>
#include <vector>

namespace zra_eng {

// The caller's side of a patch (ZraHipDiffArchives, ZraHipDiffSignature): the writes' three host arrays, the packed data, the four
// output words. One struct, so the two calls check, fill and refuse alike.
struct PatchOut {
  uint64_t* hOff; uint64_t* hSize; uint64_t* hDataOff; size_t writeCap;
  uint64_t* nWrites; uint8_t* dData; size_t dataCap;
  uint64_t* dataSize; uint64_t* appendOffset; uint64_t* appendSize;
  bool args_ok() const { return nWrites && dataSize && appendOffset && appendSize && !(writeCap && (!hOff || !hSize || !hDataOff)) && !(!dData && dataCap); }
  bool data_overlaps(const void* p, uint64_t n) const { return dataCap && n && (uintptr_t)dData < (uintptr_t)p + n && (uintptr_t)p < (uintptr_t)dData + dataCap; }
};

struct FramePasses {
  // bytes of the window, of the flags, dirty flags, tables and list of Engine::fp_ (0: not reserved); decode jobs and slots of a pass
  // (the decoder's job arrays; window 0, a call without a pass: not reserved either)
  // copies: the frames of a pass that may be staged from a handle's cache (0: no view, or one without slots)
  struct Scratch { size_t window, flags, dirty, tables, list, jobs, slots, copies; };
  // cv (optional, plain passes of one side): the view of the handle the call goes through; its counters say what the passes did
  struct Side { const ArchiveView* arc; uint32_t jobBase; uint8_t* window; ScanCacheView* cv = nullptr; };

  Engine& E;
  hipStream_t s;
  double* ms;                                  // the call's milliseconds: gains every span of (time)
  uint8_t* win = nullptr; uint8_t* flags = nullptr; uint8_t* dirty = nullptr; uint8_t* tables = nullptr; uint64_t* list = nullptr;
  uint64_t* frameOff = nullptr; uint64_t* outOff = nullptr; uint32_t* expect = nullptr;
  bool timed = false, stageTimed = false;
  ScanCacheView* view = nullptr;               // the running plan's Side::cv: gains the stage kernel's time in take_time

  FramePasses(Engine& e, double* callMs) : E(e), s(e.stream_), ms(callMs) {}

  // behind the argument checks of a call: the device, the decode counters
  Status start() { HIPCHK_CLR(hipSetDevice(E.device_)); E.reset_decode_stats(); return ok(); }
  // THE RULE of Engine::stage_, for the window and the tables alike: reserved once, here; the pointers hold until the call returns
  Status open(const Scratch& n) {
    if ((n.window && !E.stage_.reserve(n.window)) || (n.flags && !E.fp_.flags.reserve(n.flags)) || (n.dirty && !E.fp_.dirty.reserve(n.dirty)) ||
        (n.tables && !E.fp_.tables.reserve(n.tables)) || (n.list && !E.fp_.list.reserve(n.list)) ||
        (n.window && (!E.frameOff_.reserve((n.jobs + 1) * 16) || !E.outOff_.reserve((n.slots + 1) * 8) || !E.expect_.reserve((n.jobs + 1) * 4))) ||
        (n.window && n.copies && !E.upd_.copies.reserve((n.copies + 1) * 16)))
      return zerr(64);
    if (!E.call_events()) return zerr(1);
    win = E.stage_.as<uint8_t>(); flags = E.fp_.flags.as<uint8_t>(); dirty = E.fp_.dirty.as<uint8_t>(); tables = E.fp_.tables.as<uint8_t>();
    list = E.fp_.list.as<uint64_t>();
    frameOff = E.frameOff_.as<uint64_t>(); outOff = E.outOff_.as<uint64_t>(); expect = E.expect_.as<uint32_t>();
    return ok();
  }
  // in front of the first pass: the first hdrBytes of `hdr` (the call's header words) zeroed, the first span opened
  Status begin(void* hdr, size_t hdrBytes) {
    if (hdrBytes) HIPCHK_CLR(hipMemsetAsync(hdr, 0, hdrBytes, s));
    HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
    return ok();
  }
  // (behind a synchronisation of the stream)
  void take_time() {
    if (timed) *ms += Engine::elapsed_ms(E.evCall_[0], E.evCall_[1]);
    if (stageTimed) view->stageMs += Engine::elapsed_ms(E.evCall_[4], E.evCall_[5]);
    timed = stageTimed = false;
  }

  // The passes of plan P, as the file head has them. jobCount == nullptr: plain passes; else flagged ones, whose `before` leaves the
  // pass's job count in that device word. b: the second side, or nullptr. before(const FramePass&) -> Status, or nullptr: none;
  // after(const FramePass&, uint32_t nDec) -> Status, nDec the jobs the pass decoded (per side). *decoded (optional) gains them.
  template <class Before, class After>
  Status run(const PassPlan& P, const Side& a, const Side* b, const uint32_t* jobCount, uint64_t* decoded, Before&& before, After&& after) {
    if ((a.cv && (jobCount || b)) || (b && b->cv)) return zerr(1);            // a view serves plain passes of one side
    view = a.cv;
    const bool cached = view && view->slots;
    // (through a handle's cache) the pass's count words, then its copy entries, 4 words each
    uint32_t* const counts = cached ? E.upd_.copies.as<uint32_t>() : nullptr, * const copies = cached ? counts + 4 : nullptr;
    for (uint64_t p = 0; p < P.passes; p++) {
      const FramePass ps = frame_pass(P, p);
      if constexpr (!std::is_same_v<std::decay_t<Before>, std::nullptr_t>) STCHK(before(ps));
      if (!jobCount && !cached) search_launch_jobs(s, a.arc->table, a.arc->fs, a.arc->U, ps.first, ps.nj, frameOff, outOff, expect);
      HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
      timed = true;
      uint32_t nDec = ps.nj;
      uint64_t decBytes = 0;
      if (cached) {                                                           // 2a .. 2c
        HIPCHK_CLR(hipEventRecord(E.evCall_[2], s));
        scan_launch_split(s, view->slotOf, view->frames, a.arc->table, a.arc->fs, a.arc->U, ps.first, ps.nj, frameOff, outOff, expect, copies, counts);
        HIPCHK_CLR(hipEventRecord(E.evCall_[3], s));
        HIPCHK_CLR(hipMemcpyAsync(view->pin, counts, 16, hipMemcpyDeviceToHost, s));
        HIPCHK_CLR(hipStreamSynchronize(s));
        HIPCHK_CLR(hipGetLastError());
        take_time();
        view->stageMs += Engine::elapsed_ms(E.evCall_[2], E.evCall_[3]);
        nDec = view->pin[0];
        const uint32_t nCopy = view->pin[1];
        decBytes = (uint64_t)view->pin[2] | (uint64_t)view->pin[3] << 32;
        if (nDec > ps.nj || nCopy != ps.nj - nDec) return zerr(1);             // (cannot happen)
        if (nCopy) {
          HIPCHK_CLR(hipEventRecord(E.evCall_[4], s));
          upd_launch_stage_cached(s, copies, nCopy, 0, a.arc->fs, view->arena, a.window);
          HIPCHK_CLR(hipEventRecord(E.evCall_[5], s));
          stageTimed = true;
          view->staged += nCopy;
        }
      }
      if (jobCount) {
        HIPCHK_CLR(hipMemcpyAsync(&nDec, jobCount, 4, hipMemcpyDeviceToHost, s));
        HIPCHK_CLR(hipStreamSynchronize(s));
        HIPCHK_CLR(hipGetLastError());
        take_time();
        if (nDec > ps.nj) return zerr(1);                                     // (cannot happen)
      }
      if (nDec) {
        unsigned long long first = ~0ull;                                     // (error)
        for (const Side* sd : {&a, b}) {
          if (!sd) continue;
          unsigned long long err;
          STCHK(E.staged_pass(*sd->arc, sd->jobBase, nDec, sd->window, &err));
          if ((err >> 8) < (first >> 8)) first = err;
        }
        take_time();
        if (first != ~0ull) return zerr(reported_code(first));
        if (decoded) *decoded += nDec;
      }
      if (view) { view->decoded += nDec; view->decodedBytes += cached ? decBytes : content_bytes(a.arc->U, a.arc->fs, ps.first, ps.nj); view->passes++; }
      HIPCHK_CLR(hipEventRecord(E.evCall_[0], s));
      STCHK(after(ps, nDec));
    }
    return ok();
  }

  // behind the last pass: the call's header words, `bytes` at dev, come to `host`; the last span is taken. Returns synchronised
  Status finish(void* host, const void* dev, size_t bytes) {
    HIPCHK_CLR(hipEventRecord(E.evCall_[1], s));
    timed = true;
    HIPCHK_CLR(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    HIPCHK_CLR(hipGetLastError());
    take_time();
    return ok();
  }

  // The epilogue of a patch, behind finish: `total` writes with dirtyBytes bytes, then tailBytes of B's content behind C. The four
  // words are set; a patch that does not fit is refused (OutputTooSmall, the words say what is needed); else the starts and the nEnds
  // listed ends come to the host, once, and become {offset, size, dataOffset} triples. nEnds == total - 1: the last run is open and
  // ends at C (the signature diff's carry behind its last pass).
  Status patch(const PatchOut& o, const uint64_t* starts, const uint64_t* ends, uint64_t total, uint64_t nEnds, uint64_t C, uint64_t dirtyBytes, uint64_t tailBytes) {
    *o.nWrites = total; *o.dataSize = dirtyBytes + tailBytes; *o.appendOffset = dirtyBytes; *o.appendSize = tailBytes;
    if (total > o.writeCap || dirtyBytes + tailBytes > o.dataCap) return {kOutputTooSmall, 0};
    if (!total) return ok();
    std::vector<uint64_t> se(2 * (size_t)total);
    HIPCHK_CLR(hipMemcpyAsync(se.data(), starts, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    if (nEnds) HIPCHK_CLR(hipMemcpyAsync(se.data() + total, ends, (size_t)nEnds * 8, hipMemcpyDeviceToHost, s));
    HIPCHK_CLR(hipStreamSynchronize(s));
    if (nEnds < total) se[2 * (size_t)total - 1] = C;
    uint64_t at = 0;
    for (size_t i = 0; i < total; i++) { o.hOff[i] = se[i]; o.hSize[i] = se[total + i] - se[i]; o.hDataOff[i] = at; at += o.hSize[i]; }
    return ok();
  }
};

}  // namespace zra_eng
