// zra_amd — host-side helpers shared by the engine's translation units (not part of the interface in zra_engine.h).
#pragma once
#include <chrono>
#include <cstdio>
#include <initializer_list>
#include "zra_engine.h"
#include "zra_env.h"

// a failed HIP call ends the enclosing function with zstd's generic error; the second form also clears the runtime's last error
#define HIPCHK(x) do { if ((x) != hipSuccess) return zerr(1); } while (0)
#define HIPCHK_CLR(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return zerr(1); } } while (0)
// a call that failed ends the enclosing function with its status
#define STCHK(x) do { const Status st_ = (x); if (st_.zra) return st_; } while (0)

namespace zra_eng {

// What a device-archive call leaves behind, decided here for all of them (zra_hip.h documents it per call). stats / ms: the call's row
// of Engine::callStats_ / callMs_ (ms nullptr: the call has none); words: its output words, n at p (p may be nullptr). Counters,
// milliseconds and words are zero before `run`. On any failure the counters and the milliseconds are zero again, and so are the words,
// unless tooSmallKeeps and the status is OutputTooSmall: then the words say what the call needs. A success keeps what `run` wrote, an
// early return with only `frames` set included.
struct OutWords { uint64_t* p; size_t n; };
template <class Run>
Status entry_call(uint64_t (&stats)[8], double* ms, std::initializer_list<OutWords> words, bool tooSmallKeeps, Run&& run) {
  auto clear = [&](bool alsoWords) {
    for (auto& v : stats) v = 0;
    if (ms) *ms = 0;
    if (alsoWords) for (const OutWords& w : words) for (size_t i = 0; w.p && i < w.n; i++) w.p[i] = 0;
  };
  clear(true);
  const Status st = run();
  if (st.zra) clear(!(tooSmallKeeps && st.zra == kOutputTooSmall));
  return st;
}

// diagnostics: ZRA_RA_TRACE prints the host microseconds between the marks of a random-access call
struct RaTrace {
  const char* prefix; int width;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void mark(const char* what) {
    static const bool on = zra_env::env_set("ZRA_RA_TRACE");
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "%s %-*s %7.1f us\n", prefix, width, what, std::chrono::duration<double, std::micro>(t - last).count());
    last = t;
  }
};

}  // namespace zra_eng
