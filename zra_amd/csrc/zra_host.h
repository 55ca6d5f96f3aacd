// zra_amd — host-side helpers shared by the engine's translation units (not part of the interface in zra_engine.h).
#pragma once
#include <chrono>
#include <cstdio>
#include "zra_engine.h"
#include "zra_env.h"

// a failed HIP call ends the enclosing function with zstd's generic error; the second form also clears the runtime's last error
#define HIPCHK(x) do { if ((x) != hipSuccess) return zerr(1); } while (0)
#define HIPCHK_CLR(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return zerr(1); } } while (0)

namespace zra_eng {

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
