// scratch.h - Scratch: the device buffers one call needs and nothing keeps (temporaries, as opposed to what the engine owns
// through dalloc / dfree and its allocs list, host_state.h).  Every buffer handed out is freed when the scope ends, whichever
// way it ends.  The rule the callers rely on: hipFree waits for outstanding device work, so a scope may be left by an early
// return while kernels and copies that use the buffers are still queued.
// Names hipError_t, hipSuccess, hipErrorOutOfMemory, hipMalloc and hipFree and includes nothing of HIP: the translation unit
// brings the runtime (engine.hip) or stand-ins for these five (tests/native/scratch_check.cpp) first.
#pragma once
#include <cstddef>

struct Scratch {
  static constexpr int CAP = 12;   // buffers per scope (the most a call takes today: eight, ts_costfield_compute)
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { for (int k = 0; k < n; k++) (void)hipFree(p[k]); }
  // *out <- max(count, 1) elements of T; on failure (the device's, or a scope that is full) *out is null
  template <typename T>
  hipError_t get(T** out, size_t count) {
    *out = nullptr;
    if (n == CAP) return hipErrorOutOfMemory;
    void* q = nullptr;
    const hipError_t r = hipMalloc(&q, (count ? count : 1) * sizeof(T));
    if (r != hipSuccess) return r;
    p[n++] = q;
    *out = (T*)q;
    return hipSuccess;
  }

 private:
  void* p[CAP] = {};
  int n = 0;
};
