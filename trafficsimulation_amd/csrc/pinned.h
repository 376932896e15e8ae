// pinned.h - regrow_pinned: growth of a pinned host buffer (hipHostMalloc) that survives a refused allocation.  Allocate, then
// free the old buffer, then assign: on refusal *p is untouched and still live, so a group of buffers that share one capacity
// stays usable at that capacity, and is freed exactly once, when any of them cannot grow.  Contents are not kept.
// Names hipError_t, hipSuccess, hipHostMalloc and hipHostFree and includes nothing of HIP: the translation unit brings the
// runtime (engine.hip) or stand-ins for these four (tests/native/pinned_check.cpp) first.
#pragma once
#include <cstddef>

template <typename T>
hipError_t regrow_pinned(T** p, size_t n) {
  void* q = nullptr;
  const hipError_t r = hipHostMalloc(&q, n * sizeof(T));
  if (r != hipSuccess) return r;
  if (*p) (void)hipHostFree(*p);
  *p = (T*)q;
  return hipSuccess;
}
