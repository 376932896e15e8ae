// scratch_check.cpp - csrc/scratch.h (the scoped type for a call's temporary device buffers) on the CPU: the five HIP names
// the header uses are stand-ins on malloc / free that count, and whose hipMalloc refuses the call it is told to.  Built with
// -fsanitize=address,undefined by tests/test_host_scratch.py, so a write past a buffer, a double free or a leak ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static int g_calls = 0, g_refuse = 0, g_live = 0;   // hipMalloc calls so far, the call to refuse (0: none), buffers not freed yet
static hipError_t hipMalloc(void** p, size_t bytes) {
  if (++g_calls == g_refuse) return hipErrorOutOfMemory;
  *p = malloc(bytes);   // (exactly as many bytes as asked for: the sanitizer sees every byte beyond them)
  if (!*p) return hipErrorOutOfMemory;
  g_live++;
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  if (p) { free(p); g_live--; }
  return hipSuccess;
}

#include "../../trafficsimulation_amd/csrc/scratch.h"

static_assert(!std::is_copy_constructible<Scratch>::value && !std::is_copy_assignable<Scratch>::value, "Scratch must not be copyable");

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d (refuse = %d): %s\n", __LINE__, g_refuse, #cond); g_bad++; } } while (0)

// eight buffers of 0, 1, ..., 7 doubles; hipMalloc refuses call number `refuse` (0: none)
static void eight(int refuse) {
  g_calls = 0; g_refuse = refuse;
  {
    Scratch s;
    double* p[8];
    for (int i = 0; i < 8; i++) {
      p[i] = (double*)&p;   // (anything but null: a refused get has to clear it)
      const hipError_t r = s.get(&p[i], (size_t)i);
      if (i + 1 == refuse) { CHECK(r != hipSuccess); CHECK(p[i] == nullptr); continue; }
      CHECK(r == hipSuccess); CHECK(p[i] != nullptr);
      if (!p[i]) continue;
      for (int k = 0; k < (i ? i : 1); k++) p[i][k] = 100.0 * i + k;   // (a request for no element still has one)
    }
    // what was handed out before and after the refusal is still there and still holds what was written
    for (int i = 0; i < 8; i++)
      for (int k = 0; p[i] && k < (i ? i : 1); k++) { CHECK(p[i][k] == 100.0 * i + k); p[i][k] = -1.0; }
    CHECK(g_calls == 8);
    CHECK(g_live == (refuse ? 7 : 8));
  }
  CHECK(g_live == 0);
}

// one buffer more than a scope has room for: refused without a call to hipMalloc, the others untouched
static void one_too_many() {
  g_calls = 0; g_refuse = 0;
  {
    Scratch s;
    unsigned char* p[Scratch::CAP + 1];
    for (int i = 0; i < Scratch::CAP; i++) {
      CHECK(s.get(&p[i], 3) == hipSuccess && p[i]);
      if (p[i]) memset(p[i], i, 3);
    }
    p[Scratch::CAP] = (unsigned char*)&p;
    CHECK(s.get(&p[Scratch::CAP], 3) != hipSuccess);
    CHECK(p[Scratch::CAP] == nullptr);
    CHECK(g_calls == Scratch::CAP && g_live == Scratch::CAP);
    for (int i = 0; i < Scratch::CAP; i++) CHECK(p[i] && p[i][0] == i && p[i][2] == i);
  }
  CHECK(g_live == 0);
}

int main() {
  for (int refuse = 0; refuse <= 8; refuse++) eight(refuse);
  one_too_many();
  {   // sizes follow the element type
    g_calls = 0; g_refuse = 0;
    Scratch s;
    unsigned long long* q = nullptr;
    CHECK(s.get(&q, 5) == hipSuccess && q);
    if (q) q[4] = ~0ull;
  }
  CHECK(g_live == 0);
  if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
  printf("ok scratch\n");
  return 0;
}
