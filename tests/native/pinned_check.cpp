// pinned_check.cpp - csrc/pinned.h (growth of pinned host buffers that survives a refused allocation) on the CPU: the four HIP
// names the header uses are stand-ins on malloc / free that keep a list of what is live, and whose hipHostMalloc refuses the
// call it is told to.  A group of three buffers that share one capacity is grown as ensure_vehicle_capacity grows hF, hR and
// hrank.  Built with -fsanitize=address,undefined by tests/test_host_pinned.py, so a touch of a freed buffer, a double free
// or a leak ends the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static int g_calls = 0, g_refuse = 0;   // hipHostMalloc calls so far, the call to refuse (0: none)
static struct { void* p; size_t bytes; } g_live[16];
static int g_nlive = 0;
static hipError_t hipHostMalloc(void** p, size_t bytes) {
  if (++g_calls == g_refuse || g_nlive == 16) return hipErrorOutOfMemory;
  *p = malloc(bytes);   // (exactly as many bytes as asked for: the sanitizer sees every byte beyond them)
  if (!*p) return hipErrorOutOfMemory;
  g_live[g_nlive].p = *p; g_live[g_nlive++].bytes = bytes;
  return hipSuccess;
}
static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d (refuse = %d): %s\n", __LINE__, g_refuse, #cond); g_bad++; } } while (0)
static hipError_t hipHostFree(void* p) {
  int k = 0;
  while (k < g_nlive && g_live[k].p != p) k++;
  CHECK(k < g_nlive);   // (freed twice, or never handed out)
  if (k < g_nlive) g_live[k] = g_live[--g_nlive];
  free(p);
  return hipSuccess;
}
// bytes of the live buffer that starts at p (0: p is not one)
static size_t live_bytes(const void* p) {
  for (int k = 0; k < g_nlive; k++) if (g_live[k].p == p) return g_live[k].bytes;
  return 0;
}

#include "../../trafficsimulation_amd/csrc/pinned.h"

// three buffers of `cap` elements each; the capacity is raised only after every one of them has grown
struct Group { uint8_t *f = nullptr, *r = nullptr; uint32_t* rank = nullptr; int cap = 0; };
static hipError_t grow(Group& g, int nc) {
  hipError_t e;
  if ((e = regrow_pinned(&g.f, (size_t)nc)) != hipSuccess) return e;
  if ((e = regrow_pinned(&g.r, (size_t)nc)) != hipSuccess) return e;
  if ((e = regrow_pinned(&g.rank, (size_t)nc)) != hipSuccess) return e;
  g.cap = nc;
  return hipSuccess;
}
// every buffer of the group is live and holds at least g.cap elements: each of them is written and read
static void usable(Group& g) {
  CHECK(live_bytes(g.f) >= (size_t)g.cap && live_bytes(g.r) >= (size_t)g.cap && live_bytes(g.rank) >= (size_t)g.cap * 4);
  for (int k = 0; k < g.cap; k++) { g.f[k] = (uint8_t)k; g.r[k] = (uint8_t)(k + 1); g.rank[k] = (uint32_t)k * 3u; }
  for (int k = 0; k < g.cap; k++) CHECK(g.f[k] == (uint8_t)k && g.r[k] == (uint8_t)(k + 1) && g.rank[k] == (uint32_t)k * 3u);
}

// a group of 1024 grows to 3072 while allocation number `refuse` of that growth is refused (0: none), then to 7168
static void run(int refuse) {
  Group g;
  g_calls = 0; g_refuse = 0;
  CHECK(grow(g, 1024) == hipSuccess && g.cap == 1024 && g_nlive == 3);
  usable(g);
  g_calls = 0; g_refuse = refuse;
  const hipError_t e = grow(g, 3072);
  CHECK(g_calls == (refuse ? refuse : 3));
  if (refuse) CHECK(e != hipSuccess && g.cap == 1024);   // (some buffers may be larger already: the capacity is the old one)
  else CHECK(e == hipSuccess && g.cap == 3072);
  CHECK(g_nlive == 3);
  usable(g);
  g_calls = 0; g_refuse = 0;
  CHECK(grow(g, 7168) == hipSuccess && g.cap == 7168 && g_nlive == 3);
  usable(g);
  // ts_destroy: each pointer freed once
  (void)hipHostFree(g.f); (void)hipHostFree(g.r); (void)hipHostFree(g.rank);
  CHECK(g_nlive == 0);
}

int main() {
  for (int refuse = 0; refuse <= 3; refuse++) run(refuse);
  if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
  printf("ok pinned\n");
  return 0;
}
