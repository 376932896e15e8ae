// cfroute.h - routes along a cost field (include/trafficsim_cfroute.h): the kernel that turns the settled labels of a compute
// into the hop plane, and the walks over that plane - count, write, load - with the small kernels around them.  Part of the
// single translation unit engine.hip (included from there, behind costfield.h whose labels and cell words it reads).
//
// The hop plane holds decisions only.  What a walk needs besides it stays from the compute as well: the cell words of
// k_cf_cells (a TO walk adds up its steps, because the cost of a state with a heading is in no plane) and the seeds by cell
// (the seed a TO route ends at is the smallest label on its last cell, which need not be that cell's owner).
#pragma once
#include "../../include/trafficsim_cfroute.h"

namespace {

constexpr uint32_t CFR_ALL = 1u | (1u << 3) | (1u << 6) | (1u << 9) | (1u << 12);   // one value in all five fields

// the step u -> v in direction d under the query's modes: does it exist, and what it costs in half units before the turn
__device__ __forceinline__ bool cfr_edge(const CostFieldArgs& a, uint32_t cw_u, uint32_t cw_v, int d, uint32_t& base2) {
  const bool flow = ((cw_u >> d) & 1u) != 0u;
  base2 = (cw_v >> CW_COST) + (flow ? 0u : (uint32_t)a.contra2);
  return ((cw_v >> CW_ENTER) & 1u) && (flow || (a.ignore_flow && ((cw_v >> CW_ROAD) & 1u)));
}
// label l is the label of a seed on (x, y): its low half names the seed, which lies there and costs what l says
__device__ __forceinline__ bool cfr_seed_here(u64 l, int x, int y, const int32_t* sxy, const int32_t* scost) {
  const uint32_t i = (uint32_t)l;
  return sxy[2 * i] == x && sxy[2 * i + 1] == y && (scost ? (uint32_t)scost[i] : 0u) == (uint32_t)(l >> 32);
}

// ---- the hop plane -----------------------------------------------------------------------------------------------------
// One thread per cell, over the labels as the relaxation left them (the rule is in the header, word for word).
template <int NH, bool TO>
__global__ void k_cfr_hops(CostFieldArgs a, const int32_t* sxy, const int32_t* scost, uint16_t* hops) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.N) return;
  const int y = c / a.W, x = c - y * a.W;
  const uint32_t cwc = a.cw[c];
  // the four edges of the cell: TO c -> v = c + off[d], FROM u = c - off[d] -> c
  bool ok[4]; uint32_t b2[4]; size_t nb[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int s = TO ? 1 : -1;
    const int nx = x + s * ((d == 1) - (d == 3)), ny = y + s * ((d == 0) - (d == 2));
    ok[d] = false; b2[d] = 0u; nb[d] = 0;
    if ((unsigned)nx >= (unsigned)a.W || (unsigned)ny >= (unsigned)a.H) continue;
    nb[d] = (size_t)ny * a.W + nx;
    const uint32_t cwn = a.cw[nb[d]];
    ok[d] = TO ? cfr_edge(a, cwc, cwn, d, b2[d]) : cfr_edge(a, cwn, cwc, d, b2[d]);
  }
  uint32_t f[5];
  if (NH == 1) {
    const u64 l = a.lab[c];
    uint32_t v = TS_CFR_NONE;
    if (l != CF_NONE) {
      if (cfr_seed_here(l, x, y, sxy, scost)) v = TS_CFR_STOP;
      else
        for (int d = 3; d >= 0; d--)
          if (ok[d] && cf_add(a.lab[nb[d]], b2[d] >> 1, a.limit) == l) v = (uint32_t)d;
    }
    hops[c] = (uint16_t)(v * CFR_ALL);
    return;
  }
  if (TO) {
    u64 lv[4];   // L(v, d): the neighbour in direction d, held with the heading it was entered with
#pragma unroll
    for (int d = 0; d < 4; d++) lv[d] = ok[d] ? a.lab[(size_t)d * a.N + nb[d]] : CF_NONE;
#pragma unroll
    for (int k = 0; k < 5; k++) {
      u64 l;
      if (k == 0) {   // "no heading": the turn-free relaxation, as k_cf_finish forms it
        l = a.seed[c];
#pragma unroll
        for (int d = 0; d < 4; d++) l = min(l, cf_add(lv[d], b2[d] >> 1, a.limit));
      } else l = a.lab[(size_t)(k - 1) * a.N + c];
      uint32_t v = TS_CFR_NONE;
      if (l != CF_NONE) {
        if (cfr_seed_here(l, x, y, sxy, scost)) v = TS_CFR_STOP;
        else
          for (int d = 3; d >= 0; d--)
            if (ok[d] && cf_add(lv[d], (b2[d] + ((k > 0 && k - 1 != d) ? (uint32_t)a.turn2 : 0u)) >> 1, a.limit) == l) v = (uint32_t)d;
      }
      f[k] = v;
    }
  } else {
    const u64 ls = a.seed[c];
    u64 ld[4], l = ls;
#pragma unroll
    for (int d = 0; d < 4; d++) { ld[d] = a.lab[(size_t)d * a.N + c]; l = min(l, ld[d]); }
    f[0] = TS_CFR_NONE;
    if (l != CF_NONE) {
      if (ls == l) f[0] = TS_CFR_STOP;
      else
        for (int d = 3; d >= 0; d--)
          if (ld[d] == l) f[0] = (uint32_t)d;
    }
#pragma unroll
    for (int d = 0; d < 4; d++) {
      uint32_t v = TS_CFR_NONE;
      if (ld[d] != CF_NONE && ok[d]) {
        if (cf_add(a.seed[nb[d]], b2[d] >> 1, a.limit) == ld[d]) v = TS_CFR_STOP;
        else
          for (int h = 3; h >= 0; h--)
            if (cf_add(a.lab[(size_t)h * a.N + nb[d]], (b2[d] + (h != d ? (uint32_t)a.turn2 : 0u)) >> 1, a.limit) == ld[d]) v = (uint32_t)h;
      }
      f[1 + d] = v;
    }
  }
  hops[c] = (uint16_t)(f[0] | (f[1] << 3) | (f[2] << 6) | (f[3] << 9) | (f[4] << 12));
}

// ---- walking the plane ---------------------------------------------------------------------------------------------------
// what a walk reads: the planes the compute left and the scalars of its query
struct CfrPlane {
  int W, H, N, to, nh, turn2, contra2, n_seed_cells;
  long long cap;              // steps a walk may take: the number of states
  const uint16_t* hops;       // [N]
  const uint32_t* cw;         // [N] the cell words of the compute
  const uint32_t* val;        // [N] the cost field's planes
  const int32_t* own;
  const int32_t* seed_cell;   // [n_seed_cells] the cells that hold seeds, ascending
  const u64* seed_lab;        // ... and the smallest seed label on each
};
enum { CFR_ENDED = 0, CFR_NO_ROUTE = 1, CFR_FAULT = 2 };
// ctl words of the walking kernels
enum { CFR_C_FAULT = 0, CFR_C_UNREACHED, CFR_C_LONGEST, CFR_C_STEPS, CFR_C_N };

struct CfrWalk {
  long long steps;   // taken
  int status;        // CFR_ENDED: on a seed; CFR_NO_ROUTE: the start has none; CFR_FAULT: the plane led off the map or in circles
  int end;           // the cell of that seed
  u64 cost;          // TO: the steps' costs added up
};

// Follow the plane from (x, y), held with heading p (TO), to the seed; emit(d, cell) for every step, as "cell was entered in
// direction d" - a TO walk emits its route first step first, a FROM walk last step first.  Every iteration checks the step
// cap and the map's edge, so no plane, whatever it holds, keeps a thread for more than cap steps or sends it outside.
template <typename F>
__device__ __forceinline__ CfrWalk cfr_walk(const CfrPlane& P, int x, int y, int p, F emit) {
  CfrWalk w{0, CFR_ENDED, y * P.W + x, 0};
  int c = w.end;
  if (P.to) {
    for (;;) {
      const int d = (P.hops[c] >> (3 * (p + 1))) & 7;
      if (d == TS_CFR_STOP) { w.end = c; return w; }
      if (d > 3) { w.status = (d == TS_CFR_NONE && w.steps == 0) ? CFR_NO_ROUTE : CFR_FAULT; return w; }
      const int nx = x + (d == 1) - (d == 3), ny = y + (d == 0) - (d == 2);
      if ((unsigned)nx >= (unsigned)P.W || (unsigned)ny >= (unsigned)P.H || w.steps >= P.cap) { w.status = CFR_FAULT; return w; }
      const int v = ny * P.W + nx;
      const uint32_t cw_u = P.cw[c], cw_v = P.cw[v];
      const uint32_t base2 = (cw_v >> CW_COST) + (((cw_u >> d) & 1u) ? 0u : (uint32_t)P.contra2);
      w.cost += (base2 + ((p >= 0 && p != d) ? (uint32_t)P.turn2 : 0u)) >> 1;
      x = nx; y = ny; c = v; p = d; w.steps++;
      emit(d, c);
    }
  }
  int d = P.hops[c] & 7;
  for (;;) {
    if (d == TS_CFR_STOP) { w.end = c; return w; }
    if (d > 3) { w.status = (d == TS_CFR_NONE && w.steps == 0) ? CFR_NO_ROUTE : CFR_FAULT; return w; }
    const int ux = x - ((d == 1) - (d == 3)), uy = y - ((d == 0) - (d == 2));
    if ((unsigned)ux >= (unsigned)P.W || (unsigned)uy >= (unsigned)P.H || w.steps >= P.cap) { w.status = CFR_FAULT; return w; }
    emit(d, c);
    const int u = uy * P.W + ux;
    d = P.nh == 4 ? (P.hops[c] >> (3 * (d + 1))) & 7 : P.hops[u] & 7;
    x = ux; y = uy; c = u; w.steps++;
  }
}

// the smallest seed label on `cell`, CF_NONE when it holds no seed
__device__ __forceinline__ u64 cfr_seed_on(const CfrPlane& P, int cell) {
  int lo = 0, hi = P.n_seed_cells;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P.seed_cell[mid] < cell) lo = mid + 1; else hi = mid;
  }
  return (lo < P.n_seed_cells && P.seed_cell[lo] == cell) ? P.seed_lab[lo] : CF_NONE;
}

__device__ __forceinline__ unsigned long long cfr_wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long cfr_wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, o));
  return v;
}

// count pass: one thread per start (the host has checked cells and headings); len[n] = 0 closes the scan's input
__global__ void k_cfr_count(CfrPlane P, int n, const int32_t* xy, const int8_t* head, long long* len, uint32_t* cost, int32_t* owner,
                            unsigned long long* ctl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long steps = 0, unreached = 0, fault = 0;
  if (i == n) len[n] = 0;
  if (i < n) {
    const int x = xy[2 * i], y = xy[2 * i + 1];
    const CfrWalk w = cfr_walk(P, x, y, head ? (int)head[i] : -1, [](int, int) {});
    uint32_t v = TS_CF_UNREACHABLE; int32_t o = -1;
    if (w.status == CFR_ENDED) {
      steps = (unsigned long long)w.steps;
      if (!P.to) { v = P.val[y * P.W + x]; o = P.own[y * P.W + x]; }
      else {
        const u64 l = cfr_seed_on(P, w.end);
        if (l == CF_NONE) fault = 1;
        else { v = (uint32_t)(w.cost + (l >> 32)); o = (int32_t)(uint32_t)l; }
      }
    } else if (w.status == CFR_NO_ROUTE) unreached = 1;
    else fault = 1;
    if (fault) { steps = 0; v = TS_CF_UNREACHABLE; o = -1; }
    len[i] = (long long)steps; cost[i] = v; owner[i] = o;
  }
  const unsigned long long nf = cfr_wave_sum(fault), nu = cfr_wave_sum(unreached), mx = cfr_wave_max(steps);
  if ((threadIdx.x & 63) == 0) {
    if (nf) atomicAdd(&ctl[CFR_C_FAULT], nf);
    if (nu) atomicAdd(&ctl[CFR_C_UNREACHED], nu);
    if (mx) atomicMax(&ctl[CFR_C_LONGEST], mx);
  }
}

// write pass: the same walks, their directions into the CSR slots the scan gave them (a FROM walk from the slot's end)
__global__ void k_cfr_write(CfrPlane P, int n, const int32_t* xy, const int8_t* head, const long long* off, uint8_t* dirs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long lo = off[i], hi = off[i + 1];
  if (hi == lo) return;
  long long k = P.to ? lo : hi - 1;
  const long long s = P.to ? 1 : -1;
  // (the count pass took the same walk: k stays inside [lo, hi); the check keeps a plane that changed in between harmless)
  cfr_walk(P, xy[2 * i], xy[2 * i + 1], head ? (int)head[i] : -1, [&](int d, int) {
    if (k >= lo && k < hi) dirs[k] = (uint8_t)d;
    k += s;
  });
}

// load: one walk per start, its weight added to plane d of every cell it enters in direction d; nothing is returned to the
// thread, so the adds are fire-and-forget.  ctl: faults, starts without a route, the weighted steps.
__global__ void k_cfr_load(CfrPlane P, int n, const int32_t* xy, const int8_t* head, const uint32_t* weight, uint32_t* planes,
                           unsigned long long* ctl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long steps = 0, unreached = 0, fault = 0;
  if (i < n) {
    const uint32_t wgt = weight ? weight[i] : 1u;
    const size_t N = (size_t)P.N;
    const CfrWalk w = cfr_walk(P, xy[2 * i], xy[2 * i + 1], head ? (int)head[i] : -1, [&](int d, int c) {
      if (wgt) (void)__hip_atomic_fetch_add(&planes[(size_t)d * N + c], wgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    if (w.status == CFR_ENDED) steps = (unsigned long long)w.steps * wgt;
    else if (w.status == CFR_NO_ROUTE) unreached = 1;
    else fault = 1;
  }
  const unsigned long long nf = cfr_wave_sum(fault), nu = cfr_wave_sum(unreached), ns = cfr_wave_sum(steps);
  if ((threadIdx.x & 63) == 0) {
    if (nf) atomicAdd(&ctl[CFR_C_FAULT], nf);
    if (nu) atomicAdd(&ctl[CFR_C_UNREACHED], nu);
    if (ns) atomicAdd(&ctl[CFR_C_STEPS], ns);
  }
}

// routes first .. first + count - 1 as cells, one thread per route: the route's first cell is the start (TO) or the start
// moved back over all of its steps (FROM); every step's cell goes to xy at the route's offset from the first route's
__global__ void k_cfr_cells(int W, int to, int first, int count, const int32_t* starts, const long long* off, const uint8_t* dirs,
                            int32_t* xy) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= count) return;
  const long long lo = off[first + r], hi = off[first + r + 1], base = off[first];
  int x = starts[2 * (first + r)], y = starts[2 * (first + r) + 1];
  if (!to)
    for (long long k = lo; k < hi; k++) { const int d = dirs[k]; x -= (d == 1) - (d == 3); y -= (d == 0) - (d == 2); }
  for (long long k = lo; k < hi; k++) {
    const int d = dirs[k];
    x += (d == 1) - (d == 3); y += (d == 0) - (d == 2);
    xy[2 * (k - base)] = x; xy[2 * (k - base) + 1] = y;
  }
}

}  // namespace
