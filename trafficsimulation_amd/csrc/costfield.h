// costfield.h - cost fields (include/trafficsim_costfield.h): the pre-pass that turns the maps into one word per cell, the
// tile kernel that relaxes the labels of a T x T tile in LDS until nothing in it changes, and the small kernels around them
// (seeds, the final planes, gather, bands).  Part of the single translation unit engine.hip (included from there, behind
// astar.h whose cost helpers it uses).
//
// A label is (value << 32) | seed index, so that an aligned 64-bit minimum is the lexicographic minimum the owner rule asks
// for; 2^64 - 1 is "not reached".  There is one label per (cell, heading) when a turn costs something (NH = 4), one per cell
// otherwise (NH = 1):
//   FROM  label (v, d) = the cheapest way to arrive at v moving in direction d.  A seed has no heading, so with NH = 4 the
//         seeds lie in a plane of their own (never relaxed) and every step out of one is free of the turn penalty.
//   TO    label (v, p) = the cheapest way from v to a seed for a vehicle that arrived at v with heading p: the same
//         relaxation over reversed edges.  A seed's four labels start at its cost; the value of a cell is the label "no
//         heading", formed by k_cf_finish from its neighbours' labels.
// Labels only ever decrease, and every relaxation is a minimum over what a neighbour holds: the fixpoint is the same in
// whatever order tiles run and whatever (older) value of a neighbouring tile's border a tile happens to read.
#pragma once
#include "../../include/trafficsim_costfield.h"

namespace {

constexpr uint32_t CF_INF = 0x3F3F3F3Fu;      // the reference's INF: a value of this much or more does not exist
constexpr u64 CF_NONE = ~0ull;
// the word of a cell (k_cf_cells): bits 0-3 allowed_dirs, 4 is_road, 5 "can be entered", 8-31 what entering it costs in half
// units before turn and contraflow (2 + vehicle + stop + road type: each below 2^21, astar_half_units)
constexpr int CW_ROAD = 4, CW_ENTER = 5, CW_COST = 8;

struct CostFieldArgs {
  int W, H, N, T, tiles_x, tiles_y;
  int ignore_flow, turn2, contra2;
  uint32_t limit;            // a value of `limit` or more is not stored (INF, or max_cost + 1)
  const uint32_t* cw;        // [N]
  u64* lab;                  // [NH][N]
  u64* seed;                 // [N], NH == 4 only
  const int32_t* list_cur;   // the tiles of this round
  int32_t* list_next;        // ... of the next one, appended to at n_next by whoever raises a tile's flag_next from 0
  uint32_t *n_next, *flag_cur, *flag_next;
};

__device__ __forceinline__ u64 cf_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cf_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// label + cost, CF_NONE when the label is none or the sum reaches the limit (value < 2^30, cost < 2^24: no wrap)
__device__ __forceinline__ u64 cf_add(u64 l, uint32_t cost, uint32_t limit) {
  const uint32_t v = (uint32_t)(l >> 32);
  const uint32_t s = v + cost;
  return (v < limit && s < limit) ? (((u64)s << 32) | (uint32_t)l) : CF_NONE;
}
__device__ __forceinline__ void cf_activate(uint32_t* flag, int32_t* list, uint32_t* n, int t) {
  if (atomicExch(&flag[t], 1u) == 0u) list[atomicAdd(n, 1u)] = t;
}

// ---- pre-pass: the maps as one word per cell --------------------------------------------------------------------------
// soft / free_flow are the query's; dens_on = soft && dynamic_penalties_enabled (astar_wave's C.dens_on)
__global__ void k_cf_cells(Dev d, int soft, int free_flow, int dens_on, int rt_on, double veh_pen, double dyn_scale, HalfCosts hc,
                           uint32_t* cw) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.N) return;
  const Cell& x = d.cell[c];
  const uint32_t stat = x.stat;
  const bool occ = !free_flow && x.occ == 1, stop = !free_flow && x.stop == 1;
  int cost2 = 2;
  if (occ) cost2 += dens_on ? 2 * (int)occ_penalty_dyn(veh_pen, dyn_scale, d.density[c]) : hc.veh2;
  if (stop) cost2 += hc.stop2;
  if (rt_on && st_is_road((uint8_t)stat)) cost2 += rt2_of(hc, (uint32_t)st_road_type((uint8_t)stat));
  const bool enter = soft || !(occ || stop);
  cw[c] = (stat & 15u) | ((uint32_t)st_is_road((uint8_t)stat) << CW_ROAD) | ((enter ? 1u : 0u) << CW_ENTER) | ((uint32_t)cost2 << CW_COST);
}

// ---- seeds ---------------------------------------------------------------------------------------------------------------
// Seed i's label goes to its cell by a 64-bit minimum (several seeds may share a cell).  Its tile is put on the first
// round's list, and so are the tiles of its four neighbours: a tile only re-activates a neighbour over a border label it
// changed itself, and a seed's label is nobody's change.
template <int NH, bool TO>
__global__ void k_cf_seed(CostFieldArgs a, int n, const int32_t* xy, const int32_t* cost) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = xy[2 * i], y = xy[2 * i + 1];
  const uint32_t v = cost ? (uint32_t)cost[i] : 0u;
  if ((unsigned)x >= (unsigned)a.W || (unsigned)y >= (unsigned)a.H || v >= a.limit) return;   // (the host has refused the former)
  const u64 l = ((u64)v << 32) | (uint32_t)i;
  const size_t c = (size_t)y * a.W + x;
  if (NH == 1) atomicMin(&a.lab[c], l);
  else {
    atomicMin(&a.seed[c], l);
    if (TO)
      for (int h = 0; h < 4; h++) atomicMin(&a.lab[(size_t)h * a.N + c], l);
  }
  for (int k = 0; k < 5; k++) {
    const int nx = x + (k == 1) - (k == 3), ny = y + (k == 0) - (k == 2);   // (k = 4: the cell itself)
    if ((unsigned)nx < (unsigned)a.W && (unsigned)ny < (unsigned)a.H)
      cf_activate(a.flag_next, a.list_next, a.n_next, (ny / a.T) * a.tiles_x + nx / a.T);
  }
}

__device__ __forceinline__ u64 cf_lds_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void cf_lds_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- the labels one relaxation gives cell `me` of an (S x S) array of cell words and labels -------------------------------
// cwp / lab / seed: LDS arrays with a one-cell halo (lab: NH planes of SS); me: the cell's index in them
template <int NH, bool TO>
__device__ __forceinline__ void cf_relax(const CostFieldArgs& a, const uint32_t* cwp, const u64* lab, const u64* seed, int S, int SS,
                                         int me, u64 (&out)[NH]) {
  const int off[4] = {S, 1, -S, -1};
#pragma unroll
  for (int h = 0; h < NH; h++) out[h] = CF_NONE;
  const uint32_t cwv = cwp[me];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    // the edge u -> v in direction d: FROM pulls into v = me from u = me - off[d], TO pulls into u = me from v = me + off[d]
    const int other = TO ? me + off[d] : me - off[d];
    const uint32_t cwo = cwp[other];
    const uint32_t cw_u = TO ? cwv : cwo, cw_v = TO ? cwo : cwv;
    const bool flow = ((cw_u >> d) & 1u) != 0u;
    const bool ok = ((cw_v >> CW_ENTER) & 1u) && (flow || (a.ignore_flow && ((cw_v >> CW_ROAD) & 1u)));
    if (!ok) continue;
    const uint32_t base2 = (cw_v >> CW_COST) + (flow ? 0u : (uint32_t)a.contra2);
    if (NH == 1) {
      out[0] = min(out[0], cf_add(cf_lds_ld(&lab[other]), base2 >> 1, a.limit));
    } else if (!TO) {
      // arriving at me with heading d: from u's seed (no heading: no turn) or from u held with heading h
      u64 best = cf_add(seed[other], base2 >> 1, a.limit);
#pragma unroll
      for (int h = 0; h < 4; h++) best = min(best, cf_add(cf_lds_ld(&lab[h * SS + other]), (base2 + (h != d ? (uint32_t)a.turn2 : 0u)) >> 1, a.limit));
      out[d] = best;
    } else {
      // leaving me in direction d, having arrived with heading p
      const u64 l = cf_lds_ld(&lab[d * SS + other]);
#pragma unroll
      for (int p = 0; p < 4; p++) out[p] = min(out[p], cf_add(l, (base2 + (p != d ? (uint32_t)a.turn2 : 0u)) >> 1, a.limit));
    }
  }
}

// ---- the tile kernel -------------------------------------------------------------------------------------------------------
// One workgroup of T * T threads per active tile, one thread per cell.  The tile's words and labels and a one-cell halo of
// its neighbours' go to LDS; then sweeps: every cell takes the minimum over what its neighbours hold - as they are at that
// moment, some already lowered in this sweep: any label ever held is the cost of a real path, so an early value is as good an
// upper bound as a late one - and stores its labels where they fell.  One barrier per sweep; a sweep in which no label moved
// read the final labels everywhere, so they are the tile's fixpoint.  Cells whose labels changed are written back - own cells
// only - and the tiles across a border on which a label changed are put on the next round's list.  The halo is read from HBM
// while its owner may be writing: an older value is only a worse upper bound, and the owner's activation brings this tile
// back in the next launch, which sees everything this one wrote.  The workgroup waits for nobody but itself.
template <int NH, bool TO>
__global__ void __launch_bounds__(1024) k_cf_tile(CostFieldArgs a) {
  // (all LDS is dynamic and starts 16-byte aligned: label planes of SS 8-byte words, the cell words, then eight ints)
  extern __shared__ __attribute__((aligned(16))) u64 cf_lds[];
  const int T = a.T, S = T + 2, SS = S * S;
  constexpr bool SEEDS = NH == 4 && !TO;
  u64* s_lab = cf_lds;
  u64* s_seed = cf_lds + NH * SS;
  uint32_t* s_cw = (uint32_t*)(cf_lds + (NH + (SEEDS ? 1 : 0)) * SS);
  int* s_mark = (int*)(s_cw + SS);   // [0, 4): a label changed on the border towards N, E, S, W
  int* s_moved = s_mark + 4;         // [0, 3): "a label moved in sweep k", slot k % 3
  const int t = a.list_cur[blockIdx.x];
  const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
  const int x0 = tx * T, y0 = ty * T;
  if (threadIdx.x < 8) s_mark[threadIdx.x] = 0;
  if (threadIdx.x == 0) a.flag_cur[t] = 0u;   // (this round nobody else touches the flags of its own parity)
  for (int i = threadIdx.x; i < SS; i += blockDim.x) {
    const int ly = i / S, lx = i - ly * S;
    const int gx = x0 + lx - 1, gy = y0 + ly - 1;
    const bool in = (unsigned)gx < (unsigned)a.W && (unsigned)gy < (unsigned)a.H;
    const size_t c = in ? (size_t)gy * a.W + gx : 0;
    s_cw[i] = in ? a.cw[c] : 0u;
#pragma unroll
    for (int h = 0; h < NH; h++) s_lab[h * SS + i] = in ? cf_ld(&a.lab[(size_t)h * a.N + c]) : CF_NONE;
    if (SEEDS) s_seed[i] = in ? a.seed[c] : CF_NONE;
  }
  const int ly = threadIdx.x / T, lx = threadIdx.x - ly * T;
  const int me = (ly + 1) * S + lx + 1;
  const int gx = x0 + lx, gy = y0 + ly;
  const bool own = gx < a.W && gy < a.H;   // (the last tiles of a ragged map hang over its edge)
  __syncthreads();
  u64 cur[NH], cand[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) cur[h] = s_lab[h * SS + me];
  bool dirty = false;
  for (int sweep = 0;; sweep++) {
    const int slot = sweep % 3;
    bool ch = false;
    if (own) {
      cf_relax<NH, TO>(a, s_cw, s_lab, s_seed, S, SS, me, cand);
#pragma unroll
      for (int h = 0; h < NH; h++)
        if (cand[h] < cur[h]) { cur[h] = cand[h]; cf_lds_st(&s_lab[h * SS + me], cand[h]); ch = true; }
    }
    if (ch) { dirty = true; s_moved[slot] = 1; }
    __syncthreads();
    const int moved = s_moved[slot];
    // (the slot of sweep + 2 was last read before this barrier and is next written behind the next one)
    if (threadIdx.x == 0) s_moved[(sweep + 2) % 3] = 0;
    if (!moved) break;
  }
  if (dirty) {
    const size_t c = (size_t)gy * a.W + gx;
#pragma unroll
    for (int h = 0; h < NH; h++) cf_st(&a.lab[(size_t)h * a.N + c], cur[h]);
    if (ly == T - 1) s_mark[0] = 1;
    if (lx == T - 1) s_mark[1] = 1;
    if (ly == 0) s_mark[2] = 1;
    if (lx == 0) s_mark[3] = 1;
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_mark[threadIdx.x]) {
    const int k = threadIdx.x;
    const int ntx = tx + (k == 1) - (k == 3), nty = ty + (k == 0) - (k == 2);
    if ((unsigned)ntx < (unsigned)a.tiles_x && (unsigned)nty < (unsigned)a.tiles_y)
      cf_activate(a.flag_next, a.list_next, a.n_next, nty * a.tiles_x + ntx);
  }
}

// ---- the planes ------------------------------------------------------------------------------------------------------------
// value and owner of every cell from its labels (TO with four headings: one more relaxation, for "no heading"); tot[0] counts
// the cells reached, tot[1] is the largest value
template <int NH, bool TO>
__global__ void k_cf_finish(CostFieldArgs a, uint32_t* val, int32_t* own, unsigned long long* tot) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  u64 l = CF_NONE;
  if (c < a.N) {
    if (NH == 1) l = a.lab[c];
    else {
      l = a.seed[c];
      if (!TO) {
        for (int h = 0; h < 4; h++) l = min(l, a.lab[(size_t)h * a.N + c]);
      } else {
        const int y = c / a.W, x = c - y * a.W;
        const uint32_t cw_u = a.cw[c];
        for (int d = 0; d < 4; d++) {
          const int nx = x + (d == 1) - (d == 3), ny = y + (d == 0) - (d == 2);
          if ((unsigned)nx >= (unsigned)a.W || (unsigned)ny >= (unsigned)a.H) continue;
          const size_t w = (size_t)ny * a.W + nx;
          const uint32_t cw_v = a.cw[w];
          const bool flow = ((cw_u >> d) & 1u) != 0u;
          if (!(((cw_v >> CW_ENTER) & 1u) && (flow || (a.ignore_flow && ((cw_v >> CW_ROAD) & 1u))))) continue;
          l = min(l, cf_add(a.lab[(size_t)d * a.N + w], ((cw_v >> CW_COST) + (flow ? 0u : (uint32_t)a.contra2)) >> 1, a.limit));
        }
      }
    }
    const uint32_t v = (uint32_t)(l >> 32);
    const bool hit = v < a.limit;
    val[c] = hit ? v : TS_CF_UNREACHABLE;
    own[c] = hit ? (int32_t)(uint32_t)l : -1;
    if (!hit) l = CF_NONE;
  }
  const bool hit = l != CF_NONE;
  const unsigned long long n = __popcll(__ballot(hit));
  unsigned int m = hit ? (uint32_t)(l >> 32) : 0u;
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && n) { atomicAdd(&tot[0], n); atomicMax(&tot[1], (unsigned long long)m); }
}

// out[i] = plane[xy[i]] (the host has checked the cells)
__global__ void k_cf_gather(const uint32_t* plane, int W, int n, const int32_t* xy, uint32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = plane[(size_t)xy[2 * i + 1] * W + xy[2 * i]];
}

// hist[k] += road cells whose value lies in (thr[k - 1], thr[k]] (the host adds them up); thr ascends, n <= TS_CF_MAX_BANDS
__global__ void __launch_bounds__(BLK) k_cf_bands(const uint32_t* val, const int8_t* is_road, int N, int n, const uint32_t* thr,
                                                   unsigned long long* hist) {
  __shared__ uint32_t s_thr[TS_CF_MAX_BANDS], s_hist[TS_CF_MAX_BANDS];
  for (int k = threadIdx.x; k < n; k += blockDim.x) { s_thr[k] = thr[k]; s_hist[k] = 0u; }
  __syncthreads();
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long long)gridDim.x * blockDim.x) {
    if (is_road[c] != 1) continue;
    const uint32_t v = val[c];
    int lo = 0, hi = n;   // the first k with thr[k] >= v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_thr[mid] >= v) hi = mid; else lo = mid + 1;
    }
    if (lo < n) atomicAdd(&s_hist[lo], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += blockDim.x)
    if (s_hist[k]) atomicAdd(&hist[k], (unsigned long long)s_hist[k]);
}

}  // namespace
