// jams.h - jam detection (include/trafficsim_jams.h): connected-component labelling of the standing cells on the device.  The
// kernels, in the order ts_jams_compute (jams_api.h) launches them: mark (the count plane), init (own index as label, the list of
// occupied tiles), tile (components inside a tile, in LDS), merge (lock-free unions across the tile borders), flatten, number
// (roots -> jam numbers behind a hipcub scan), records, finish; and the per-group rows over the result.
// Part of the single translation unit engine.hip (included from there, behind observe.h whose wave sum it uses).
//
// The invariant every stage keeps: label[c] of a standing cell is the index of a standing cell of the same component that is not
// larger than c.  Labels only ever fall.  So a reader that sees an older value of a label - another workgroup's store that has not
// reached it yet - follows a pointer that is still correct, only longer; nothing here needs one workgroup's store to be seen by
// another inside a launch, and no workgroup waits for another.  The words other workgroups change inside a launch are written
// with atomicMin and read with agent-scope loads, which do not stop at a CU's L1.
// Every loop is capped: the tile sweeps at T * T + 1, a find at N hops, a union at N rounds.  A component's smallest label moves
// at least one cell per sweep, a find descends strictly, a union's pair descends strictly, so no cap is reached whatever the
// planes hold; one that is reached sets JamCtl::fault and the compute publishes nothing.
#pragma once
#include "../../include/trafficsim_jams.h"

namespace {

struct JamCtl {
  unsigned int n_tiles, fault;
  int n_jams, largest, standing_cells, pad_;
  unsigned long long standing_vehicles;
};

struct JamArgs {
  int W, H, N, n_active, n_vehicles, min_ticks, link, T, tiles_x, n_tile_slots, n_jams;
  const int32_t *active, *pos, *stuck_ticks;
  const uint16_t* flags;
  const Cell* cell;
  const uint8_t* mask;    // mask mode: the caller's bytes on the device
  uint32_t* count;        // [N]
  int32_t* label;         // [N]
  int32_t* tiles;         // [n_tile_slots]: the tiles that hold a standing cell, in no order
  uint32_t* tile_flag;    // [n_tile_slots], zeroed by the host: the tile is on the list
  int32_t *root, *num;    // [N + 1]: 1 at a root / the exclusive sum of that
  TsJamRecord* rec;       // [n_jams]
  int32_t* veh_jam;       // [n_vehicles], preset to -1 by the host
  JamCtl* ctl;            // zeroed by the host
};

__device__ __forceinline__ int jam_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// whether standing 4-neighbours u -> v in direction d (0 N, 1 E) are linked, from their stat bytes
__device__ __forceinline__ bool jam_linked(int link, uint8_t su, uint8_t sv, int d) {
  return link == TS_JAM_GRID || ((st_allowed(su) >> d) & 1) || ((st_allowed(sv) >> (d + 2)) & 1);
}

// 1a. one thread per entry of the active list: a standing vehicle adds 1 at its cell
__global__ void k_jam_mark_vehicles(JamArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_active) return;
  const int vid = a.active[i];
  if ((unsigned)vid >= (unsigned)a.n_vehicles) return;
  const int p = a.pos[vid];
  if ((unsigned)p >= (unsigned)a.N) return;
  if (a.stuck_ticks[vid] >= a.min_ticks && !(a.flags[vid] & VF_PARKED)) atomicAdd(&a.count[p], 1u);
}

// 1b. mask mode: one thread per cell widens the byte
__global__ void k_jam_mark_mask(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < a.N) a.count[c] = a.mask[c];
}

// 1c. one thread per cell: the cell's own index where it stands, -1 elsewhere; the first standing lane of a tile's run inside the
// wave (the lanes of a wave are consecutive cells: those of one tile and row are a run of up to T lanes) puts the tile on the
// list unless its flag says that it is there
__global__ void k_jam_init(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  const bool st = c < a.N && a.count[c] > 0;
  if (c < a.N) a.label[c] = st ? c : -1;
  const unsigned long long b = __ballot(st);
  if (!a.T || !st) return;
  const int y = c / a.W, x = c - y * a.W;
  const int lo = max(lane - x % a.T, 0);   // the run's first lane in this wave
  const unsigned long long before = b & ((1ull << lane) - 1ull) & ~((1ull << lo) - 1ull);
  if (before) return;
  const int t = (y / a.T) * a.tiles_x + x / a.T;
  if (atomicExch(&a.tile_flag[t], 1u) == 0u) {
    const unsigned int k = atomicAdd(&a.ctl->n_tiles, 1u);
    if (k < (unsigned)a.n_tile_slots) a.tiles[k] = t;
  }
}

// 2. one workgroup per listed tile, one thread per cell.  Standing bits, stat bytes and labels lie in LDS, rows padded by one
// element so that a column's cells fall into different banks.  A label here is the cell's position ly * T + lx in the tile.  Per
// sweep a thread takes the minimum over its own label and its linked neighbours' inside the tile, follows it (l = lab[l]) and
// stores it when it is smaller; only the cell's own thread stores its label, so it only falls.  __syncthreads_or is the sweep's
// one barrier and its block-wide "changed".  A sweep that changes nothing read nothing that moved: every cell then holds the
// smallest position of its component in the tile.
template <int T>
__global__ void __launch_bounds__(T * T) k_jam_tile(JamArgs a) {
  constexpr int P = T + 1;
  __shared__ int32_t s_lab[T * P];
  __shared__ uint8_t s_stat[T * P], s_st[T * P];
  if (blockIdx.x >= a.ctl->n_tiles || blockIdx.x >= (unsigned)a.n_tile_slots) return;   // (the whole workgroup)
  const int t = a.tiles[blockIdx.x];
  const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
  const int lx = threadIdx.x % T, ly = threadIdx.x / T, me = ly * P + lx;
  const int x = tx * T + lx, y = ty * T + ly, c = y * a.W + x;
  const bool st = x < a.W && y < a.H && a.count[c] > 0;
  s_st[me] = st;
  s_stat[me] = st ? a.cell[c].stat : 0;
  s_lab[me] = (int)threadIdx.x;
  __syncthreads();
  // the padded positions of the linked neighbours inside the tile, -1 = none
  int nb[4] = {-1, -1, -1, -1};
  if (st) {
    const uint8_t su = s_stat[me];
    if (ly + 1 < T && s_st[me + P] && jam_linked(a.link, su, s_stat[me + P], 0)) nb[0] = me + P;
    if (lx + 1 < T && s_st[me + 1] && jam_linked(a.link, su, s_stat[me + 1], 1)) nb[1] = me + 1;
    if (ly > 0 && s_st[me - P] && jam_linked(a.link, s_stat[me - P], su, 0)) nb[2] = me - P;
    if (lx > 0 && s_st[me - 1] && jam_linked(a.link, s_stat[me - 1], su, 1)) nb[3] = me - 1;
  }
  int mine = (int)threadIdx.x, sweeps = 0;
  for (;;) {
    int m = mine;
    for (int k = 0; k < 4; k++)
      if (nb[k] >= 0) m = min(m, s_lab[nb[k]]);
    m = s_lab[(m / T) * P + m % T];
    m = s_lab[(m / T) * P + m % T];
    const bool changed = m < mine;
    if (changed) { mine = m; s_lab[me] = m; }
    if (!__syncthreads_or(changed)) break;
    if (++sweeps > T * T + 1) {   // (uniform: every thread counts the same sweeps)
      if (threadIdx.x == 0) atomicOr(&a.ctl->fault, 1u);
      break;
    }
  }
  if (st) a.label[c] = (ty * T + mine / T) * a.W + tx * T + mine % T;
}

// the root of c: labels descend strictly until one points at itself.  -1: the cap was reached
__device__ __forceinline__ int jam_find(const JamArgs& a, int c) {
  for (int hops = 0; hops <= a.N; hops++) {
    const int l = jam_load(&a.label[c]);
    if (l == c) return c;
    if ((unsigned)l >= (unsigned)c) break;   // (no label a stage wrote: labels fall)
    c = l;
  }
  atomicOr(&a.ctl->fault, 2u);
  return -1;
}

// the union of the components of u and v: find both roots, lower the larger root's label to the smaller root; when that label
// had moved meanwhile (the root was no root any more) go on with what it held.  (hi, lo) falls strictly from round to round.
__device__ void jam_union(const JamArgs& a, int u, int v) {
  for (int rounds = 0; rounds <= a.N; rounds++) {
    const int ru = jam_find(a, u), rv = jam_find(a, v);
    if (ru < 0 || rv < 0 || ru == rv) return;
    const int hi = max(ru, rv), lo = min(ru, rv);
    const int old = atomicMin(&a.label[hi], lo);
    if (old == hi) return;
    u = old; v = lo;
  }
  atomicOr(&a.ctl->fault, 4u);
}

// 3. one thread per cell: a standing cell unites itself with its linked E and N neighbours where the tile stage has not
__global__ void k_jam_merge(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.N || a.count[c] == 0) return;
  const int y = c / a.W, x = c - y * a.W;
  const uint8_t su = a.link == TS_JAM_FLOW ? a.cell[c].stat : 0;
  if (x + 1 < a.W && (!a.T || (x + 1) % a.T == 0) && a.count[c + 1] > 0 &&
      jam_linked(a.link, su, a.link == TS_JAM_FLOW ? a.cell[c + 1].stat : 0, 1))
    jam_union(a, c, c + 1);
  if (y + 1 < a.H && (!a.T || (y + 1) % a.T == 0) && a.count[c + a.W] > 0 &&
      jam_linked(a.link, su, a.link == TS_JAM_FLOW ? a.cell[c + a.W].stat : 0, 0))
    jam_union(a, c, c + a.W);
}

// 4. one thread per cell: a standing cell stores its root, and the roots are flagged for the scan (root[N] = 0 closes it)
__global__ void k_jam_flatten(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > a.N) return;
  int r = -1;
  if (c < a.N && a.count[c] > 0) {
    r = jam_find(a, c);
    if (r >= 0) a.label[c] = r;   // (still a correct pointer for whoever walks through c)
  }
  a.root[c] = r == c && c < a.N ? 1 : 0;
}

// 5. one thread per cell: root -> jam number; a root fills in where its record starts
__global__ void k_jam_number(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.N) return;
  const int r = a.label[c];
  if (r < 0) return;
  const int j = (unsigned)a.num[r] < (unsigned)a.n_jams ? a.num[r] : -1;   // (always inside: num counts the roots)
  a.label[c] = j;
  if (j < 0) return;   // (num, not label, is read at r: the plane is rewritten in place)
  if (r == c) {
    TsJamRecord& R = a.rec[j];
    const int y = c / a.W;
    R.root_x = c - y * a.W; R.root_y = y;
    R.x0 = R.y0 = 0x7FFFFFFF; R.x1 = R.y1 = -1;
  }
}

__device__ __forceinline__ unsigned int jam_wave_sum(unsigned int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 6a. one thread per cell adds into its jam's record.  The lanes of a wave are consecutive cells, so a queue along a row fills
// many lanes with one jam: per distinct (jam, row) in the wave one lane adds what all of them hold - the run's cells and its
// ends from the ballot, the counts by a wave sum.  Integer adds, min and max only: the record does not depend on the order.
__global__ void k_jam_record_cells(JamArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  const int j = c < a.N && (unsigned)a.label[c] < (unsigned)a.n_jams ? a.label[c] : -1;
  const int y = c / a.W, x = c - y * a.W;
  const unsigned int cnt = j >= 0 ? a.count[c] : 0u;
  const bool inter = j >= 0 && st_inter(a.cell[c].stat);
  unsigned long long todo = __ballot(j >= 0);
  if (!todo) return;
  const unsigned int cells = (unsigned)__popcll(todo), veh = jam_wave_sum(cnt);
  if (lane == 0) {
    atomicAdd(&a.ctl->standing_cells, (int)cells);
    atomicAdd(&a.ctl->standing_vehicles, (unsigned long long)veh);
  }
  while (todo) {   // (uniform: todo is the same in every lane)
    const int lead = __ffsll((long long)todo) - 1;
    const int jl = __shfl(j, lead), yl = __shfl(y, lead);
    const bool mate = j == jl && y == yl;
    const unsigned long long m = __ballot(mate), mi = __ballot(mate && inter);
    const unsigned int v = jam_wave_sum(mate ? cnt : 0u);
    if (lane == lead) {
      TsJamRecord& R = a.rec[jl];
      atomicAdd(&R.cells, __popcll(m));
      atomicAdd(&R.vehicles, v);
      if (mi) atomicAdd(&R.inter_cells, __popcll(mi));
      atomicMin(&R.x0, x);
      atomicMax(&R.x1, x + (63 - __clzll((long long)m)) - lead);
      atomicMin(&R.y0, y);
      atomicMax(&R.y1, y);
    }
    todo &= ~m;
  }
}

// 6b. one thread per entry of the active list: a standing vehicle's jam by spawn index, its stuck_ticks into the record.  (The
// active list is in no order of space: its lanes seldom share a jam, and a wave-wide search for mates costs more than it saves.)
__global__ void k_jam_record_vehicles(JamArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_active) return;
  const int vid = a.active[i];
  if ((unsigned)vid >= (unsigned)a.n_vehicles) return;
  const int p = a.pos[vid];
  if ((unsigned)p >= (unsigned)a.N) return;
  const int s = a.stuck_ticks[vid];
  if (s < a.min_ticks || (a.flags[vid] & VF_PARKED)) return;
  const int j = a.label[p];
  if ((unsigned)j >= (unsigned)a.n_jams) return;
  a.veh_jam[vid] = j;
  atomicMax(&a.rec[j].stuck_max, s);
  atomicAdd((unsigned long long*)&a.rec[j].stuck_sum, (unsigned long long)s);
}

// 6c. one thread per jam: the extent, and the largest jam's cells through a wave maximum
__global__ void k_jam_finish(JamArgs a, int n_jams) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  int cells = 0;
  if (j < n_jams) {
    TsJamRecord& R = a.rec[j];
    R.extent = max(R.x1 - R.x0, R.y1 - R.y0) + 1;
    cells = R.cells;
  }
  for (int o = 32; o; o >>= 1) cells = max(cells, __shfl_xor(cells, o));
  if ((threadIdx.x & 63) == 0 && cells > 0) atomicMax(&a.ctl->largest, cells);
}

// the five values of one CSR list of a group, by the whole wave: lanes stride over the list in rounds of 64; the entry at
// position k counts when no earlier position of the list holds the same jam (a plain scan of the earlier entries: the lists are
// a few dozen cells).  Returns the standing cells of the list.
__device__ __forceinline__ long long jam_group_list(const int32_t* label, const TsJamRecord* rec, const int32_t* off, const int32_t* cells,
                                                    int g, int lane, long long* v) {
  const int k0 = off[g], k1 = off[g + 1];
  unsigned long long n = 0, sc = 0, sv = 0, standing = 0;
  int smax = 0, ext = 0;
  for (int k = k0 + lane; k < k1; k += 64) {
    const int j = label[cells[k]];
    if (j < 0) continue;
    standing++;
    bool first = true;
    for (int p = k0; p < k && first; p++) first = label[cells[p]] != j;
    if (!first) continue;
    const TsJamRecord& R = rec[j];
    n++; sc += (unsigned long long)R.cells; sv += R.vehicles;
    smax = max(smax, R.stuck_max); ext = max(ext, R.extent);
  }
  n = obs_wave_sum(n); sc = obs_wave_sum(sc); sv = obs_wave_sum(sv); standing = obs_wave_sum(standing);
  for (int o = 32; o; o >>= 1) { smax = max(smax, __shfl_down(smax, o)); ext = max(ext, __shfl_down(ext, o)); }
  v[0] = (long long)n; v[1] = (long long)sc; v[2] = (long long)sv; v[3] = smax; v[4] = ext;   // (valid in lane 0)
  return (long long)standing;
}

// 7. one wavefront per light group over the CSR tables the move phase uses (g_nsin, g_ewin, g_icell)
__global__ void k_jam_groups(Dev d, const int32_t* label, const TsJamRecord* rec, long long* rows) {
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= d.G) return;   // (whole waves leave: the shuffles stay inside one wave)
  long long v[TS_JG_NFIELDS], box[5];
  jam_group_list(label, rec, d.g_nsin_off, d.g_nsin, g, lane, v + TS_JG_NS_JAMS);
  jam_group_list(label, rec, d.g_ewin_off, d.g_ewin, g, lane, v + TS_JG_EW_JAMS);
  v[TS_JG_BOX_CELLS] = jam_group_list(label, rec, d.g_icell_off, d.g_icell, g, lane, box);
  v[TS_JG_BOX_JAMS] = box[0];
  if (lane == 0)
    for (int k = 0; k < TS_JG_NFIELDS; k++) rows[(size_t)g * TS_JG_NFIELDS + k] = v[k];
}

}  // namespace
