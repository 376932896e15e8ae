// selectlink.h - select-link analysis (include/trafficsim_selectlink.h): the kernel that walks the remaining main path of every
// live vehicle over the gate plane and leaves the per-vehicle values and the cross / pair tables, and the small kernels around
// it (the scatter that builds the gate plane, the selection, the OD counts).  Part of the single translation unit engine.hip
// (included from there, behind demand.h whose conventions and reductions it uses).
#pragma once
#include "../../include/trafficsim_selectlink.h"

namespace {

// the walk's tables in LDS and, with 64-bit entries, on the device: cross[32][8][4], pair[32][32], then the three scalar totals
constexpr int SL_G = TS_SL_MAX_GATES, SL_NCROSS = SL_G * TS_DEMAND_MAX_BINS * 4, SL_NPAIR = SL_G * SL_G;
constexpr int SL_CROSS = 0, SL_PAIR = SL_NCROSS, SL_TOT = SL_NCROSS + SL_NPAIR;
constexpr int SL_T_VEH = 0, SL_T_CROSSING = 1, SL_T_CROSSINGS = 2, SL_NTOT = 3, SL_NTAB = SL_TOT + SL_NTOT;

// the result's per-vehicle arrays, by spawn index.  pos < 0: the index was no vehicle walked
struct SlVeh {
  uint32_t *mask, *crossings;
  int32_t *first_step, *pos, *target;
  int8_t* first_gate;
  uint8_t* select;
};

struct SelectLinkArgs {
  int W, N, n_active, n_vehicles;
  const int32_t *active, *pos, *target, *path_len, *path_cur;
  const uint32_t *path_off, *pool;
  const uint32_t* gates;     // [N]: byte d = 1 + the gate of a step entering in direction d, 0 = none
  SlVeh v;                   // preset by the host to "not walked"
  unsigned long long* tab;   // [SL_NTAB], zeroed by the host
  int n_bins, bin_cells, open_tail;
  int limit;                 // min(n_bins * bin_cells, INT_MAX): the first step beyond the last bin
  int spl;                   // path steps per lane and iteration (a team covers spl * T)
};

// gate plane: one thread per gate cell ORs its word in (a cell may stand in the list once per direction)
__global__ void k_selectlink_scatter(int n, const int32_t* cell, const uint32_t* word, uint32_t* plane) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) atomicOr(&plane[cell[k]], word[k]);
}

template <int T>
__device__ __forceinline__ uint32_t sl_team_or(uint32_t v) {
  for (int o = T >> 1; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, T);
  return v;
}
template <int T>
__device__ __forceinline__ uint32_t sl_team_sum(uint32_t v) {
  for (int o = T >> 1; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, T);
  return v;
}
template <int T>
__device__ __forceinline__ unsigned long long sl_team_min(unsigned long long v) {
  for (int o = T >> 1; o; o >>= 1) { const unsigned long long u = __shfl_xor(v, o, T); v = u < v ? u : v; }
  return v;
}

// k_demand_walk's shape (demand.h): a team of T lanes per vehicle, 64 / T vehicles per wavefront in the active list's order; per
// iteration lane l decodes steps [l * spl, (l + 1) * spl) into their displacement, a prefix sum over the team gives the cell in
// front of every lane's first step, and the lane walks its steps again.  Where the demand walk issues an atomic per step, this one
// loads the cell's gate word.  A hit updates the lane's registers - the mask, the count, its first (step, gate), which is its
// smallest: a lane's steps ascend - and adds 1 to the block's cross table in LDS.  At the end of a vehicle the team reduces the
// four values with shuffles ((step, gate) as one 64-bit key: a step can need 31 bits), lane 0 stores them by spawn index with the
// copy of pos / target, and the team adds the mask's pairs into the block's pair table.  At the end of the block the tables go to
// the 64-bit ones with one atomic per non-zero entry.  No workgroup waits for another; every loop is bounded by path_len or 32.
// (An LDS entry is 32 bits: it would wrap only if one block counted 2^32 crossings of one gate, bin and direction - a sixteenth
// of the largest path pool there can be, in the hands of one block of up to a couple of thousand.)
template <int T>
__global__ void __launch_bounds__(BLK) k_selectlink_walk(SelectLinkArgs a) {
  constexpr int VPW = 64 / T;
  __shared__ uint32_t s_cross[SL_NCROSS];
  __shared__ uint32_t s_pair[SL_NPAIR];
  __shared__ unsigned long long s_tot[SL_NTOT];
  const int lane = threadIdx.x & 63, tl = lane & (T - 1), team = lane / T;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
  const int chunk = a.spl * T, last_bin = a.n_bins - 1;
  for (int k = threadIdx.x; k < SL_NCROSS; k += blockDim.x) s_cross[k] = 0;
  for (int k = threadIdx.x; k < SL_NPAIR; k += blockDim.x) s_pair[k] = 0;
  if (threadIdx.x < SL_NTOT) s_tot[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long ncross_lane = 0;
  unsigned int nveh = 0, ncrossing = 0;
  for (long long first = (long long)wave * VPW; first < a.n_active; first += (long long)n_waves * VPW) {
    const long long i = first + team;
    int plen = 0, pcur = 0, carry = 0, vid = -1, pos0 = 0;
    uint32_t off = 0;
    if (i < a.n_active) {
      const int id = a.active[i];
      if ((unsigned)id < (unsigned)a.n_vehicles) {
        carry = a.pos[id];
        if ((unsigned)carry < (unsigned)a.N) {
          vid = id; pos0 = carry;
          pcur = a.path_cur[id]; plen = a.path_len[id] - pcur; off = a.path_off[id];
          if (!a.open_tail) plen = min(plen, a.limit);
        }
      }
    }
    uint32_t m = 0, nc = 0;
    unsigned long long key = ~0ull;   // (step << 8 | gate) of the lane's first crossing
    // (plen is the same in all lanes of a team: the shuffles below stay among lanes that run the same iterations)
    for (int base = 0; base < plen; base += chunk) {
      const int k0 = base + tl * a.spl, nv = max(0, min(a.spl, plen - k0));
      int disp = 0;
      uint32_t w = 0;
      for (int j = 0, s = pcur + k0; j < nv; j++, s++) {
        if (j == 0 || (s & PATH_STEP_MASK) == 0) w = a.pool[off + ((uint32_t)s >> PATH_STEP_SHIFT)];
        disp += dir_delta((w >> ((s & PATH_STEP_MASK) * PATH_DIR_BITS)) & PATH_DIR_MASK, a.W);
      }
      int incl = disp;
      for (int o = 1; o < T; o <<= 1) {
        const int u = __shfl_up(incl, o, T);
        if (tl >= o) incl += u;
      }
      int c = carry + incl - disp;
      carry += __shfl(incl, T - 1, T);
      int bin = last_bin, rem = 0;
      if (k0 < a.limit) { bin = k0 / a.bin_cells; rem = k0 - bin * a.bin_cells; }
      for (int j = 0, s = pcur + k0; j < nv; j++, s++) {
        if (j == 0 || (s & PATH_STEP_MASK) == 0) w = a.pool[off + ((uint32_t)s >> PATH_STEP_SHIFT)];
        const int dir = (w >> ((s & PATH_STEP_MASK) * PATH_DIR_BITS)) & PATH_DIR_MASK;
        c += dir_delta(dir, a.W);
        if ((unsigned)c < (unsigned)a.N) {
          const uint32_t g1 = (a.gates[c] >> (dir * 8)) & 0xFFu;
          if (g1) {
            const uint32_t g = g1 - 1;
            m |= 1u << g;
            nc++;
            if (key == ~0ull) key = ((unsigned long long)(unsigned)(k0 + j) << 8) | g;
            atomicAdd(&s_cross[(g * TS_DEMAND_MAX_BINS + bin) * 4 + dir], 1u);
          }
        }
        if (++rem == a.bin_cells) { rem = 0; bin = min(bin + 1, last_bin); }
      }
    }
    // every lane of the wave is here again: the team's four values
    ncross_lane += nc;
    m = sl_team_or<T>(m);
    nc = sl_team_sum<T>(nc);
    key = sl_team_min<T>(key);
    if (vid >= 0) {
      if (tl == 0) {
        a.v.mask[vid] = m;
        a.v.crossings[vid] = nc;
        a.v.first_step[vid] = key == ~0ull ? -1 : (int)(key >> 8);
        a.v.first_gate[vid] = key == ~0ull ? (int8_t)-1 : (int8_t)(key & 0xFF);
        a.v.pos[vid] = pos0;
        a.v.target[vid] = a.target[vid];
        a.v.select[vid] = 1;
        nveh++;
        if (m) ncrossing++;
      }
      for (int ga = tl; ga < SL_G; ga += T)
        if ((m >> ga) & 1u)
          for (uint32_t r = m; r; r &= r - 1) atomicAdd(&s_pair[ga * SL_G + (__ffs((int)r) - 1)], 1u);
    }
  }
  const unsigned long long t_veh = obs_wave_sum((unsigned long long)nveh), t_crossing = obs_wave_sum((unsigned long long)ncrossing),
                           t_crossings = obs_wave_sum(ncross_lane);
  if (lane == 0) {
    if (t_veh) atomicAdd(&s_tot[SL_T_VEH], t_veh);
    if (t_crossing) atomicAdd(&s_tot[SL_T_CROSSING], t_crossing);
    if (t_crossings) atomicAdd(&s_tot[SL_T_CROSSINGS], t_crossings);
  }
  __syncthreads();   // (every thread arrives: nothing above returns)
  for (int k = threadIdx.x; k < SL_NCROSS; k += blockDim.x)
    if (s_cross[k]) atomicAdd(&a.tab[SL_CROSS + k], (unsigned long long)s_cross[k]);
  for (int k = threadIdx.x; k < SL_NPAIR; k += blockDim.x)
    if (s_pair[k]) atomicAdd(&a.tab[SL_PAIR + k], (unsigned long long)s_pair[k]);
  if (threadIdx.x < SL_NTOT && s_tot[threadIdx.x]) atomicAdd(&a.tab[SL_TOT + threadIdx.x], s_tot[threadIdx.x]);
}

// whether spawn index i of a result is selected by (any, all, none)
__device__ __forceinline__ bool sl_selected(const SlVeh& v, int i, uint32_t any, uint32_t all, uint32_t none) {
  if (v.pos[i] < 0) return false;
  const uint32_t m = v.mask[i];
  return (any == 0 || (m & any)) && (m & all) == all && (m & none) == 0;
}

// one thread per spawn index: the select byte, and the number selected
__global__ void k_selectlink_select(SlVeh v, int n, uint32_t any, uint32_t all, uint32_t none, unsigned long long* count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool sel = i < n && sl_selected(v, i, any, all, none);
  if (i < n) v.select[i] = sel ? 1 : 0;
  const unsigned long long b = __ballot(sel);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(b));
}

// one thread per spawn index: counts[zone(pos)][zone(target)] of the selected, out[nz * nz] = those without a zone at either end
__global__ void k_selectlink_od(SlVeh v, int n, uint32_t any, uint32_t all, uint32_t none, const int32_t* zone, int nz, int N,
                                unsigned long long* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool unzoned = false;
  if (i < n && sl_selected(v, i, any, all, none)) {
    const int p = v.pos[i], t = v.target[i];
    const int zo = (unsigned)p < (unsigned)N ? zone[p] : -1, zd = (unsigned)t < (unsigned)N ? zone[t] : -1;
    if (zo < 0 || zd < 0 || zo >= nz || zd >= nz) unzoned = true;
    else atomicAdd(&out[(size_t)zo * nz + zd], 1ull);
  }
  const unsigned long long b = __ballot(unzoned);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(&out[(size_t)nz * nz], (unsigned long long)__popcll(b));
}

}  // namespace
