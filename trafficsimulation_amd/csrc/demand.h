// demand.h - route demand (include/trafficsim_demand.h): the kernel that walks the remaining main path of every live
// vehicle and counts each planned step into a [bin][direction] plane, and the small kernels that bring the planes off
// the device (the sum of a bin's four planes, the group rows).  Part of the single translation unit engine.hip
// (included from there, behind observe.h whose reductions it uses).
#pragma once
#include "../../include/trafficsim_demand.h"

namespace {

// k_demand_walk's totals: [0, 8) steps counted per bin, [8] vehicles counted
constexpr int DM_VEH = TS_DEMAND_MAX_BINS, DM_NTOT = TS_DEMAND_MAX_BINS + 1;

struct DemandArgs {
  int W, N, n_active, n_vehicles;
  const int32_t *active, *pos, *path_len, *path_cur;
  const uint32_t *path_off, *pool;
  const uint8_t* select;     // per spawn index, nullptr = every vehicle
  uint32_t* planes;          // [n_bins][4][N]
  unsigned long long* tot;   // [DM_NTOT], zeroed by the host
  int n_bins, bin_cells, open_tail;
  int limit;                 // min(n_bins * bin_cells, INT_MAX): the first step beyond the last bin
  int spl;                   // path steps per lane and iteration (a team covers spl * T)
};

// A team of T lanes per vehicle, 64 / T vehicles per wavefront, taken in the active list's order.  Per iteration a team
// covers spl * T steps of the path: lane l decodes steps [l * spl, (l + 1) * spl) into the displacement they add up to
// (the packed words start at path_cur, mid-word as a rule), an exclusive prefix sum over the team turns the displacements
// into the cell in front of every lane's first step, and the lane walks its steps again with one return-less atomicAdd
// per step.  A cell index is one int (N is + W, E is + 1), so one prefix sum serves both axes.  The totals are counted in
// registers, reduced per wave with shuffles and per block through LDS: one atomic per block and total.
template <int T>
__global__ void __launch_bounds__(BLK) k_demand_walk(DemandArgs a) {
  constexpr int VPW = 64 / T;
  __shared__ unsigned long long s_tot[DM_NTOT];
  const int lane = threadIdx.x & 63, tl = lane & (T - 1), team = lane / T;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
  const int chunk = a.spl * T, last_bin = a.n_bins - 1;
  if (threadIdx.x < DM_NTOT) s_tot[threadIdx.x] = 0;
  unsigned long long cnt[TS_DEMAND_MAX_BINS] = {};
  unsigned int nveh = 0;
  for (long long first = (long long)wave * VPW; first < a.n_active; first += (long long)n_waves * VPW) {
    const long long i = first + team;
    int plen = 0, pcur = 0, carry = 0;   // (carry: the cell in front of the iteration's first step)
    uint32_t off = 0;
    if (i < a.n_active) {
      const int vid = a.active[i];
      if ((unsigned)vid < (unsigned)a.n_vehicles && (!a.select || a.select[vid])) {
        carry = a.pos[vid];
        if ((unsigned)carry < (unsigned)a.N) {
          pcur = a.path_cur[vid]; plen = a.path_len[vid] - pcur; off = a.path_off[vid];
          if (!a.open_tail) plen = min(plen, a.limit);
          if (tl == 0) nveh++;
        }
      }
    }
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
      unsigned long long pk = 0;   // eight 8-bit counts, one per bin
      for (int j = 0, s = pcur + k0; j < nv; j++, s++) {
        if (j == 0 || (s & PATH_STEP_MASK) == 0) w = a.pool[off + ((uint32_t)s >> PATH_STEP_SHIFT)];
        const int dir = (w >> ((s & PATH_STEP_MASK) * PATH_DIR_BITS)) & PATH_DIR_MASK;
        c += dir_delta(dir, a.W);
        if ((unsigned)c < (unsigned)a.N) {
          atomicAdd(&a.planes[(size_t)(bin * 4 + dir) * (size_t)a.N + (size_t)c], 1u);
          pk += 1ull << (bin * 8);
        }
        if (++rem == a.bin_cells) { rem = 0; bin = min(bin + 1, last_bin); }
        if ((j & 127) == 127 || j == nv - 1) {
#pragma unroll
          for (int b = 0; b < TS_DEMAND_MAX_BINS; b++) cnt[b] += (pk >> (b * 8)) & 0xFF;
          pk = 0;
        }
      }
    }
  }
  __syncthreads();   // (s_tot is zero; every thread arrives: nothing above returns)
#pragma unroll
  for (int b = 0; b < TS_DEMAND_MAX_BINS; b++) {
    const unsigned long long v = obs_wave_sum(cnt[b]);
    if (lane == 0 && v) atomicAdd(&s_tot[b], v);
  }
  const unsigned long long nv_wave = obs_wave_sum((unsigned long long)nveh);
  if (lane == 0 && nv_wave) atomicAdd(&s_tot[DM_VEH], nv_wave);
  __syncthreads();
  if (threadIdx.x < DM_NTOT && s_tot[threadIdx.x]) atomicAdd(&a.tot[threadIdx.x], s_tot[threadIdx.x]);
}

// dst = the sum of a bin's four direction planes
__global__ void k_demand_sum4(const uint32_t* p, int N, uint32_t* dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  dst[i] = p[i] + p[(size_t)N + i] + p[2 * (size_t)N + i] + p[3 * (size_t)N + i];
}

// the sum of the four planes at `bin4` over one CSR row, by one wavefront (lane 0 holds it)
__device__ __forceinline__ unsigned long long dm_csr_sum4(const int32_t* off, const int32_t* cells, int g, int lane,
                                                          const uint32_t* bin4, int N) {
  unsigned long long s = 0;
  for (int k = off[g] + lane; k < off[g + 1]; k += 64) {
    const int c = cells[k];
    s += (unsigned long long)bin4[c] + bin4[(size_t)N + c] + bin4[2 * (size_t)N + c] + bin4[3 * (size_t)N + c];
  }
  return obs_wave_sum(s);
}

// one wavefront per (light group, bin) over the CSR tables k_obs_groups uses: rows[G][n_bins][TS_DG_NFIELDS]
__global__ void k_demand_groups(Dev d, const uint32_t* planes, int n_bins, long long* rows) {
  const int item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= d.G * n_bins) return;   // (whole waves leave: the shuffles below stay inside one wave)
  const int g = item / n_bins, bin = item - g * n_bins;
  const uint32_t* bin4 = planes + (size_t)bin * 4 * (size_t)d.N;
  unsigned long long v[TS_DG_NFIELDS];
  v[TS_DG_NS_IN] = dm_csr_sum4(d.g_nsin_off, d.g_nsin, g, lane, bin4, d.N);
  v[TS_DG_EW_IN] = dm_csr_sum4(d.g_ewin_off, d.g_ewin, g, lane, bin4, d.N);
  obs_csr_sum2(d.g_icell_off, d.g_icell, g, lane, bin4, bin4 + (size_t)d.N, v[TS_DG_ENTER_N], v[TS_DG_ENTER_E]);
  obs_csr_sum2(d.g_icell_off, d.g_icell, g, lane, bin4 + 2 * (size_t)d.N, bin4 + 3 * (size_t)d.N, v[TS_DG_ENTER_S], v[TS_DG_ENTER_W]);
  if (lane == 0)
    for (int k = 0; k < TS_DG_NFIELDS; k++) rows[(size_t)item * TS_DG_NFIELDS + k] = (long long)v[k];
}

}  // namespace
