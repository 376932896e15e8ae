// observe.h - traffic observation (include/trafficsim_observe.h): the increment the move kernel makes for every cell a
// vehicle enters, the end-of-tick sampling kernel, and the reductions that bring a plane off the device small.
// Part of the single translation unit engine.hip (included from there, in front of kernels.h).
#pragma once

namespace {

constexpr uint32_t OBS_SAMPLED = (1u << TS_OBS_PRESENT) | (1u << TS_OBS_WAITING) | (1u << TS_OBS_SPEED);   // k_obs_sample's planes
constexpr uint32_t OBS_ENTER = (1u << TS_OBS_ENTER_N) | (1u << TS_OBS_ENTER_E) | (1u << TS_OBS_ENTER_S) | (1u << TS_OBS_ENTER_W);

// One step of a vehicle into cell `nc` in direction `dir` (N0 E1 S2 W3).  The caller has tested d.obs_enter.
__device__ __forceinline__ void obs_enter_dev(const Dev& d, int dir, int nc) {
  uint32_t* p = d.obs[TS_OBS_ENTER_N + dir];
  if (p) atomicAdd(&p[nc], 1u);
}

// End of a tick: every entry of the (compacted) active list is a live vehicle - a row of ts_download_vehicles.
__global__ void k_obs_sample(Dev d, int n_active) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_active) return;
  const int vid = d.active[i];
  if (vid < 0) return;
  const int pos = d.pos[vid];
  if ((unsigned)pos >= (unsigned)d.N) return;
  if (d.obs[TS_OBS_PRESENT]) atomicAdd(&d.obs[TS_OBS_PRESENT][pos], 1u);
  if (d.obs[TS_OBS_WAITING] && d.stuck_ticks[vid] > 0 && !(d.flags[vid] & VF_PARKED)) atomicAdd(&d.obs[TS_OBS_WAITING][pos], 1u);
  if (d.obs[TS_OBS_SPEED]) {
    const uint32_t v = (uint32_t)(int)d.cur_speed[vid];
    if (v) atomicAdd(&d.obs[TS_OBS_SPEED][pos], v);
  }
}

__device__ __forceinline__ unsigned long long obs_wave_sum(unsigned long long v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  return v;   // (lane 0 holds the sum)
}

// Sum of plane[y0..y1) x [x0..x1) by the whole block, 64-bit: lanes stride over the rectangle row by row, waves reduce
// with shuffles, the block through LDS.  The result is valid in thread 0.  An empty rectangle sums to 0.
__device__ unsigned long long obs_block_rect_sum(const uint32_t* plane, int W, int x0, int y0, int x1, int y1) {
  __shared__ unsigned long long wsum[BLK / 64];
  unsigned long long acc = 0;
  const int tw = x1 - x0, th = y1 - y0;
  if (tw > 0 && th > 0) {
    const long long n = (long long)tw * th;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
      const int ry = (int)(i / tw), rx = (int)(i - (long long)ry * tw);
      acc += plane[(size_t)(y0 + ry) * W + (x0 + rx)];
    }
  }
  acc = obs_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  unsigned long long t = 0;
  if (threadIdx.x == 0) for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += wsum[w];
  return t;
}

// one block per output cell: the factor x factor tile (partial at the edges) it stands for
__global__ void k_obs_pool(const uint32_t* plane, int W, int H, int f, int ow, unsigned long long* out) {
  const int bx = blockIdx.x, by = blockIdx.y;
  const int x0 = bx * f, y0 = by * f;
  const unsigned long long t = obs_block_rect_sum(plane, W, x0, y0, min(W, x0 + f), min(H, y0 + f));
  if (threadIdx.x == 0) out[(size_t)by * ow + bx] = t;
}

// one block per rectangle (x0, y0, x1, y1, half-open), clipped to the map here
__global__ void k_obs_regions(const uint32_t* plane, int W, int H, const int32_t* rects, unsigned long long* out) {
  const int32_t* r = rects + (size_t)blockIdx.x * 4;
  const int x0 = max(r[0], 0), y0 = max(r[1], 0), x1 = min(r[2], W), y1 = min(r[3], H);
  const unsigned long long t = obs_block_rect_sum(plane, W, x0, y0, x1, y1);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

__device__ __forceinline__ void obs_csr_sum2(const int32_t* off, const int32_t* cells, int g, int lane, const uint32_t* a,
                                             const uint32_t* b, unsigned long long& sa, unsigned long long& sb) {
  sa = 0; sb = 0;
  for (int k = off[g] + lane; k < off[g + 1]; k += 64) { const int c = cells[k]; sa += a[c]; sb += b[c]; }
  sa = obs_wave_sum(sa); sb = obs_wave_sum(sb);
}

// one wavefront per light group over the CSR tables the move phase uses (g_nsin, g_ewin, g_icell)
__global__ void k_obs_groups(Dev d, long long* rows) {
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= d.G) return;   // (whole waves leave: the shuffles below stay inside one wave)
  unsigned long long v[TS_OG_NFIELDS];
  obs_csr_sum2(d.g_nsin_off, d.g_nsin, g, lane, d.obs[TS_OBS_WAITING], d.obs[TS_OBS_PRESENT], v[TS_OG_NS_WAITING], v[TS_OG_NS_PRESENT]);
  obs_csr_sum2(d.g_ewin_off, d.g_ewin, g, lane, d.obs[TS_OBS_WAITING], d.obs[TS_OBS_PRESENT], v[TS_OG_EW_WAITING], v[TS_OG_EW_PRESENT]);
  obs_csr_sum2(d.g_icell_off, d.g_icell, g, lane, d.obs[TS_OBS_ENTER_N], d.obs[TS_OBS_ENTER_E], v[TS_OG_ENTER_N], v[TS_OG_ENTER_E]);
  obs_csr_sum2(d.g_icell_off, d.g_icell, g, lane, d.obs[TS_OBS_ENTER_S], d.obs[TS_OBS_ENTER_W], v[TS_OG_ENTER_S], v[TS_OG_ENTER_W]);
  if (lane == 0)
    for (int k = 0; k < TS_OG_NFIELDS; k++) rows[(size_t)g * TS_OG_NFIELDS + k] = (long long)v[k];
}

}  // namespace
