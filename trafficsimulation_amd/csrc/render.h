// render.h - the device renderer (include/trafficsim_render.h): a pre-pass that gathers what changes per cell into one byte
// plane, and the frame kernels that turn the byte planes into RGBA8 pixels.  The kernels take an argument struct of their
// own (RenderArgs), not Dev.  Part of the single translation unit engine.hip (included from there, behind kernels.h).
#pragma once
#include "../../include/trafficsim_render.h"

namespace {

// the dynamic byte of a cell: the top vehicle's palette code + 1 in the low bits (0: no vehicle), route and pending bits
constexpr uint8_t RN_VEH_MASK = 0x1F, RN_ROUTE = 0x40, RN_PEND = 0x80;
constexpr int RN_ROWS = 8;   // output rows per block of the frame kernel: the palettes are staged in LDS once per block

struct RenderArgs {
  // the map and the engine's state (read only)
  int W, H, N, G;
  const int8_t *stop, *rain;
  const uint8_t* type;              // nullptr: ts_render_set_cells has not been called, every cell is background
  const int32_t *pos, *next_in_cell, *path_len, *path_cur, *gs_pend, *g_icell_off, *g_icell;
  const uint16_t* flags;
  const uint32_t *path_off, *pool;
  const uint32_t* heat[4];          // the planes whose sum is the heat value (n_heat of them)
  int n_heat;
  // the renderer's tables
  uint8_t* dyn;                     // [N], rewritten by the pre-pass of every frame that needs it
  const uint32_t *cell_pal, *veh_pal, *lut;   // packed RGBA (R in the low byte)
  int n_pal;                        // n_types * 8
  const int32_t* routes;
  int n_routes;
  int n_vehicles;                   // vehicle ids handed out
  // the view
  int x0, y0, cells_w, cells_h, zoom, shrink, flip_y, flash, team;
  uint32_t layers, heat_max, bg, route_rgba;
  unsigned long long r2;            // (2 * R * zoom)^2
  int out_w, out_h;
  uint32_t* out;
};

// c = (c * (255 - A) + o * A + 127) / 255 per colour channel, A = o's alpha; the result's alpha is 255
__device__ __forceinline__ uint32_t rn_blend(uint32_t c, uint32_t o) {
  const uint32_t a = o >> 24;
  uint32_t r = 0xFF000000u;
  for (int k = 0; k < 24; k += 8) r |= ((((c >> k) & 255u) * (255u - a) + ((o >> k) & 255u) * a + 127u) / 255u) << k;
  return r;
}

// ---- pre-pass -------------------------------------------------------------------------------------------------------
// (the plane is zeroed first; the three kernels run one after the other on the engine's stream)

// one thread per light group with a pending phase: the pending bit on its intersection cells (plain byte stores)
__global__ void k_render_pend(RenderArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.G || a.gs_pend[g] < 0) return;
  for (int k = a.g_icell_off[g]; k < a.g_icell_off[g + 1]; k++) {
    const int c = a.g_icell[k];
    if ((unsigned)c < (unsigned)a.N) a.dyn[c] = RN_PEND;
  }
}

// one thread per vehicle id: a live vehicle that is the tail of its cell's list is the one a CanvasGrid draws last.  A
// cell has one tail, so one thread writes a given byte.
__global__ void k_render_vehicles(RenderArgs a) {
  const int vid = blockIdx.x * blockDim.x + threadIdx.x;
  if (vid >= a.n_vehicles) return;
  const uint16_t f = a.flags[vid];
  if (!(f & VF_ALIVE) || a.next_in_cell[vid] >= 0) return;
  const int c = a.pos[vid];
  if ((unsigned)c >= (unsigned)a.N) return;
  const int kind = (f & VF_SVC) ? 2 : (f & (VF_OVER | VF_DETOUR)) ? 1 : 0;
  const int status = (f & VF_COLL) ? 1 : (f & VF_MALF) ? 2 : (f & VF_PARKED) ? 3 : 0;
  a.dyn[c] = (uint8_t)(a.dyn[c] | (1 + kind * 4 + status));
}

// one wavefront per listed vehicle: 64 packed 2-bit directions per step become cells by a wave prefix sum of (dx, dy).
// Several waves may set the route bit of one byte; all of them write the same value over bits nobody changes here.
__global__ void k_render_routes(RenderArgs a) {
  const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= a.n_routes) return;   // (whole waves leave: the shuffles below stay inside one wave)
  const int vid = a.routes[r];
  if ((unsigned)vid >= (unsigned)a.n_vehicles || !(a.flags[vid] & VF_ALIVE)) return;
  const int pcur = a.path_cur[vid], plen = a.path_len[vid] - pcur, p0 = a.pos[vid];
  if ((unsigned)p0 >= (unsigned)a.N) return;
  const uint32_t off = a.path_off[vid];
  int x = p0 % a.W, y = p0 / a.W;
  for (int base = 0; base < plen; base += 64) {
    const int k = base + lane;
    int dx = 0, dy = 0;
    if (k < plen) {
      const int dir = path_dir(a.pool, off, pcur + k);
      dx = dir_dx(dir); dy = dir_dy(dir);
    }
    for (int o = 1; o < 64; o <<= 1) {   // inclusive prefix sums
      const int ux = __shfl_up(dx, o), uy = __shfl_up(dy, o);
      if (lane >= o) { dx += ux; dy += uy; }
    }
    const int cx = x + dx, cy = y + dy;
    if (k < plen && (unsigned)cx < (unsigned)a.W && (unsigned)cy < (unsigned)a.H) {
      uint8_t* p = a.dyn + (size_t)cy * a.W + cx;
      *p = (uint8_t)(*p | RN_ROUTE);
    }
    x += __shfl(dx, 63); y += __shfl(dy, 63);
  }
}

// ---- frames ---------------------------------------------------------------------------------------------------------

struct RenderLds {
  uint32_t cell[TS_RENDER_MAX_TYPES * 8], lut[256], veh[24];
};

__device__ __forceinline__ void rn_stage(const RenderArgs& a, RenderLds& s) {
  for (int k = threadIdx.x; k < a.n_pal; k += blockDim.x) s.cell[k] = a.cell_pal[k];
  if (a.layers & TS_RL_HEAT) for (int k = threadIdx.x; k < 256; k += blockDim.x) s.lut[k] = a.lut[k];
  if ((a.layers & TS_RL_VEHICLES) && threadIdx.x < 24) s.veh[threadIdx.x] = a.veh_pal[threadIdx.x];
  __syncthreads();
}

// steps 1 to 3 of the pixel rule from the bytes of one cell inside the map; `veh` = the vehicle's colour, 0 = none (a
// palette colour is never 0: its alpha is forced to 255 on upload)
__device__ __forceinline__ uint32_t rn_cell_color(const RenderArgs& a, const RenderLds& s, size_t c, int t, int stopb, int rainb,
                                                  int dynb, uint32_t& veh) {
  const int sig = (a.layers & TS_RL_SIGNALS) != 0;
  const int pend = sig & ((dynb & RN_PEND) != 0), stop = sig & (stopb == 1), rain = ((a.layers & TS_RL_RAIN) != 0) & (rainb > 0);
  uint32_t col = s.cell[((t * 2 + pend) * 2 + stop) * 2 + rain];
  if (a.layers & TS_RL_HEAT) {
    unsigned long long v = 0;
    for (int p = 0; p < a.n_heat; p++) v += a.heat[p][c];
    const unsigned long long i = v * 255ull / a.heat_max;
    col = rn_blend(col, s.lut[i > 255 ? 255 : (int)i]);
  }
  if ((a.layers & TS_RL_ROUTES) && (dynb & RN_ROUTE)) col = rn_blend(col, a.route_rgba);
  const int code = dynb & RN_VEH_MASK;
  veh = ((a.layers & TS_RL_VEHICLES) && code) ? s.veh[(code - 1) * 2 + a.flash] : 0u;
  return col;
}

__device__ __forceinline__ uint32_t rn_cell_at(const RenderArgs& a, const RenderLds& s, int x, int y, uint32_t& veh) {
  veh = 0;
  if (!a.type || (unsigned)x >= (unsigned)a.W || (unsigned)y >= (unsigned)a.H) return a.bg;
  const size_t c = (size_t)y * a.W + x;
  const int dynb = (a.layers & (TS_RL_SIGNALS | TS_RL_ROUTES | TS_RL_VEHICLES)) ? a.dyn[c] : 0;
  return rn_cell_color(a, s, c, a.type[c], a.stop[c], a.rain[c], dynb, veh);
}

// four bytes of a plane at cells c .. c + 3 (all inside one map row): one dword load where the address allows it
__device__ __forceinline__ uint32_t rn_load4(const void* plane, size_t c) {
  const uint8_t* p = (const uint8_t*)plane + c;
  if (((uintptr_t)p & 3) == 0) return *(const uint32_t*)p;
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__device__ __forceinline__ void rn_store4(const RenderArgs& a, int row, int px, const uint32_t* v) {
  uint32_t* o = a.out + (size_t)row * a.out_w + px;
  if (px + 4 <= a.out_w && (a.out_w & 3) == 0) *(uint4*)o = make_uint4(v[0], v[1], v[2], v[3]);   // (16 bytes per lane)
  else for (int k = 0; k < 4 && px + k < a.out_w; k++) o[k] = v[k];
}

// zoom >= 1 (and shrink 1): every lane makes four neighbouring pixels of one output row, RN_ROWS rows per block
__global__ void __launch_bounds__(BLK) k_render_frame(RenderArgs a) {
  __shared__ RenderLds s;
  rn_stage(a, s);
  const int px = (blockIdx.x * BLK + threadIdx.x) * 4;
  if (px >= a.out_w) return;
  const int z = a.zoom;
  for (int rr = 0; rr < RN_ROWS; rr++) {
    const int row = blockIdx.y * RN_ROWS + rr;
    if (row >= a.out_h) break;
    const int vy = a.flip_y ? a.out_h - 1 - row : row;
    const int y = a.y0 + vy / z, j = vy % z;
    uint32_t v[4];
    if (z == 1) {
      const int x = a.x0 + px;
      if (a.type && (unsigned)y < (unsigned)a.H && x >= 0 && x + 3 < a.W) {   // four cells inside the map: dword loads
        const size_t c = (size_t)y * a.W + x;
        const bool dyn = (a.layers & (TS_RL_SIGNALS | TS_RL_ROUTES | TS_RL_VEHICLES)) != 0;
        const uint32_t t4 = rn_load4(a.type, c), s4 = rn_load4(a.stop, c), r4 = rn_load4(a.rain, c), d4 = dyn ? rn_load4(a.dyn, c) : 0u;
        for (int k = 0; k < 4; k++) {
          uint32_t veh;
          const uint32_t col = rn_cell_color(a, s, c + k, (t4 >> (8 * k)) & 255, (int8_t)(s4 >> (8 * k)), (int8_t)(r4 >> (8 * k)),
                                             (d4 >> (8 * k)) & 255, veh);
          v[k] = veh ? veh : col;
        }
      } else {
        for (int k = 0; k < 4; k++) {
          uint32_t veh;
          const uint32_t col = rn_cell_at(a, s, x + k, y, veh);
          v[k] = veh ? veh : col;
        }
      }
    } else {
      int cx = px / z, i = px - cx * z;
      uint32_t veh, col = rn_cell_at(a, s, a.x0 + cx, y, veh);
      const long long dj = 2 * j + 1 - z;
      for (int k = 0; k < 4; k++) {
        const long long di = 2 * i + 1 - z;
        v[k] = (veh && (unsigned long long)(di * di + dj * dj) * 65536ull <= a.r2) ? veh : col;
        if (++i == z && k < 3) { i = 0; cx++; col = rn_cell_at(a, s, a.x0 + cx, y, veh); }
      }
    }
    rn_store4(a, row, px, v);
  }
}

// shrink s > 1: a team of a.team lanes (a power of two <= 64) per output pixel strides over the s x s cells of its box and
// adds the channels up with shuffles; integer sums, so the order does not matter
__global__ void __launch_bounds__(BLK) k_render_shrink(RenderArgs a) {
  __shared__ RenderLds s;
  rn_stage(a, s);
  const int T = a.team, sh = a.shrink;
  const long long pix = ((long long)blockIdx.x * BLK + threadIdx.x) / T;
  const int tl = threadIdx.x & (T - 1);
  const bool live = pix < (long long)a.out_w * a.out_h;   // (teams never straddle a wave: dead lanes still shuffle)
  const int row = live ? (int)(pix / a.out_w) : 0, col = live ? (int)(pix - (long long)row * a.out_w) : 0;
  const int by = a.flip_y ? a.out_h - 1 - row : row;
  uint32_t sum[3] = {0, 0, 0};
  if (live)
    for (int q = tl; q < sh * sh; q += T) {
      const int qy = q / sh, qx = q - qy * sh;
      const int vx = col * sh + qx, vy = by * sh + qy;   // cell of the view
      uint32_t veh, c = a.bg;
      if (vx < a.cells_w && vy < a.cells_h) { c = rn_cell_at(a, s, a.x0 + vx, a.y0 + vy, veh); if (veh) c = veh; }
      sum[0] += c & 255u; sum[1] += (c >> 8) & 255u; sum[2] += (c >> 16) & 255u;
    }
  for (int o = T >> 1; o; o >>= 1)
    for (int k = 0; k < 3; k++) sum[k] += __shfl_xor(sum[k], o);
  if (live && tl == 0) {
    const uint32_t n = (uint32_t)(sh * sh), h = n / 2;
    a.out[pix] = 0xFF000000u | ((sum[0] + h) / n) | ((sum[1] + h) / n) << 8 | ((sum[2] + h) / n) << 16;
  }
}

}  // namespace
