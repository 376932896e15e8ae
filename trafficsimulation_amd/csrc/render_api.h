// render_api.h - the ts_render_* entries (include/trafficsim_render.h): the host side of the renderer whose kernels are in
// render.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_render.h"

namespace {

// frame size of a view, or TS_E_INVALID / TS_E_CAPACITY (no handle: ts_render_size is pure arithmetic)
int rn_size(const TsRenderView* v, int32_t* ow, int32_t* oh, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (v->cells_w < 1 || v->cells_h < 1) { *why = "render: cells_w and cells_h must be at least 1"; return TS_E_INVALID; }
  if (v->zoom < 1 || v->zoom > TS_RENDER_MAX_SCALE || v->shrink < 1 || v->shrink > TS_RENDER_MAX_SCALE || (v->zoom > 1 && v->shrink > 1)) {
    *why = "render: zoom and shrink are 1..64 and at most one of them is above 1"; return TS_E_INVALID;
  }
  if (v->x0 < -(1 << 24) || v->x0 > (1 << 24) || v->y0 < -(1 << 24) || v->y0 > (1 << 24)) { *why = "render: x0 / y0 beyond +-2^24"; return TS_E_INVALID; }
  if (v->layers & ~(uint32_t)TS_RL_ALL) { *why = "render: unknown layer bits"; return TS_E_INVALID; }
  if (v->vehicle_radius_256 < 0 || v->vehicle_radius_256 > 65535) { *why = "render: vehicle_radius_256 outside 0..65535"; return TS_E_INVALID; }
  if (v->layers & TS_RL_HEAT) {
    if (v->heat_plane < 0 || v->heat_plane > TS_OBS_NPLANES) { *why = "render: heat_plane out of range"; return TS_E_INVALID; }
    if (v->heat_max == 0) { *why = "render: heat_max must be above 0"; return TS_E_INVALID; }
  }
  const long long w = v->shrink > 1 ? ((long long)v->cells_w + v->shrink - 1) / v->shrink : (long long)v->cells_w * v->zoom;
  const long long h = v->shrink > 1 ? ((long long)v->cells_h + v->shrink - 1) / v->shrink : (long long)v->cells_h * v->zoom;
  if (w > TS_RENDER_MAX_SIDE || h > TS_RENDER_MAX_SIDE) { *why = "render: the frame is above 8192 x 8192 pixels"; return TS_E_CAPACITY; }
  *ow = (int32_t)w; *oh = (int32_t)h;
  return TS_OK;
}

template <typename T>
int rn_upload(E* e, T** dst, const void* src, size_t n) {
  T* p = nullptr;
  if (dalloc(e, &p, n) != hipSuccess) { (void)hipGetLastError(); return fail(e, TS_E_DEVICE, "render: no device memory for a table"); }
  const hipError_t r = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
  if (r != hipSuccess) { dfree(e, p); return fail(e, TS_E_DEVICE, std::string("render: upload: ") + hipGetErrorString(r)); }
  HIPOK(hipStreamSynchronize(e->stream));   // (a frame in flight may still read the old table)
  dfree(e, *dst);
  *dst = p;
  return TS_OK;
}

// packed RGBA words of n colours, alpha forced to 255 (a frame's alpha is 255 whatever the tables say)
std::vector<uint32_t> rn_opaque(const uint8_t* rgba, size_t n) {
  std::vector<uint32_t> w(n);
  for (size_t k = 0; k < n; k++) w[k] = 0xFF000000u | rgba[4 * k] | (uint32_t)rgba[4 * k + 1] << 8 | (uint32_t)rgba[4 * k + 2] << 16;
  return w;
}

// validate, size the frame, make sure of the buffers, run the pre-pass and the frame kernel; the frame lies in e->rn.out
int rn_frame(E* e, const TsRenderView* v) {
  auto& R = e->rn;
  const Dev& d = e->d;
  int32_t ow = 0, oh = 0;
  const char* why = "";
  if (int rc = rn_size(v, &ow, &oh, &why)) return fail(e, rc, why);
  if ((v->layers & TS_RL_VEHICLES) && !R.has_veh) return fail(e, TS_E_STATE, "render: TS_RL_VEHICLES without a vehicle palette");
  RenderArgs a{};
  if (v->layers & TS_RL_HEAT) {
    if (!R.has_lut) return fail(e, TS_E_STATE, "render: TS_RL_HEAT without a heat LUT");
    const uint32_t need = v->heat_plane == TS_OBS_NPLANES ? OBS_ENTER : 1u << v->heat_plane;
    if ((e->obs_mask & need) != need) return fail(e, TS_E_STATE, "render: TS_RL_HEAT needs its plane observed (flow: the four ENTER planes)");
    if (v->heat_plane == TS_OBS_NPLANES) { for (int p = 0; p < 4; p++) a.heat[p] = d.obs[TS_OBS_ENTER_N + p]; a.n_heat = 4; }
    else { a.heat[0] = d.obs[v->heat_plane]; a.n_heat = 1; }
  }
  const size_t pixels = (size_t)ow * oh;
  if (pixels > R.out_cap) {   // the old buffer goes only once the new one is there
    uint32_t* p = nullptr;
    if (dalloc(e, &p, pixels) != hipSuccess) { (void)hipGetLastError(); return fail(e, TS_E_DEVICE, "render: no device memory for the frame buffer"); }
    HIPOK(hipStreamSynchronize(e->stream));
    dfree(e, R.out);
    R.out = p; R.out_cap = pixels;
  }
  const bool need_dyn = R.type && (v->layers & (TS_RL_SIGNALS | TS_RL_ROUTES | TS_RL_VEHICLES));
  if (need_dyn && !R.dyn && dalloc(e, &R.dyn, (size_t)e->N) != hipSuccess) {
    (void)hipGetLastError();
    R.dyn = nullptr;
    return fail(e, TS_E_DEVICE, "render: no device memory for the dynamic plane");
  }
  a.W = e->W; a.H = e->H; a.N = e->N; a.G = d.G;
  a.stop = d.stop; a.rain = d.rain; a.type = R.type;
  a.pos = d.pos; a.next_in_cell = d.next_in_cell; a.path_len = d.path_len; a.path_cur = d.path_cur;
  a.gs_pend = d.gs_pend; a.g_icell_off = d.g_icell_off; a.g_icell = d.g_icell;
  a.flags = d.flags; a.path_off = d.path_off; a.pool = d.pool;
  a.dyn = R.dyn; a.cell_pal = R.cell_pal; a.veh_pal = R.veh_pal; a.lut = R.lut; a.n_pal = R.n_types * 8;
  a.routes = R.routes; a.n_routes = R.n_routes; a.n_vehicles = e->n_vehicles_total;
  a.x0 = v->x0; a.y0 = v->y0; a.cells_w = v->cells_w; a.cells_h = v->cells_h; a.zoom = v->zoom; a.shrink = v->shrink;
  a.flip_y = v->flip_y != 0; a.flash = (e->C.step_count % 2) == 0;
  a.layers = v->layers; a.heat_max = v->heat_max;
  a.bg = rn_opaque(v->background, 1)[0]; a.route_rgba = R.route_rgba;
  const unsigned long long rz = 2ull * (unsigned)v->vehicle_radius_256 * (unsigned)v->zoom;
  a.r2 = rz * rz;
  a.out_w = ow; a.out_h = oh; a.out = R.out;
  a.team = 64;
  while (a.team > 1 && (a.team >> 1) >= v->shrink * v->shrink) a.team >>= 1;   // the smallest power of two >= s^2, at most 64
  hipStream_t st = e->stream;
  if (need_dyn) {
    HIPOK(hipMemsetAsync(R.dyn, 0, (size_t)e->N, st));
    if ((v->layers & TS_RL_SIGNALS) && d.G > 0 && d.gs_pend && d.g_icell_off)
      hipLaunchKernelGGL(k_render_pend, dim3(nblk(d.G)), dim3(BLK), 0, st, a);
    if ((v->layers & TS_RL_VEHICLES) && a.n_vehicles > 0)
      hipLaunchKernelGGL(k_render_vehicles, dim3(nblk(a.n_vehicles)), dim3(BLK), 0, st, a);
    if ((v->layers & TS_RL_ROUTES) && R.n_routes > 0 && a.n_vehicles > 0)
      hipLaunchKernelGGL(k_render_routes, dim3((R.n_routes + BLK / 64 - 1) / (BLK / 64)), dim3(BLK), 0, st, a);
  }
  if (v->shrink > 1) {
    const long long threads = (long long)pixels * a.team;
    hipLaunchKernelGGL(k_render_shrink, dim3((unsigned)((threads + BLK - 1) / BLK)), dim3(BLK), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_render_frame, dim3((ow + BLK * 4 - 1) / (BLK * 4), (oh + RN_ROWS - 1) / RN_ROWS), dim3(BLK), 0, st, a);
  }
  HIPOK(hipGetLastError());
  R.last_w = ow; R.last_h = oh;
  R.frames++;
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_render_set_cells(ts_handle e, const uint8_t* type_plane, int32_t n_types, const uint8_t* cell_palette) {
  if (!e) return TS_E_INVALID;
  if (!type_plane || !cell_palette) return fail(e, TS_E_INVALID, "render: null pointer");
  if (n_types < 1 || n_types > TS_RENDER_MAX_TYPES) return fail(e, TS_E_INVALID, "render: n_types outside 1..64");
  for (size_t c = 0; c < (size_t)e->N; c++)
    if (type_plane[c] >= n_types) return fail(e, TS_E_INVALID, "render: a type code is not below n_types");
  const std::vector<uint32_t> pal = rn_opaque(cell_palette, (size_t)n_types * 8);
  uint32_t* dpal = nullptr;
  TRY(rn_upload(e, &dpal, pal.data(), pal.size()));
  if (int rc = rn_upload(e, &e->rn.type, type_plane, (size_t)e->N)) { dfree(e, dpal); return rc; }
  dfree(e, e->rn.cell_pal);
  e->rn.cell_pal = dpal;
  e->rn.n_types = n_types;
  return TS_OK;
}

int ts_render_set_vehicle_palette(ts_handle e, const uint8_t* pal) {
  if (!e) return TS_E_INVALID;
  if (!pal) return fail(e, TS_E_INVALID, "render: null pointer");
  const std::vector<uint32_t> w = rn_opaque(pal, 24);
  TRY(rn_upload(e, &e->rn.veh_pal, w.data(), w.size()));
  e->rn.has_veh = true;
  return TS_OK;
}

int ts_render_set_heat_lut(ts_handle e, const uint8_t* lut) {
  if (!e) return TS_E_INVALID;
  if (!lut) return fail(e, TS_E_INVALID, "render: null pointer");
  TRY(rn_upload(e, &e->rn.lut, lut, 256));   // (the alpha byte stays: it is the blend weight)
  e->rn.has_lut = true;
  return TS_OK;
}

int ts_render_set_routes(ts_handle e, int32_t n, const int32_t* spawn_idx, const uint8_t rgba[4]) {
  if (!e) return TS_E_INVALID;
  if (n < 0 || n > TS_RENDER_MAX_ROUTES) return fail(e, TS_E_INVALID, "render: route count outside 0..4096");
  if (n > 0 && (!spawn_idx || !rgba)) return fail(e, TS_E_INVALID, "render: null pointer");
  for (int k = 0; k < n; k++)
    if (spawn_idx[k] < 0 || spawn_idx[k] >= e->n_vehicles_total) return fail(e, TS_E_INVALID, "render: a route id is not a spawn index handed out so far");
  if (n > 0) {
    TRY(rn_upload(e, &e->rn.routes, spawn_idx, (size_t)n));
    e->rn.route_rgba = (uint32_t)rgba[0] | (uint32_t)rgba[1] << 8 | (uint32_t)rgba[2] << 16 | (uint32_t)rgba[3] << 24;
  }
  e->rn.n_routes = n;
  return TS_OK;
}

int ts_render_size(const TsRenderView* v, int32_t* out_w, int32_t* out_h) {
  if (!v || !out_w || !out_h) return TS_E_INVALID;
  return rn_size(v, out_w, out_h, nullptr);
}

int ts_render_device(ts_handle e, const TsRenderView* v, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!v || !ptr) return fail(e, TS_E_INVALID, "render: null pointer");
  TRY(rn_frame(e, v));
  HIPOK(hipStreamSynchronize(e->stream));
  *ptr = (void*)e->rn.out;
  return TS_OK;
}

int ts_render(ts_handle e, const TsRenderView* v, uint8_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!v || !dst) return fail(e, TS_E_INVALID, "render: null pointer");
  TRY(rn_frame(e, v));
  return read_back(e, dst, e->rn.out, (size_t)e->rn.last_w * e->rn.last_h * 4);
}

int ts_render_info(ts_handle e, TsRenderInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  const auto& R = e->rn;
  memset(out, 0, sizeof(*out));
  out->n_types = R.n_types;
  out->has_vehicle_palette = R.has_veh; out->has_heat_lut = R.has_lut; out->n_routes = R.n_routes;
  out->last_w = R.last_w; out->last_h = R.last_h;
  out->frames = R.frames;
  out->device_bytes = (uint64_t)R.out_cap * 4 + (R.type ? (uint64_t)e->N + (uint64_t)R.n_types * 32 : 0) + (R.dyn ? (uint64_t)e->N : 0) +
                      (R.veh_pal ? 96 : 0) + (R.lut ? 1024 : 0) + (R.routes ? (uint64_t)R.n_routes * 4 : 0);
  return TS_OK;
}

}  // extern "C"
