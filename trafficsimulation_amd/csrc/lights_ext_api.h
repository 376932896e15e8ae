// lights_ext_api.h - the ts_lights_ext_* entries (include/trafficsim_lights_ext.h): the host side of the external light
// control whose kernels are in lights_ext.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_lights_ext.h"

static_assert(sizeof(TsLightsExtInfo) == 32 && sizeof(TsLightsExtDevice) == 40, "lights_ext structs as the Python binding declares them");

namespace {

bool le_dim_ok(int d) { return d == 7 || d == 11 || d == 13 || d == 17 || d == 19; }

// the checks every entry starts with
int le_enter(E* e) {
  if (e->P.light_algorithm != TS_LIGHTS_EXTERNAL) return fail(e, TS_E_UNSUPPORTED, "lights_ext: the handle's light algorithm is not TS_LIGHTS_EXTERNAL");
  if (!e->le.ready) return fail(e, TS_E_STATE, "lights_ext: ts_set_lights has not run");
  return TS_OK;
}

// ... of the three entries of the simple protocol: not once another protocol is configured (lights_proto_api.h)
int le_enter_simple(E* e) {
  TRY(le_enter(e));
  if (e->lp.protocol) return fail(e, TS_E_STATE, "lights_ext: the handle is configured for another protocol (ts_lights_proto_config)");
  return TS_OK;
}

int le_grid(const E* e, int per_block_items) { return std::max(1, (e->le.x.G + per_block_items - 1) / per_block_items); }

int le_sums(E* e) {
  const LightsExt& x = e->le.x;
  const int team = e->le.team, nb = le_grid(e, BLK / team);
  switch (team) {
    case 4: hipLaunchKernelGGL(k_le_sums<4>, dim3(nb), dim3(BLK), 0, e->stream, x); break;
    case 16: hipLaunchKernelGGL(k_le_sums<16>, dim3(nb), dim3(BLK), 0, e->stream, x); break;
    case 32: hipLaunchKernelGGL(k_le_sums<32>, dim3(nb), dim3(BLK), 0, e->stream, x); break;
    default: hipLaunchKernelGGL(k_le_sums<8>, dim3(nb), dim3(BLK), 0, e->stream, x); break;
  }
  HIPOK(hipGetLastError());
  return TS_OK;
}

// phase A on the maps as they stand: sums, state vectors, commit of the stored pressures
int le_phase_a(E* e) {
  const LightsExt& x = e->le.x;
  TRY(le_sums(e));
  hipLaunchKernelGGL(k_le_state, dim3(le_grid(e, e->le.gblock)), dim3(e->le.gblock), 0, e->stream, x, e->le.calls == 0 ? 1 : 0);
  hipLaunchKernelGGL(k_le_commit, dim3(le_grid(e, e->le.gblock)), dim3(e->le.gblock), 0, e->stream, x);
  HIPOK(hipGetLastError());
  e->le.calls++;
  e->le.observed = true;
  return TS_OK;
}

// the G bytes of an action / phase vector, range-checked, as a device pointer (host vectors go through the staging)
int le_bytes(E* e, const int8_t* v, int on_device, int lo, const char* what, const int8_t** dev) {
  const int G = e->le.x.G;
  if (!on_device) {
    for (int g = 0; g < G; g++) if (v[g] < lo || v[g] > 1) return fail(e, TS_E_INVALID, std::string("lights_ext: ") + what + " out of range");
    if (G) HIPOK(hipMemcpyAsync(e->le.stage, v, (size_t)G, hipMemcpyHostToDevice, e->stream));
    HIPOK(hipStreamSynchronize(e->stream));   // (the caller's buffer is free again when the entry returns)
    *dev = e->le.stage;
    return TS_OK;
  }
  int bad = 0;
  HIPOK(hipMemsetAsync(e->le.x.bad, 0, sizeof(int), e->stream));
  hipLaunchKernelGGL(k_le_check, dim3(le_grid(e, e->le.gblock)), dim3(e->le.gblock), 0, e->stream, v, G, lo, e->le.x.bad);
  HIPOK(hipGetLastError());
  TRY(read_back(e, &bad, e->le.x.bad, sizeof(int)));
  if (bad) return fail(e, TS_E_INVALID, std::string("lights_ext: ") + what + " out of range");
  *dev = v;
  return TS_OK;
}

int le_rows_out(E* e, const float* src, float* dst) {
  const LightsExt& x = e->le.x;
  if (dst && x.G) HIPOK(hipMemcpyAsync(dst, src, (size_t)x.G * x.dim * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

}  // namespace

// ts_set_lights under TS_LIGHTS_EXTERNAL: the extension's arrays (sized for the largest dimension, so that
// ts_lights_ext_config never allocates), controller state zero (intersection_light_group.py:91-92), static features
static int le_init(ts_handle e) {
  Dev& d = e->d;
  LightsExt& x = e->le.x;
  const size_t G = (size_t)d.G;
  x = LightsExt{};
  x.G = d.G; x.dim = TS_LIGHTS_EXT_DEFAULT_DIM; x.min_green = TS_LIGHTS_EXT_DEFAULT_MIN_GREEN;
  x.cell = d.cell;
  x.nsin_off = d.g_nsin_off; x.nsin = d.g_nsin; x.ewin_off = d.g_ewin_off; x.ewin = d.g_ewin;
  x.nsout_off = d.g_nsout_off; x.nsout = d.g_nsout; x.ewout_off = d.g_ewout_off; x.ewout = d.g_ewout;
  x.nb = d.g_nb; x.nb_ctor = d.g_nb_ctor; x.repop = d.gs_repop;
  x.gs_cur = d.gs_cur; x.gs_pend = d.gs_pend;
  HIPOK(dalloc(e, &x.sums, G * 4)); HIPOK(dalloc(e, &x.stored, G * 2)); HIPOK(dalloc(e, &x.ctrl, G * 2));
  HIPOK(dalloc(e, &x.size, G)); HIPOK(dalloc(e, &x.pen, G));
  HIPOK(dalloc(e, &x.state, G * TS_LIGHTS_EXT_MAX_DIM)); HIPOK(dalloc(e, &x.next, G * TS_LIGHTS_EXT_MAX_DIM));
  HIPOK(dalloc(e, &x.bad, 1)); HIPOK(dalloc(e, &e->le.stage, G));
  if (G) {
    HIPOK(hipMemsetAsync(x.sums, 0, G * 16, e->stream));
    HIPOK(hipMemsetAsync(x.stored, 0, G * 8, e->stream));
    HIPOK(hipMemsetAsync(x.ctrl, 0, G * 8, e->stream));
    HIPOK(hipMemsetAsync(x.state, 0, G * TS_LIGHTS_EXT_MAX_DIM * 4, e->stream));
    HIPOK(hipMemsetAsync(x.next, 0, G * TS_LIGHTS_EXT_MAX_DIM * 4, e->stream));
  }
  e->le.bytes = G * (16 + 8 + 8 + 8 + 8 + 2 * TS_LIGHTS_EXT_MAX_DIM * 4 + 1) + 4;
  const char* dbg = getenv("TS_DEBUG_LIGHTS_TEAM");   // lanes per group of the sums pass (tests and the probe: 4, 8, 16, 32)
  const int team = dbg ? atoi(dbg) : 8;
  e->le.team = (team == 4 || team == 16 || team == 32) ? team : 8;
  const char* dbb = getenv("TS_DEBUG_LIGHTS_BLOCK");   // threads per block of the one-thread-per-group kernels (tests: several blocks at small G)
  const int gb = dbb ? atoi(dbb) : BLK;
  e->le.gblock = (gb == 8 || gb == 16 || gb == 32 || gb == 64 || gb == 128) ? gb : BLK;
  hipLaunchKernelGGL(k_le_static, dim3(std::max(1, nblk(d.G))), dim3(BLK), 0, e->stream, x, e->P.road_type_penalty_r1,
                     e->P.road_type_penalty_r2, e->P.road_type_penalty_r3);
  HIPOK(hipGetLastError());
  HIPOK(hipStreamSynchronize(e->stream));
  e->le.calls = 0; e->le.observed = false;
  // (a protocol is configured per set of light tables: none now, and none of the previous one's arrays)
  e->lp.p = LightsProto{}; e->lp.protocol = 0; e->lp.calls = 0; e->lp.bytes = 0;
  e->lp.d_eps = nullptr; e->lp.q_stage = nullptr; e->lp.eps.clear();
  e->le.ready = true;
  return TS_OK;
}

extern "C" {

int ts_lights_ext_config(ts_handle e, int32_t state_dim, int32_t min_green) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter_simple(e));
  if (!le_dim_ok(state_dim) || min_green < 0) return fail(e, TS_E_INVALID, "lights_ext: state_dim must be 7, 11, 13, 17 or 19 and min_green >= 0");
  if (e->le.calls > 0) return fail(e, TS_E_STATE, "lights_ext: configure before the first control call");
  e->le.x.dim = state_dim; e->le.x.min_green = min_green;
  return TS_OK;
}

int ts_lights_ext_set_static(ts_handle e, const double* intersection_size, const double* penalty_score) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter(e));
  if (e->le.calls > 0 || e->lp.calls > 0) return fail(e, TS_E_STATE, "lights_ext: set the static features before the first control call");
  const size_t n = (size_t)e->le.x.G * sizeof(double);
  if (intersection_size && n) HIPOK(hipMemcpyAsync(e->le.x.size, intersection_size, n, hipMemcpyHostToDevice, e->stream));
  if (penalty_score && n) HIPOK(hipMemcpyAsync(e->le.x.pen, penalty_score, n, hipMemcpyHostToDevice, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_lights_ext_observe(ts_handle e, float* out) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter_simple(e));
  if (!e->le.observed) TRY(le_phase_a(e));
  return le_rows_out(e, e->le.x.state, out);
}

int ts_lights_ext_act(ts_handle e, const int8_t* actions, int32_t on_device, float* next_state) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter_simple(e));
  if (!actions) return fail(e, TS_E_INVALID, "lights_ext: null pointer");
  const int8_t* dev = nullptr;
  TRY(le_bytes(e, actions, on_device, 0, "an action", &dev));
  if (!e->le.observed) TRY(le_phase_a(e));
  else TRY(le_sums(e));   // (the maps have not moved since phase A; the sums are scratch and not kept across a checkpoint)
  hipLaunchKernelGGL(k_le_act, dim3(le_grid(e, e->le.gblock)), dim3(e->le.gblock), 0, e->stream, e->le.x, dev);
  HIPOK(hipGetLastError());
  e->le.observed = false;
  return le_rows_out(e, e->le.x.next, next_state);
}

int ts_lights_ext_request(ts_handle e, const int8_t* phases, int32_t on_device) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter(e));
  if (!phases) return fail(e, TS_E_INVALID, "lights_ext: null pointer");
  const int8_t* dev = nullptr;
  TRY(le_bytes(e, phases, on_device, -1, "a requested phase", &dev));
  hipLaunchKernelGGL(k_le_request, dim3(le_grid(e, e->le.gblock)), dim3(e->le.gblock), 0, e->stream, e->le.x, dev);
  HIPOK(hipGetLastError());
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_lights_ext_download(ts_handle e, int32_t* rows) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter(e));
  if (!rows) return fail(e, TS_E_INVALID, "lights_ext: null pointer");
  if (e->le.x.G) HIPOK(hipMemcpyAsync(rows, e->le.x.ctrl, (size_t)e->le.x.G * 8, hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_lights_ext_device(ts_handle e, TsLightsExtDevice* out) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter(e));
  if (!out) return fail(e, TS_E_INVALID, "lights_ext: null pointer");
  HIPOK(hipStreamSynchronize(e->stream));
  const LightsExt& x = e->le.x;
  out->state = x.state; out->next_state = x.next; out->controller = x.ctrl; out->stored = x.stored;
  out->n_groups = x.G; out->state_dim = x.dim;
  return TS_OK;
}

int ts_lights_ext_info(ts_handle e, TsLightsExtInfo* out) {
  if (!e) return TS_E_INVALID;
  TRY(le_enter(e));
  if (!out) return fail(e, TS_E_INVALID, "lights_ext: null pointer");
  const LightsExt& x = e->le.x;
  out->state_dim = x.dim; out->min_green = x.min_green; out->n_groups = x.G;
  out->observed = e->le.observed ? 1 : 0;
  out->calls = e->le.calls;
  out->device_bytes = e->le.bytes;
  return TS_OK;
}

}  // extern "C"
