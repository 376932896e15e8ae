// observe_api.h - the ts_observe_* entries (include/trafficsim_observe.h): the host side of the observation planes whose
// kernels are in observe.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_observe.h"

namespace {

void obs_free(E* e) {
  for (int p = 0; p < TS_OBS_NPLANES; p++) { dfree(e, e->d.obs[p]); e->d.obs[p] = nullptr; }
  e->d.obs_enter = nullptr;
  e->obs_mask = 0;
  e->obs_ticks = 0;
}

int obs_zero(E* e) {
  for (int p = 0; p < TS_OBS_NPLANES; p++)
    if (e->d.obs[p]) HIPOK(hipMemsetAsync(e->d.obs[p], 0, (size_t)e->N * sizeof(uint32_t), e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  e->obs_ticks = 0;
  return TS_OK;
}

// the plane behind a plane index, or an error code (with ts_last_error set)
int obs_plane(E* e, int32_t plane, const uint32_t** out) {
  if (plane < 0 || plane >= TS_OBS_NPLANES) return fail(e, TS_E_INVALID, "observe: plane index out of range");
  if (!e->obs_mask) return fail(e, TS_E_STATE, "observe: observation has not been started");
  if (!(e->obs_mask & (1u << plane))) return fail(e, TS_E_STATE, "observe: plane " + std::to_string(plane) + " is not in the mask");
  *out = e->d.obs[plane];
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_observe_start(ts_handle e, uint32_t plane_mask) {
  if (!e) return TS_E_INVALID;
  if (plane_mask == 0 || (plane_mask & ~TS_OBS_ALL)) return fail(e, TS_E_INVALID, "observe: the plane mask is empty or names a plane that does not exist");
  HIPOK(hipStreamSynchronize(e->stream));
  obs_free(e);
  for (int p = 0; p < TS_OBS_NPLANES; p++) {
    if (!(plane_mask & (1u << p))) continue;
    if (dalloc(e, &e->d.obs[p], (size_t)e->N) != hipSuccess) {
      (void)hipGetLastError();
      e->d.obs[p] = nullptr;
      obs_free(e);
      return fail(e, TS_E_DEVICE, "observe: no device memory for the planes (observation is off)");
    }
  }
  e->obs_mask = plane_mask;
  if (int rc = obs_zero(e)) { obs_free(e); return rc; }
  for (int p = TS_OBS_ENTER_N; p <= TS_OBS_ENTER_W; p++) if (e->d.obs[p]) e->d.obs_enter = e->d.obs[p];
  return TS_OK;
}

int ts_observe_stop(ts_handle e) {
  if (!e) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  obs_free(e);
  return TS_OK;
}

int ts_observe_reset(ts_handle e) {
  if (!e) return TS_E_INVALID;
  if (!e->obs_mask) return fail(e, TS_E_STATE, "observe: observation has not been started");
  return obs_zero(e);
}

int ts_observe_info(ts_handle e, TsObserveInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->plane_mask = e->obs_mask;
  out->width = e->W; out->height = e->H;
  out->ticks = e->obs_ticks;
  out->device_bytes = (uint64_t)__builtin_popcount(e->obs_mask) * (uint64_t)e->N * sizeof(uint32_t);
  return TS_OK;
}

int ts_observe_download(ts_handle e, int32_t plane, uint32_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "observe: null pointer");
  const uint32_t* src = nullptr;
  TRY(obs_plane(e, plane, &src));
  return read_back(e, dst, src, (size_t)e->N * sizeof(uint32_t));
}

int ts_observe_pooled(ts_handle e, int32_t plane, int32_t factor, uint64_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst || factor < 1) return fail(e, TS_E_INVALID, "observe: null pointer or factor < 1");
  const uint32_t* src = nullptr;
  TRY(obs_plane(e, plane, &src));
  return pool_plane(e, "observe: ", factor, dst, [&](auto use) { return use(src); });
}

int ts_observe_regions(ts_handle e, int32_t plane, int32_t n, const int32_t* rects, uint64_t* sums) {
  if (!e) return TS_E_INVALID;
  if (n < 0 || (n > 0 && (!rects || !sums))) return fail(e, TS_E_INVALID, "observe: negative count or null pointer");
  const uint32_t* src = nullptr;
  TRY(obs_plane(e, plane, &src));
  if (n == 0) return TS_OK;
  Scratch tmp;
  int32_t* drects = nullptr;   // four per rectangle
  HIPOK(tmp.get(&drects, (size_t)n * 4));
  HIPOK(hipMemcpyAsync(drects, rects, (size_t)n * 16, hipMemcpyHostToDevice, e->stream));
  return launch_read<unsigned long long>(e, (size_t)n, sums, [&](unsigned long long* out) {
    hipLaunchKernelGGL(k_obs_regions, dim3(n), dim3(BLK), 0, e->stream, src, e->W, e->H, drects, out);
  });
}

int ts_observe_groups(ts_handle e, int64_t* rows) {
  if (!e) return TS_E_INVALID;
  if (!rows) return fail(e, TS_E_INVALID, "observe: null pointer");
  if (!e->obs_mask) return fail(e, TS_E_STATE, "observe: observation has not been started");
  const uint32_t need = (1u << TS_OBS_PRESENT) | (1u << TS_OBS_WAITING) | OBS_ENTER;
  if ((e->obs_mask & need) != need) return fail(e, TS_E_STATE, "observe: the group report needs PRESENT, WAITING and the four ENTER planes in the mask");
  const int G = e->d.G;
  if (G == 0) return TS_OK;
  const int per_block = BLK / 64;
  return launch_read<long long>(e, (size_t)G * TS_OG_NFIELDS, rows, [&](long long* out) {
    hipLaunchKernelGGL(k_obs_groups, dim3((G + per_block - 1) / per_block), dim3(BLK), 0, e->stream, e->d, out);
  });
}

int ts_observe_device(ts_handle e, int32_t plane, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "observe: null pointer");
  const uint32_t* src = nullptr;
  TRY(obs_plane(e, plane, &src));
  HIPOK(hipStreamSynchronize(e->stream));
  *ptr = (void*)src;
  return TS_OK;
}

}  // extern "C"
