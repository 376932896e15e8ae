// jams_api.h - the ts_jams_* entries (include/trafficsim_jams.h): the host side of the jam detection whose kernels are in jams.h.
// Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_jams.h"

namespace {

// the default tile side: none.  profiles/jams_probe.py compares 0, 8, 16 and 32 at 4096^2 with 945 072 standing vehicles in 50 318
// jams: 6.56 ms (6.52 .. 6.61) without the tile stage against 6.71 ms (6.67 .. 6.79) at 32 - queues of a few dozen cells leave the
// merge little to do, and the tile stage costs a launch over every tile
constexpr int JAM_TILE = 0;

void jam_launch_tile(int T, int blocks, hipStream_t st, const JamArgs& a) {
  switch (T) {
    case 8: hipLaunchKernelGGL(k_jam_tile<8>, dim3(blocks), dim3(64), 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_jam_tile<16>, dim3(blocks), dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL(k_jam_tile<32>, dim3(blocks), dim3(1024), 0, st, a); break;
    default: break;
  }
}

uint64_t jam_bytes(const E* e) {
  const auto& S = e->jm;
  const uint64_t plane = (uint64_t)e->N * 4;
  return ((S.label ? 1 : 0) + (S.count ? 1 : 0) + (S.spare_label ? 1 : 0) + (S.spare_count ? 1 : 0)) * plane +
         (S.rec ? (uint64_t)std::max(S.info.n_jams, 1) * sizeof(TsJamRecord) : 0) + (S.veh ? (uint64_t)std::max(S.info.n_spawned, 1) * 4 : 0);
}

void jam_fill_info(const E* e, TsJamInfo* out) {
  memset(out, 0, sizeof(*out));
  if (e->jm.held) *out = e->jm.info;
  out->width = e->W; out->height = e->H;
  out->device_bytes = jam_bytes(e);
}

int jam_need_result(E* e) {
  return e->jm.held ? TS_OK : fail(e, TS_E_STATE, "jams: nothing has been computed");
}

}  // namespace

extern "C" {

int ts_jams_compute(ts_handle e, const TsJamQuery* q, TsJamInfo* out) {
  if (!e) return TS_E_INVALID;
  if (!q) return fail(e, TS_E_INVALID, "jams: null pointer");
  if (q->min_ticks < 1) return fail(e, TS_E_INVALID, "jams: min_ticks must be at least 1");
  if (q->link != TS_JAM_GRID && q->link != TS_JAM_FLOW) return fail(e, TS_E_INVALID, "jams: link is TS_JAM_GRID or TS_JAM_FLOW");
  if (q->source != TS_JAM_VEHICLES && q->source != TS_JAM_MASK) return fail(e, TS_E_INVALID, "jams: source is TS_JAM_VEHICLES or TS_JAM_MASK");
  const bool masked = q->source == TS_JAM_MASK;
  if (masked && !q->mask) return fail(e, TS_E_INVALID, "jams: TS_JAM_MASK without a mask");
  if (masked && (q->mask_on_device | 1) != 1) return fail(e, TS_E_INVALID, "jams: mask_on_device is 0 or 1");
  if (e->fatal) return e->fatal;
  int T = JAM_TILE;
  if (const char* s = getenv("TS_DEBUG_JAMS_TILE")) { const int v = atoi(s); if (v == 8 || v == 16 || v == 32) T = v; }
  auto& S = e->jm;
  const size_t N = (size_t)e->N, nv = (size_t)e->n_vehicles_total;
  hipStream_t st = e->stream;
  JamArgs a{};
  a.W = e->W; a.H = e->H; a.N = e->N; a.n_active = masked ? 0 : e->n_active; a.n_vehicles = e->n_vehicles_total;
  a.min_ticks = q->min_ticks; a.link = q->link; a.T = T;
  a.tiles_x = T ? (e->W + T - 1) / T : 0;
  a.n_tile_slots = T ? a.tiles_x * ((e->H + T - 1) / T) : 0;
  const Dev& d = e->d;
  a.active = d.active; a.pos = d.pos; a.stuck_ticks = d.stuck_ticks; a.flags = d.flags; a.cell = d.cell;
  // Everything this call needs is allocated before anything of the previous result goes: the planes it writes are the spare pair
  // or new ones, never the result's.
  int32_t *label = S.spare_label, *veh = nullptr;
  uint32_t* count = S.spare_count;
  TsJamRecord* rec = nullptr;
  // (the spare planes stay the engine's whatever happens; what this call allocated on top is dropped when it is refused)
  auto keep_spares = [&] { S.spare_label = label; S.spare_count = count; };
  Scratch tmp;
  uint8_t *d_mask = nullptr, *cub = nullptr;
  size_t cub_bytes = 0;
  hipError_t r = hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, a.root, a.num, (int)N + 1, st);
  if (r == hipSuccess && !label && (r = dalloc(e, &label, N)) != hipSuccess) label = nullptr;
  if (r == hipSuccess && !count && (r = dalloc(e, &count, N)) != hipSuccess) count = nullptr;
  if (r == hipSuccess && (r = dalloc(e, &veh, nv)) != hipSuccess) veh = nullptr;
  if (r == hipSuccess) r = tmp.get(&a.root, N + 1);
  if (r == hipSuccess) r = tmp.get(&a.num, N + 1);
  if (r == hipSuccess) r = tmp.get(&cub, cub_bytes);
  if (r == hipSuccess) r = tmp.get(&a.ctl, 1);
  if (r == hipSuccess && T) r = tmp.get(&a.tiles, (size_t)a.n_tile_slots);
  if (r == hipSuccess && T) r = tmp.get(&a.tile_flag, (size_t)a.n_tile_slots);
  if (r == hipSuccess && masked && !q->mask_on_device) r = tmp.get(&d_mask, N);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    keep_spares();
    dfree(e, veh);
    return fail(e, TS_E_DEVICE, "jams: no device memory (the previous result stays)");
  }
  keep_spares();
  a.count = count; a.label = label; a.veh_jam = veh;
  a.mask = masked ? (q->mask_on_device ? q->mask : d_mask) : nullptr;
  const int cell_blocks = nblk((long long)N), veh_blocks = nblk((long long)a.n_active);
  JamCtl ctl{};
  int n_jams = 0;
  r = hipMemsetAsync(a.ctl, 0, sizeof(JamCtl), st);
  if (r == hipSuccess) r = hipMemsetAsync(veh, 0xFF, std::max<size_t>(nv, 1) * 4, st);
  if (r == hipSuccess && T) r = hipMemsetAsync(a.tile_flag, 0, (size_t)a.n_tile_slots * 4, st);
  if (r == hipSuccess && d_mask) r = hipMemcpyAsync(d_mask, q->mask, N, hipMemcpyHostToDevice, st);
  if (r == hipSuccess && !masked) r = hipMemsetAsync(count, 0, N * 4, st);
  if (r == hipSuccess) {
    if (masked) hipLaunchKernelGGL(k_jam_mark_mask, dim3(cell_blocks), dim3(BLK), 0, st, a);
    else if (a.n_active > 0) hipLaunchKernelGGL(k_jam_mark_vehicles, dim3(veh_blocks), dim3(BLK), 0, st, a);
    hipLaunchKernelGGL(k_jam_init, dim3(cell_blocks), dim3(BLK), 0, st, a);
    // (the number of listed tiles stays on the device: a workgroup beyond it leaves at once)
    if (T) jam_launch_tile(T, a.n_tile_slots, st, a);
    hipLaunchKernelGGL(k_jam_merge, dim3(cell_blocks), dim3(BLK), 0, st, a);
    hipLaunchKernelGGL(k_jam_flatten, dim3(nblk((long long)N + 1)), dim3(BLK), 0, st, a);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.root, a.num, (int)N + 1, st);
  if (r == hipSuccess) r = hipMemcpyAsync(&n_jams, a.num + N, 4, hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipMemcpyAsync(&ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r == hipSuccess && !ctl.fault && dalloc(e, &rec, (size_t)n_jams) != hipSuccess) {
    (void)hipGetLastError();
    dfree(e, veh);
    return fail(e, TS_E_DEVICE, "jams: no device memory for the records (the previous result stays)");
  }
  if (r == hipSuccess && !ctl.fault) {
    a.rec = rec; a.n_jams = n_jams;
    r = hipMemsetAsync(rec, 0, std::max<size_t>((size_t)n_jams, 1) * sizeof(TsJamRecord), st);
    if (r == hipSuccess) {
      hipLaunchKernelGGL(k_jam_number, dim3(cell_blocks), dim3(BLK), 0, st, a);
      hipLaunchKernelGGL(k_jam_record_cells, dim3(cell_blocks), dim3(BLK), 0, st, a);
      if (a.n_active > 0) hipLaunchKernelGGL(k_jam_record_vehicles, dim3(veh_blocks), dim3(BLK), 0, st, a);
      if (n_jams > 0) hipLaunchKernelGGL(k_jam_finish, dim3(nblk((long long)n_jams)), dim3(BLK), 0, st, a, n_jams);
      r = hipGetLastError();
    }
    if (r == hipSuccess) r = hipMemcpyAsync(&ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipStreamSynchronize(st);
  }
  if (r != hipSuccess || ctl.fault) {
    dfree(e, veh); dfree(e, rec);
    if (r != hipSuccess) return fail(e, TS_E_DEVICE, std::string("jams: ") + hipGetErrorString(r));
    return fail(e, TS_E_CAPACITY, "jams: a capped loop of the labelling reached its cap (nothing is published; the previous result stays)");
  }
  // the new result takes the previous one's place; the planes it displaced are the next compute's
  std::swap(S.label, S.spare_label); std::swap(S.count, S.spare_count);
  dfree(e, S.rec); dfree(e, S.veh);
  S.rec = rec; S.veh = veh;
  S.held = true;
  TsJamInfo& I = S.info;
  memset(&I, 0, sizeof(I));
  I.min_ticks = q->min_ticks; I.link = q->link; I.source = q->source; I.mask_on_device = masked ? q->mask_on_device : 0;
  I.held = 1; I.width = e->W; I.height = e->H; I.n_spawned = e->n_vehicles_total;
  I.n_jams = n_jams; I.standing_cells = ctl.standing_cells; I.largest_cells = ctl.largest; I.tile = T;
  I.tick = e->C.step_count; I.standing_vehicles = (int64_t)ctl.standing_vehicles;
  if (out) jam_fill_info(e, out);
  return TS_OK;
}

int ts_jams_info(ts_handle e, TsJamInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  jam_fill_info(e, out);
  return TS_OK;
}

int ts_jams_records(ts_handle e, int32_t first, int32_t n, TsJamRecord* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "jams: null pointer");
  TRY(jam_need_result(e));
  const auto& S = e->jm;
  if (first < 0 || n < 0 || (long long)first + n > S.info.n_jams) return fail(e, TS_E_INVALID, "jams: range outside the jams of the result");
  if (n == 0) return TS_OK;
  return read_back(e, dst, S.rec + first, (size_t)n * sizeof(TsJamRecord));
}

int ts_jams_vehicles(ts_handle e, int32_t first, int32_t n, int32_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "jams: null pointer");
  TRY(jam_need_result(e));
  const auto& S = e->jm;
  if (first < 0 || n < 0 || (long long)first + n > S.info.n_spawned) return fail(e, TS_E_INVALID, "jams: range outside the spawn indices of the compute");
  if (n == 0) return TS_OK;
  return read_back(e, dst, S.veh + first, (size_t)n * 4);
}

int ts_jams_download(ts_handle e, int32_t which, void* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "jams: null pointer");
  if (which != TS_JAM_PLANE_LABEL && which != TS_JAM_PLANE_COUNT) return fail(e, TS_E_INVALID, "jams: `which` is TS_JAM_PLANE_LABEL or TS_JAM_PLANE_COUNT");
  TRY(jam_need_result(e));
  const auto& S = e->jm;
  return read_back(e, dst, which == TS_JAM_PLANE_LABEL ? (const void*)S.label : (const void*)S.count, (size_t)e->N * 4);
}

int ts_jams_groups(ts_handle e, int64_t* rows) {
  if (!e) return TS_E_INVALID;
  if (!rows) return fail(e, TS_E_INVALID, "jams: null pointer");
  TRY(jam_need_result(e));
  if (e->d.G == 0) return TS_OK;
  const int per_block = BLK / 64;
  return launch_read<long long>(e, (size_t)e->d.G * TS_JG_NFIELDS, rows, [&](long long* out) {
    hipLaunchKernelGGL(k_jam_groups, dim3((e->d.G + per_block - 1) / per_block), dim3(BLK), 0, e->stream, e->d, e->jm.label, e->jm.rec, out);
  });
}

int ts_jams_device(ts_handle e, int32_t which, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "jams: null pointer");
  if (which < TS_JAM_PLANE_LABEL || which > TS_JAM_VEHICLE_JAM) return fail(e, TS_E_INVALID, "jams: `which` out of range");
  TRY(jam_need_result(e));
  HIPOK(hipStreamSynchronize(e->stream));
  const auto& S = e->jm;
  *ptr = which == TS_JAM_PLANE_LABEL ? (void*)S.label : which == TS_JAM_PLANE_COUNT ? (void*)S.count : which == TS_JAM_RECORDS ? (void*)S.rec : (void*)S.veh;
  return TS_OK;
}

int ts_jams_release(ts_handle e) {
  if (!e) return TS_E_INVALID;
  auto& S = e->jm;
  HIPOK(hipStreamSynchronize(e->stream));
  dfree(e, S.label); dfree(e, S.spare_label); dfree(e, S.count); dfree(e, S.spare_count); dfree(e, S.rec); dfree(e, S.veh);
  S.label = S.spare_label = nullptr; S.count = S.spare_count = nullptr; S.rec = nullptr; S.veh = nullptr;
  S.held = false;
  memset(&S.info, 0, sizeof(S.info));
  return TS_OK;
}

}  // extern "C"
