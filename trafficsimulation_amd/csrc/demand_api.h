// demand_api.h - the ts_demand_* entries (include/trafficsim_demand.h): the host side of the route demand whose kernels
// are in demand.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_demand.h"

namespace {

// lanes per vehicle and path steps per team iteration of k_demand_walk (profiles/demand_probe.py settled them)
constexpr int DM_TEAM = 32, DM_CHUNK = 32, DM_CHUNK_MAX = 65536;

size_t dm_plane_words(const E* e, int n_bins) { return (size_t)n_bins * 4 * (size_t)e->N; }

// the four planes of a bin, or an error code (with ts_last_error set); dir is checked against [dir_min, 3]
int dm_bin(E* e, int32_t bin, int32_t dir, int dir_min, const uint32_t** out) {
  if (!e->dm.planes) return fail(e, TS_E_STATE, "demand: nothing has been computed");
  if (bin < 0 || bin >= e->dm.n_bins) return fail(e, TS_E_INVALID, "demand: bin index out of range");
  if (dir < dir_min || dir > 3) return fail(e, TS_E_INVALID, "demand: direction out of range");
  *out = e->dm.planes + (size_t)bin * 4 * (size_t)e->N;
  return TS_OK;
}

// run `use` on the plane (bin, dir): the engine's own for dir 0..3, a temporary sum of the four for dir -1
template <typename F>
int dm_with_plane(E* e, int32_t bin, int32_t dir, F use) {
  const uint32_t* bin4 = nullptr;
  TRY(dm_bin(e, bin, dir, -1, &bin4));
  if (dir >= 0) return use(bin4 + (size_t)dir * (size_t)e->N);
  Scratch tmp;
  uint32_t* sum = nullptr;
  HIPOK(tmp.get(&sum, (size_t)e->N));
  hipLaunchKernelGGL(k_demand_sum4, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, bin4, e->N, sum);
  return use(sum);
}

void dm_launch_walk(int team, int blocks, hipStream_t st, const DemandArgs& a) {
  switch (team) {
    case 8: hipLaunchKernelGGL(k_demand_walk<8>, dim3(blocks), dim3(BLK), 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_demand_walk<16>, dim3(blocks), dim3(BLK), 0, st, a); break;
    case 64: hipLaunchKernelGGL(k_demand_walk<64>, dim3(blocks), dim3(BLK), 0, st, a); break;
    default: hipLaunchKernelGGL(k_demand_walk<32>, dim3(blocks), dim3(BLK), 0, st, a); break;
  }
}

void dm_fill_info(const E* e, TsDemandInfo* out) {
  const auto& D = e->dm;
  memset(out, 0, sizeof(*out));
  out->width = e->W; out->height = e->H;
  if (!D.planes) return;
  out->n_bins = D.n_bins; out->bin_cells = D.bin_cells; out->open_tail = D.open_tail; out->selected = D.selected;
  out->tick = D.tick; out->vehicles = D.vehicles;
  for (int b = 0; b < D.n_bins; b++) { out->bin_steps[b] = D.bin_steps[b]; out->steps += D.bin_steps[b]; }
  out->device_bytes = (uint64_t)dm_plane_words(e, D.n_bins) * sizeof(uint32_t);
}

}  // namespace

extern "C" {

int ts_demand_compute(ts_handle e, const TsDemandQuery* q, TsDemandInfo* out) {
  if (!e) return TS_E_INVALID;
  if (!q) return fail(e, TS_E_INVALID, "demand: null pointer");
  if (q->n_bins < 1 || q->n_bins > TS_DEMAND_MAX_BINS) return fail(e, TS_E_INVALID, "demand: n_bins outside 1..8");
  if (q->bin_cells < 1) return fail(e, TS_E_INVALID, "demand: bin_cells must be at least 1");
  if ((q->open_tail | 1) != 1 || (q->select_on_device | 1) != 1 || q->reserved != 0)
    return fail(e, TS_E_INVALID, "demand: open_tail and select_on_device are 0 or 1, reserved is 0");
  if (q->select && q->n_select != e->n_vehicles_total)
    return fail(e, TS_E_INVALID, "demand: n_select must be the number of vehicles spawned so far (ts_num_spawned)");
  if (e->fatal) return e->fatal;
  auto& D = e->dm;
  // the walk's shape: lanes per vehicle (TS_DEBUG_DEMAND_TEAM: the probe's 8, 16, 32, 64) and steps per team iteration
  // (TS_DEBUG_DEMAND_CHUNK: tests walk several iterations on short paths), rounded up to whole steps per lane
  int team = DM_TEAM, chunk = DM_CHUNK;
  if (const char* s = getenv("TS_DEBUG_DEMAND_TEAM")) { const int v = atoi(s); if (v == 8 || v == 16 || v == 32 || v == 64) team = v; }
  if (const char* s = getenv("TS_DEBUG_DEMAND_CHUNK")) chunk = std::min(std::max(atoi(s), 1), DM_CHUNK_MAX);
  if (!D.cus) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 64; }
    D.cus = cus;
  }
  // Everything this call needs is allocated before anything of the previous result goes.  Planes of the size held are
  // computed in place (a per-tick caller allocates once): by then nothing is left that could refuse the call.
  const size_t words = dm_plane_words(e, q->n_bins);
  const bool in_place = D.planes && D.n_bins == q->n_bins;
  uint32_t* planes = in_place ? D.planes : nullptr;
  Scratch tmp;
  uint8_t* dsel = nullptr;
  if (!D.tot && dalloc(e, &D.tot, (size_t)DM_NTOT) != hipSuccess) {
    (void)hipGetLastError();
    D.tot = nullptr;
    return fail(e, TS_E_DEVICE, "demand: no device memory for the totals");
  }
  if (!in_place && dalloc(e, &planes, words) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "demand: no device memory for the planes (the previous result stays)");
  }
  const bool stage = q->select && !q->select_on_device && e->n_vehicles_total > 0;
  if (stage && tmp.get(&dsel, (size_t)e->n_vehicles_total) != hipSuccess) {
    (void)hipGetLastError();
    if (!in_place) dfree(e, planes);
    return fail(e, TS_E_DEVICE, "demand: no device memory for the selection (the previous result stays)");
  }
  DemandArgs a{};
  const Dev& d = e->d;
  a.W = e->W; a.N = e->N; a.n_active = e->n_active; a.n_vehicles = e->n_vehicles_total;
  a.active = d.active; a.pos = d.pos; a.path_len = d.path_len; a.path_cur = d.path_cur; a.path_off = d.path_off; a.pool = d.pool;
  a.select = stage ? dsel : q->select_on_device ? q->select : nullptr;   // (a host array of no vehicles is not staged)
  a.planes = planes; a.tot = D.tot;
  a.n_bins = q->n_bins; a.bin_cells = q->bin_cells; a.open_tail = q->open_tail;
  a.limit = (int)std::min<long long>((long long)q->n_bins * q->bin_cells, 0x7FFFFFFF);
  a.spl = (chunk + team - 1) / team;
  unsigned long long tot[DM_NTOT] = {};
  hipStream_t st = e->stream;
  hipError_t r = hipMemsetAsync(planes, 0, words * sizeof(uint32_t), st);
  if (r == hipSuccess) r = hipMemsetAsync(D.tot, 0, sizeof(tot), st);
  if (r == hipSuccess && stage) r = hipMemcpyAsync(dsel, q->select, (size_t)e->n_vehicles_total, hipMemcpyHostToDevice, st);
  if (r == hipSuccess && a.n_active > 0) {
    // whole waves of 64 / team vehicles; no more blocks than keep every CU full, each wave strides over the list
    const long long waves = ((long long)a.n_active + 64 / team - 1) / (64 / team);
    const int blocks = (int)std::min<long long>((waves + BLK / 64 - 1) / (BLK / 64), (long long)D.cus * 8);
    dm_launch_walk(team, blocks, st, a);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(tot, D.tot, sizeof(tot), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) {   // the device failed under an accepted call: planes computed in place hold nothing usable any more
    dfree(e, planes);
    if (in_place) { D.planes = nullptr; D.n_bins = D.bin_cells = D.open_tail = D.selected = 0; }
    return fail(e, TS_E_DEVICE, std::string("demand: ") + hipGetErrorString(r));
  }
  if (!in_place) dfree(e, D.planes);
  D.planes = planes;
  D.n_bins = q->n_bins; D.bin_cells = q->bin_cells; D.open_tail = q->open_tail; D.selected = q->select != nullptr;
  D.tick = e->C.step_count; D.vehicles = (long long)tot[DM_VEH];
  for (int b = 0; b < TS_DEMAND_MAX_BINS; b++) D.bin_steps[b] = tot[b];
  if (out) dm_fill_info(e, out);
  return TS_OK;
}

int ts_demand_info(ts_handle e, TsDemandInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  dm_fill_info(e, out);
  return TS_OK;
}

int ts_demand_download(ts_handle e, int32_t bin, int32_t dir, uint32_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "demand: null pointer");
  return dm_with_plane(e, bin, dir, [&](const uint32_t* src) { return read_back(e, dst, src, (size_t)e->N * sizeof(uint32_t)); });
}

int ts_demand_pooled(ts_handle e, int32_t bin, int32_t dir, int32_t factor, uint64_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst || factor < 1) return fail(e, TS_E_INVALID, "demand: null pointer or factor < 1");
  return pool_plane(e, "demand: ", factor, dst, [&](auto use) { return dm_with_plane(e, bin, dir, use); });
}

int ts_demand_groups(ts_handle e, int64_t* rows) {
  if (!e) return TS_E_INVALID;
  if (!rows) return fail(e, TS_E_INVALID, "demand: null pointer");
  if (!e->dm.planes) return fail(e, TS_E_STATE, "demand: nothing has been computed");
  const int items = e->d.G * e->dm.n_bins;
  if (items == 0) return TS_OK;
  const int per_block = BLK / 64;
  return launch_read<long long>(e, (size_t)items * TS_DG_NFIELDS, rows, [&](long long* out) {
    hipLaunchKernelGGL(k_demand_groups, dim3((items + per_block - 1) / per_block), dim3(BLK), 0, e->stream, e->d, e->dm.planes,
                       e->dm.n_bins, out);
  });
}

int ts_demand_device(ts_handle e, int32_t bin, int32_t dir, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "demand: null pointer");
  const uint32_t* bin4 = nullptr;
  TRY(dm_bin(e, bin, dir, 0, &bin4));
  HIPOK(hipStreamSynchronize(e->stream));
  *ptr = (void*)(bin4 + (size_t)dir * (size_t)e->N);
  return TS_OK;
}

int ts_demand_release(ts_handle e) {
  if (!e) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  dfree(e, e->dm.planes);
  e->dm.planes = nullptr;
  e->dm.n_bins = e->dm.bin_cells = e->dm.open_tail = e->dm.selected = 0;
  return TS_OK;
}

}  // extern "C"
