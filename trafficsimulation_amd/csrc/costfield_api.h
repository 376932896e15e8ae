// costfield_api.h - the ts_costfield_* entries (include/trafficsim_costfield.h): the host side of the cost fields whose
// kernels are in costfield.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_costfield.h"

namespace {

void cf_fill_info(const E* e, TsCostFieldInfo* out) {
  memset(out, 0, sizeof(*out));
  if (e->cf.val) *out = e->cf.info;
  out->width = e->W; out->height = e->H;
}

// the plane `which` of the result held, or an error code (with ts_last_error set)
int cf_plane(E* e, int32_t which, const uint32_t** out) {
  if (which != TS_CF_VALUE && which != TS_CF_OWNER) return fail(e, TS_E_INVALID, "cost field: which is 0 (values) or 1 (owners)");
  if (!e->cf.val) return fail(e, TS_E_STATE, "cost field: nothing has been computed");
  *out = which == TS_CF_VALUE ? e->cf.val : (const uint32_t*)e->cf.own;
  return TS_OK;
}

template <int NH, bool TO>
void cf_launch_seed(const CostFieldArgs& a, int n, const int32_t* xy, const int32_t* cost, hipStream_t st) {
  hipLaunchKernelGGL((k_cf_seed<NH, TO>), dim3(nblk(n)), dim3(BLK), 0, st, a, n, xy, cost);
}
template <int NH, bool TO>
void cf_launch_tile(const CostFieldArgs& a, int n_tiles, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((k_cf_tile<NH, TO>), dim3(n_tiles), dim3(a.T * a.T), lds, st, a);
}
template <int NH, bool TO>
void cf_launch_finish(const CostFieldArgs& a, uint32_t* val, int32_t* own, unsigned long long* tot, hipStream_t st) {
  hipLaunchKernelGGL((k_cf_finish<NH, TO>), dim3(nblk((long long)a.N)), dim3(BLK), 0, st, a, val, own, tot);
}
// (the four instantiations behind one switch each)
#define CF_DISPATCH(fn, nh, to, ...)                                  \
  do {                                                                \
    if ((nh) == 4) { if (to) fn<4, true>(__VA_ARGS__); else fn<4, false>(__VA_ARGS__); } \
    else { if (to) fn<1, true>(__VA_ARGS__); else fn<1, false>(__VA_ARGS__); }           \
  } while (0)

// cfroute_api.h, for a compute that is to leave a hop plane (ts_cfroute_compute): room for the new plane beside the one held,
// with the cell words that stay with it; the plane from the settled labels; the new plane in place of the old.  And for
// whatever ends a field: the hop plane goes with it.
hipError_t cfr_stage(E* e, const TsCostFieldQuery* q, uint32_t** cw);
hipError_t cfr_hops(E* e, const CostFieldArgs& a, int NH, bool to, const int32_t* d_xy, const int32_t* d_cost);
void cfr_publish(E* e, const TsCostFieldQuery* q, const CostFieldArgs& a, int NH);
void cfr_drop(E* e);

// ts_costfield_compute, and with `hops` ts_cfroute_compute: the same field, and the hop plane while the labels exist
int cf_compute(E* e, const TsCostFieldQuery* q, TsCostFieldInfo* out, bool hops) {
  if (!e) return TS_E_INVALID;
  if (!q || !q->seed_xy) return fail(e, TS_E_INVALID, "cost field: null pointer");
  if ((q->mode != TS_CF_FROM && q->mode != TS_CF_TO) || (q->soft_obstacles | 1) != 1 || (q->ignore_flow | 1) != 1 || (q->free_flow | 1) != 1 ||
      q->reserved != 0)
    return fail(e, TS_E_INVALID, "cost field: mode is TS_CF_FROM or TS_CF_TO, the flags are 0 or 1, reserved is 0");
  if (q->n_seeds < 1 || q->n_seeds > TS_CF_MAX_SEEDS) return fail(e, TS_E_INVALID, "cost field: n_seeds outside 1..1048576");
  for (int i = 0; i < q->n_seeds; i++) {
    const int x = q->seed_xy[2 * i], y = q->seed_xy[2 * i + 1];
    if (x < 0 || x >= e->W || y < 0 || y >= e->H) return fail(e, TS_E_INVALID, "cost field: seed " + std::to_string(i) + " is outside the map");
    if (q->seed_cost && (q->seed_cost[i] < 0 || (uint32_t)q->seed_cost[i] >= CF_INF))
      return fail(e, TS_E_INVALID, "cost field: the cost of seed " + std::to_string(i) + " is negative or not below 0x3F3F3F3F");
  }
  const TsParams& P = e->P;
  if (!astar_half_units(P)) return fail(e, TS_E_UNSUPPORTED, "cost field: the penalties are not all multiples of 0.5 (the kernels work in half units)");
  if (P.respect_awareness && !q->free_flow)
    return fail(e, TS_E_UNSUPPORTED, "cost field: with respect_awareness only free_flow fields exist (a field has no start to cast a field of view from)");
  if (e->fatal) return e->fatal;
  auto& D = e->cf;
  int T = 32;
  if (const char* s = getenv("TS_DEBUG_COSTFIELD_TILE")) { const int v = atoi(s); if (v == 8 || v == 16) T = v; }
  const bool to = q->mode == TS_CF_TO;
  const HalfCosts hc = half_costs(P);
  const int NH = (P.turn_penalty_enabled && P.turn_penalty > 0) ? 4 : 1;
  const int n = q->n_seeds;
  const size_t N = (size_t)e->N;
  const int tiles_x = (e->W + T - 1) / T, tiles_y = (e->H + T - 1) / T;
  const size_t n_tiles = (size_t)tiles_x * tiles_y;
  hipStream_t st = e->stream;
  // Everything is allocated before anything is computed, the new planes beside the ones held (the spare pair of the previous
  // compute when there is one): whatever refuses this call from here on leaves the previous result as it is.
  Scratch S;   // what the call holds on the device besides the result
  uint32_t* cw = nullptr; u64 *lab = nullptr, *seed = nullptr;
  uint32_t* ctl = nullptr;           // [0, 2) list lengths by parity, [2, 2 + 2 n_tiles) flags by parity
  int32_t *lists = nullptr, *d_xy = nullptr, *d_cost = nullptr;
  unsigned long long* tot = nullptr;
  hipError_t r = hops ? cfr_stage(e, q, &cw) : S.get(&cw, N);
  if (r == hipSuccess) r = S.get(&lab, (size_t)NH * N);
  if (r == hipSuccess && NH == 4) r = S.get(&seed, N);
  if (r == hipSuccess) r = S.get(&ctl, 2 + 2 * n_tiles);
  if (r == hipSuccess) r = S.get(&lists, 2 * n_tiles);
  if (r == hipSuccess) r = S.get(&d_xy, (size_t)2 * n);
  if (r == hipSuccess && q->seed_cost) r = S.get(&d_cost, (size_t)n);
  if (r == hipSuccess) r = S.get(&tot, 2);
  if (r == hipSuccess && !D.spare_val) r = dalloc(e, &D.spare_val, N);
  if (r == hipSuccess && !D.spare_own) r = dalloc(e, &D.spare_own, N);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "cost field: no device memory for the labels and planes (the previous result stays)");
  }
  // the maps ts_astar would see now; the cached density planes and the snapshot are dropped afterwards, as there
  const bool soft = q->soft_obstacles != 0, free_flow = q->free_flow != 0;
  const bool dens_on = soft && !free_flow && P.dynamic_penalties_enabled;
  if (dens_on) { TRY(ensure_density(e, e->d.occ)); }
  e->density_valid = false;
  e->amap_valid = false;
  hipLaunchKernelGGL(k_cf_cells, dim3(nblk((long long)N)), dim3(BLK), 0, st, e->d, soft ? 1 : 0, free_flow ? 1 : 0, dens_on ? 1 : 0,
                     P.road_type_penalties_enabled ? 1 : 0, (double)P.obstacle_penalty_vehicle, (double)P.dynamic_penalty_scale, hc, cw);
  CostFieldArgs a{};
  a.W = e->W; a.H = e->H; a.N = e->N; a.T = T; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
  a.ignore_flow = q->ignore_flow; a.turn2 = NH == 4 ? hc.turn2 : 0; a.contra2 = hc.contra2;
  a.limit = (q->max_cost != 0 && q->max_cost < CF_INF - 1) ? q->max_cost + 1 : CF_INF;
  a.cw = cw; a.lab = lab; a.seed = seed;
  uint32_t* n_list = ctl;
  uint32_t* flags[2] = {ctl + 2, ctl + 2 + n_tiles};
  int32_t* list[2] = {lists, lists + n_tiles};
  r = hipMemsetAsync(lab, 0xFF, (size_t)NH * N * sizeof(u64), st);
  if (r == hipSuccess && seed) r = hipMemsetAsync(seed, 0xFF, N * sizeof(u64), st);
  if (r == hipSuccess) r = hipMemsetAsync(ctl, 0, (2 + 2 * n_tiles) * sizeof(uint32_t), st);
  if (r == hipSuccess) r = hipMemsetAsync(tot, 0, 2 * sizeof(unsigned long long), st);
  if (r == hipSuccess) r = hipMemcpyAsync(d_xy, q->seed_xy, (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (r == hipSuccess && d_cost) r = hipMemcpyAsync(d_cost, q->seed_cost, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st);
  uint32_t n_cur = 0;
  if (r == hipSuccess) {
    a.list_next = list[0]; a.n_next = &n_list[0]; a.flag_next = flags[0];
    CF_DISPATCH(cf_launch_seed, NH, to, a, n, d_xy, d_cost, st);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(&n_cur, &n_list[0], sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  // Rounds: one launch over the tiles on the list, which leaves the next list; every launch ends by itself.  Labels only
  // decrease and each round that activates a tile lowered one, so the loop ends long before the cap.
  const int SS = (T + 2) * (T + 2);
  const size_t lds = (size_t)(NH + ((NH == 4 && !to) ? 1 : 0)) * SS * sizeof(u64) + (size_t)SS * sizeof(uint32_t) + 8 * sizeof(int);
  const long long cap = (long long)std::min<unsigned long long>((unsigned long long)NH * N, 0x7FFFFFFFull);
  long long rounds = 0, visits = 0;
  while (r == hipSuccess && n_cur > 0) {
    if (rounds >= cap) return fail(e, TS_E_CAPACITY, "cost field: the relaxation did not settle within as many rounds as there are states");
    const int cp = (int)(rounds & 1), np = cp ^ 1;
    a.list_cur = list[cp]; a.flag_cur = flags[cp];
    a.list_next = list[np]; a.n_next = &n_list[np]; a.flag_next = flags[np];
    r = hipMemsetAsync(&n_list[np], 0, sizeof(uint32_t), st);
    if (r != hipSuccess) break;
    CF_DISPATCH(cf_launch_tile, NH, to, a, (int)n_cur, lds, st);
    r = hipGetLastError();
    rounds++; visits += n_cur;
    if (r == hipSuccess) r = hipMemcpyAsync(&n_cur, &n_list[np], sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipStreamSynchronize(st);
    if (r == hipSuccess && n_cur > n_tiles) r = hipErrorUnknown;   // (a list cannot outgrow the tiles: the flags keep entries unique)
  }
  if (r == hipSuccess && hops) r = cfr_hops(e, a, NH, to, d_xy, d_cost);
  unsigned long long h_tot[2] = {0, 0};
  if (r == hipSuccess) {
    CF_DISPATCH(cf_launch_finish, NH, to, a, D.spare_val, D.spare_own, tot, st);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(h_tot, tot, sizeof(h_tot), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) return fail(e, TS_E_DEVICE, std::string("cost field: ") + hipGetErrorString(r));
  std::swap(D.val, D.spare_val);
  std::swap(D.own, D.spare_own);
  if (hops) cfr_publish(e, q, a, NH); else cfr_drop(e);
  TsCostFieldInfo& I = D.info;
  memset(&I, 0, sizeof(I));
  I.mode = q->mode; I.soft_obstacles = q->soft_obstacles; I.ignore_flow = q->ignore_flow; I.free_flow = q->free_flow;
  I.max_cost = q->max_cost; I.n_seeds = n; I.tile = T; I.headings = NH;
  I.tick = e->C.step_count; I.reached = (int64_t)h_tot[0]; I.max_value = (uint32_t)h_tot[1];
  I.rounds = (int32_t)rounds; I.tile_visits = visits;
  I.device_bytes = (uint64_t)N * (sizeof(uint32_t) + sizeof(int32_t));
  if (out) cf_fill_info(e, out);
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_costfield_compute(ts_handle e, const TsCostFieldQuery* q, TsCostFieldInfo* out) { return cf_compute(e, q, out, false); }

int ts_costfield_info(ts_handle e, TsCostFieldInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  cf_fill_info(e, out);
  return TS_OK;
}

int ts_costfield_download(ts_handle e, int32_t which, void* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "cost field: null pointer");
  const uint32_t* src = nullptr;
  TRY(cf_plane(e, which, &src));
  return read_back(e, dst, src, (size_t)e->N * sizeof(uint32_t));
}

int ts_costfield_gather(ts_handle e, int32_t which, int32_t n, const int32_t* xy, void* out) {
  if (!e) return TS_E_INVALID;
  if (n < 0 || (n > 0 && (!xy || !out))) return fail(e, TS_E_INVALID, "cost field: null pointer or n < 0");
  const uint32_t* src = nullptr;
  TRY(cf_plane(e, which, &src));
  for (int i = 0; i < n; i++)
    if (xy[2 * i] < 0 || xy[2 * i] >= e->W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= e->H)
      return fail(e, TS_E_INVALID, "cost field: cell " + std::to_string(i) + " is outside the map");
  if (n == 0) return TS_OK;
  Scratch S;   // what the call holds on the device besides the result
  int32_t* d_xy = nullptr; uint32_t* d_out = nullptr;
  if (S.get(&d_xy, (size_t)2 * n) != hipSuccess || S.get(&d_out, (size_t)n) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "cost field: no device memory for the gather");
  }
  HIPOK(hipMemcpyAsync(d_xy, xy, (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_cf_gather, dim3(nblk(n)), dim3(BLK), 0, e->stream, src, e->W, n, d_xy, d_out);
  return read_back(e, out, d_out, (size_t)n * sizeof(uint32_t));
}

int ts_costfield_bands(ts_handle e, int32_t n, const uint32_t* thresholds, uint64_t* counts) {
  if (!e) return TS_E_INVALID;
  if (!thresholds || !counts) return fail(e, TS_E_INVALID, "cost field: null pointer");
  if (n < 1 || n > TS_CF_MAX_BANDS) return fail(e, TS_E_INVALID, "cost field: 1..1024 thresholds");
  for (int k = 1; k < n; k++)
    if (thresholds[k] < thresholds[k - 1]) return fail(e, TS_E_INVALID, "cost field: the thresholds must ascend");
  if (!e->cf.val) return fail(e, TS_E_STATE, "cost field: nothing has been computed");
  Scratch S;   // what the call holds on the device besides the result
  uint32_t* d_thr = nullptr; unsigned long long* d_hist = nullptr;
  if (S.get(&d_thr, (size_t)n) != hipSuccess || S.get(&d_hist, (size_t)n) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "cost field: no device memory for the bands");
  }
  HIPOK(hipMemcpyAsync(d_thr, thresholds, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPOK(hipMemsetAsync(d_hist, 0, (size_t)n * sizeof(unsigned long long), e->stream));
  const int blocks = (int)std::min<long long>(nblk((long long)e->N), 1024);
  hipLaunchKernelGGL(k_cf_bands, dim3(blocks), dim3(BLK), 0, e->stream, e->cf.val, e->d.is_road, e->N, n, d_thr, d_hist);
  std::vector<unsigned long long> hist((size_t)n);
  TRY(read_back(e, hist.data(), d_hist, (size_t)n * sizeof(unsigned long long)));
  unsigned long long sum = 0;
  for (int k = 0; k < n; k++) { sum += hist[k]; counts[k] = sum; }
  return TS_OK;
}

int ts_costfield_device(ts_handle e, int32_t which, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "cost field: null pointer");
  const uint32_t* src = nullptr;
  TRY(cf_plane(e, which, &src));
  HIPOK(hipStreamSynchronize(e->stream));
  *ptr = (void*)src;
  return TS_OK;
}

int ts_costfield_release(ts_handle e) {
  if (!e) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  auto& D = e->cf;
  cfr_drop(e);
  dfree(e, D.val); dfree(e, D.own); dfree(e, D.spare_val); dfree(e, D.spare_own);
  D.val = D.spare_val = nullptr; D.own = D.spare_own = nullptr;
  memset(&D.info, 0, sizeof(D.info));
  return TS_OK;
}

}  // extern "C"
