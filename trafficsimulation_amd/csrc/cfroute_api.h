// cfroute_api.h - the ts_cfroute_* entries (include/trafficsim_cfroute.h): the host side of the routes along a cost field
// whose kernels are in cfroute.h.  Part of the single translation unit engine.hip (included at its end, behind
// costfield_api.h whose compute it shares).
#pragma once
#include "../../include/trafficsim_cfroute.h"

namespace {

// ---- the compute's side (declared in costfield_api.h) ------------------------------------------------------------------------
// Room for a new hop plane beside the one held: the spare plane and cell words (kept from compute to compute, like the spare
// value and owner planes) and the seeds by cell - for every cell that holds seeds the smallest label among them -, sorted on
// the host and staged on the device.  Nothing of the plane held is touched; a staging that a refused compute leaves behind
// is freed by the next one.
hipError_t cfr_stage(E* e, const TsCostFieldQuery* q, uint32_t** cw) {
  auto& R = e->cfr;
  dfree(e, R.stage_cell); dfree(e, R.stage_lab);
  R.stage_cell = nullptr; R.stage_lab = nullptr; R.stage_n = 0;
  const size_t N = (size_t)e->N;
  hipError_t r = hipSuccess;
  if (!R.spare_hops) r = dalloc(e, &R.spare_hops, N);
  if (r == hipSuccess && !R.spare_cw) r = dalloc(e, &R.spare_cw, N);
  if (r != hipSuccess) return r;
  std::vector<std::pair<int32_t, u64>> s((size_t)q->n_seeds);
  for (int i = 0; i < q->n_seeds; i++)
    s[i] = {q->seed_xy[2 * i + 1] * e->W + q->seed_xy[2 * i], ((u64)(uint32_t)(q->seed_cost ? q->seed_cost[i] : 0) << 32) | (uint32_t)i};
  std::sort(s.begin(), s.end());
  std::vector<int32_t> cell; std::vector<u64> lab;
  for (const auto& p : s)
    if (cell.empty() || cell.back() != p.first) { cell.push_back(p.first); lab.push_back(p.second); }
  r = dalloc(e, &R.stage_cell, cell.size());
  if (r == hipSuccess) r = dalloc(e, &R.stage_lab, lab.size());
  if (r == hipSuccess) r = hipMemcpy(R.stage_cell, cell.data(), cell.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(R.stage_lab, lab.data(), lab.size() * sizeof(u64), hipMemcpyHostToDevice);
  if (r != hipSuccess) return r;
  R.stage_n = (int)cell.size();
  *cw = R.spare_cw;
  return hipSuccess;
}

template <int NH, bool TO>
void cfr_launch_hops(const CostFieldArgs& a, const int32_t* d_xy, const int32_t* d_cost, uint16_t* hops, hipStream_t st) {
  hipLaunchKernelGGL((k_cfr_hops<NH, TO>), dim3(nblk((long long)a.N)), dim3(BLK), 0, st, a, d_xy, d_cost, hops);
}

// the hop plane of the settled labels, into the spare plane
hipError_t cfr_hops(E* e, const CostFieldArgs& a, int NH, bool to, const int32_t* d_xy, const int32_t* d_cost) {
  CF_DISPATCH(cfr_launch_hops, NH, to, a, d_xy, d_cost, e->cfr.spare_hops, e->stream);
  return hipGetLastError();
}

// the compute has succeeded: what was staged becomes what is held
void cfr_publish(E* e, const TsCostFieldQuery* q, const CostFieldArgs& a, int NH) {
  auto& R = e->cfr;
  std::swap(R.hops, R.spare_hops);
  std::swap(R.cw, R.spare_cw);
  dfree(e, R.seed_cell); dfree(e, R.seed_lab);
  R.seed_cell = R.stage_cell; R.seed_lab = R.stage_lab; R.n_seed_cells = R.stage_n;
  R.stage_cell = nullptr; R.stage_lab = nullptr; R.stage_n = 0;
  R.mode = q->mode; R.headings = NH; R.n_seeds = q->n_seeds; R.turn2 = a.turn2; R.contra2 = a.contra2;
  R.tick = e->C.step_count;
}

// the field under the hop plane is gone: so is the plane (the batch and the load planes are results of their own)
void cfr_drop(E* e) {
  auto& R = e->cfr;
  if (!R.hops && !R.spare_hops && !R.stage_cell) return;
  (void)hipStreamSynchronize(e->stream);
  dfree(e, R.hops); dfree(e, R.spare_hops); dfree(e, R.cw); dfree(e, R.spare_cw);
  dfree(e, R.seed_cell); dfree(e, R.seed_lab); dfree(e, R.stage_cell); dfree(e, R.stage_lab);
  R.hops = R.spare_hops = nullptr; R.cw = R.spare_cw = nullptr;
  R.seed_cell = R.stage_cell = nullptr; R.seed_lab = R.stage_lab = nullptr;
  R.n_seed_cells = R.stage_n = 0;
  R.mode = R.headings = R.n_seeds = R.turn2 = R.contra2 = 0;
  R.tick = 0;
}

// ---- walks ----------------------------------------------------------------------------------------------------------------
CfrPlane cfr_plane(const E* e) {
  const auto& R = e->cfr;
  CfrPlane P{};
  P.W = e->W; P.H = e->H; P.N = e->N; P.to = R.mode == TS_CF_TO; P.nh = R.headings; P.turn2 = R.turn2; P.contra2 = R.contra2;
  P.n_seed_cells = R.n_seed_cells;
  P.cap = (long long)(R.headings == 4 ? 5 : 1) * e->N;
  P.hops = R.hops; P.cw = R.cw; P.val = e->cf.val; P.own = e->cf.own; P.seed_cell = R.seed_cell; P.seed_lab = R.seed_lab;
  return P;
}

// what ts_cfroute_trace and ts_cfroute_load refuse alike
int cfr_check_starts(E* e, int32_t n, const int32_t* xy, const int8_t* head) {
  if (!xy) return fail(e, TS_E_INVALID, "cost-field routes: null pointer");
  if (n < 1 || n > TS_CFR_MAX_STARTS) return fail(e, TS_E_INVALID, "cost-field routes: n outside 1..16777216");
  if (!e->cfr.hops || !e->cf.val) return fail(e, TS_E_STATE, "cost-field routes: there is no hop plane (ts_cfroute_compute leaves one)");
  const bool to = e->cfr.mode == TS_CF_TO;
  for (int i = 0; i < n; i++) {
    const int x = xy[2 * i], y = xy[2 * i + 1];
    if (x < 0 || x >= e->W || y < 0 || y >= e->H) return fail(e, TS_E_INVALID, "cost-field routes: start " + std::to_string(i) + " is outside the map");
    if (head && (head[i] < -1 || head[i] > 3 || (!to && head[i] != -1)))
      return fail(e, TS_E_INVALID, "cost-field routes: the heading of start " + std::to_string(i) + (to ? " is outside -1..3" : " must be -1 (a FROM route ends at its start)"));
  }
  if (e->fatal) return e->fatal;
  return TS_OK;
}

void cfr_fill_info(const E* e, TsCfRouteInfo* out) {
  const auto& R = e->cfr;
  memset(out, 0, sizeof(*out));
  out->width = e->W; out->height = e->H;
  if (R.hops) {
    out->held = 1; out->mode = R.mode; out->headings = R.headings; out->n_seeds = R.n_seeds; out->tick = R.tick;
    out->device_bytes = (uint64_t)e->N * (sizeof(uint16_t) + sizeof(uint32_t)) + (uint64_t)R.n_seed_cells * (sizeof(int32_t) + sizeof(u64));
  }
  const TsCfRouteBatch& B = R.batch;
  out->trace_n = B.n; out->trace_unreached = B.unreached; out->trace_steps = B.steps; out->trace_longest = B.longest;
  out->trace_tick = B.tick; out->trace_device_bytes = B.device_bytes;
  const TsCfRouteLoadInfo& L = R.load_info;
  out->load_routes = L.routes; out->load_unreached = L.unreached; out->load_steps = L.steps; out->load_tick = L.tick;
  out->load_device_bytes = L.device_bytes;
}

// a range of the batch, or an error code
int cfr_range(E* e, int32_t first, int32_t count) {
  const auto& R = e->cfr;
  if (R.batch.n == 0) return fail(e, TS_E_STATE, "cost-field routes: nothing has been traced");
  if (first < 0 || count < 0 || (long long)first + count > R.batch.n) return fail(e, TS_E_INVALID, "cost-field routes: the range lies outside the batch");
  return TS_OK;
}

// off[0 .. count] of the range, counted from its first step, which is step `base` of the batch
int cfr_read_off(E* e, int32_t first, int32_t count, std::vector<long long>& off, long long& base) {
  off.resize((size_t)count + 1);
  TRY(read_back(e, off.data(), e->cfr.off + first, ((size_t)count + 1) * sizeof(long long)));
  base = off[0];
  for (auto& v : off) v -= base;
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_cfroute_compute(ts_handle e, const TsCostFieldQuery* q, TsCostFieldInfo* out) { return cf_compute(e, q, out, true); }

int ts_cfroute_info(ts_handle e, TsCfRouteInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  cfr_fill_info(e, out);
  return TS_OK;
}

int ts_cfroute_trace(ts_handle e, int32_t n, const int32_t* start_xy, const int8_t* start_heading, TsCfRouteBatch* out) {
  if (!e) return TS_E_INVALID;
  TRY(cfr_check_starts(e, n, start_xy, start_heading));
  auto& R = e->cfr;
  hipStream_t st = e->stream;
  const size_t nn = (size_t)n;
  // the new batch lies beside the one held until it is whole: whatever refuses the call leaves that one readable
  long long* off = nullptr; uint8_t* dirs = nullptr; uint32_t* cost = nullptr; int32_t *owner = nullptr, *starts = nullptr;
  auto drop = [&] { dfree(e, off); dfree(e, dirs); dfree(e, cost); dfree(e, owner); dfree(e, starts); };
  Scratch S;   // what the call holds on the device besides the result
  int8_t* d_head = nullptr; long long* len = nullptr; unsigned long long* ctl = nullptr; uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  hipError_t r = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, len, off, n + 1, st);
  if (r == hipSuccess) r = dalloc(e, &off, nn + 1);
  if (r == hipSuccess) r = dalloc(e, &cost, nn);
  if (r == hipSuccess) r = dalloc(e, &owner, nn);
  if (r == hipSuccess) r = dalloc(e, &starts, 2 * nn);
  if (r == hipSuccess && start_heading) r = S.get(&d_head, nn);
  if (r == hipSuccess) r = S.get(&len, nn + 1);
  if (r == hipSuccess) r = S.get(&ctl, (size_t)CFR_C_N);
  if (r == hipSuccess) r = S.get(&tmp, tmp_bytes);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    drop();
    return fail(e, TS_E_DEVICE, "cost-field routes: no device memory for the batch (the previous one stays)");
  }
  const CfrPlane P = cfr_plane(e);
  unsigned long long h_ctl[CFR_C_N] = {};
  long long total = 0;
  r = hipMemsetAsync(ctl, 0, sizeof(h_ctl), st);
  if (r == hipSuccess) r = hipMemcpyAsync(starts, start_xy, 2 * nn * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (r == hipSuccess && d_head) r = hipMemcpyAsync(d_head, start_heading, nn, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(k_cfr_count, dim3(nblk((long long)n + 1)), dim3(BLK), 0, st, P, n, starts, d_head, len, cost, owner, ctl);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, len, off, n + 1, st);
  if (r == hipSuccess) r = hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipMemcpyAsync(&total, off + n, sizeof(total), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) { drop(); return fail(e, TS_E_DEVICE, std::string("cost-field routes: ") + hipGetErrorString(r)); }
  if (h_ctl[CFR_C_FAULT]) {
    drop();
    return fail(e, TS_E_CAPACITY, "cost-field routes: a walk left the map or took more steps than there are states (nothing is published)");
  }
  if (dalloc(e, &dirs, (size_t)total) != hipSuccess) {
    (void)hipGetLastError();
    dirs = nullptr;
    drop();
    return fail(e, TS_E_DEVICE, "cost-field routes: no device memory for the steps (the previous batch stays)");
  }
  if (total > 0) {
    hipLaunchKernelGGL(k_cfr_write, dim3(nblk(n)), dim3(BLK), 0, st, P, n, starts, d_head, off, dirs);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) { drop(); return fail(e, TS_E_DEVICE, std::string("cost-field routes: ") + hipGetErrorString(r)); }
  dfree(e, R.off); dfree(e, R.dirs); dfree(e, R.cost); dfree(e, R.owner); dfree(e, R.starts);
  R.off = off; R.dirs = dirs; R.cost = cost; R.owner = owner; R.starts = starts;
  R.batch_to = P.to;
  TsCfRouteBatch& B = R.batch;
  B.n = n; B.unreached = (int32_t)h_ctl[CFR_C_UNREACHED]; B.steps = total; B.longest = (int64_t)h_ctl[CFR_C_LONGEST]; B.tick = R.tick;
  B.device_bytes = (uint64_t)(nn + 1) * sizeof(long long) + (uint64_t)std::max<long long>(total, 1) + (uint64_t)nn * (sizeof(uint32_t) + 3 * sizeof(int32_t));
  if (out) *out = B;
  return TS_OK;
}

int ts_cfroute_read(ts_handle e, int32_t first, int32_t count, int64_t* off, uint8_t* dirs, uint32_t* cost, int32_t* owner) {
  if (!e) return TS_E_INVALID;
  TRY(cfr_range(e, first, count));
  const auto& R = e->cfr;
  std::vector<long long> h_off;
  long long base = 0;
  TRY(cfr_read_off(e, first, count, h_off, base));
  if (off) memcpy(off, h_off.data(), h_off.size() * sizeof(long long));
  if (dirs && h_off[count] > 0) TRY(read_back(e, dirs, R.dirs + base, (size_t)h_off[count]));
  if (cost && count > 0) TRY(read_back(e, cost, R.cost + first, (size_t)count * sizeof(uint32_t)));
  if (owner && count > 0) TRY(read_back(e, owner, R.owner + first, (size_t)count * sizeof(int32_t)));
  return TS_OK;
}

int ts_cfroute_cells(ts_handle e, int32_t first, int32_t count, int64_t* off, int32_t* xy) {
  if (!e) return TS_E_INVALID;
  TRY(cfr_range(e, first, count));
  const auto& R = e->cfr;
  std::vector<long long> h_off;
  long long base = 0;
  TRY(cfr_read_off(e, first, count, h_off, base));
  if (off) memcpy(off, h_off.data(), h_off.size() * sizeof(long long));
  const long long steps = h_off[count];
  if (!xy || steps == 0) return TS_OK;
  Scratch S;   // what the call holds on the device besides the result
  int32_t* d_xy = nullptr;
  if (S.get(&d_xy, (size_t)steps * 2) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "cost-field routes: no device memory for the cells");
  }
  hipLaunchKernelGGL(k_cfr_cells, dim3(nblk(count)), dim3(BLK), 0, e->stream, e->W, R.batch_to, first, count, R.starts, R.off, R.dirs, d_xy);
  HIPOK(hipGetLastError());
  return read_back(e, xy, d_xy, (size_t)steps * 2 * sizeof(int32_t));
}

int ts_cfroute_device(ts_handle e, int32_t which, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "cost-field routes: null pointer");
  if (which < TS_CFR_HOPS || which > TS_CFR_OWNER) return fail(e, TS_E_INVALID, "cost-field routes: which is 0 (hops), 1 (off), 2 (dirs), 3 (cost) or 4 (owner)");
  const auto& R = e->cfr;
  if (which == TS_CFR_HOPS ? !R.hops : R.batch.n == 0)
    return fail(e, TS_E_STATE, which == TS_CFR_HOPS ? "cost-field routes: there is no hop plane" : "cost-field routes: nothing has been traced");
  HIPOK(hipStreamSynchronize(e->stream));
  void* const p[5] = {R.hops, R.off, R.dirs, R.cost, R.owner};
  *ptr = p[which];
  return TS_OK;
}

int ts_cfroute_load(ts_handle e, int32_t n, const int32_t* start_xy, const int8_t* start_heading, const uint32_t* weight,
                    TsCfRouteLoadInfo* out) {
  if (!e) return TS_E_INVALID;
  TRY(cfr_check_starts(e, n, start_xy, start_heading));
  auto& R = e->cfr;
  hipStream_t st = e->stream;
  const size_t nn = (size_t)n, words = 4 * (size_t)e->N;
  // the planes are added up beside the ones held, which change places with them at the end
  Scratch S;   // what the call holds on the device besides the result
  int32_t* d_xy = nullptr; int8_t* d_head = nullptr; uint32_t* d_w = nullptr; unsigned long long* ctl = nullptr;
  hipError_t r = S.get(&d_xy, 2 * nn);
  if (r == hipSuccess && start_heading) r = S.get(&d_head, nn);
  if (r == hipSuccess && weight) r = S.get(&d_w, nn);
  if (r == hipSuccess) r = S.get(&ctl, (size_t)CFR_C_N);
  if (r == hipSuccess && !R.spare_load) r = dalloc(e, &R.spare_load, words);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "cost-field routes: no device memory for the load planes (the previous load stays)");
  }
  unsigned long long h_ctl[CFR_C_N] = {};
  r = hipMemsetAsync(ctl, 0, sizeof(h_ctl), st);
  if (r == hipSuccess) r = hipMemsetAsync(R.spare_load, 0, words * sizeof(uint32_t), st);
  if (r == hipSuccess) r = hipMemcpyAsync(d_xy, start_xy, 2 * nn * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (r == hipSuccess && d_head) r = hipMemcpyAsync(d_head, start_heading, nn, hipMemcpyHostToDevice, st);
  if (r == hipSuccess && d_w) r = hipMemcpyAsync(d_w, weight, nn * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(k_cfr_load, dim3(nblk(n)), dim3(BLK), 0, st, cfr_plane(e), n, d_xy, d_head, d_w, R.spare_load, ctl);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) return fail(e, TS_E_DEVICE, std::string("cost-field routes: ") + hipGetErrorString(r));
  if (h_ctl[CFR_C_FAULT])
    return fail(e, TS_E_CAPACITY, "cost-field routes: a walk left the map or took more steps than there are states (nothing is published)");
  std::swap(R.load, R.spare_load);
  TsCfRouteLoadInfo& L = R.load_info;
  L.unreached = (int64_t)h_ctl[CFR_C_UNREACHED]; L.routes = (int64_t)n - L.unreached; L.steps = h_ctl[CFR_C_STEPS]; L.tick = R.tick;
  L.device_bytes = (uint64_t)words * sizeof(uint32_t);
  if (out) *out = L;
  return TS_OK;
}

int ts_cfroute_load_download(ts_handle e, int32_t dir, uint32_t* dst) {
  if (!e) return TS_E_INVALID;
  if (!dst) return fail(e, TS_E_INVALID, "cost-field routes: null pointer");
  if (dir < -1 || dir > 3) return fail(e, TS_E_INVALID, "cost-field routes: dir is -1 (the sum) or 0..3");
  const auto& R = e->cfr;
  if (!R.load) return fail(e, TS_E_STATE, "cost-field routes: no load has been computed");
  const size_t N = (size_t)e->N;
  if (dir >= 0) return read_back(e, dst, R.load + (size_t)dir * N, N * sizeof(uint32_t));
  Scratch S;   // what the call holds on the device besides the result
  uint32_t* sum = nullptr;
  HIPOK(S.get(&sum, N));
  hipLaunchKernelGGL(k_demand_sum4, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, R.load, e->N, sum);
  return read_back(e, dst, sum, N * sizeof(uint32_t));
}

int ts_cfroute_load_device(ts_handle e, int32_t dir, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "cost-field routes: null pointer");
  if (dir < 0 || dir > 3) return fail(e, TS_E_INVALID, "cost-field routes: dir is 0..3");
  if (!e->cfr.load) return fail(e, TS_E_STATE, "cost-field routes: no load has been computed");
  HIPOK(hipStreamSynchronize(e->stream));
  *ptr = (void*)(e->cfr.load + (size_t)dir * (size_t)e->N);
  return TS_OK;
}

int ts_cfroute_release(ts_handle e) {
  if (!e) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  cfr_drop(e);
  auto& R = e->cfr;
  dfree(e, R.off); dfree(e, R.dirs); dfree(e, R.cost); dfree(e, R.owner); dfree(e, R.starts);
  dfree(e, R.load); dfree(e, R.spare_load);
  R.off = nullptr; R.dirs = nullptr; R.cost = nullptr; R.owner = nullptr; R.starts = nullptr;
  R.load = R.spare_load = nullptr;
  R.batch = TsCfRouteBatch{};
  R.load_info = TsCfRouteLoadInfo{};
  return TS_OK;
}

}  // extern "C"
