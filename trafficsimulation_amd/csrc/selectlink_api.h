// selectlink_api.h - the ts_selectlink_* entries (include/trafficsim_selectlink.h): the host side of the select-link analysis
// whose kernels are in selectlink.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_selectlink.h"

namespace {

// lanes per vehicle and path steps per team iteration of k_selectlink_walk (profiles/selectlink_probe.py settled them: four
// steps per lane, where the demand walk with its atomic per step does best with one)
constexpr int SL_TEAM = 32, SL_CHUNK = 128, SL_CHUNK_MAX = 65536;
// bytes of a spawn index in the result's one allocation: five 32-bit arrays, first_gate, select
constexpr size_t SL_VEH_BYTES = 5 * 4 + 1 + 1;

// the arrays of a result of `cap` spawn indices inside its allocation: [mask][crossings] (preset 0), [first_step][pos][target]
// [first_gate] (preset -1), [select] (preset 0)
SlVeh sl_carve(uint8_t* buf, size_t cap) {
  SlVeh v;
  v.mask = (uint32_t*)buf; v.crossings = v.mask + cap;
  v.first_step = (int32_t*)(v.crossings + cap); v.pos = v.first_step + cap; v.target = v.pos + cap;
  v.first_gate = (int8_t*)(v.target + cap);
  v.select = (uint8_t*)(v.first_gate + cap);
  return v;
}

void sl_launch_walk(int team, int blocks, hipStream_t st, const SelectLinkArgs& a) {
  switch (team) {
    case 8: hipLaunchKernelGGL(k_selectlink_walk<8>, dim3(blocks), dim3(BLK), 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_selectlink_walk<16>, dim3(blocks), dim3(BLK), 0, st, a); break;
    case 64: hipLaunchKernelGGL(k_selectlink_walk<64>, dim3(blocks), dim3(BLK), 0, st, a); break;
    default: hipLaunchKernelGGL(k_selectlink_walk<32>, dim3(blocks), dim3(BLK), 0, st, a); break;
  }
}

void sl_drop_result(E* e) {
  auto& S = e->sl;
  S.held = false;
  S.n_bins = S.bin_cells = S.open_tail = S.n_spawned = 0;
  S.tick = 0;
  std::fill(S.tab.begin(), S.tab.end(), 0ull);
}

void sl_fill_info(const E* e, TsSelectLinkInfo* out) {
  const auto& S = e->sl;
  memset(out, 0, sizeof(*out));
  out->width = e->W; out->height = e->H;
  out->n_gates = S.n_gates; out->n_gate_cells = S.n_gate_cells; out->n_zones = S.n_zones;
  out->device_bytes = (S.gates ? (uint64_t)e->N * 4 : 0) + (S.buf ? (uint64_t)S.cap * SL_VEH_BYTES : 0) +
                      (S.d_tab ? (uint64_t)SL_NTAB * 8 : 0) + (S.zone ? (uint64_t)e->N * 4 : 0);
  if (!S.held) return;
  out->held = 1;
  out->n_bins = S.n_bins; out->bin_cells = S.bin_cells; out->open_tail = S.open_tail; out->n_spawned = S.n_spawned;
  out->tick = S.tick;
  out->vehicles = (int64_t)S.tab[SL_TOT + SL_T_VEH]; out->crossing = (int64_t)S.tab[SL_TOT + SL_T_CROSSING];
  out->crossings = S.tab[SL_TOT + SL_T_CROSSINGS];
}

// a read's preconditions: a result, and a selection inside its gates
int sl_need_result(E* e) {
  return e->sl.held ? TS_OK : fail(e, TS_E_STATE, "selectlink: nothing has been computed");
}
int sl_check_selection(E* e, uint32_t any, uint32_t all, uint32_t none) {
  const uint32_t known = e->sl.n_gates >= 32 ? 0xFFFFFFFFu : (1u << e->sl.n_gates) - 1u;
  if ((any | all | none) & ~known) return fail(e, TS_E_INVALID, "selectlink: a selection names a gate at or above n_gates");
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_selectlink_set_gates(ts_handle e, int32_t n_gates, const int32_t* gate_off, const int32_t* cells_xy, const uint8_t* dir_mask) {
  if (!e) return TS_E_INVALID;
  if (!gate_off || !cells_xy || !dir_mask) return fail(e, TS_E_INVALID, "selectlink: null pointer");
  if (n_gates < 1 || n_gates > TS_SL_MAX_GATES) return fail(e, TS_E_INVALID, "selectlink: n_gates outside 1..32");
  if (gate_off[0] != 0) return fail(e, TS_E_INVALID, "selectlink: gate_off must start at 0");
  for (int g = 0; g < n_gates; g++) {
    if (gate_off[g + 1] <= gate_off[g]) return fail(e, TS_E_INVALID, "selectlink: gate_off is not monotone, or a gate is empty");
    if (gate_off[g + 1] > TS_SL_MAX_CELLS) return fail(e, TS_E_INVALID, "selectlink: more than 2^20 gate cells");
  }
  const int n = gate_off[n_gates];
  // one (cell, word) per gate cell for the scatter, and the sorted (cell, direction) keys that show a pair claimed twice
  std::vector<int32_t> cell((size_t)n);
  std::vector<uint32_t> word((size_t)n);
  std::vector<uint64_t> keys;
  keys.reserve((size_t)n * 2);
  for (int g = 0, k = 0; g < n_gates; g++)
    for (; k < gate_off[g + 1]; k++) {
      const int x = cells_xy[2 * (size_t)k], y = cells_xy[2 * (size_t)k + 1], dm = dir_mask[k];
      if (x < 0 || x >= e->W || y < 0 || y >= e->H) return fail(e, TS_E_INVALID, "selectlink: a gate cell outside the map");
      if (dm < 1 || dm > TS_SL_DIR_ALL) return fail(e, TS_E_INVALID, "selectlink: a direction mask of 0 or above 15");
      cell[k] = y * e->W + x;
      word[k] = 0;
      for (int d = 0; d < 4; d++)
        if ((dm >> d) & 1) { word[k] |= (uint32_t)(g + 1) << (8 * d); keys.push_back((uint64_t)cell[k] * 4 + d); }
    }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
    return fail(e, TS_E_INVALID, "selectlink: a (cell, direction) is claimed twice");
  if (e->fatal) return e->fatal;
  auto& S = e->sl;
  // the plane held is rebuilt in place: from here on only a broken device can fail the call
  const bool had_plane = S.gates != nullptr;
  Scratch tmp;
  int32_t* d_cell = nullptr;
  uint32_t* d_word = nullptr;
  if (tmp.get(&d_cell, (size_t)n) != hipSuccess || tmp.get(&d_word, (size_t)n) != hipSuccess ||
      (!had_plane && dalloc(e, &S.gates, (size_t)e->N) != hipSuccess)) {
    (void)hipGetLastError();
    if (!had_plane) S.gates = nullptr;
    return fail(e, TS_E_DEVICE, "selectlink: no device memory for the gate plane (the previous gates stay)");
  }
  hipStream_t st = e->stream;
  hipError_t r = hipMemsetAsync(S.gates, 0, (size_t)e->N * 4, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d_cell, cell.data(), (size_t)n * 4, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(d_word, word.data(), (size_t)n * 4, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(k_selectlink_scatter, dim3(nblk((long long)n)), dim3(BLK), 0, st, n, d_cell, d_word, S.gates);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  sl_drop_result(e);
  if (r != hipSuccess) {   // the device failed under an accepted call: the plane holds nothing usable any more
    dfree(e, S.gates);
    S.gates = nullptr; S.n_gates = S.n_gate_cells = 0;
    return fail(e, TS_E_DEVICE, std::string("selectlink: ") + hipGetErrorString(r));
  }
  S.n_gates = n_gates; S.n_gate_cells = n;
  return TS_OK;
}

int ts_selectlink_compute(ts_handle e, const TsSelectLinkQuery* q, TsSelectLinkInfo* out) {
  if (!e) return TS_E_INVALID;
  if (!q) return fail(e, TS_E_INVALID, "selectlink: null pointer");
  if (q->n_bins < 1 || q->n_bins > TS_DEMAND_MAX_BINS) return fail(e, TS_E_INVALID, "selectlink: n_bins outside 1..8");
  if (q->bin_cells < 1) return fail(e, TS_E_INVALID, "selectlink: bin_cells must be at least 1");
  if ((q->open_tail | 1) != 1 || q->reserved != 0) return fail(e, TS_E_INVALID, "selectlink: open_tail is 0 or 1, reserved is 0");
  auto& S = e->sl;
  if (!S.gates) return fail(e, TS_E_STATE, "selectlink: no gates are set");
  if (e->fatal) return e->fatal;
  // the walk's shape, as ts_demand_compute reads its own
  int team = SL_TEAM, chunk = SL_CHUNK;
  if (const char* s = getenv("TS_DEBUG_SELECTLINK_TEAM")) { const int v = atoi(s); if (v == 8 || v == 16 || v == 32 || v == 64) team = v; }
  if (const char* s = getenv("TS_DEBUG_SELECTLINK_CHUNK")) chunk = std::min(std::max(atoi(s), 1), SL_CHUNK_MAX);
  if (!S.cus) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 64; }
    S.cus = cus;
  }
  // Everything this call needs is allocated before anything of the previous result goes.  Arrays large enough are written in
  // place: by then nothing is left that could refuse the call.
  const size_t n = (size_t)e->n_vehicles_total;
  const bool in_place = S.buf && S.cap >= n;
  const size_t cap = in_place ? S.cap : std::max<size_t>(n, 1);
  uint8_t* buf = in_place ? S.buf : nullptr;
  if (!S.d_tab && dalloc(e, &S.d_tab, (size_t)SL_NTAB) != hipSuccess) {
    (void)hipGetLastError();
    S.d_tab = nullptr;
    return fail(e, TS_E_DEVICE, "selectlink: no device memory for the tables");
  }
  if (!in_place && dalloc(e, &buf, cap * SL_VEH_BYTES) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, TS_E_DEVICE, "selectlink: no device memory for the per-vehicle arrays (the previous result stays)");
  }
  S.tab.resize(SL_NTAB);
  SelectLinkArgs a{};
  const Dev& d = e->d;
  a.W = e->W; a.N = e->N; a.n_active = e->n_active; a.n_vehicles = e->n_vehicles_total;
  a.active = d.active; a.pos = d.pos; a.target = d.target; a.path_len = d.path_len; a.path_cur = d.path_cur;
  a.path_off = d.path_off; a.pool = d.pool;
  a.gates = S.gates; a.v = sl_carve(buf, cap); a.tab = S.d_tab;
  a.n_bins = q->n_bins; a.bin_cells = q->bin_cells; a.open_tail = q->open_tail;
  a.limit = (int)std::min<long long>((long long)q->n_bins * q->bin_cells, 0x7FFFFFFF);
  a.spl = (chunk + team - 1) / team;
  std::vector<unsigned long long> tab((size_t)SL_NTAB);
  hipStream_t st = e->stream;
  hipError_t r = hipMemsetAsync(a.v.mask, 0, cap * 8, st);
  if (r == hipSuccess) r = hipMemsetAsync(a.v.first_step, 0xFF, cap * 13, st);
  if (r == hipSuccess) r = hipMemsetAsync(a.v.select, 0, cap, st);
  if (r == hipSuccess) r = hipMemsetAsync(S.d_tab, 0, (size_t)SL_NTAB * 8, st);
  if (r == hipSuccess && a.n_active > 0) {
    // whole waves of 64 / team vehicles; no more blocks than keep every CU full, each wave strides over the list
    const long long waves = ((long long)a.n_active + 64 / team - 1) / (64 / team);
    const int blocks = (int)std::min<long long>((waves + BLK / 64 - 1) / (BLK / 64), (long long)S.cus * 8);
    sl_launch_walk(team, blocks, st, a);
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipMemcpyAsync(tab.data(), S.d_tab, (size_t)SL_NTAB * 8, hipMemcpyDeviceToHost, st);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) {   // the device failed under an accepted call: arrays written in place hold nothing usable any more
    dfree(e, buf);
    if (in_place) { S.buf = nullptr; S.cap = 0; sl_drop_result(e); }
    return fail(e, TS_E_DEVICE, std::string("selectlink: ") + hipGetErrorString(r));
  }
  if (!in_place) { dfree(e, S.buf); S.buf = buf; S.cap = cap; }
  S.held = true;
  S.n_bins = q->n_bins; S.bin_cells = q->bin_cells; S.open_tail = q->open_tail; S.n_spawned = e->n_vehicles_total;
  S.tick = e->C.step_count;
  for (int k = 0; k < SL_NTAB; k++) S.tab[k] = tab[k];
  if (out) sl_fill_info(e, out);
  return TS_OK;
}

int ts_selectlink_info(ts_handle e, TsSelectLinkInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  sl_fill_info(e, out);
  return TS_OK;
}

int ts_selectlink_tables(ts_handle e, uint64_t* cross, uint64_t* pair) {
  if (!e) return TS_E_INVALID;
  TRY(sl_need_result(e));
  const auto& S = e->sl;   // (the walk's tables came to the host with the compute)
  if (cross)
    for (int g = 0; g < S.n_gates; g++)
      for (int k = 0; k < S.n_bins * 4; k++) cross[((size_t)g * S.n_bins) * 4 + k] = S.tab[SL_CROSS + g * TS_DEMAND_MAX_BINS * 4 + k];
  if (pair)
    for (int g = 0; g < S.n_gates; g++)
      for (int b = 0; b < S.n_gates; b++) pair[(size_t)g * S.n_gates + b] = S.tab[SL_PAIR + g * SL_G + b];
  return TS_OK;
}

int ts_selectlink_vehicles(ts_handle e, int32_t first, int32_t n, uint32_t* mask, int32_t* first_step, int8_t* first_gate, uint32_t* crossings) {
  if (!e) return TS_E_INVALID;
  TRY(sl_need_result(e));
  const auto& S = e->sl;
  if (first < 0 || n < 0 || (long long)first + n > S.n_spawned) return fail(e, TS_E_INVALID, "selectlink: range outside the spawn indices of the compute");
  if (n == 0) return TS_OK;
  const SlVeh v = sl_carve(S.buf, S.cap);
  hipStream_t st = e->stream;
  if (mask) HIPOK(hipMemcpyAsync(mask, v.mask + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (first_step) HIPOK(hipMemcpyAsync(first_step, v.first_step + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (first_gate) HIPOK(hipMemcpyAsync(first_gate, v.first_gate + first, (size_t)n, hipMemcpyDeviceToHost, st));
  if (crossings) HIPOK(hipMemcpyAsync(crossings, v.crossings + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  return TS_OK;
}

int ts_selectlink_select(ts_handle e, uint32_t any, uint32_t all, uint32_t none, uint8_t* dst, int64_t* count) {
  if (!e) return TS_E_INVALID;
  TRY(sl_need_result(e));
  TRY(sl_check_selection(e, any, all, none));
  const auto& S = e->sl;
  const SlVeh v = sl_carve(S.buf, S.cap);
  Scratch tmp;
  unsigned long long *d_count = nullptr, got = 0;
  HIPOK(tmp.get(&d_count, 1));
  HIPOK(hipMemsetAsync(d_count, 0, 8, e->stream));
  if (S.n_spawned > 0) {
    hipLaunchKernelGGL(k_selectlink_select, dim3(nblk((long long)S.n_spawned)), dim3(BLK), 0, e->stream, v, S.n_spawned, any, all, none, d_count);
    HIPOK(hipGetLastError());
    if (dst) HIPOK(hipMemcpyAsync(dst, v.select, (size_t)S.n_spawned, hipMemcpyDeviceToHost, e->stream));
  }
  TRY(read_back(e, &got, d_count, 8));
  if (count) *count = (int64_t)got;
  return TS_OK;
}

int ts_selectlink_set_zones(ts_handle e, const int32_t* zone_of_cell, int32_t n_zones) {
  if (!e) return TS_E_INVALID;
  if (n_zones < 0 || n_zones > TS_SL_MAX_ZONES) return fail(e, TS_E_INVALID, "selectlink: n_zones out of range (0 .. 1024)");
  if (n_zones > 0 && !zone_of_cell) return fail(e, TS_E_INVALID, "selectlink: null pointer");
  auto& S = e->sl;
  HIPOK(hipStreamSynchronize(e->stream));
  if (n_zones == 0) {
    dfree(e, S.zone);
    S.zone = nullptr;
  } else {
    if (!S.zone && dalloc(e, &S.zone, (size_t)e->N) != hipSuccess) {
      (void)hipGetLastError();
      S.zone = nullptr;
      return fail(e, TS_E_DEVICE, "selectlink: no device memory for the zone plane");
    }
    HIPOK(hipMemcpy(S.zone, zone_of_cell, (size_t)e->N * 4, hipMemcpyHostToDevice));
  }
  S.n_zones = n_zones;
  return TS_OK;
}

int ts_selectlink_od(ts_handle e, uint32_t any, uint32_t all, uint32_t none, int64_t* counts, int64_t* unzoned) {
  if (!e) return TS_E_INVALID;
  if (!counts) return fail(e, TS_E_INVALID, "selectlink: null pointer");
  TRY(sl_need_result(e));
  const auto& S = e->sl;
  if (!S.zone) return fail(e, TS_E_STATE, "selectlink: no zone plane is set");
  TRY(sl_check_selection(e, any, all, none));
  const size_t nz2 = (size_t)S.n_zones * S.n_zones;
  Scratch tmp;
  unsigned long long* buf = nullptr;   // the matrix, then the unzoned counter
  HIPOK(tmp.get(&buf, nz2 + 1));
  HIPOK(hipMemsetAsync(buf, 0, (nz2 + 1) * 8, e->stream));
  if (S.n_spawned > 0) {
    hipLaunchKernelGGL(k_selectlink_od, dim3(nblk((long long)S.n_spawned)), dim3(BLK), 0, e->stream, sl_carve(S.buf, S.cap), S.n_spawned,
                       any, all, none, S.zone, S.n_zones, e->N, buf);
    HIPOK(hipGetLastError());
  }
  HIPOK(hipMemcpyAsync(counts, buf, nz2 * 8, hipMemcpyDeviceToHost, e->stream));
  if (unzoned) HIPOK(hipMemcpyAsync(unzoned, buf + nz2, 8, hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_selectlink_device(ts_handle e, int32_t which, void** ptr) {
  if (!e) return TS_E_INVALID;
  if (!ptr) return fail(e, TS_E_INVALID, "selectlink: null pointer");
  if (which < TS_SL_MASK || which > TS_SL_GATES) return fail(e, TS_E_INVALID, "selectlink: `which` out of range");
  const auto& S = e->sl;
  if (which == TS_SL_GATES) {
    if (!S.gates) return fail(e, TS_E_STATE, "selectlink: no gates are set");
  } else TRY(sl_need_result(e));
  HIPOK(hipStreamSynchronize(e->stream));
  const SlVeh v = sl_carve(S.buf, S.cap);
  *ptr = which == TS_SL_GATES ? (void*)S.gates : which == TS_SL_MASK ? (void*)v.mask : which == TS_SL_FIRST_STEP ? (void*)v.first_step
       : which == TS_SL_FIRST_GATE ? (void*)v.first_gate : which == TS_SL_CROSSINGS ? (void*)v.crossings : (void*)v.select;
  return TS_OK;
}

int ts_selectlink_release(ts_handle e) {
  if (!e) return TS_E_INVALID;
  auto& S = e->sl;
  HIPOK(hipStreamSynchronize(e->stream));
  dfree(e, S.gates); dfree(e, S.buf); dfree(e, S.d_tab); dfree(e, S.zone);
  S.gates = nullptr; S.buf = nullptr; S.d_tab = nullptr; S.zone = nullptr;
  S.cap = 0; S.n_gates = S.n_gate_cells = S.n_zones = 0;
  sl_drop_result(e);
  return TS_OK;
}

}  // extern "C"
