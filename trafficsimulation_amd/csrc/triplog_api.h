// triplog_api.h - the ts_triplog_* entries (include/trafficsim_triplog.h): the host side of the trip log whose hooks and
// kernels are in triplog.h.  Part of the single translation unit engine.hip (included at its end).
#pragma once
#include "../../include/trafficsim_triplog.h"

static_assert(sizeof(TsTripRecord) == 72 && offsetof(TsTripRecord, depart_elapsed) == 56, "TsTripRecord is 72 bytes without padding");

namespace {

// the pointer part of the device struct <- the host's copy
int tl_upload(E* e) {
  HIPOK(hipMemcpyAsync(e->d.tlog, &e->tl, TL_HOST_PART, hipMemcpyHostToDevice, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

size_t tl_bitmap_words(size_t vehicles) { return vehicles / 32 + 1; }

void tl_free(E* e) {
  TripLog& t = e->tl;
  void* ptrs[] = {t.origin, t.spawn_step, t.end_step, t.end_elapsed, t.vtype, t.end_reason, t.staged, t.bitmap, t.rec,
                  e->tl_zone, e->tl_bsum, e->d.tlog};
  for (void* p : ptrs) dfree(e, p);
  t = TripLog{};
  e->tl_zone = nullptr; e->tl_bsum = nullptr; e->tl_cap_bsum = 0;
  e->d.tlog = nullptr;
  e->tl_on = false;
  e->tl_pending = 0;
}

int tl_zero_counters(E* e) {
  HIPOK(hipMemsetAsync((uint8_t*)e->d.tlog + TL_HOST_PART, 0, sizeof(TripLog) - TL_HOST_PART, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  e->tl_pending = 0;
  return TS_OK;
}

// the log's device counters, after sealing what is staged
int tl_counters(E* e, TripLog* out) {
  TRY(tl_seal(e));
  return read_back(e, out, e->d.tlog, sizeof(TripLog));
}

}  // namespace

// every vehicle id handed out so far: placed before the log could see it.  The service types come from the host's fleet.
static int tl_forget_origins(ts_handle e) {
  TripLog& t = e->tl;
  const size_t nv = (size_t)e->n_vehicles_total;
  if (nv) {
    HIPOK(hipMemsetAsync(t.origin, 0xFF, nv * 4, e->stream));
    HIPOK(hipMemsetAsync(t.spawn_step, 0xFF, nv * 4, e->stream));
    HIPOK(hipMemsetAsync(t.vtype, 0, nv, e->stream));
  }
  HIPOK(hipStreamSynchronize(e->stream));
  for (const auto& v : e->svc) {
    const int8_t ty = (int8_t)v.type;
    if (v.vid >= 0 && (size_t)v.vid < nv) HIPOK(hipMemcpy(t.vtype + v.vid, &ty, 1, hipMemcpyHostToDevice));
  }
  return TS_OK;
}

// the per-vehicle arrays, the staging list and the bitmap for `nc` vehicle ids; the first `keep` ids are in use
static int tl_grow(ts_handle e, size_t keep, size_t nc) {
  TripLog& t = e->tl;
  TRY(regrow(e, &t.origin, keep, nc)); TRY(regrow(e, &t.spawn_step, keep, nc)); TRY(regrow(e, &t.end_step, keep, nc));
  TRY(regrow(e, &t.end_elapsed, keep, nc)); TRY(regrow(e, &t.vtype, keep, nc)); TRY(regrow(e, &t.end_reason, keep, nc));
  TRY(regrow(e, &t.staged, (size_t)t.staged_cap, nc));   // (a spawn in the middle of a tick: removals may be staged)
  // the bitmap is all zero outside a seal
  TRY(regrow(e, &t.bitmap, 0, tl_bitmap_words(nc)));
  HIPOK(hipMemsetAsync(t.bitmap, 0, tl_bitmap_words(nc) * 4, e->stream));
  t.staged_cap = (int)nc;
  const int nb = nblk((long long)tl_bitmap_words(nc), e->tl_wpb) + 1;
  TRY(grow(e, &e->tl_bsum, e->tl_cap_bsum, (size_t)nb, (size_t)nb));
  return tl_upload(e);
}

// staged removals -> one group of records in ascending vehicle id (triplog.h).  Nothing staged: nothing changes.
static int tl_seal(ts_handle e) {
  if (!e->d.tlog) return TS_OK;
  hipStream_t st = e->stream;
  const int n_words = (int)tl_bitmap_words((size_t)e->n_vehicles_total);
  const int wpb = e->tl_wpb, nb = nblk(n_words, wpb);
  hipLaunchKernelGGL(k_tl_mark, dim3(std::min(std::max(nblk(e->tl_pending), 1), 1024)), dim3(BLK), 0, st, e->d.tlog);
  hipLaunchKernelGGL(k_tl_count, dim3(nb), dim3(BLK), 0, st, e->d.tlog, n_words, wpb, e->tl_bsum);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, st, e->tl_bsum, nb, e->d_total);
  hipLaunchKernelGGL(k_tl_emit, dim3(nb), dim3(BLK), 0, st, e->d, n_words, wpb, e->tl_bsum);
  hipLaunchKernelGGL(k_tl_finish, dim3(1), dim3(64), 0, st, e->d.tlog);
  HIPOK(hipGetLastError());
  e->tl_pending = 0;
  return TS_OK;
}

extern "C" {

int ts_triplog_start(ts_handle e, int64_t capacity_records) {
  if (!e) return TS_E_INVALID;
  if (capacity_records < 1) return fail(e, TS_E_INVALID, "triplog: capacity < 1");
  HIPOK(hipStreamSynchronize(e->stream));
  tl_free(e);
  auto nomem = [&]() {
    (void)hipGetLastError();
    tl_free(e);
    return fail(e, TS_E_DEVICE, "triplog: no device memory for the log (the log is off)");
  };
  if ((uint64_t)capacity_records > (1ull << 40) / sizeof(TsTripRecord)) return nomem();
  TripLog& t = e->tl;
  if (dalloc(e, &e->d.tlog, 1) != hipSuccess) return nomem();
  if (dalloc(e, &t.rec, (size_t)capacity_records) != hipSuccess) return nomem();
  t.capacity = capacity_records;
  const char* dbg = getenv("TS_DEBUG_TRIPLOG_BLOCK");   // bitmap words per block of the seal (tests: many blocks on a small map)
  e->tl_wpb = dbg ? std::min(std::max(atoi(dbg), 1), TL_WORDS) : TL_WORDS;
  e->tl_on = true;
  if (tl_grow(e, 0, (size_t)std::max(e->cap_v, 1)) != TS_OK || tl_zero_counters(e) != TS_OK || tl_forget_origins(e) != TS_OK) return nomem();
  return TS_OK;
}

int ts_triplog_stop(ts_handle e) {
  if (!e) return TS_E_INVALID;
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  HIPOK(hipStreamSynchronize(e->stream));
  tl_free(e);
  return TS_OK;
}

int ts_triplog_clear(ts_handle e) {
  if (!e) return TS_E_INVALID;
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  return tl_zero_counters(e);
}

int ts_triplog_info(ts_handle e, TsTripLogInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  memset(out, 0, sizeof(*out));
  if (!e->tl_on) return TS_OK;
  TripLog c;
  TRY(tl_counters(e, &c));
  out->capacity = c.capacity; out->count = c.count; out->dropped = c.dropped; out->groups = c.groups;
  const uint64_t nv = (uint64_t)e->tl.staged_cap;
  out->device_bytes = sizeof(TripLog) + (uint64_t)c.capacity * sizeof(TsTripRecord) + nv * (3 * 4 + 8 + 2 + 4) +
                      tl_bitmap_words(nv) * 4 + (uint64_t)e->tl_cap_bsum * 4 + (e->tl_zone ? (uint64_t)e->N * 4 : 0);
  return TS_OK;
}

int64_t ts_triplog_read(ts_handle e, int64_t first, int64_t n, TsTripRecord* out) {
  if (!e) return TS_E_INVALID;
  if (first < 0 || n < 0 || (n > 0 && !out)) return fail(e, TS_E_INVALID, "triplog: negative range or null pointer");
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  TripLog c;
  TRY(tl_counters(e, &c));
  const int64_t k = std::max<int64_t>(0, std::min<int64_t>(n, c.count - first));
  if (k > 0) TRY(read_back(e, out, e->tl.rec + first, (size_t)k * sizeof(TsTripRecord)));
  return k;
}

int ts_triplog_device(ts_handle e, void** ptr, int64_t* count) {
  if (!e) return TS_E_INVALID;
  if (!ptr || !count) return fail(e, TS_E_INVALID, "triplog: null pointer");
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  TripLog c;
  TRY(tl_counters(e, &c));   // (waits for the stream)
  *ptr = (void*)e->tl.rec;
  *count = c.count;
  return TS_OK;
}

int ts_triplog_set_zones(ts_handle e, const int32_t* zone_of_cell, int32_t n_zones) {
  if (!e) return TS_E_INVALID;
  if (n_zones < 0 || n_zones > TS_TRIPLOG_MAX_ZONES) return fail(e, TS_E_INVALID, "triplog: n_zones out of range (0 .. 1024)");
  if (n_zones > 0 && !zone_of_cell) return fail(e, TS_E_INVALID, "triplog: null pointer");
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  HIPOK(hipStreamSynchronize(e->stream));
  if (n_zones == 0) {
    dfree(e, e->tl_zone);
    e->tl_zone = nullptr;
  } else {
    if (!e->tl_zone && dalloc(e, &e->tl_zone, (size_t)e->N) != hipSuccess) {
      (void)hipGetLastError();
      e->tl_zone = nullptr;
      return fail(e, TS_E_DEVICE, "triplog: no device memory for the zone plane");
    }
    HIPOK(hipMemcpy(e->tl_zone, zone_of_cell, (size_t)e->N * 4, hipMemcpyHostToDevice));
  }
  e->tl.zone = e->tl_zone;
  e->tl.n_zones = n_zones;
  return tl_upload(e);
}

int ts_triplog_od(ts_handle e, uint32_t reason_mask, uint64_t* count, double* duration, uint64_t* distance, uint64_t* unzoned) {
  if (!e) return TS_E_INVALID;
  if (!unzoned || (reason_mask & ~TS_TRIP_END_ALL)) return fail(e, TS_E_INVALID, "triplog: null pointer or a reason that does not exist");
  if (!e->tl_on) return fail(e, TS_E_STATE, "triplog: the log has not been started");
  if (!e->tl_zone) return fail(e, TS_E_STATE, "triplog: no zone plane is set");
  TripLog c;
  TRY(tl_counters(e, &c));
  const size_t nz2 = (size_t)e->tl.n_zones * e->tl.n_zones;
  Scratch tmp;
  unsigned long long* buf = nullptr;   // count, duration, distance, then the unzoned counter
  HIPOK(tmp.get(&buf, 3 * nz2 + 1));
  HIPOK(hipMemsetAsync(buf, 0, (3 * nz2 + 1) * 8, e->stream));   // (all-zero bits are 0.0 too)
  if (c.count > 0) {
    hipLaunchKernelGGL(k_triplog_od, dim3(nblk(c.count)), dim3(BLK), 0, e->stream, e->d, c.count, reason_mask, count ? buf : nullptr,
                       duration ? (double*)(buf + nz2) : nullptr, distance ? buf + 2 * nz2 : nullptr, buf + 3 * nz2);
    HIPOK(hipGetLastError());
  }
  if (count) HIPOK(hipMemcpyAsync(count, buf, nz2 * 8, hipMemcpyDeviceToHost, e->stream));
  if (duration) HIPOK(hipMemcpyAsync(duration, buf + nz2, nz2 * 8, hipMemcpyDeviceToHost, e->stream));
  if (distance) HIPOK(hipMemcpyAsync(distance, buf + 2 * nz2, nz2 * 8, hipMemcpyDeviceToHost, e->stream));
  return read_back(e, unzoned, buf + 3 * nz2, 8);
}

}  // extern "C"
