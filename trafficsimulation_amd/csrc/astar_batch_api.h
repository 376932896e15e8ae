// astar_batch_api.h - ts_astar_batch / _fetch / _device (include/trafficsim_astar_batch.h): the host side of the query batches
// whose kernels are in astar_batch.h.  Part of the single translation unit engine.hip (included at its end, after the C-ABI
// entries whose helpers it reuses).
#pragma once
#include <climits>
#include "../../include/trafficsim_astar_batch.h"

namespace {

// one launch of k_astar_batch over `n_run` entries of B.order, bookkeeping read back into `out`
int batch_launch(E* e, int n_run, int usable, unsigned long long stage_start, BatchCtl& out) {
  E::Batch& B = e->batch;
  hipStream_t st = e->stream;
  BatchCtl c0{};
  c0.first_bad = INT_MAX;
  c0.stage_used = stage_start;
  HIPOK(hipMemcpyAsync(B.ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, st));
  HIPOK(hipStreamSynchronize(st));      // (c0 is on this frame)
  BatchQ q;
  q.q = B.q; q.order = B.order; q.n_run = n_run; q.len = B.len; q.soff = B.soff; q.stage = B.stage;
  q.stage_cap = B.cap_stage; q.retry = B.retry; q.ctl = B.ctl;
  const int grid = std::min(n_run, usable);
  B.last_waves = std::max(B.last_waves, grid);
  B.last_passes++;
  if (g_trace_launches) { fprintf(stderr, "[launch] k_astar_batch queries=%d waves=%d\n", n_run, grid); fflush(stderr); }
  hipLaunchKernelGGL(k_astar_batch, dim3(grid), dim3(64), 0, st, e->d, e->P, e->slots, q);
  return read_back(e, &out, B.ctl, sizeof(out));
}

}  // namespace

extern "C" {

int ts_astar_batch(ts_handle e, int32_t n, const int32_t* queries, int64_t* total_cells) {
  if (!e) return TS_E_INVALID;
  if (n < 0 || !total_cells || (n > 0 && !queries)) return fail(e, TS_E_INVALID, "astar batch: negative count or null pointer");
  for (int i = 0; i < n; i++) {
    const int32_t* a = queries + (size_t)i * TS_ASTAR_QUERY_INTS;
    if (a[0] < 0 || a[0] >= e->W || a[1] < 0 || a[1] >= e->H || a[2] < 0 || a[2] >= e->W || a[3] < 0 || a[3] >= e->H)
      return fail(e, TS_E_INVALID, "astar endpoints out of bounds (query " + std::to_string(i) + ")");
    if (a[6] < e->N && a[6] > A_STEPS_MAX)
      return fail(e, TS_E_UNSUPPORTED, "a binding maximum_steps above 4094 is not carried (use >= width * height for 'unlimited') (query " +
                                           std::to_string(i) + ")");
  }
  E::Batch& B = e->batch;
  hipStream_t st = e->stream;
  B.valid = false;
  const size_t nn = (size_t)n;
  if (nn > B.cap_q) {
    const size_t nc = nn * 2 + 256;
    TRY(regrow(e, &B.q, 0, nc * TS_ASTAR_QUERY_INTS));
    TRY(regrow(e, &B.order, 0, nc));
    TRY(regrow(e, &B.retry, 0, nc));
    TRY(regrow(e, &B.len, 0, nc));
    TRY(regrow(e, &B.soff, 0, nc));
    B.cap_q = nc;
  }
  if (nn + 1 > B.cap_off) {
    const size_t nc = nn * 2 + 256;
    TRY(regrow(e, &B.len64, 0, nc));
    TRY(regrow(e, &B.off, 0, nc));
    B.cap_off = nc;
  }
  if (!B.ctl) HIPOK(dalloc(e, &B.ctl, 1));
  if (!B.xy) { HIPOK(dalloc(e, &B.xy, 2)); B.cap_xy = 1; }
  if (n == 0) {
    HIPOK(hipMemsetAsync(B.off, 0, sizeof(long long), st));
    HIPOK(hipStreamSynchronize(st));
    B.n = 0; B.total = 0; B.valid = true;
    *total_cells = 0;
    return TS_OK;
  }
  // "evaluated on the engine's current maps": density planes and snapshot once for the whole batch, dropped afterwards (ts_astar)
  TRY(search_maps_now(e));
  // While the quads hold the shared part of the table arena only the side waves' slots are usable: a query batch never
  // clears or moves the arena (and so never touches the quads' tables or epochs)
  const int usable = (e->arena_shared && e->arena_quad) ? std::max(1, std::min(e->side_slots, e->slots.n_slots)) : e->slots.n_slots;
  HIPOK(hipMemcpyAsync(B.q, queries, nn * TS_ASTAR_QUERY_INTS * 4, hipMemcpyHostToDevice, st));
  B.last_waves = 0; B.last_passes = 0; B.last_usable = usable; B.last_arena_quad = (e->arena_shared && e->arena_quad) ? 1 : 0;
  // order of service (k_batch_keys); short queues are served as they come
  if (n >= 256) {
    if (nn > e->cap_sortbuf) {
      const size_t nc = nn * 2;
      TRY(regrow(e, &e->sort_keys, 0, nc * 2));
      TRY(regrow(e, &e->sort_keys_alt, 0, nc * 2));
      TRY(regrow(e, &e->sort_vals_alt, 0, nc));
      e->cap_sortbuf = nc;
    }
    hipLaunchKernelGGL(k_batch_keys, dim3(nblk(n)), dim3(BLK), 0, st, B.q, n, e->sort_keys, B.retry);
    auto sort = [&](void* tmp, size_t& tmp_bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, e->sort_keys, e->sort_keys_alt, B.retry, B.order, n, 0, BATCH_KEY_BITS, st);
    };
    size_t tmp_bytes = 0;
    HIPOK(sort(nullptr, tmp_bytes));
    TRY(grow(e, &e->sort_tmp, e->cap_sorttmp, tmp_bytes, tmp_bytes * 2));
    HIPOK(sort(e->sort_tmp, tmp_bytes));
  } else {
    hipLaunchKernelGGL(k_batch_iota, dim3(nblk(n)), dim3(BLK), 0, st, B.order, n);
  }
  // staging arena: a guess that is grown when it was too small (TS_DEBUG_BATCH_STAGE: a test's way to a small first guess)
  {
    const char* dbg = getenv("TS_DEBUG_BATCH_STAGE");
    const size_t want = dbg ? (size_t)std::max(1, atoi(dbg)) : nn * 256 + 65536;
    // (the debugging size is this batch's first guess every time, whatever an earlier batch grew the arena to)
    if (B.cap_stage == 0 || (dbg ? want != B.cap_stage : want > B.cap_stage)) { TRY(regrow(e, &B.stage, 0, want)); B.cap_stage = want; }
  }
  int n_run = n;
  unsigned long long stage_start = 0;
  for (int pass = 0;; pass++) {
    BatchCtl c;
    TRY(batch_launch(e, n_run, usable, stage_start, c));
    if (c.first_bad != INT_MAX)
      return fail(e, TS_E_CAPACITY, "an A* search exceeded its heap or path buffers (query " + std::to_string(c.first_bad) + ")");
    if (c.n_retry == 0) break;
    if (pass >= 4) return fail(e, TS_E_DEVICE, "astar batch: the staging arena kept overflowing (internal error)");
    // paths that found the arena full: those that fit stay where they are (below the old capacity), the arena grows by what
    // the others asked for - every one of them starts above (old capacity - longest path) - and only they are queued again
    const size_t old_cap = B.cap_stage;
    const size_t nc = (size_t)c.stage_used + (size_t)e->slots.cap + 64;
    TRY(regrow(e, &B.stage, old_cap, nc));
    B.cap_stage = nc;
    HIPOK(hipMemcpyAsync(B.order, B.retry, (size_t)c.n_retry * 4, hipMemcpyDeviceToDevice, st));
    n_run = c.n_retry;
    stage_start = old_cap;
  }
  // CSR offsets, then the (x, y) pairs in query order
  hipLaunchKernelGGL(k_batch_lens, dim3(nblk((long long)n + 1)), dim3(BLK), 0, st, B.len, n, B.len64);
  {
    size_t tmp_bytes = 0;
    HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, B.len64, B.off, n + 1, st));
    TRY(grow(e, &B.scan_tmp, B.cap_scan, tmp_bytes, tmp_bytes * 2));
    HIPOK(hipcub::DeviceScan::ExclusiveSum(B.scan_tmp, tmp_bytes, B.len64, B.off, n + 1, st));
  }
  long long total = 0;
  TRY(read_back(e, &total, B.off + n, sizeof(total)));
  if ((size_t)total > B.cap_xy) {
    const size_t nc = (size_t)total + (size_t)total / 2 + 1024;
    TRY(regrow(e, &B.xy, 0, nc * 2));
    B.cap_xy = nc;
  }
  if (total > 0)
    hipLaunchKernelGGL(k_batch_gather, dim3(nblk((long long)n * 64)), dim3(BLK), 0, st, e->d, n, B.len, B.soff, B.stage, B.off, B.xy);
  HIPOK(hipStreamSynchronize(st));
  B.n = n; B.total = total; B.valid = true;
  *total_cells = total;
  return TS_OK;
}

int ts_astar_batch_fetch(ts_handle e, int64_t* off, int32_t* xy) {
  if (!e) return TS_E_INVALID;
  const E::Batch& B = e->batch;
  if (!B.valid) return fail(e, TS_E_INVALID, "no query batch result to fetch (none was run, or the engine has changed since)");
  if (!off || (!xy && B.total > 0)) return fail(e, TS_E_INVALID, "astar batch fetch: null pointer");
  HIPOK(hipMemcpyAsync(off, B.off, ((size_t)B.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
  if (B.total > 0) HIPOK(hipMemcpyAsync(xy, B.xy, (size_t)B.total * 8, hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_astar_batch_device(ts_handle e, const int64_t** d_off, const int32_t** d_xy, int32_t* n, int64_t* total_cells) {
  if (!e) return TS_E_INVALID;
  const E::Batch& B = e->batch;
  if (!B.valid) return fail(e, TS_E_INVALID, "no query batch result to hand out (none was run, or the engine has changed since)");
  if (d_off) *d_off = (const int64_t*)B.off;
  if (d_xy) *d_xy = B.xy;
  if (n) *n = B.n;
  if (total_cells) *total_cells = B.total;
  return TS_OK;
}

// debugging hook (not part of the headers under include/): what the searcher slots look like and what the last query batch ran
// on, as int32 - [0] searcher slots, [1] slots that stay k_replan's while the quads hold the shared table arena, [2] the
// quads' tables alias the arena, [3] the quads hold it now, [4] waves of the last batch's widest launch, [5] slots it was
// allowed, [6] the quads held the arena when it ran, [7] launches it took (> 1: the staging arena was grown), [8] the
// device the engine lives on.  Writes min(n, TS_BATCH_INFO_N) words and returns TS_BATCH_INFO_N.
constexpr int TS_BATCH_INFO_N = 9;
int ts_debug_batch_info(ts_handle e, int32_t* out, int32_t n) {
  if (!e || (!out && n > 0) || n < 0) return TS_E_INVALID;
  const E::Batch& B = e->batch;
  const int32_t v[TS_BATCH_INFO_N] = {e->slots_ready ? e->slots.n_slots : 0, e->side_slots, e->arena_shared ? 1 : 0, e->arena_quad ? 1 : 0,
                                      B.last_waves, B.last_usable, B.last_arena_quad, B.last_passes, e->device};
  for (int k = 0; k < std::min<int>(n, TS_BATCH_INFO_N); k++) out[k] = v[k];
  return TS_BATCH_INFO_N;
}

}  // extern "C"
