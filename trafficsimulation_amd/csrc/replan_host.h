// replan_host.h - the host side of replanning: searcher slots and the table arena k_replan and k_replan_quad share, the A* snapshot
// and the density map a search reads, the ordering of a tick's work queue, the quad pass and k_replan's passes (run_replans).
// Part of the single translation unit engine.hip (included from there, in order).
#pragma once

namespace {

// entries in the replanning work queue (RQueue, replan.h) as k_decide_main or the last pass left it
inline int replan_pending(const ReplanCtl& r) { return r.class_n[0] + r.class_n[1] + r.class_n[2] + r.class_n[3]; }
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
// the quads' slots to ask for (a multiple of sixteen) and the bytes each takes beside its table
struct QuadRequest { long long want; size_t side; };
inline QuadRequest quad_request() {
  const long long want = getenv("TS_QUAD_SLOTS") ? atoll(getenv("TS_QUAD_SLOTS")) : (long long)TS_QUAD_WAVES_PER_CU * 256 * 16;
  return {std::max<long long>(16, (want / 16) * 16),
          (size_t)Q_SPILL * 8 + (size_t)Q_DWORDS * 4 + slot_cell_ints(Q_CELLS) * 4 + SLOG_INTS * 4 + 4};
}

// Searcher slots for k_replan (one search per wave): per slot a direct-indexed table of one 8-byte record per search node
// (road cells, numbered in tiled order: 36 MB at 4096^2), the part of the heap that does not fit LDS, and the path
// staging buffers.  TS_REPLAN_WAVES x 1024 slots, at most 78 % of the free HBM (TS_ASTAR_MEM_FRAC).
// k_replan_quad's slots (astar_quad.h; with TS_QUAD=1): per search a 4-byte-per-cell table over a window of at most
// 1152 x 1152 cells (5.3 MB), the heap's HBM spill, the direction words and the path staging buffers - sixteen slots per wave,
// TS_QUAD_WAVES_PER_CU waves per CU (TS_QUAD_SLOTS overrides the count).  The two kernels never need all their tables at
// once - a replanning wave runs on the quads with a few k_replan waves beside them, every other tick on k_replan alone - so
// the quads' tables ALIAS the tables of k_replan's slots beyond the first `side_slots`.  The arena changes hands twice per
// six ticks and is not cleared for it (arena_to_quads / arena_to_waves below: the two record formats cannot collide; the
// clears it replaces took 22 ms for 152 GB and about as long for 165 GB each time).
int ensure_slots(E* e) {
  if (e->slots_ready) return TS_OK;
  {
    // the host tail's switches (TS_TAIL=0: off, the A/B and bisection switch).  Like the quads it carries half-unit costs without a
    // field-of-view mask.  A pass has a tail worth a snapshot copy when its queue is many times longer than the tail itself.
    E::TailHost& th = e->tail;
    const bool can = astar_half_units(e->P) && !e->P.respect_awareness;
    th.on = env_int("TS_TAIL", 1) != 0 && can;
    th.t_max = std::max(1, env_int("TS_TAIL_MAX", 32));
    th.floor = std::max(0, env_int("TS_TAIL_FLOOR", 65536));
    th.threads = env_int("TS_TAIL_THREADS", 0);
    th.force = std::max(0, env_int("TS_TAIL_FORCE", 0));
    th.min_queue = env_int("TS_TAIL_MIN_QUEUE", 16 * th.t_max);
    th.astar_host = env_int("TS_ASTAR_HOST", 0) != 0 && can;
  }
  // (the quad searcher, astar_quad.h: on unless TS_QUAD=0; it carries half-unit costs without a field-of-view mask)
  e->quad_on = !(getenv("TS_QUAD") && atoi(getenv("TS_QUAD")) == 0) && astar_half_units(e->P) && !e->P.respect_awareness;
  ASlots& T = e->slots;
  const long long N = e->N;
  T.tab_entries = (size_t)std::max(e->d.n_nodes, 1) + 1;   // (+ the spare record that the idle lanes of a masked store write to)
  T.cap = (int)std::min<long long>(N, 65536);
  // (the frontier BFS tests plain occupancy / red: with field-of-view masking the strict search decides for itself)
  T.use_reach = (getenv("TS_NO_REACH") || e->P.respect_awareness) ? 0 : 1;
  T.heap_cap = LDS_HEAP + (int)std::min<long long>(4 * N, 1ll << 18);   // (the deepest heap seen on 4096^2 runs is ~1500 entries)
  const size_t spill = (size_t)(T.heap_cap - LDS_HEAP);
  const size_t per_slot = T.tab_entries * sizeof(TEnt) + spill * (sizeof(HQ) + 1) + slot_cell_ints((size_t)T.cap) * 4 + 4;
  size_t free_b = 0, total_b = 0;
  HIPOK(hipMemGetInfo(&free_b, &total_b));
  // (headroom for what grows later - the path pool doubles under load, the vehicle arrays regrow, a second engine in the
  // process has slots of its own: twice the current pool and a gigabyte stay out of the budget)
  free_b -= std::min(free_b / 4, e->pool_cap * 4 * 2 + ((size_t)1 << 30));
  // the quads' own buffers (everything but their tables) come out of the budget first
  QSlots& Q = e->qslots;
  if (e->quad_on) {
    Q.tw = std::min(QT_MAX, (e->W + 7) / 8 * 8);
    Q.th = std::min(QT_MAX, (e->H + 7) / 8 * 8);
    Q.chk_x = e->W > Q.tw ? 1 : 0;
    Q.chk_y = e->H > Q.th ? 1 : 0;
    Q.tab_entries = (size_t)Q.tw * (size_t)Q.th;
    const QuadRequest qr = quad_request();
    free_b -= std::min(free_b / 2, (size_t)qr.want * qr.side);    // (set aside: ensure_qslots takes it when the first big queue arrives)
  }
  // one searcher per wave slot of the chip (TS_REPLAN_WAVES per SIMD x 1024 SIMDs), as far as 78 % of the free HBM carries
  long long want = getenv("TS_ASTAR_SLOTS") ? atoll(getenv("TS_ASTAR_SLOTS")) : (long long)TS_REPLAN_WAVES * 1024;
  const double frac = getenv("TS_ASTAR_MEM_FRAC") ? atof(getenv("TS_ASTAR_MEM_FRAC")) : 0.78;
  const long long fit = (long long)((double)free_b * frac / (double)per_slot);
  T.n_slots = (int)std::max<long long>(1, std::min<long long>(want, fit));
  const size_t S = (size_t)T.n_slots;
  HIPOK(dalloc(e, &T.tab, S * T.tab_entries));
  HIPOK(dalloc(e, &T.gq, S * spill));
  HIPOK(dalloc(e, &T.gd, S * spill));
  HIPOK(dalloc(e, &T.cells, S * slot_cell_ints((size_t)T.cap)));
  HIPOK(dalloc(e, &T.slot_epoch, S));
  HIPOK(dalloc(e, &T.big_flag, 1));
  T.big_thr = getenv("TS_DEBUG_ARENA_BIGDIST") ? (uint32_t)std::max(1, atoi(getenv("TS_DEBUG_ARENA_BIGDIST"))) : ARENA_BIGDIST;
  HIPOK(hipMemsetAsync(T.tab, 0, S * T.tab_entries * sizeof(TEnt), e->stream));
  HIPOK(hipMemsetAsync(T.slot_epoch, 0, S * 4, e->stream));     // (0: a fresh slot - its first stamp is the first of k_replan's range)
  HIPOK(hipMemsetAsync(T.big_flag, 0, sizeof(uint32_t), e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  e->slots_ready = true;
  return TS_OK;
}
// The quads' slots, set up when the first big queue arrives (engines that never see one - tests, the operator seam - never pay
// for them).  When device memory does not carry them the quad searcher is switched off for this engine and k_replan does it all.
int ensure_qslots(E* e) {
  if (e->qslots_ready || !e->quad_on) return TS_OK;
  ASlots& T = e->slots;
  QSlots& Q = e->qslots;
  const auto [q_want, q_side] = quad_request();
  Q.epoch_max = quad_epoch_limit(getenv("TS_DEBUG_QUAD_EPOCH_MAX") ? atoll(getenv("TS_DEBUG_QUAD_EPOCH_MAX")) : 0);
  // the quads' tables: inside k_replan's table arena behind the slots of the side waves when they fit there, in memory of
  // their own otherwise (small maps: a node-indexed table is smaller than a window then)
  e->side_slots = std::max(1, std::min(T.n_slots / 4, 1024));
  // (less 256 bytes: the quads' tables start on a 256-byte boundary, so that 32 of their records are one 128-byte line)
  const size_t alias_raw = (size_t)(T.n_slots - e->side_slots) * T.tab_entries * sizeof(TEnt), alias_bytes = alias_raw > 256 ? alias_raw - 256 : 0;
  const size_t need = (size_t)q_want * Q.tab_entries * 4;
  size_t f2 = 0, t2 = 0;
  HIPOK(hipMemGetInfo(&f2, &t2));
  // (the share of what is free NOW - k_replan's arena is allocated - that the quads' side buffers, and their tables when those do not fit
  // the arena, may take: the rest stays for the path pool's growth)
  const double qfrac = getenv("TS_QUAD_MEM_FRAC") ? atof(getenv("TS_QUAD_MEM_FRAC")) : 0.70;
  auto off = [&]() { e->quad_on = false; e->side_slots = T.n_slots; return TS_OK; };
  if (alias_bytes >= need / 2 && alias_bytes >= (size_t)256 * Q.tab_entries * 4) {
    Q.n_slots = (int)std::min<long long>(q_want, (long long)(alias_bytes / (Q.tab_entries * 4)) / 16 * 16);
    if ((double)Q.n_slots * (double)q_side > (double)f2 * qfrac) return off();
    Q.tab = (uint32_t*)(((uintptr_t)(T.tab + (size_t)e->side_slots * T.tab_entries) + 255) & ~(uintptr_t)255);
    e->arena_shared = true;
    e->arena_quad = false;
  } else {
    const long long fitq = (long long)((double)f2 * qfrac / (double)(Q.tab_entries * 4 + q_side));
    Q.n_slots = (int)(std::min<long long>(q_want, fitq) / 16 * 16);
    if (Q.n_slots < 256) return off();
    if (dalloc(e, &Q.tab, (size_t)Q.n_slots * Q.tab_entries) != hipSuccess) return off();
    HIPOK(hipMemsetAsync(Q.tab, 0, (size_t)Q.n_slots * Q.tab_entries * 4, e->stream));
    e->arena_shared = false;
    e->side_slots = T.n_slots;
  }
  const size_t QS = (size_t)Q.n_slots;
  if (dalloc(e, &Q.gq, QS * Q_SPILL) != hipSuccess || dalloc(e, &Q.gdw, QS * Q_DWORDS) != hipSuccess ||
      dalloc(e, &Q.cells, QS * slot_cell_ints(Q_CELLS)) != hipSuccess || dalloc(e, &Q.log, QS * SLOG_INTS) != hipSuccess ||
      dalloc(e, &Q.slot_epoch, QS) != hipSuccess || dalloc(e, &Q.stats, QST_N) != hipSuccess) { e->arena_shared = false; return off(); }
  HIPOK(hipMemsetAsync(Q.slot_epoch, 0, QS * 4, e->stream));
  HIPOK(hipMemsetAsync(Q.stats, 0, QST_N * sizeof(unsigned long long), e->stream));
  if (!e->quad_stream) {
    HIPOK(hipStreamCreateWithFlags(&e->quad_stream, hipStreamNonBlocking));
    HIPOK(hipEventCreateWithFlags(&e->quad_ev0, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&e->quad_ev1, hipEventDisableTiming));
  }
  HIPOK(hipStreamSynchronize(e->stream));
  e->qslots_ready = true;
  return TS_OK;
}
// The shared part of the table arena changes hands WITHOUT a clear: the two kernels' records cannot pass for each other's
// (arena_epochs.h: stamps disjoint in the top byte of a word, zero no stamp of either), and the epochs of both kinds of slot
// are kept across hand-overs, so what a slot left behind before it lost its table is as stale to it afterwards as anything
// it wrote before.  The one exception is a k_replan dist word of 2^24 or more (ASlots::big_thr): a search that stored one raised
// ASlots::big_flag, and the next hand-over to the quads clears their tables as every hand-over used to.  TS_ARENA_CLEAR=1 keeps
// that behaviour for both directions (A/B runs, bisection).
// A hand-over clear: the tables of the slots that take the shared part of the arena and their epochs (TS_DEBUG_REPLAN times it
// with HIP events of its own)
int arena_clear(E* e, void* tab, size_t tab_bytes, uint32_t* epochs, size_t n_epochs, const char* to) {
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = getenv("TS_DEBUG_REPLAN") != nullptr;
  if (timed) { HIPOK(hipEventCreate(&ev[0])); HIPOK(hipEventCreate(&ev[1])); HIPOK(hipEventRecord(ev[0], e->stream)); }
  HIPOK(hipMemsetAsync(tab, 0, tab_bytes, e->stream));
  HIPOK(hipMemsetAsync(epochs, 0, n_epochs * 4, e->stream));
  e->arena_clears++;
  if (timed) {
    float ms = 0.0f;
    HIPOK(hipEventRecord(ev[1], e->stream));
    HIPOK(hipEventSynchronize(ev[1]));
    HIPOK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    HIPOK(hipEventDestroy(ev[0])); HIPOK(hipEventDestroy(ev[1]));
    fprintf(stderr, "[replan] tick %lld: the table arena goes to %s, %.1f GB cleared in %.2f ms\n", (long long)e->C.step_count, to, (double)tab_bytes * 1e-9, (double)ms);
  }
  return TS_OK;
}
inline bool arena_always_clear() { return env_int("TS_ARENA_CLEAR", 0) != 0; }
int arena_to_quads(E* e) {
  if (!e->arena_shared || e->arena_quad) return TS_OK;
  // (read here rather than with a pass' counters: query batches and spawn-time searches use these tables too)
  uint32_t big = 0;
  TRY(read_back(e, &big, e->slots.big_flag, sizeof(big)));
  if (big) e->arena_big_seen++;
  if (big || arena_always_clear()) {
    TRY(arena_clear(e, e->qslots.tab, (size_t)e->qslots.n_slots * e->qslots.tab_entries * 4, e->qslots.slot_epoch, (size_t)e->qslots.n_slots, "the quads"));
    if (big) HIPOK(hipMemsetAsync(e->slots.big_flag, 0, sizeof(uint32_t), e->stream));
  }
  e->arena_quad = true;
  e->arena_to_q++;
  return TS_OK;
}
int arena_to_waves(E* e) {
  if (!e->arena_shared || !e->arena_quad) return TS_OK;
  const ASlots& T = e->slots;
  const size_t n = (size_t)(T.n_slots - e->side_slots);
  if (arena_always_clear())
    TRY(arena_clear(e, T.tab + (size_t)e->side_slots * T.tab_entries, n * T.tab_entries * sizeof(TEnt), T.slot_epoch + e->side_slots, n, "k_replan's waves"));
  e->arena_quad = false;
  e->arena_to_w++;
  return TS_OK;
}

// Dev::amap <- the cell records as they are now (the decide phase's snapshot, or the maps a spawn-time planner sees)
int ensure_amap(E* e) {
  if (!e->d.amap) {
    const size_t n = (size_t)e->d.W8 * e->d.H8 * 64;
    HIPOK(dalloc(e, &e->d.amap, n));
    HIPOK(hipMemsetAsync(e->d.amap, 0, n * 8, e->stream));
    e->amap_valid = false;
  }
  if (e->amap_valid) return TS_OK;
  // the vehicle penalty of every cell rides in the entry (searches in half units): callers materialise the density map first
  const int pen_mode = !astar_half_units(e->P) ? 0 : e->P.dynamic_penalties_enabled ? 2 : 1;
  if (pen_mode == 2 && !e->d.density) return fail(e, TS_E_STATE, "the A* snapshot needs the density map (internal error)");
  hipLaunchKernelGGL(k_amap_build, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, e->d, pen_mode,
                     (double)e->P.obstacle_penalty_vehicle, (double)e->P.dynamic_penalty_scale);
  e->amap_valid = true;
  return TS_OK;
}

// density_map as of the last tick start (city_model.py:1853), materialised only when a search may need it
int ensure_density(E* e, const int8_t* occ_src) {
  const size_t N = e->N;
  if (!e->dens_t0) { HIPOK(dalloc(e, &e->dens_t0, N)); HIPOK(dalloc(e, &e->dens_t1, N)); }
  if (!e->d.density) HIPOK(dalloc(e, &e->d.density, N));
  const int r = e->P.vehicle_awareness_range;
  int tok = prof_begin(e, PK_DENSITY, (long long)N);
  hipLaunchKernelGGL(k_density_pass0, dim3(nblk((long long)N)), dim3(BLK), 0, e->stream, occ_src, e->d.is_road, e->W, e->H, r,
                     e->dens_t0, e->dens_t1);
  hipLaunchKernelGGL(k_density_pass1, dim3(nblk((long long)N)), dim3(BLK), 0, e->stream, e->dens_t0, e->dens_t1, e->W, e->H, r,
                     e->d.density);
  prof_end(e, tok);
  return TS_OK;
}

// The maps a query "on the engine's current maps" reads (ts_astar, ts_astar_batch_run, the probes): the density planes and the
// snapshot from the cell records as they are now, built once for the call and dropped afterwards - the next tick, whose
// searches read the tick-start state, builds its own.
int search_maps_now(E* e) {
  TRY(ensure_density(e, e->d.occ));
  e->density_valid = false;
  TRY(ensure_slots(e));
  e->amap_valid = false;
  TRY(ensure_amap(e));
  e->amap_valid = false;
  return TS_OK;
}

// Order class list h (n entries) by its sort key.  Sharded, the order must be total and the same on every rank: 64-bit keys
// that end in the entry itself; otherwise key/value pairs.
int sort_replan_list(E* e, int h, int n, bool sharded) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  int32_t* list = e->class_list.l[h];
  if ((size_t)n > e->cap_sortbuf) {
    const size_t nc = (size_t)n * 2;
    TRY(regrow(e, &e->sort_keys, 0, nc * 2));          // (room for 64-bit keys)
    TRY(regrow(e, &e->sort_keys_alt, 0, nc * 2));
    TRY(regrow(e, &e->sort_vals_alt, 0, nc));
    e->cap_sortbuf = nc;
  }
  unsigned long long* k0 = (unsigned long long*)e->sort_keys;
  unsigned long long* k1 = (unsigned long long*)e->sort_keys_alt;
  auto sort = [&](void* tmp, size_t& tmp_bytes) {
    return sharded ? hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, k0, k1, n, 0, 32 + REPLAN_KEY_BITS, st)
                   : hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, e->sort_keys, e->sort_keys_alt, list, e->sort_vals_alt, n, 0,
                                                        REPLAN_KEY_BITS, st);
  };
  if (sharded) hipLaunchKernelGGL(k_replan_keys64, dim3(nblk(n)), dim3(BLK), 0, st, d, list, n, k0);
  else hipLaunchKernelGGL(k_replan_keys, dim3(nblk(n)), dim3(BLK), 0, st, d, list, n, e->sort_keys);
  size_t tmp_bytes = 0;
  HIPOK(sort(nullptr, tmp_bytes));
  TRY(grow(e, &e->sort_tmp, e->cap_sorttmp, tmp_bytes, tmp_bytes * 2));
  HIPOK(sort(e->sort_tmp, tmp_bytes));
  if (sharded) hipLaunchKernelGGL(k_replan_unkey64, dim3(nblk(n)), dim3(BLK), 0, st, k1, n, list);
  else HIPOK(hipMemcpyAsync(list, e->sort_vals_alt, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  return TS_OK;
}

// What is left of a replanning pass becomes the whole queue, in list 0: `left` entries of `handed_back` (the quads' hand-backs
// k_replan did not get to), then the `retry` entries that found the path pool full, once there is room for them.  owned_n
// (the entries this rank planned) is kept.
int requeue_in_list0(E* e, const int32_t* handed_back, int left, int retry) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  if (retry > 0) {
    d.pool_cap_words = e->pool_cap;
    TRY(pool_make_room(e, (size_t)retry * 1024 + (1u << 20)));
  }
  if (left > 0) HIPOK(hipMemcpyAsync(e->class_list.l[0], handed_back, (size_t)left * 4, hipMemcpyDeviceToDevice, st));
  if (retry > 0) HIPOK(hipMemcpyAsync(e->class_list.l[0] + left, e->retry_list, (size_t)retry * 4, hipMemcpyDeviceToDevice, st));
  ReplanCtl& r = e->hm->replan;
  const int keep_owned = r.owned_n;
  r = ReplanCtl{};
  r.class_n[0] = left + retry; r.owned_n = keep_owned;
  HIPOK(hipMemcpyAsync(&d.cnt->replan, &r, sizeof(ReplanCtl), hipMemcpyHostToDevice, st));
  return TS_OK;
}

// The end of a replanning pass: the queue's counters and the sticky error come back; a search that outgrew its buffers fails the tick
int replan_pass_done(E* e) {
  HIPOK(hipMemcpyAsync(&e->hm->replan, &e->d.cnt->replan, sizeof(ReplanCtl), hipMemcpyDeviceToHost, e->stream));
  TRY(read_back(e, &e->hm->error, &e->d.cnt->error, sizeof(int)));
  return e->hm->error == TS_E_CAPACITY ? fail(e, TS_E_CAPACITY, "an A* search exceeded its heap or path buffers") : TS_OK;
}

// ---- the host tail (replan.h RTail) -------------------------------------------------------------
inline ahost::Map tail_map(const E* e) {
  return ahost::Map{e->tail.h_amap, e->W, e->H, e->d.W8, e->N, (uint32_t)std::max(e->d.n_nodes, 1), e->slots.heap_cap};
}
inline size_t amap_words(const E* e) { return (size_t)e->d.W8 * e->d.H8 * 64; }
// the pool (created on first use: sixteen threads at the most, never more than this process may run on) and the side stream
int tail_setup(E* e) {
  E::TailHost& th = e->tail;
  if (!th.pool) th.pool = new ahost::Pool(th.threads > 0 ? std::min(th.threads, 64) : ahost::pool_default_threads());
  if (!th.stream) {
    HIPOK(hipStreamCreateWithFlags(&th.stream, hipStreamNonBlocking));
    HIPOK(hipEventCreateWithFlags(&th.ev_go, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&th.ev_copied, hipEventDisableTiming));
  }
  if (th.cap_amap < amap_words(e)) {
    HIPOK(hipStreamSynchronize(th.stream));
    HIPOK(regrow_pinned(&th.h_amap, amap_words(e)));
    th.cap_amap = amap_words(e);
  }
  return TS_OK;
}
// Dev::amap as the engine's stream leaves it at this point -> the pinned copy, on the side stream (it travels under whatever the
// engine's stream runs next); tail_snapshot_wait: the copy has landed
int tail_snapshot_begin(E* e) {
  E::TailHost& th = e->tail;
  TRY(tail_setup(e));
  HIPOK(hipEventRecord(th.ev_go, e->stream));
  HIPOK(hipStreamWaitEvent(th.stream, th.ev_go, 0));
  HIPOK(hipMemcpyAsync(th.h_amap, e->d.amap, amap_words(e) * 8, hipMemcpyDeviceToHost, th.stream));
  HIPOK(hipEventRecord(th.ev_copied, th.stream));
  return TS_OK;
}
int tail_snapshot_wait(E* e) {
  HIPOK(hipEventSynchronize(e->tail.ev_copied));
  return TS_OK;
}
// a pass with a tail is about to be launched: its control block (zeroed), the slots' logs, the snapshot copy
int tail_begin(E* e, RTail& tl) {
  E::TailHost& th = e->tail;
  if (!th.ctl) {
    const size_t S = (size_t)e->slots.n_slots;
    uint8_t* raw = nullptr;
    HIPOK(dalloc(e, &raw, sizeof(TailCtl) + S * sizeof(TailEnt)));
    th.ctl = (TailCtl*)raw;
    HIPOK(dalloc(e, &th.log, S * SLOG_INTS));
    const TailCtl first = {0, 0, e->slots.n_slots, 0};
    HIPOK(hipMemcpy(th.ctl, &first, sizeof(first), hipMemcpyHostToDevice));
  }
  HIPOK(hipMemsetAsync(th.ctl, 0, 2 * sizeof(int), e->stream));     // idle, n
  TRY(tail_snapshot_begin(e));
  tl = RTail{th.ctl, th.log, th.t_max, th.floor, th.force, 0};
  return TS_OK;
}
// ... and has drained (replan_pass_done): the searches its waves abandoned run on the pool, their paths and results go where the
// device would have put them, and k_replan_tail runs those step_decides again.  *handed: how many there were.
int tail_finish(E* e, const RQueueArgs& qa, const RTail& tl, double t_launch, int* handed) {
  E::TailHost& th = e->tail;
  const TsParams& P = e->P;
  const double t_pass = now_ms();
  *handed = 0;
  HIPOK(hipStreamWaitEvent(e->stream, th.ev_copied, 0));     // (whatever rebuilds the snapshot next waits for the copy)
  TailCtl h{};
  TRY(read_back(e, &h, th.ctl, sizeof(h)));
  const int n = std::min(h.n, h.cap);
  if (n <= 0) return TS_OK;
  std::vector<TailEnt> list((size_t)n);
  TRY(read_back(e, list.data(), th.ctl + 1, (size_t)n * sizeof(TailEnt)));
  TRY(tail_snapshot_wait(e));
  const ahost::Map map = tail_map(e);
  const ahost::Costs costs = ahost::costs_of(P);
  std::vector<std::unique_ptr<int32_t[]>> out((size_t)n);
  std::vector<int32_t> res((size_t)n * 3);
  for (int k = 0; k < n; k++) out[(size_t)k].reset(new int32_t[(size_t)std::max(list[(size_t)k].out_cap, 1)]);
  const double t_host = now_ms();
  th.pool->run(n, [&](ahost::Searcher& s, int k) {
    const TailEnt& t = list[(size_t)k];
    const ahost::Result r = s.run(map, costs, ahost::Query{t.start, t.goal, t.soft != 0, false, 0x7FFFFFFF}, out[(size_t)k].get(), t.out_cap);
    res[3 * (size_t)k] = r.len; res[3 * (size_t)k + 1] = r.n_exp; res[3 * (size_t)k + 2] = r.n_relax;
  });
  const double t_up = now_ms();
  for (int k = 0; k < n; k++) {
    const TailEnt& t = list[(size_t)k];
    const int len = res[3 * (size_t)k];
    if (len > 0) HIPOK(hipMemcpyAsync(e->slots.cells + (size_t)t.slot * slot_cell_ints((size_t)e->slots.cap) + t.out_off, out[(size_t)k].get(), (size_t)len * 4, hipMemcpyHostToDevice, e->stream));
    HIPOK(hipMemcpyAsync(th.log + (size_t)t.slot * SLOG_INTS + 3 * t.ord, &res[3 * (size_t)k], 12, hipMemcpyHostToDevice, e->stream));
  }
  LAUNCH(e, PK_REPLAN, n, k_replan_tail, dim3(n), dim3(64), e->d, P, e->slots, qa, tl, n);
  const int rc = replan_pass_done(e);       // (the stream drains here: the staged paths and results are no longer read)
  const double t_end = now_ms();
  th.passes++; th.searches += n;
  host_prof(e, PH_REPLAN_TAIL, t_end - t_pass, n);
  if (getenv("TS_DEBUG_REPLAN")) {
    long long ex = 0, ex_max = 0;
    for (int k = 0; k < n; k++) { ex += res[3 * (size_t)k + 1]; ex_max = std::max<long long>(ex_max, res[3 * (size_t)k + 1]); }
    fprintf(stderr, "[replan] tick %lld: host tail: %.2f ms to the hand-off, %d searches handed over (%lld expansions, the longest %lld), "
            "host %.2f ms on %d threads, re-run %.2f ms\n", (long long)e->C.step_count, t_pass - t_launch, n, ex, ex_max, t_up - t_host,
            th.pool->threads(), t_end - t_up);
  }
  *handed = n;
  return rc;
}
// what the pass left in the queue because its waves ended on hand-offs, into tail.unserved; *left: how many entries
int tail_unserved(E* e, const RQueueArgs& qa, int from, int total, int* left) {
  E::TailHost& th = e->tail;
  *left = 0;
  if (from >= total) return TS_OK;
  TRY(grow(e, &th.unserved, th.cap_unserved, (size_t)(total - from), (size_t)(total - from) * 2));
  HIPOK(hipMemsetAsync(e->d_status, 0, sizeof(int), e->stream));
  hipLaunchKernelGGL(k_tail_unserved, dim3(nblk(total - from)), dim3(BLK), 0, e->stream, e->d, qa, from, total, th.unserved, e->d_status);
  TRY(read_back(e, &e->hm->scratch, e->d_status, sizeof(int)));
  *left = e->hm->scratch;
  return TS_OK;
}

// The quad pass of a big queue (see run_replans): the classes in TS_QUAD_CLASSES go to k_replan_quad while k_replan serves the
// others and the quads' hand-backs beside it (RQueue, replan.h).  What neither got to is queued again in list 0.
int run_quad_pass(E* e) {
  Dev& d = e->d;
  const TsParams& P = e->P;
  hipStream_t st = e->stream;
  HostMirror& hm = *e->hm;
  const int quad_mask = env_int("TS_QUAD_CLASSES", 7) & 15;
  int nq = 0, nw = 0, qgrid = 0;
  for (int c = 0; c < 4; c++) { if ((quad_mask >> c) & 1) nq += hm.replan.class_n[c]; else nw += hm.replan.class_n[c]; }
  const double tl = now_ms();
  TRY(arena_to_quads(e));
  HIPOK(hipMemsetAsync(&d.cnt->handback_n, 0, sizeof(int) * 4, st));      // (the four hand-back words, handback_n .. quad_waves_done)
  int tok = prof_begin(e, PK_REPLAN, nq + nw);
  RQueueArgs qa = {.lists = e->class_list, .class_mask = quad_mask, .retry_list = e->retry_list, .handback_list = e->handback_list,
                   .rank = e->dist_rank, .world = e->dist_world, .owned_list = e->dist_world > 1 ? e->owned_list : nullptr, .fb_waves = 0};
  if (nq > 0) {
    HIPOK(hipMemsetAsync(e->handback_list, 0xFF, (size_t)nq * 4, st));     // (hand-back entries: -1 = not written yet)
    HIPOK(hipEventRecord(e->quad_ev0, st));
    HIPOK(hipStreamWaitEvent(e->quad_stream, e->quad_ev0, 0));
    qgrid = std::min((nq + 15) / 16, e->qslots.n_slots / 16);
    if (g_trace_launches) { fprintf(stderr, "[launch] k_replan_quad items=%d grid=%d\n", nq, qgrid); fflush(stderr); }
    hipLaunchKernelGGL(k_replan_quad, dim3(qgrid), dim3(64), 0, e->quad_stream, d, P, e->qslots, qa);
    HIPOK(hipEventRecord(e->quad_ev1, e->quad_stream));
  }
  // (k_replan never holds anything the quads wait for: were the two launches ever serialised, it would simply find the
  // hand-back list complete)
  // k_replan's waves beside the quads serve the most expensive class and the quads' hand-backs: 512 of them for a wave that hands back
  // thousands, 384 once the previous wave handed back few (they take issue slots from the quads: measured on the bench workload's four
  // waves, 5 678 / 2 895 / 1 379 / 2 514 hand-backs: 4.18 / 3.65 / 3.22 / 2.69 s with 512, 4.56 / 3.33 / 2.88 / 2.44 s with 384)
  const int side_waves = env_int("TS_QUAD_SIDE_WAVES", e->quad_last_fb < 0 || e->quad_last_fb > 4096 ? 512 : 384);
  const int wgrid = std::min(e->side_slots, std::max(std::min(nw, e->side_slots), nq > 0 ? side_waves : 1));
  qa.class_mask = 15 & ~quad_mask; qa.fb_waves = qgrid;
  if (nw > 0 || nq > 0) hipLaunchKernelGGL(k_replan, dim3(wgrid), dim3(64), 0, st, d, P, e->slots, qa, RTail{});   // (no host tail beside the quads)
  if (nq > 0) HIPOK(hipStreamWaitEvent(st, e->quad_ev1, 0));
  prof_end(e, tok);
  struct { int handback_n, quad_cursor, handback_claimed, quad_waves_done; } hb{};   // (the four words, as in DevCnt)
  unsigned long long qst[QST_N];
  HIPOK(hipMemcpyAsync(qst, e->qslots.stats, sizeof(qst), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&hb, &d.cnt->handback_n, sizeof(hb), hipMemcpyDeviceToHost, st));
  const int rc = replan_pass_done(e);
  if (rc && rc != TS_E_CAPACITY) return rc;   // (a capacity failure - fail() hands TS_E_CAPACITY back - waits until the pass' statistics are kept)
  HIPOK(hipMemsetAsync(e->qslots.stats, 0, sizeof(qst), st));
  for (int k = 0; k < QST_N; k++) e->quad_stats[k] += (long long)qst[k];
  e->quad_passes++;
  if (g_trace_launches) { fprintf(stderr, "[done] replanning pass with the quads\n"); fflush(stderr); }
  TRY(rc);
  const int retry = hm.replan.retry_n, fb = hb.handback_n;
  e->quad_jobs += nq; e->quad_fallbacks += fb; e->quad_last_fb = fb;
#ifdef TS_QUAD_PROF
  {
    long long pf[8];
    HIPOK(hipMemcpy(pf, d.cnt->prof, sizeof(pf), hipMemcpyDeviceToHost));
    fprintf(stderr, "[quadprof] wave cycles %lld, in the lockstep loop %lld, wave turns %lld, quad turns %lld: %.0f cycles per turn, %.1f quads per turn\n",
            pf[0], pf[1], pf[2], pf[3], pf[2] ? (double)pf[1] / (double)pf[2] : 0.0, pf[2] ? (double)pf[3] / (double)pf[2] : 0.0);
    HIPOK(hipMemset(d.cnt->prof, 0, sizeof(pf)));
    long long qf[8];
    HIPOK(hipMemcpy(qf, d.cnt->qprof, sizeof(qf), hipMemcpyDeviceToHost));
    fprintf(stderr, "[quadprof] per wave turn: pop+loads %.0f, sift LDS %.0f, sift deep %.0f, goal/stale %.0f, eval %.0f, pushes(+skipped) %.0f, tail %.0f, between turns %.0f\n",
            (double)qf[0] / pf[2], (double)qf[1] / pf[2], (double)qf[2] / pf[2], (double)qf[3] / pf[2], (double)qf[4] / pf[2], (double)qf[5] / pf[2], (double)qf[6] / pf[2], (double)qf[7] / pf[2]);
    // (stamped apart from "sift LDS" / "sift deep": the wait for the entry the pop moves to the root; the deep sift's first step, on
    // the entries fetched ahead - "sift deep" is what follows it, the blocking levels)
    fprintf(stderr, "[quadprof] per wave turn: delivery of the last entry %.0f, deep sift's first step %.0f\n", (double)pf[4] / pf[2], (double)pf[5] / pf[2]);
    HIPOK(hipMemset(d.cnt->qprof, 0, sizeof(qf)));
    // (outside the lockstep loop: every quad stamps its own segments, and quads that leave the loop together share their cycles)
    const double out = (double)(pf[0] - pf[1]), seg[4] = {(double)qst[QST_PROF], (double)qst[QST_PROF + 1], (double)qst[QST_PROF + 2], (double)qst[QST_PROF + 3]};
    fprintf(stderr, "[quadprof] outside the lockstep loop %.0f wave cycles: policy passes %.0f, search set-up %.0f, path walk %.0f, shift copy %.0f, rest %.0f\n",
            out, seg[0], seg[1], seg[2], seg[3], out - seg[0] - seg[1] - seg[2] - seg[3]);
  }
#endif
  if (getenv("TS_DEBUG_REPLAN")) {
    const long long* qs = e->quad_stats;
    fprintf(stderr, "[replan] quad hand-backs this pass by reason: window / g %llu, heap %llu, expansion budget %llu, path buffer %llu, "
            "policy bail (step-limited / contraflow search) %llu, policy overflow %llu; %llu searches started, %llu table-epoch wraps\n",
            qst[QST_WINDOW], qst[QST_HEAP], qst[QST_BUDGET], qst[QST_PATHBUF], qst[QST_BAIL], qst[QST_OVERFLOW], qst[QST_SEARCHES], qst[QST_WRAPS]);
    fprintf(stderr, "[replan] quad hand-backs so far %lld of %lld jobs: window / g %lld, heap %lld, expansion budget %lld, path buffer %lld, "
            "policy bail %lld, policy overflow %lld; %lld searches started, %lld table-epoch wraps\n",
            e->quad_fallbacks, e->quad_jobs, qs[QST_WINDOW], qs[QST_HEAP], qs[QST_BUDGET], qs[QST_PATHBUF], qs[QST_BAIL], qs[QST_OVERFLOW],
            qs[QST_SEARCHES], qs[QST_WRAPS]);
    fprintf(stderr, "[replan] tick %lld: %d entries to the quads (%d waves of %d), %d to k_replan (%d waves); handed over %d, pool-full %d, %.2f ms\n",
            (long long)e->C.step_count, nq, qgrid, e->qslots.n_slots / 16, nw, wgrid, fb, retry, now_ms() - tl);
  }
  // what k_replan did not get to serve of the hand-backs (it only gives up on them when the two kernels were not run side
  // by side) and what found the path pool full is queued again
  const int served = std::min(hb.handback_claimed, fb);
  return requeue_in_list0(e, e->handback_list + served, fb - served, retry);
}

int run_replans(E* e) {   // e->hm->replan = the queue as k_decide_main left it
  Dev& d = e->d;
  const TsParams& P = e->P;
  HostMirror& hm = *e->hm;
  TRY(ensure_slots(e));
  if (!e->density_valid) { TRY(ensure_density(e, d.occ_snap)); e->density_valid = true; }
  TRY(ensure_amap(e));
  // room in the path pool for what these replans will write (a planner that finds the pool full throws its searches
  // away and is run again): 128 words = 2048 path cells per entry, garbage-collecting / growing the pool if need be
  // (TS_DEBUG_POOL_PER_ENTRY shrinks the reservation so that tests can walk the pool-full retry path)
  const char* dbg_per = getenv("TS_DEBUG_POOL_PER_ENTRY");
  const size_t per_entry = dbg_per ? (size_t)atoi(dbg_per) : 128;
  TRY(pool_make_room(e, (size_t)replan_pending(hm.replan) * per_entry + (dbg_per ? 64u : (1u << 20))));
  if (dbg_per) d.pool_cap_words = std::min(e->pool_cap, e->pool_used + (size_t)replan_pending(hm.replan) * per_entry + 64u);
  if (dbg_per && getenv("TS_DEBUG_REPLAN")) fprintf(stderr, "[replan] pool used %zu cap %zu -> logical cap %llu\n", e->pool_used, e->pool_cap, d.pool_cap_words);
  // Order every class list by expected cost (largest first: the longest search of a tick bounds it) and, among equals, in
  // space (Morton order of 32 x 32-cell blocks of the vehicles' positions): the searches that run at the same time then
  // read the same few megabytes of the map snapshot, which stay in the XCDs' L2s instead of competing with thousands of
  // private tables for the MALL.  The order of the queue does not touch any result.
  static const bool spatial = !getenv("TS_NO_SPATIAL_QUEUE");
  const bool sharded = e->dist_world > 1;      // (then the order must be total and the same on every rank: 64-bit keys, every list)
  for (int h = 0; h < 4 && (spatial || sharded); h++)
    if (hm.replan.class_n[h] >= (sharded ? 2 : 256)) TRY(sort_replan_list(e, h, hm.replan.class_n[h], sharded));
  // The quad searcher (astar_quad.h; TS_QUAD=0 switches it off): a big
  // queue (a replanning wave of TS_QUAD_MIN entries or more) sends the classes in TS_QUAD_CLASSES to k_replan_quad (sixteen
  // searches per wave, on its own stream) while k_replan runs beside it on the most expensive class and on every vehicle
  // the quads hand back as they work (searches that outgrow their window, heap or expansion budget, step-limited ones).
  // Smaller queues are bounded by their longest search, and that one is faster alone on a wave.
  // (a queue is the quads' when it is long against what k_replan can have in flight: 262 144 entries on the 5 751 slots a 4096^2
  // map leaves it, in proportion fewer where its node tables are bigger and its slots fewer - 1 534 at 8192^2)
  const int quad_min = env_int("TS_QUAD_MIN", (int)std::min<long long>(262144, std::max<long long>(16384, 46ll * e->slots.n_slots)));
  bool split_done = false;      // (the queue is split between the ranks once; what is queued again - pool-full entries, hand-backs - is this rank's own)
  // (in the sharded multi-GPU mode the threshold applies to this rank's share: every world-th entry of the queue)
  const bool quad_queue = replan_pending(hm.replan) / std::max(e->dist_world, 1) >= std::max(quad_min, 1);
  // (set up with the first replans of a population that will fill such a queue - its first replanning wave - rather than inside that wave)
  const bool quad_soon = e->n_active / std::max(e->dist_world, 1) >= std::max(quad_min, 1);
  if (e->quad_on && (quad_queue || quad_soon)) TRY(ensure_qslots(e));
  if (e->quad_on && e->qslots_ready && quad_queue) {
    TRY(run_quad_pass(e));
    split_done = true;
  }
  while (replan_pending(hm.replan) > 0) {
    const int n = replan_pending(hm.replan);
    const int grid = std::min(n, e->slots.n_slots);
    if (grid > e->side_slots && e->quad_on) TRY(arena_to_waves(e));
    const RQueueArgs qa = {.lists = e->class_list, .class_mask = 15, .retry_list = e->retry_list, .handback_list = nullptr,
                           .rank = split_done ? 0 : e->dist_rank, .world = split_done ? 1 : e->dist_world,
                           .owned_list = e->dist_world > 1 ? e->owned_list : nullptr, .fb_waves = 0};
    split_done = true;
#ifdef TS_TRACE_REPLAN
    static int4* tr_buf = nullptr;
    const int tr_cap = 1 << 22;
    if (!tr_buf) {
      HIPOK(hipMalloc(&tr_buf, (size_t)tr_cap * sizeof(int4)));
      HIPOK(hipMemcpyToSymbol(HIP_SYMBOL(g_rtrace), &tr_buf, sizeof(tr_buf)));
      HIPOK(hipMemcpyToSymbol(HIP_SYMBOL(g_rtrace_cap), &tr_cap, sizeof(tr_cap)));
    }
    HIPOK(hipMemsetAsync(tr_buf, 0, (size_t)std::min(n, tr_cap) * sizeof(int4), e->stream));
#endif
    // the host tail: a pass whose queue is long against the tail carries a control block, and the snapshot copy travels under it
    // (TS_TAIL_FORCE: every pass does)
    const E::TailHost& th = e->tail;
    const bool tail_pass = th.on && (th.force > 0 || n >= th.min_queue);
    RTail tail{};
    if (tail_pass) TRY(tail_begin(e, tail));
    LAUNCH(e, PK_REPLAN, n, k_replan, dim3(grid), dim3(64), d, P, e->slots, qa, tail);
    const double tl = now_ms();
    int rc = replan_pass_done(e);
    int handed = 0, left = 0;
    if (tail_pass && rc == TS_OK) {
      rc = tail_finish(e, qa, tail, tl, &handed);
      // (waves that end on a hand-off can leave entries in the queue: with TS_TAIL_FORCE, or where the launch has no more waves than t_max)
      if (rc == TS_OK) rc = tail_unserved(e, qa, std::min(hm.replan.cursor, n), n, &left);
    }
#ifdef TS_TRACE_REPLAN
    if (n >= 1000) {
      std::vector<int4> h((size_t)std::min(n, tr_cap));
      HIPOK(hipMemcpy(h.data(), tr_buf, h.size() * sizeof(int4), hipMemcpyDeviceToHost));
      char name[128];
      snprintf(name, sizeof(name), "gpurun_out/rtrace_tick%lld.bin", (long long)e->C.step_count);
      if (FILE* f = fopen(name, "wb")) { fwrite(h.data(), sizeof(int4), h.size(), f); fclose(f); }
      fprintf(stderr, "[rtrace] tick %lld: %d entries, %d searchers, %.2f ms\n", (long long)e->C.step_count, n, grid, now_ms() - tl);
    }
#endif
    if (getenv("TS_DEBUG_REPLAN")) {
      DevCnt c;
      HIPOK(hipMemcpy(&c, d.cnt, sizeof(DevCnt), hipMemcpyDeviceToHost));
      fprintf(stderr, "[replan] deepest heap so far %d, longest search so far %d expansions, %lld expansions so far with part of the heap in HBM\n",
              c.max_heap, c.max_search_exp, c.spill_exp);
    }
    TRY(rc);
    const int retry = hm.replan.retry_n;
    if (getenv("TS_DEBUG_REPLAN"))
      fprintf(stderr, "[replan] tick %lld: %d entries (classes %d/%d/%d/%d) on %d searchers, retry=%d, handed to the host %d, left in the queue %d, %.2f ms\n",
              (long long)e->C.step_count, n, hm.replan.class_n[0], hm.replan.class_n[1], hm.replan.class_n[2], hm.replan.class_n[3], grid, retry,
              handed, left, now_ms() - tl);
    if (handed > 0 && left == 0) {
      // a wave that ends on a hand-off does not draw past the end of the queue as every other wave does once: the cursor is put
      // where a pass without hand-offs leaves it, so that the counters a checkpoint stores do not depend on how many there were
      hm.replan.cursor = n + grid;
      HIPOK(hipMemcpyAsync(&d.cnt->replan.cursor, &hm.replan.cursor, sizeof(int), hipMemcpyHostToDevice, e->stream));
      HIPOK(hipStreamSynchronize(e->stream));
    }
    if (retry == 0 && left == 0) break;
    // the path pool filled up: make room (GC, then growth) and run the entries that could not commit again - with what a pass
    // that ended on hand-offs left in the queue
    TRY(requeue_in_list0(e, e->tail.unserved, left, retry));
  }
  d.pool_cap_words = e->pool_cap;
  return TS_OK;
}

}  // namespace
