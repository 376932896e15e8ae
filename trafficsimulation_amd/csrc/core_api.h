// core_api.h - the C-ABI entries of include/trafficsim.h, ts_default_params ... ts_astar, and the spawn paths behind
// ts_add_vehicles (add_vehicles_core, add_vehicle_planned, plan_vehicle, add_vehicles_any).
// Part of the single translation unit engine.hip (included from there, in order).
#pragma once

static int g_device = 0;  // ts_set_device
extern "C" {

void ts_default_params(TsParams* p) {
  memset(p, 0, sizeof(*p));
  p->vehicle_min_speed = 1; p->vehicle_max_speed = 5; p->vehicle_awareness_range = 10;
  p->rain_enabled = 1; p->rain_speed_reduction = 2;
  p->pathfinding_cooldown = 5; p->pathfinding_cache = 1;
  p->stuck_recompute_threshold = 30; p->stuck_recompute_threshold_intersection = 1;
  p->contraflow_overtake_active = 1; p->max_contraflow_overtake_steps = 6; p->contraflow_overtake_duration = 30;
  p->stuck_contraflow_enabled = 1; p->stuck_contraflow_threshold = 60; p->stuck_contraflow_threshold_intersection = 10;
  p->max_contraflow_stuck_detour_steps = 20; p->contraflow_stuck_detour_duration = 10;
  p->malfunction_active = 1; p->malfunction_duration = 400; p->malfunction_chance = 1e-7;
  p->sideswipe_active = 1; p->sideswipe_duration = 600; p->sideswipe_chance = 1e-9;
  p->contraflow_penalty = 5000; p->obstacle_penalty_vehicle = 1000; p->obstacle_penalty_stop = 500;
  p->road_type_penalties_enabled = 1; p->turn_penalty_enabled = 1; p->turn_penalty = 10;
  p->dynamic_penalties_enabled = 1;
  p->road_type_penalty_r1 = 0.5; p->road_type_penalty_r2 = 5; p->road_type_penalty_r3 = 50.0;
  p->dynamic_penalty_scale = 4.0;
  p->light_algorithm = TS_LIGHTS_QUEUE_ACTUATED;
  p->transition_duration_enabled = 0; p->transition_clearance_enabled = 1; p->all_red_duration = 2;
  p->green_duration = 20; p->qa_min_green = 5; p->qa_max_green = 30; p->qa_gap = 3;
  p->enable_traffic = 1; p->time_per_step_seconds = 6; p->eager_density = 0;
  p->rain_radius_min = 50; p->rain_radius_max = 100; p->rain_occurrences_max = 3; p->rain_cooldown = 86400;
  p->rain_spawn_offset = 10; p->rain_spawn_chance = 0.1;
  p->stuck_despawn_enabled = 0; p->stuck_despawn_threshold = 3600; p->stuck_despawn_threshold_intersection = 20;
  p->pathfinding_batching = 1;
}

int ts_create(const TsWorld* w, const TsParams* params, ts_handle* out) {
  if (!w || !params || !out || w->width <= 0 || w->height <= 0 || !w->allowed_dirs_map || !w->is_road_map ||
      !w->road_type_map || !w->intersection_map)
    return TS_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return TS_E_DEVICE;
  if (hipSetDevice(g_device) != hipSuccess) return TS_E_DEVICE;
  {
    // ranges the kernels rely on (int8 speed fields, the MAXB-cell bypass buffers, clz of the speed span)
    const TsParams& q = *params;
    if (q.vehicle_min_speed < 0 || q.vehicle_max_speed < q.vehicle_min_speed || q.vehicle_max_speed > 127) return TS_E_INVALID;
    if (q.max_contraflow_overtake_steps < 0 || q.max_contraflow_stuck_detour_steps < 0 || q.vehicle_awareness_range < 0 ||
        q.rain_speed_reduction < 0 || q.pathfinding_cooldown < 0)
      return TS_E_INVALID;
    if (q.max_contraflow_overtake_steps > MAXB || q.max_contraflow_stuck_detour_steps > MAXB) return TS_E_UNSUPPORTED;
    if (w->width > A_XY_MAX || w->height > A_XY_MAX) return TS_E_UNSUPPORTED;   // (heap entries carry a cell as 16 + 16 bits)
  }
  E* e = new E();
  memset(&e->d, 0, sizeof(e->d));
  memset(&e->C, 0, sizeof(e->C));
  e->P = *params;
  e->W = w->width; e->H = w->height; e->N = w->width * w->height;
  {
    Fp fw;
    fw.mix((uint64_t)(uint32_t)w->width << 32 | (uint32_t)w->height);
    const size_t n = (size_t)w->width * w->height;
    fw.bytes(w->allowed_dirs_map, n); fw.bytes(w->is_road_map, n); fw.bytes(w->road_type_map, n); fw.bytes(w->intersection_map, n);
    e->fp_world = fw.h;
    Fp fpar;   // (every named field; the struct's trailing padding is not part of it)
    fpar.bytes(params, offsetof(TsParams, pathfinding_batching) + sizeof(params->pathfinding_batching));
    e->fp_params = fpar.h;
  }
  Dev& d = e->d;
  d.W = e->W; d.H = e->H; d.N = e->N;
  d.W8 = (e->W + 7) / 8; d.H8 = (e->H + 7) / 8;
  d.w_magic = (!getenv("TS_NO_MAGIC") && e->W < (1 << 14) && (long long)e->N <= (1ll << 26)) ? ((1ull << 40) / (unsigned long long)e->W + 1ull) : 0ull;
  size_t N = e->N;
  auto bail = [&](int code) { ts_destroy(e); return code; };
  if (hipStreamCreate(&e->stream) != hipSuccess) return bail(TS_E_DEVICE);
#define A(ptr, n) if (dalloc(e, &ptr, (size_t)(n)) != hipSuccess) return bail(TS_E_DEVICE);
  A(d.occ, N) A(d.stop, N) A(d.rain, N) A(d.is_road, N) A(d.cell, N) A(d.gclaim_r, 1)
  Scratch tmp;                    // static planes only needed to build the cell records: they go when this call returns
  uint8_t* t_allowed = nullptr;
  int8_t *t_road_type = nullptr, *t_inter = nullptr;
  if (tmp.get(&t_allowed, N) != hipSuccess || tmp.get(&t_road_type, N) != hipSuccess || tmp.get(&t_inter, N) != hipSuccess)
    return bail(TS_E_DEVICE);
  A(d.cnt, 1) A(e->d_total, 1) A(e->d_crc, 256) A(d.occ_snap, N) A(e->d_status, 4)
#undef A
  hipStream_t st = e->stream;
  bool ok = true;
  ok &= hipMemsetAsync(d.occ, 0, N, st) == hipSuccess;
  ok &= hipMemsetAsync(d.stop, 0, N, st) == hipSuccess;
  ok &= hipMemsetAsync(d.rain, 0, N, st) == hipSuccess;
  ok &= hipMemsetAsync(d.occ_snap, 0, N, st) == hipSuccess;  // _update_density_map() on the fresh, empty model
  ok &= hipMemsetAsync(d.cnt, 0, sizeof(DevCnt), st) == hipSuccess;
  ok &= hipMemcpyAsync(t_allowed, w->allowed_dirs_map, N, hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipMemcpyAsync(d.is_road, w->is_road_map, N, hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipMemcpyAsync(t_road_type, w->road_type_map, N, hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipMemcpyAsync(t_inter, w->intersection_map, N, hipMemcpyHostToDevice, st) == hipSuccess;
  // search nodes: every cell a search can stand on - roads, cells with flow bits, cells a neighbour's flow bit points at
  // - numbered in the 8 x 8-tiled order of the A* snapshot
  int32_t* t_node = nullptr;
  {
    const int W = e->W, H = e->H;
    std::vector<uint8_t> is_node(N, 0);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const size_t c = (size_t)y * W + x;
        const int a = w->allowed_dirs_map[c] & 15;
        if (w->is_road_map[c] == 1 || a) is_node[c] = 1;
        if ((a & 1) && y + 1 < H) is_node[c + W] = 1;
        if ((a & 2) && x + 1 < W) is_node[c + 1] = 1;
        if ((a & 4) && y > 0) is_node[c - W] = 1;
        if ((a & 8) && x > 0) is_node[c - 1] = 1;
      }
    std::vector<int32_t> node(N, -1);
    int n_nodes = 0;
    for (int ty = 0; ty < d.H8; ty++)
      for (int tx = 0; tx < d.W8; tx++)
        for (int yy = 0; yy < 8; yy++)
          for (int xx = 0; xx < 8; xx++) {
            const int x = tx * 8 + xx, y = ty * 8 + yy;
            if (x < W && y < H && is_node[(size_t)y * W + x]) node[(size_t)y * W + x] = n_nodes++;
          }
    d.n_nodes = n_nodes;
    if (tmp.get(&t_node, N) != hipSuccess) return bail(TS_E_DEVICE);
    ok &= hipMemcpy(t_node, node.data(), N * 4, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (params->respect_awareness) {
    // straight runs of road cells ending in each cell, for the field-of-view test of the searches (Dev::fovrun)
    const int W = e->W, H = e->H;
    std::vector<uint16_t> run((size_t)N * 4, 0);
    auto road = [&](int x, int y) { return w->is_road_map[(size_t)y * W + x] == 1; };
    for (int x = 0; x < W; x++) {
      for (int y = 0; y < H; y++) run[((size_t)y * W + x) * 4 + 0] = road(x, y) ? (uint16_t)std::min(65535, (y > 0 ? run[((size_t)(y - 1) * W + x) * 4 + 0] : 0) + 1) : 0;
      for (int y = H - 1; y >= 0; y--) run[((size_t)y * W + x) * 4 + 1] = road(x, y) ? (uint16_t)std::min(65535, (y + 1 < H ? run[((size_t)(y + 1) * W + x) * 4 + 1] : 0) + 1) : 0;
    }
    for (int y = 0; y < H; y++) {
      for (int x = 0; x < W; x++) run[((size_t)y * W + x) * 4 + 2] = road(x, y) ? (uint16_t)std::min(65535, (x > 0 ? run[((size_t)y * W + x - 1) * 4 + 2] : 0) + 1) : 0;
      for (int x = W - 1; x >= 0; x--) run[((size_t)y * W + x) * 4 + 3] = road(x, y) ? (uint16_t)std::min(65535, (x + 1 < W ? run[((size_t)y * W + x + 1) * 4 + 3] : 0) + 1) : 0;
    }
    const size_t nt = (size_t)d.W8 * d.H8 * 64;
    std::vector<unsigned long long> tiled(nt, 0ull);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const size_t t = ((((size_t)(y >> 3) * d.W8 + (size_t)(x >> 3)) << 6) | (size_t)((y & 7) << 3) | (size_t)(x & 7));
        const uint16_t* r = &run[((size_t)y * W + x) * 4];
        tiled[t] = (unsigned long long)r[0] | ((unsigned long long)r[1] << 16) | ((unsigned long long)r[2] << 32) | ((unsigned long long)r[3] << 48);
      }
    unsigned long long* fr = nullptr;
    ok &= dalloc(e, &fr, nt) == hipSuccess;
    if (fr) ok &= hipMemcpy(fr, tiled.data(), nt * 8, hipMemcpyHostToDevice) == hipSuccess;
    d.fovrun = fr;
  }
  hipLaunchKernelGGL(k_cells_init, dim3(nblk((long long)N)), dim3(BLK), 0, st, d.cell, (int)N, t_allowed, d.is_road, t_road_type, t_inter, t_node);
  uint32_t table[256];
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320U ^ (c >> 1)) : (c >> 1);
    table[i] = c;
  }
  ok &= hipMemcpyAsync(e->d_crc, table, sizeof(table), hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipHostMalloc((void**)&e->hcnt, sizeof(DevCnt)) == hipSuccess;
  ok &= hipHostMalloc((void**)&e->hm, sizeof(HostMirror)) == hipSuccess;
  ok &= hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return bail(TS_E_DEVICE);
  ok = hipHostMalloc((void**)&e->h_words, MTPipe::TW_CAP * 4) == hipSuccess;
  ok &= dalloc(e, &d.words, (size_t)MTPipe::TW_CAP) == hipSuccess;
  ok &= hipStreamCreate(&e->copy_stream) == hipSuccess;
  ok &= hipStreamCreateWithFlags(&e->perm_stream, hipStreamNonBlocking) == hipSuccess;
  ok &= hipEventCreateWithFlags(&e->perm_ev, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&e->take_ev, hipEventDisableTiming) == hipSuccess;
  e->device = g_device;
  ok &= hipEventCreateWithFlags(&e->words_ev, hipEventDisableTiming) == hipSuccess;
  if (!ok) return bail(TS_E_DEVICE);
  e->rng_global.use_storage(e->h_words);
  e->cap_take = 6u << 20;
  if (dalloc(e, &e->d_take, e->cap_take) != hipSuccess) return bail(TS_E_DEVICE);
  if (hipHostMalloc((void**)&e->h_take, e->cap_take) != hipSuccess) return bail(TS_E_DEVICE);
  e->epoch = 0;
  e->rng_global.set_roll((uint32_t)std::max(1, params->vehicle_max_speed - params->vehicle_min_speed + 1));
  if (ensure_vehicle_capacity(e, 1024, 1024) != TS_OK) return bail(TS_E_DEVICE);
  if (ensure_pool(e, 1 << 16) != TS_OK) return bail(TS_E_DEVICE);
  *out = e;
  return TS_OK;
}

int ts_destroy(ts_handle e) {
  if (!e) return TS_OK;
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->sh_thread.joinable()) {
    { std::lock_guard<std::mutex> lk(e->sh_mu); e->sh_quit = true; }
    e->sh_cv.notify_all();
    e->sh_thread.join();
    e->sh2_thread.join();
  }
  if (e->perm_stream) { (void)hipStreamSynchronize(e->perm_stream); (void)hipStreamDestroy(e->perm_stream); }
  if (e->perm_ev) (void)hipEventDestroy(e->perm_ev);
  if (e->take_ev) (void)hipEventDestroy(e->take_ev);
  for (void* p : e->allocs) (void)hipFree(p);
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  if (e->hF) (void)hipHostFree(e->hF);
  if (e->hR) (void)hipHostFree(e->hR);
  if (e->hrank) (void)hipHostFree(e->hrank);
  if (e->hcnt) (void)hipHostFree(e->hcnt);
  if (e->h_rollD) (void)hipHostFree(e->h_rollD);
  if (e->h_Tcum) (void)hipHostFree(e->h_Tcum);
  if (e->h_take) (void)hipHostFree(e->h_take);
  if (e->words_ev) (void)hipEventDestroy(e->words_ev);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->quad_stream) { (void)hipStreamSynchronize(e->quad_stream); (void)hipStreamDestroy(e->quad_stream); }
  if (e->quad_ev0) (void)hipEventDestroy(e->quad_ev0);
  if (e->quad_ev1) (void)hipEventDestroy(e->quad_ev1);
  delete e->tail.pool;            // joins the host tail's workers
  if (e->tail.stream) { (void)hipStreamSynchronize(e->tail.stream); (void)hipStreamDestroy(e->tail.stream); }
  if (e->tail.ev_go) (void)hipEventDestroy(e->tail.ev_go);
  if (e->tail.ev_copied) (void)hipEventDestroy(e->tail.ev_copied);
  if (e->tail.h_amap) (void)hipHostFree(e->tail.h_amap);
  if (e->hm) (void)hipHostFree(e->hm);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  uint32_t* hw = e->h_words;
  delete e;                       // stops the producer threads before their ring storage goes away
  if (hw) (void)hipHostFree(hw);
  return TS_OK;
}

const char* ts_last_error(ts_handle h) { return h ? h->err.c_str() : "null handle"; }

int ts_set_lights(ts_handle e, const TsLightTables* t) {
  if (!e || !t || t->n_groups < 0 || t->n_lights < 0) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (e->lights_set) return fail(e, TS_E_STATE, "ts_set_lights may be called once");
  const int W = e->W, H = e->H, G = t->n_groups, L = t->n_lights;
  Dev& d = e->d;
  auto cells = [&](const int32_t* xy, int n, std::vector<int32_t>& out) {
    out.resize(n);
    for (int i = 0; i < n; i++) {
      int x = xy[2 * i], y = xy[2 * i + 1];
      if (x < 0 || x >= W || y < 0 || y >= H) return false;
      out[i] = y * W + x;
    }
    return true;
  };
  auto up = [&](int32_t** dst, const int32_t* src, size_t n) -> int {
    HIPOK(dalloc(e, dst, n));
    if (n) HIPOK(hipMemcpyAsync(*dst, src, n * 4, hipMemcpyHostToDevice, e->stream));
    return TS_OK;
  };
  std::vector<int32_t> tmp;
#define UPOFF(dst, src, n) TRY(up(&d.dst, t->src, (size_t)(n)));
#define UPCELLS(dst, src, n) { if (!cells(t->src, (n), tmp)) return fail(e, TS_E_INVALID, #src " out of bounds"); \
    TRY(up(&d.dst, tmp.data(), (size_t)(n))); HIPOK(hipStreamSynchronize(e->stream)); }
  UPOFF(g_light_off, g_light_off, G + 1)
  UPCELLS(light_cell, light_xy, L)
  UPOFF(light_ctrl_off, light_ctrl_off, L + 1)
  UPCELLS(light_ctrl, light_ctrl_xy, t->light_ctrl_off[L])
  UPOFF(g_ns_off, g_ns_off, G + 1) UPOFF(g_ns, g_ns, t->g_ns_off[G])
  UPOFF(g_ew_off, g_ew_off, G + 1) UPOFF(g_ew, g_ew, t->g_ew_off[G])
  for (int k = 0; k < t->g_ns_off[G]; k++) if (t->g_ns[k] < 0 || t->g_ns[k] >= L) return fail(e, TS_E_INVALID, "g_ns light index");
  for (int k = 0; k < t->g_ew_off[G]; k++) if (t->g_ew[k] < 0 || t->g_ew[k] >= L) return fail(e, TS_E_INVALID, "g_ew light index");
  UPOFF(g_icell_off, g_icell_off, G + 1) UPCELLS(g_icell, g_icell_xy, t->g_icell_off[G])
  UPOFF(g_nsin_off, g_ns_in_off, G + 1) UPCELLS(g_nsin, g_ns_in_xy, t->g_ns_in_off[G])
  UPOFF(g_nsout_off, g_ns_out_off, G + 1) UPCELLS(g_nsout, g_ns_out_xy, t->g_ns_out_off[G])
  UPOFF(g_ewin_off, g_ew_in_off, G + 1) UPCELLS(g_ewin, g_ew_in_xy, t->g_ew_in_off[G])
  UPOFF(g_ewout_off, g_ew_out_off, G + 1) UPCELLS(g_ewout, g_ew_out_xy, t->g_ew_out_off[G])
#undef UPOFF
#undef UPCELLS
  {
    // flat (cell, group, plane) list of everything a group claims in the move phase (k_move_claim_groups)
    std::vector<int32_t> fc, fg;
    std::vector<uint8_t> fp;
    std::vector<int32_t> cidx;
    const bool outs = e->P.light_algorithm == TS_LIGHTS_PRESSURE_CONTROL || e->P.light_algorithm == TS_LIGHTS_NEIGHBOR_PRESSURE_CONTROL;
    auto add_range = [&](const int32_t* off, const int32_t* xy, int g, int plane) {
      for (int k = off[g]; k < off[g + 1]; k++) { fc.push_back(xy[2 * k + 1] * W + xy[2 * k]); fg.push_back(g); fp.push_back((uint8_t)plane); }
    };
    for (int g = 0; g < G; g++) {
      add_range(t->g_icell_off, t->g_icell_xy, g, 1);
      add_range(t->g_ns_in_off, t->g_ns_in_xy, g, 1);
      add_range(t->g_ew_in_off, t->g_ew_in_xy, g, 1);
      if (outs) { add_range(t->g_ns_out_off, t->g_ns_out_xy, g, 1); add_range(t->g_ew_out_off, t->g_ew_out_xy, g, 1); }
      for (int l = t->g_light_off[g]; l < t->g_light_off[g + 1]; l++) {
        fc.push_back(t->light_xy[2 * l + 1] * W + t->light_xy[2 * l]); fg.push_back(g); fp.push_back(2);
        add_range(t->light_ctrl_off, t->light_ctrl_xy, l, 2);
        for (size_t q = fg.size() - (size_t)(t->light_ctrl_off[l + 1] - t->light_ctrl_off[l]); q < fg.size(); q++) fg[q] = g;
      }
    }
    d.gc_n = (int)fc.size();
    HIPOK(dalloc(e, &d.gc_cell, fc.size())); HIPOK(dalloc(e, &d.gc_group, fg.size())); HIPOK(dalloc(e, &d.gc_plane, fp.size()));
    if (!fc.empty()) {
      HIPOK(hipMemcpy(d.gc_cell, fc.data(), fc.size() * 4, hipMemcpyHostToDevice));
      HIPOK(hipMemcpy(d.gc_group, fg.data(), fg.size() * 4, hipMemcpyHostToDevice));
      HIPOK(hipMemcpy(d.gc_plane, fp.data(), fp.size(), hipMemcpyHostToDevice));
    }
  }
  std::vector<int32_t> nb((size_t)G * 8, -1), nbc((size_t)G * 8, -1);
  if (t->g_neighbors) nb.assign(t->g_neighbors, t->g_neighbors + (size_t)G * 8);
  const int32_t* nc = t->g_neighbors_ctor ? t->g_neighbors_ctor : t->g_neighbors;
  if (nc) nbc.assign(nc, nc + (size_t)G * 8);
  {
    // checkpoint fingerprint of the tables (checkpoint.h)
    Fp f;
    f.mix((uint64_t)(uint32_t)G << 32 | (uint32_t)L);
    auto ragged = [&](const int32_t* off, const int32_t* v, int n, int per) { f.bytes(off, (size_t)(n + 1) * 4); f.bytes(v, (size_t)off[n] * per * 4); };
    ragged(t->g_light_off, t->light_xy, G, 2);
    ragged(t->light_ctrl_off, t->light_ctrl_xy, L, 2);
    ragged(t->g_ns_off, t->g_ns, G, 1); ragged(t->g_ew_off, t->g_ew, G, 1);
    ragged(t->g_icell_off, t->g_icell_xy, G, 2);
    ragged(t->g_ns_in_off, t->g_ns_in_xy, G, 2); ragged(t->g_ns_out_off, t->g_ns_out_xy, G, 2);
    ragged(t->g_ew_in_off, t->g_ew_in_xy, G, 2); ragged(t->g_ew_out_off, t->g_ew_out_xy, G, 2);
    f.bytes(nb.data(), nb.size() * 4); f.bytes(nbc.data(), nbc.size() * 4);
    e->fp_lights = f.h;
  }
  for (int g = 0; g < G * 4; g++)
    if (nb[g * 2 + 1] >= G || nbc[g * 2 + 1] >= G) return fail(e, TS_E_INVALID, "neighbor group index out of range");
  TRY(up(&d.g_nb, nb.data(), nb.size()));
  TRY(up(&d.g_nb_ctor, nbc.data(), nbc.size()));
  HIPOK(hipStreamSynchronize(e->stream));
  // state: pending_phase = 0 unless DISABLED (intersection_light_group.py:115-116)
  int32_t** zero_fields[] = {&d.gs_trans, &d.gs_clear, &d.gs_ftphase, &d.gs_fttimer, &d.gs_qtimer, &d.gs_gap,
                             &d.gs_last, &d.gs_nsp, &d.gs_ewp, &d.gs_repop, &d.g_slot};
  for (auto f : zero_fields) {
    HIPOK(dalloc(e, f, (size_t)G));
    HIPOK(hipMemsetAsync(*f, 0, (size_t)std::max(G, 1) * 4, e->stream));
  }
  HIPOK(dalloc(e, &d.gs_cur, (size_t)G));
  HIPOK(dalloc(e, &d.gs_pend, (size_t)G));
  HIPOK(hipMemsetAsync(d.gs_cur, 0xFF, (size_t)std::max(G, 1) * 4, e->stream));
  if (e->P.light_algorithm != TS_LIGHTS_DISABLED) HIPOK(hipMemsetAsync(d.gs_pend, 0, (size_t)std::max(G, 1) * 4, e->stream));
  else HIPOK(hipMemsetAsync(d.gs_pend, 0xFF, (size_t)std::max(G, 1) * 4, e->stream));
  dfree(e, d.gclaim_r);
  d.gclaim_r = nullptr;
  HIPOK(dalloc(e, &d.gclaim_r, (size_t)G));
  HIPOK(hipMemsetAsync(d.gclaim_r, 0xFF, (size_t)std::max(G, 1) * 4, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  d.G = G;
  e->lights_set = true;
  e->groups_scheduled = 0;
  if (e->P.light_algorithm == TS_LIGHTS_EXTERNAL) TRY(le_init(e));
  return TS_OK;
}

int ts_schedule_add(ts_handle e, int32_t kind, int32_t count) {
  if (!e || count < 0) return TS_E_INVALID;
  if (kind != TS_AGENT_LIGHT_GROUP && kind != TS_AGENT_NOOP && kind != TS_AGENT_CLOCK && kind != TS_AGENT_RAIN_MANAGER &&
      kind != TS_AGENT_CITY_BLOCK)
    return fail(e, TS_E_INVALID, "bad agent kind");
  if (kind == TS_AGENT_RAIN_MANAGER && (count > 1 || e->rain_manager) && count > 0)
    return fail(e, TS_E_INVALID, "at most one rain manager");
  if (kind == TS_AGENT_LIGHT_GROUP && e->groups_scheduled + count > e->d.G)
    return fail(e, TS_E_INVALID, "more group slots than groups");
  if (kind == TS_AGENT_CLOCK && (count > 1 || e->clock_slot >= 0) && count > 0)
    return fail(e, TS_E_INVALID, "at most one clock agent");
  if (count == 0) return TS_OK;
  if (e->n_sched_vehicles > 0) e->mixed_order = true;
  TRY(ensure_vehicle_capacity(e, e->cap_v, e->n_sched + count));
  std::vector<int8_t> kinds(count, (int8_t)kind);
  std::vector<int32_t> refs(count, 0), slots(count);
  for (int i = 0; i < count; i++) {
    if (kind == TS_AGENT_LIGHT_GROUP) refs[i] = e->groups_scheduled + i;
    if (kind == TS_AGENT_CITY_BLOCK) refs[i] = e->blocks_scheduled + i;
    slots[i] = e->n_sched + i;
  }
  if (kind == TS_AGENT_CITY_BLOCK) {   // the n-th CityBlock scheduled is block n of city_blocks (city_model.py:1738)
    if (e->blocks_scheduled + count > e->cap_bslot) {
      const int nc = (e->blocks_scheduled + count) * 2 + 64;
      TRY(regrow(e, &e->d.bslot, (size_t)e->blocks_scheduled, (size_t)nc));
      e->cap_bslot = nc;
    }
    HIPOK(hipMemcpy(e->d.bslot + e->blocks_scheduled, slots.data(), (size_t)count * 4, hipMemcpyHostToDevice));
    e->blocks_scheduled += count;
  }
  HIPOK(hipMemcpy(e->d.sched_kind + e->n_sched, kinds.data(), count, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->d.sched_ref + e->n_sched, refs.data(), (size_t)count * 4, hipMemcpyHostToDevice));
  if (kind == TS_AGENT_LIGHT_GROUP) {
    HIPOK(hipMemcpy(e->d.g_slot + e->groups_scheduled, slots.data(), (size_t)count * 4, hipMemcpyHostToDevice));
    e->groups_scheduled += count;
  }
  if (kind == TS_AGENT_CLOCK) e->clock_slot = e->n_sched;
  if (kind == TS_AGENT_RAIN_MANAGER) {   // host agent id 0
    TRY(host_agent_register(e, e->n_sched));
    e->rain_manager = true;
  }
  e->n_sched += count;
  return TS_OK;
}

int ts_set_traffic_generator(ts_handle e, const TsTrafficTables* t) {
  if (!e || !t || t->n_blocks < 0 || t->n_zones < 0 || t->n_zones > 8) return TS_E_INVALID;
  if (t->blk_inner_cells && (t->food_consumption_ticks <= 0 || t->waste_production_ticks <= 0))
    return fail(e, TS_E_INVALID, "food_consumption_ticks / waste_production_ticks must be positive");
  if (!e->rng_global.seeded()) return fail(e, TS_E_STATE, "seed the global stream before constructing the traffic generator");
  auto& G = e->gen;
  G.T = *t;
  const int W = e->W, H = e->H;
  auto cellxy = [&](const int32_t* xy, int i, int& out) {
    int x = xy[2 * i], y = xy[2 * i + 1];
    if (x < 0 || x >= W || y < 0 || y >= H) return false;
    out = y * W + x;
    return true;
  };
  G.blk_type.assign(t->blk_type, t->blk_type + t->n_blocks);
  G.blk_entr.assign(t->n_blocks, {});
  for (int b = 0; b < t->n_blocks; b++) {
    for (int k = t->blk_entr_off[b]; k < t->blk_entr_off[b + 1]; k++) {
      int c;
      if (!cellxy(t->blk_entr_xy, k, c)) return fail(e, TS_E_INVALID, "block entrance out of bounds");
      G.blk_entr[b].push_back(c);
    }
    if (G.blk_entr[b].empty())
      return fail(e, TS_E_UNSUPPORTED, "a city block without entrances (random.choice([]) raises in the reference)");
  }
  G.hw_in.clear(); G.hw_out.clear();
  for (int k = 0; k < t->n_highway_entrances; k++) { int c; if (!cellxy(t->highway_entrances_xy, k, c)) return TS_E_INVALID; G.hw_in.push_back(c); }
  for (int k = 0; k < t->n_highway_exits; k++) { int c; if (!cellxy(t->highway_exits_xy, k, c)) return TS_E_INVALID; G.hw_out.push_back(c); }
  if ((G.hw_in.empty() || G.hw_out.empty()) && t->passing_population_per_day > 0)
    return fail(e, TS_E_UNSUPPORTED, "through traffic needs highway entrances and exits");
  for (int z = 0; z < t->n_zones; z++) if (t->zones[z].n_internal < 0 || t->zones[z].n_internal > 8) return TS_E_INVALID;
  e->blocks.clear();
  if (t->blk_inner_cells) {
    if (!t->blk_service_off || !t->blk_service_xy) return fail(e, TS_E_INVALID, "blk_service_* tables missing");
    e->blocks.resize(t->n_blocks);
    for (int b = 0; b < t->n_blocks; b++) {
      auto& B = e->blocks[b];
      B.cells = t->blk_inner_cells[b];
      B.needs_food = (t->needs_food_type_mask >> t->blk_type[b]) & 1;
      B.produces_waste = (t->produces_waste_type_mask >> t->blk_type[b]) & 1;
      B.max_food = (double)B.cells * t->food_capacity_per_cell;
      B.max_waste = (double)B.cells * t->waste_capacity_per_cell;
      B.food = B.max_food; B.waste = 0.0;
      B.food_rate = (double)B.cells / (double)t->food_consumption_ticks;
      B.waste_rate = (double)B.cells / (double)t->waste_production_ticks;
      for (int k = t->blk_service_off[b]; k < t->blk_service_off[b + 1]; k++) {
        int c;
        if (!cellxy(t->blk_service_xy, k, c)) return fail(e, TS_E_INVALID, "service road cell out of bounds");
        B.service_cells.push_back(c);
      }
    }
  }
  const int n_sv = t->total_service_vehicles_food + t->total_service_vehicles_waste;
  if (n_sv < 0 || t->total_service_vehicles_food < 0 || t->total_service_vehicles_waste < 0) return TS_E_INVALID;
  if (n_sv > 0 && (e->blocks.empty() || G.hw_in.empty()))
    return fail(e, TS_E_UNSUPPORTED, "service vehicles need the block tables and highway entrances");
  e->sv_live.assign((size_t)n_sv, 0);
  e->svc.clear(); e->parked_cells.clear();
  if (n_sv > 0 && !e->d.arr) {
    e->d.arr_cap = 1 << 16;
    HIPOK(dalloc(e, &e->d.arr, (size_t)e->d.arr_cap * 3));
  }
  {
    // checkpoint fingerprint of the tables (checkpoint.h): every scalar and array the generator, the blocks and the
    // service fleet read
    Fp f;
    // (field by field: the structs have padding)
    const int32_t ints[] = {t->n_blocks, t->n_highway_entrances, t->n_highway_exits, t->internal_population_per_day,
                            t->passing_population_per_day, t->start_offset_seconds, t->n_zones, t->total_service_vehicles_food,
                            t->total_service_vehicles_waste, t->service_load_time, t->gradual_city_block_resources,
                            t->food_consumption_ticks, t->waste_production_ticks, t->needs_food_type_mask,
                            t->produces_waste_type_mask, t->statistics_update_interval, t->blk_inner_cells ? 1 : 0};
    const double dbls[] = {t->service_max_load_food, t->service_max_load_waste, t->food_capacity_per_cell, t->waste_capacity_per_cell};
    f.bytes(ints, sizeof(ints)); f.bytes(dbls, sizeof(dbls));
    for (int z = 0; z < t->n_zones; z++) {
      const TsTrafficZone& Z = t->zones[z];
      const int32_t zi[3] = {Z.start_hour, Z.end_hour, Z.n_internal};
      f.bytes(zi, sizeof(zi)); f.bytes(&Z.through_distribution, 8);
      f.bytes(Z.origin_type, sizeof(Z.origin_type)); f.bytes(Z.dest_type, sizeof(Z.dest_type)); f.bytes(Z.fraction, sizeof(Z.fraction));
    }
    const int nb = t->n_blocks;
    f.bytes(t->blk_type, (size_t)nb * 4);
    f.bytes(t->blk_entr_off, (size_t)(nb + 1) * 4); f.bytes(t->blk_entr_xy, (size_t)t->blk_entr_off[nb] * 8);
    f.bytes(t->highway_entrances_xy, (size_t)std::max(0, t->n_highway_entrances) * 8);
    f.bytes(t->highway_exits_xy, (size_t)std::max(0, t->n_highway_exits) * 8);
    if (t->blk_inner_cells) {
      f.bytes(t->blk_inner_cells, (size_t)nb * 4);
      f.bytes(t->blk_service_off, (size_t)(nb + 1) * 4); f.bytes(t->blk_service_xy, (size_t)t->blk_service_off[nb] * 8);
    }
    e->fp_traffic = f.h;
  }
  G.pending.clear();
  G.current_day = 0;
  G.armed = true;
  generate_day(e, 0);
  e->words_uploaded = e->rng_global.pos();
  return TS_OK;
}

int ts_seed(ts_handle e, int32_t stream, const uint32_t* mt, uint32_t index) {
  if (!e || !mt || stream < 0 || stream > 1 || index > 624) return TS_E_INVALID;
  (stream == TS_RNG_GLOBAL ? e->rng_global : e->rng_sched).seed(mt, index);
  if (stream == TS_RNG_GLOBAL) { e->words_uploaded = e->rng_global.pos(); e->take_n = 0; }
  return TS_OK;
}
int ts_seed_int(ts_handle e, int32_t stream, uint64_t seed) {
  if (!e || stream < 0 || stream > 1) return TS_E_INVALID;
  (stream == TS_RNG_GLOBAL ? e->rng_global : e->rng_sched).seed_u64(seed);
  if (stream == TS_RNG_GLOBAL) { e->words_uploaded = e->rng_global.pos(); e->take_n = 0; }
  return TS_OK;
}
int ts_rng_state(ts_handle e, int32_t stream, uint32_t* mt_out, uint32_t* index_out) {
  if (!e || stream < 0 || stream > 1 || !mt_out || !index_out) return TS_E_INVALID;
  MTPipe& r = stream == TS_RNG_GLOBAL ? e->rng_global : e->rng_sched;
  if (!r.seeded()) return fail(e, TS_E_STATE, "stream not seeded");
  r.state(mt_out, index_out);
  return TS_OK;
}

// shared tail of the two ts_add_vehicles entries: `enc` holds the 2-bit direction words, every
// vehicle starting on a fresh word; poff[i] is relative to enc.
static int add_vehicles_core(ts_handle e, int n, std::vector<int32_t>& start, std::vector<int32_t>& goal,
                             std::vector<int32_t>& pop, std::vector<int32_t>& plen, std::vector<uint32_t>& poff,
                             std::vector<uint32_t>& enc) {
  const size_t words = enc.size();
  TRY(pool_make_room(e, words + 1));
  for (int i = 0; i < n; i++) poff[i] += (uint32_t)e->pool_used;
  // start cells shared inside the batch must be appended to the cell list in spawn order
  std::vector<uint8_t> serial(n, 0);
  {
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return start[a] < start[b] || (start[a] == start[b] && a < b); });
    for (int q = 1; q < n; q++)
      if (start[order[q]] == start[order[q - 1]]) { serial[order[q]] = 1; serial[order[q - 1]] = 1; }
  }
  TRY(ensure_vehicle_capacity(e, e->n_vehicles_total + n, e->n_sched + n));
  TRY(ensure_pool(e, e->pool_used + words + 1));
  if (n > e->cap_overflow) {
    TRY(regrow(e, &e->d_overflow, 0, (size_t)n + 1));
    e->cap_overflow = n;
  }
  hipStream_t st = e->stream;
  int32_t *ds = nullptr, *dg = nullptr, *dp = nullptr, *dl = nullptr;
  uint32_t* dof = nullptr;
  uint8_t* dser = nullptr;
  Scratch tmp;
  HIPOK(tmp.get(&ds, (size_t)n)); HIPOK(tmp.get(&dg, (size_t)n)); HIPOK(tmp.get(&dp, (size_t)n));
  HIPOK(tmp.get(&dl, (size_t)n)); HIPOK(tmp.get(&dof, (size_t)n)); HIPOK(tmp.get(&dser, (size_t)n));
  HIPOK(hipMemcpyAsync(ds, start.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(dg, goal.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(dp, pop.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(dl, plen.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(dof, poff.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(dser, serial.data(), (size_t)n, hipMemcpyHostToDevice, st));
  if (words) HIPOK(hipMemcpyAsync(e->d.pool + e->pool_used, enc.data(), words * 4, hipMemcpyHostToDevice, st));
  HIPOK(hipMemsetAsync(e->d_total, 0, sizeof(int), st));
  SpawnArgs a{ds, dg, dp, dl, dof, dser};
  e->d.tl_step = (int)e->C.step_count;
  hipLaunchKernelGGL(k_spawn, dim3(nblk(n)), dim3(BLK), 0, st, e->d, e->P, a, n, e->n_vehicles_total, e->n_active,
                     e->n_sched, e->C.elapsed, e->d_overflow, e->d_total, (e->d.amap && e->amap_valid) ? 1 : 0);
  TRY(read_back(e, &e->hm->scratch, e->d_total, sizeof(int)));
  if (e->hm->scratch > 0) hipLaunchKernelGGL(k_spawn_serial, dim3(1), dim3(64), 0, st, e->d, e->d_overflow, e->hm->scratch);
  HIPOK(hipStreamSynchronize(st));
  // live_* counters (city_model.py:1910-1918)
  long long add_int = 0, add_thr = 0;
  for (int i = 0; i < n; i++) { add_int += pop[i] == TS_POP_INTERNAL; add_thr += pop[i] == TS_POP_THROUGH; }
  if (add_int || add_thr) {
    TRY(sync_counters(e));
    e->hcnt->live_internal += add_int; e->hcnt->live_through += add_thr;
    HIPOK(hipMemcpy(e->d.cnt, e->hcnt, sizeof(DevCnt), hipMemcpyHostToDevice));
  }
  e->pool_used += words;
  TRY(pool_to_device(e));
  e->n_vehicles_total += n; e->n_active += n; e->n_sched += n; e->n_sched_vehicles += n;
  return TS_OK;
}

// VehicleAgent.__init__ for one vehicle whose path the engine plans itself: place_vehicle, then
// self.path = self._compute_path() with city._path_cache (vehicle_base.py:78-81, 143-167)
static int add_vehicle_planned(ts_handle e, int start, int goal, int pop_type) {
  if (start == goal) e->standing_possible = true;   // it despawns inside the next decide phase (tick())
  std::vector<int32_t> s1{start}, g1{goal}, p1{pop_type}, l1{0};
  std::vector<uint32_t> o1{0}, enc;
  TRY(add_vehicles_core(e, 1, s1, g1, p1, l1, o1, enc));
  return plan_vehicle(e, e->n_vehicles_total - 1, start, goal);
}

// self.path = self._compute_path() for a vehicle standing on `start` with target `goal` (both already on the
// device): city._path_cache first, then the phase 0-4 planner on the maps as they are now
static int plan_vehicle(ts_handle e, int vid, int start, int goal) {
  const uint64_t key = ((uint64_t)(uint32_t)start << 32) | (uint32_t)goal;
  Dev& d = e->d;
  if (e->P.pathfinding_cache) {
    auto it = e->path_cache.find(key);
    if (it != e->path_cache.end()) {
      const auto& cp = it->second;
      TRY(pool_make_room(e, cp.words.size() + 1));
      uint32_t off = (uint32_t)e->pool_used;
      int len = cp.len, zero = 0;
      if (!cp.words.empty()) HIPOK(hipMemcpy(d.pool + off, cp.words.data(), cp.words.size() * 4, hipMemcpyHostToDevice));
      HIPOK(hipMemcpy(d.path_off + vid, &off, 4, hipMemcpyHostToDevice));
      HIPOK(hipMemcpy(d.path_len + vid, &len, 4, hipMemcpyHostToDevice));
      HIPOK(hipMemcpy(d.path_cur + vid, &zero, 4, hipMemcpyHostToDevice));
      e->pool_used += cp.words.size();
      return pool_to_device(e);
    }
  }
  if (!e->density_valid) { TRY(ensure_density(e, d.occ_snap)); e->density_valid = true; }
  TRY(ensure_slots(e));
  TRY(ensure_amap(e));
  for (int attempt = 0; attempt < 3; attempt++) {
    hipLaunchKernelGGL(k_spawn_plan, dim3(1), dim3(64), 0, e->stream, d, e->P, e->slots, vid, e->d_status);
    TRY(read_back(e, &e->hm->scratch, e->d_status, sizeof(int)));
    if (e->hm->scratch != -2) break;
    TRY(pool_make_room(e, (size_t)e->slots.cap + (1u << 16)));  // pool full: make room and plan again
  }
  const int len = e->hm->scratch;
  if (len == -2) return fail(e, TS_E_CAPACITY, "path pool exhausted while planning a spawn");
  if (len < 0) return fail(e, TS_E_CAPACITY, "an A* search exceeded its heap or path buffers");
  TRY(pool_from_device(e));
  uint16_t fl = 0;
  HIPOK(hipMemcpy(&fl, d.flags + vid, 2, hipMemcpyDeviceToHost));
  if (e->P.pathfinding_cache && len > 0 && !(fl & (VF_OVER | VF_DETOUR))) {
    ts_engine::CachedPath cp;
    cp.len = len;
    cp.words.resize((size_t)path_words(len));
    uint32_t off = 0;
    HIPOK(hipMemcpy(&off, d.path_off + vid, 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(cp.words.data(), d.pool + off, cp.words.size() * 4, hipMemcpyDeviceToHost));
    e->path_cache[key] = std::move(cp);
  }
  return TS_OK;
}

static int add_vehicles_any(ts_handle e, int32_t n, const int32_t* start_xy, const int32_t* goal_xy,
                            const int32_t* population_type, const int32_t* off32, const int32_t* path_xy,
                            const int64_t* off64, const uint8_t* path_dirs) {
  if (!e || n < 0 || (n > 0 && (!start_xy || !goal_xy))) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (n == 0) return TS_OK;
  const int W = e->W, H = e->H;
  if (!(off32 && path_xy) && !(off64 && path_dirs)) {
    // the reference's own path: each vehicle is placed, then plans on the maps as they are at that moment
    for (int i = 0; i < n; i++) {
      int sx = start_xy[2 * i], sy = start_xy[2 * i + 1], gx = goal_xy[2 * i], gy = goal_xy[2 * i + 1];
      if (sx < 0 || sx >= W || sy < 0 || sy >= H || gx < 0 || gx >= W || gy < 0 || gy >= H)
        return fail(e, TS_E_INVALID, "vehicle start/goal out of bounds");
      if (sx == gx && sy == gy) e->standing_possible = true;   // it despawns inside the next decide phase (tick())
      if ((long long)e->n_sched + 1 >= (long long)RANK_MASK) return fail(e, TS_E_CAPACITY, "schedule exceeds 2^24 agents");
      TRY(add_vehicle_planned(e, sy * W + sx, gy * W + gx, population_type ? population_type[i] : TS_POP_UNDEFINED));
    }
    return TS_OK;
  }
  if ((long long)e->n_sched + n >= (long long)RANK_MASK) return fail(e, TS_E_CAPACITY, "schedule exceeds 2^24 agents");
  std::vector<int32_t> start(n), goal(n), pop(n), plen(n);
  std::vector<uint32_t> poff(n);
  auto O = [&](int i) -> long long { return off32 ? (long long)off32[i] : (long long)off64[i]; };
  size_t words = 0;
  for (int i = 0; i < n; i++) {
    long long len = O(i + 1) - O(i);
    if (len < 0 || len > 0x7FFFFFFF) return fail(e, TS_E_INVALID, "path_off must be non-decreasing");
    words += path_words((size_t)len);
  }
  if (e->pool_used + words >= (1ull << 32)) return fail(e, TS_E_CAPACITY, "path pool exceeds 2^32 words");
  std::vector<uint32_t> enc(words, 0);
  size_t wpos = 0;
  for (int i = 0; i < n; i++) {
    int sx = start_xy[2 * i], sy = start_xy[2 * i + 1], gx = goal_xy[2 * i], gy = goal_xy[2 * i + 1];
    if (sx < 0 || sx >= W || sy < 0 || sy >= H || gx < 0 || gx >= W || gy < 0 || gy >= H)
      return fail(e, TS_E_INVALID, "vehicle start/goal out of bounds");
    if (sx == gx && sy == gy) e->standing_possible = true;
    start[i] = sy * W + sx; goal[i] = gy * W + gx;
    pop[i] = population_type ? population_type[i] : TS_POP_UNDEFINED;
    const long long o = O(i);
    const int len = (int)(O(i + 1) - o);
    plen[i] = len;
    poff[i] = (uint32_t)wpos;
    int px = sx, py = sy;
    for (int k = 0; k < len; k++) {
      int dir;
      if (path_xy && off32) {
        int x = path_xy[2 * (o + k)], y = path_xy[2 * (o + k) + 1];
        dir = dir_of_step(x - px, y - py);
        if (dir < 0) return fail(e, TS_E_INVALID, "explicit path is not a 4-adjacent chain");
        px = x; py = y;
      } else {
        dir = path_dirs[o + k];
        if (dir > 3) return fail(e, TS_E_INVALID, "direction code out of range");
        px += dir_dx(dir); py += dir_dy(dir);
      }
      if (px < 0 || px >= W || py < 0 || py >= H) return fail(e, TS_E_INVALID, "explicit path leaves the grid");
      path_put(enc.data() + wpos, k, dir);
    }
    wpos += path_words((size_t)len);
  }
  return add_vehicles_core(e, n, start, goal, pop, plen, poff, enc);
}

int ts_add_vehicles(ts_handle e, int32_t n, const int32_t* start_xy, const int32_t* goal_xy,
                    const int32_t* population_type, const int32_t* path_off, const int32_t* path_xy) {
  return add_vehicles_any(e, n, start_xy, goal_xy, population_type, path_off, path_xy, nullptr, nullptr);
}
int ts_add_vehicles_dirs(ts_handle e, int32_t n, const int32_t* start_xy, const int32_t* goal_xy,
                         const int32_t* population_type, const int64_t* path_off, const uint8_t* path_dirs) {
  return add_vehicles_any(e, n, start_xy, goal_xy, population_type, nullptr, nullptr, path_off, path_dirs);
}

int ts_remove_vehicle(ts_handle e, int32_t spawn_idx, int32_t population_type) {
  if (!e) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (population_type != TS_POP_INTERNAL && population_type != TS_POP_THROUGH) population_type = TS_POP_UNDEFINED;
  if (spawn_idx < 0 || spawn_idx >= e->n_vehicles_total) return fail(e, TS_E_INVALID, "no such live vehicle");
  Dev& d = e->d;
  uint16_t fl = 0;
  HIPOK(hipMemcpy(&fl, d.flags + spawn_idx, 2, hipMemcpyDeviceToHost));
  if (!(fl & VF_ALIVE)) return fail(e, TS_E_INVALID, "no such live vehicle");
  if (fl & VF_SVC) return fail(e, TS_E_UNSUPPORTED, "service vehicles cannot be removed by the host");
  d.tl_step = (int)e->C.step_count;
  hipLaunchKernelGGL(k_remove_one, dim3(1), dim3(64), 0, e->stream, d, spawn_idx, (int)population_type, e->C.elapsed);
  if (d.tlog) { e->tl_pending++; TRY(tl_seal(e)); }   // a host removal is a group of its own
  // the lists close up at once (the reference's list.remove / schedule.remove): the next tick shuffles the live keys
  TRY(compact_lists(e, 1));
  HIPOK(hipMemsetAsync(&d.cnt->deaths, 0, sizeof(int), e->stream));
  e->amap_valid = false;
  return sync_counters(e);
}

int ts_upload_map(ts_handle e, int32_t which, const int8_t* src) {
  if (!e || !src) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  int8_t* m = which == TS_MAP_STOP ? e->d.stop : which == TS_MAP_RAIN ? e->d.rain : nullptr;
  if (!m) return fail(e, TS_E_INVALID, "only stop_map and rain_map are host-writable");
  HIPOK(hipMemcpy(m, src, e->N, hipMemcpyHostToDevice));
  e->amap_valid = false;
  if (which == TS_MAP_STOP) {
    hipLaunchKernelGGL(k_plane_to_cells, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, e->d.cell, e->N, e->d.stop, 1);
    HIPOK(hipStreamSynchronize(e->stream));
  }
  return TS_OK;
}
int ts_debug_set_occupancy(ts_handle e, const int8_t* src) {
  if (!e || !src) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  HIPOK(hipMemcpy(e->d.occ, src, e->N, hipMemcpyHostToDevice));
  e->amap_valid = false;
  hipLaunchKernelGGL(k_plane_to_cells, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, e->d.cell, e->N, e->d.occ, 0);
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_step(ts_handle e, int32_t n_ticks) {
  if (!e || n_ticks < 0) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (!e->rng_global.seeded() || !e->rng_sched.seeded()) return fail(e, TS_E_STATE, "both RNG streams must be seeded before step");
  if (e->groups_scheduled != e->d.G && e->d.G > 0 && e->groups_scheduled != 0)
    return fail(e, TS_E_STATE, "every light group must be scheduled (or none)");
  if (e->fatal) return e->fatal;   // model.step() raised in the reference: the run is over
  for (int t = 0; t < n_ticks; t++) TRY(tick(e));
  return TS_OK;
}

int ts_num_vehicles(ts_handle e) { return e ? e->n_active : TS_E_INVALID; }
int ts_num_groups(ts_handle e) { return e ? e->d.G : TS_E_INVALID; }
int ts_num_scheduled(ts_handle e) { return e ? e->n_sched : TS_E_INVALID; }

int ts_download_map(ts_handle e, int32_t which, int8_t* dst) {
  if (!e || !dst) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  if (which == TS_MAP_STUCK) {   // lives only in the cell records
    Scratch tmp;
    int8_t* plane = nullptr;
    HIPOK(tmp.get(&plane, (size_t)e->N));
    hipLaunchKernelGGL(k_cells_to_plane, dim3(nblk((long long)e->N)), dim3(BLK), 0, e->stream, e->d.cell, e->N, plane);
    return read_back(e, dst, plane, (size_t)e->N);
  }
  const int8_t* m = which == TS_MAP_OCCUPANCY ? e->d.occ : which == TS_MAP_STOP ? e->d.stop
                   : which == TS_MAP_RAIN ? e->d.rain : nullptr;
  if (!m) return TS_E_INVALID;
  HIPOK(hipMemcpy(dst, m, e->N, hipMemcpyDeviceToHost));
  return TS_OK;
}

int ts_download_density(ts_handle e, float* dst) {
  if (!e || !dst) return TS_E_INVALID;
  float *t0 = nullptr, *t1 = nullptr, *dn = nullptr;
  size_t N = e->N;
  Scratch tmp;
  HIPOK(tmp.get(&t0, N)); HIPOK(tmp.get(&t1, N)); HIPOK(tmp.get(&dn, N));
  const int r = e->P.vehicle_awareness_range;
  hipLaunchKernelGGL(k_density_pass0, dim3(nblk(N)), dim3(BLK), 0, e->stream, e->d.occ, e->d.is_road, e->W, e->H, r, t0, t1);
  hipLaunchKernelGGL(k_density_pass1, dim3(nblk(N)), dim3(BLK), 0, e->stream, t0, t1, e->W, e->H, r, dn);
  return read_back(e, dst, dn, N * 4);
}

int ts_download_vehicles(ts_handle e, int32_t* rows, int32_t cap_rows) {
  if (!e || !rows) return TS_E_INVALID;
  int n = e->n_active;
  if (n > cap_rows) return TS_E_CAPACITY;
  if (n == 0) return 0;
  Scratch tmp;
  int32_t* drows = nullptr;
  HIPOK(tmp.get(&drows, (size_t)n * TS_V_NFIELDS));
  hipLaunchKernelGGL(k_rows, dim3(nblk(n)), dim3(BLK), 0, e->stream, e->d, n, e->d_crc, drows);
  TRY(read_back(e, rows, drows, (size_t)n * TS_V_NFIELDS * 4));
  return n;
}

int ts_num_spawned(ts_handle e) { return e ? e->n_vehicles_total : TS_E_INVALID; }
int ts_download_vehicle_meta(ts_handle e, int32_t* rows, int32_t cap_rows) {
  if (!e || !rows) return TS_E_INVALID;
  const int n = e->n_active;
  if (n > cap_rows) return TS_E_CAPACITY;
  if (n == 0) return 0;
  Scratch tmp;
  int32_t* drows = nullptr;
  HIPOK(tmp.get(&drows, (size_t)n * TS_M_NFIELDS));
  hipLaunchKernelGGL(k_meta_rows, dim3(nblk(n)), dim3(BLK), 0, e->stream, e->d, n, drows);
  TRY(read_back(e, rows, drows, (size_t)n * TS_M_NFIELDS * 4));
  if (!e->svc.empty()) {
    std::unordered_map<int, int> type_of;
    for (const auto& v : e->svc) type_of[v.vid] = v.type;
    for (int i = 0; i < n; i++) {
      int32_t* r = rows + (size_t)i * TS_M_NFIELDS;
      if (r[TS_M_SERVICE_PHASE] >= 0) { auto it = type_of.find(r[TS_M_SPAWN_IDX]); if (it != type_of.end()) r[TS_M_VEHICLE_TYPE] = it->second; }
    }
  }
  return n;
}
int ts_download_service_vehicles(ts_handle e, int32_t* spawn_idx, double* loads, int32_t* block, int32_t cap) {
  if (!e || !spawn_idx || !loads || !block) return TS_E_INVALID;
  if ((int)e->svc.size() > cap) return TS_E_CAPACITY;
  std::vector<const ts_engine::SvcVeh*> order;
  for (const auto& v : e->svc) order.push_back(&v);
  std::sort(order.begin(), order.end(), [](const ts_engine::SvcVeh* a, const ts_engine::SvcVeh* b) { return a->vid < b->vid; });
  int n = 0;
  for (const auto* v : order) {
    spawn_idx[n] = v->vid; loads[2 * n] = v->load; loads[2 * n + 1] = v->max_load; block[n] = v->block;
    n++;
  }
  return n;
}
int ts_download_path(ts_handle e, int32_t active_pos, int32_t* xy, int32_t cap_cells) {
  if (!e || active_pos < 0 || active_pos >= e->n_active) return TS_E_INVALID;
  int vid, cur, len;
  HIPOK(hipMemcpy(&vid, e->d.active + active_pos, 4, hipMemcpyDeviceToHost));
  HIPOK(hipMemcpy(&cur, e->d.path_cur + vid, 4, hipMemcpyDeviceToHost));
  HIPOK(hipMemcpy(&len, e->d.path_len + vid, 4, hipMemcpyDeviceToHost));
  int n = len - cur;
  if (!xy) return n;
  if (n > cap_cells) return TS_E_CAPACITY;
  if (n == 0) return 0;
  Scratch tmp;
  int32_t* dxy = nullptr;
  HIPOK(tmp.get(&dxy, (size_t)n * 2));
  hipLaunchKernelGGL(k_path_cells, dim3(1), dim3(64), 0, e->stream, e->d, vid, dxy);
  TRY(read_back(e, xy, dxy, (size_t)n * 8));
  return n;
}

int ts_download_groups(ts_handle e, int32_t* rows) {
  if (!e || !rows) return TS_E_INVALID;
  int G = e->d.G;
  if (G == 0) return 0;
  Scratch tmp;
  int32_t* drows = nullptr;
  HIPOK(tmp.get(&drows, (size_t)G * TS_G_NFIELDS));
  hipLaunchKernelGGL(k_group_rows, dim3(nblk(G)), dim3(BLK), 0, e->stream, e->d, drows);
  TRY(read_back(e, rows, drows, (size_t)G * TS_G_NFIELDS * 4));
  return G;
}

int ts_num_blocks(ts_handle e) { return e ? (int)e->blocks.size() : TS_E_INVALID; }
int ts_download_blocks(ts_handle e, double* rows) {
  if (!e || !rows) return TS_E_INVALID;
  for (size_t b = 0; b < e->blocks.size(); b++) { rows[2 * b] = e->blocks[b].food; rows[2 * b + 1] = e->blocks[b].waste; }
  return TS_OK;
}
int ts_group_links(ts_handle e, int32_t group, int32_t repopulate) {
  if (!e || group < 0 || group >= e->d.G) return TS_E_INVALID;
  int v = 0;
  if (repopulate) { v = 1; HIPOK(hipMemcpy(e->d.gs_repop + group, &v, 4, hipMemcpyHostToDevice)); return 1; }
  HIPOK(hipStreamSynchronize(e->stream));
  HIPOK(hipMemcpy(&v, e->d.gs_repop + group, 4, hipMemcpyDeviceToHost));
  return v ? 1 : 0;
}
int ts_add_service_vehicle(ts_handle e, int32_t x, int32_t y, int32_t service_type) {
  if (!e || x < 0 || x >= e->W || y < 0 || y >= e->H) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (service_type != TS_TRIP_SERVICE_FOOD && service_type != TS_TRIP_SERVICE_WASTE) return fail(e, TS_E_INVALID, "service_type");
  if (e->blocks.empty()) return fail(e, TS_E_STATE, "service vehicles need the block tables (ts_set_traffic_generator)");
  if (e->fatal) return e->fatal;
  return spawn_service_at(e, y * e->W + x, service_type, -1);
}
int ts_rain_info(ts_handle e, TsRainInfo* out) {
  if (!e || !out) return TS_E_INVALID;
  out->has_manager = e->rain_manager; out->n_rains = (int32_t)e->rains.size();
  out->cooldown = e->rain_cooldown_left; out->counter = e->rain_counter;
  return TS_OK;
}
int ts_rain_spawn(ts_handle e) {
  if (!e) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (!e->rain_manager) return fail(e, TS_E_STATE, "no RainManager is scheduled");
  if (!e->rng_global.seeded()) return fail(e, TS_E_STATE, "seed the global stream first");
  HIPOK(hipStreamSynchronize(e->stream));
  return rain_add_random(e);
}
int ts_counters(ts_handle e, TsCounters* out) {
  if (!e || !out) return TS_E_INVALID;
  TRY(sync_counters(e));
  *out = e->C;
  return TS_OK;
}

int ts_cached_stats(ts_handle e, TsCachedStats* out) {
  if (!e || !out) return TS_E_INVALID;
  *out = e->gen.cs;
  return TS_OK;
}

int ts_set_replan_sharding(ts_handle e, int32_t rank, int32_t world, ts_exchange_fn fn, void* user) {
  if (!e || world < 1 || rank < 0 || rank >= world) return TS_E_INVALID;
  if (world > 1 && !fn) return fail(e, TS_E_INVALID, "sharded replans need an exchange callback");
  e->dist_rank = rank; e->dist_world = world; e->dist_fn = world > 1 ? fn : nullptr; e->dist_user = user; e->dist_dev = false;
  return TS_OK;
}
int ts_set_replan_sharding_device(ts_handle e, int32_t rank, int32_t world, ts_exchange_fn fn, void* user) {
  int rc = ts_set_replan_sharding(e, rank, world, fn, user);
  if (rc == TS_OK) e->dist_dev = world > 1;
  return rc;
}

// profiling hook (not part of include/trafficsim.h): the eight debug words the last replanning / search kernel left
int ts_debug_read(ts_handle e, int32_t* out8) {
  if (!e || !out8) return TS_E_INVALID;
  HIPOK(hipStreamSynchronize(e->stream));
  DevCnt c;
  HIPOK(hipMemcpy(&c, e->d.cnt, sizeof(DevCnt), hipMemcpyDeviceToHost));
  // words 0-1 / 2-3: the last ts_astar's cycles / 100 MHz ticks; 4: deepest heap; 5: longest search; 6-7: spilled expansions
  const long long w64[4] = {c.probe_cycles, c.probe_wall, ((long long)c.max_search_exp << 32) | (unsigned)c.max_heap, c.spill_exp};
  memcpy(out8, w64, sizeof(w64));
  if (getenv("TS_KPROF")) {
    long long pr[8];
    HIPOK(hipMemcpy(pr, e->d.cnt->prof, sizeof(pr), hipMemcpyDeviceToHost));
    fprintf(stderr, "[kprof] top %lld | issue loads %lld | sift-down %lld | goal+stale %lld | evaluate %lld | commit stores %lld | pushes %lld | loop %lld\n", pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], pr[7]);
  }
  return TS_OK;
}

// debugging hook (not part of include/trafficsim.h): the quad searcher's counters over this engine's quad passes, as int64 -
// [0] entries given to k_replan_quad, [1] hand-backs to k_replan, [2 .. 7] hand-backs by reason (window / g, heap, expansion
// budget, path buffer, policy bail, policy overflow), [8] searches started, [9] table-epoch wraps, [10] quad passes, [11] sift-down
// steps that consulted the third heap level fetched ahead, [12] blocking sift-down steps below it.  Writes
// min(n, TS_QUAD_STATS_N) words and returns TS_QUAD_STATS_N.
constexpr int TS_QUAD_STATS_N = 13;
int ts_debug_quad_stats(ts_handle e, int64_t* out, int32_t n) {
  if (!e || (!out && n > 0) || n < 0) return TS_E_INVALID;
  const long long* qs = e->quad_stats;
  const long long v[TS_QUAD_STATS_N] = {e->quad_jobs, e->quad_fallbacks, qs[QST_WINDOW], qs[QST_HEAP], qs[QST_BUDGET], qs[QST_PATHBUF],
                                        qs[QST_BAIL], qs[QST_OVERFLOW], qs[QST_SEARCHES], qs[QST_WRAPS], e->quad_passes,
                                        qs[QST_STEP3], qs[QST_DEEP]};
  for (int k = 0; k < std::min<int>(n, TS_QUAD_STATS_N); k++) out[k] = v[k];
  return TS_QUAD_STATS_N;
}

// debugging hook (not part of include/trafficsim.h): the table arena k_replan and the quads share, as int64 - [0] hand-overs to the
// quads, [1] hand-overs to k_replan's waves, [2] clears run (none unless a big dist was seen or TS_ARENA_CLEAR=1), [3] the big-dist flag
// as it stands on the device, [4] hand-overs that found it set, [5] the quads' tables alias the arena, [6] the quads hold it now.
// Writes min(n, TS_ARENA_INFO_N) words and returns TS_ARENA_INFO_N.
constexpr int TS_ARENA_INFO_N = 7;
int ts_debug_arena_info(ts_handle e, int64_t* out, int32_t n) {
  if (!e || (!out && n > 0) || n < 0) return TS_E_INVALID;
  uint32_t big = 0;
  if (e->slots_ready) TRY(read_back(e, &big, e->slots.big_flag, sizeof(big)));
  const long long v[TS_ARENA_INFO_N] = {e->arena_to_q, e->arena_to_w, e->arena_clears, (long long)big, e->arena_big_seen,
                                        e->arena_shared ? 1 : 0, e->arena_quad ? 1 : 0};
  for (int k = 0; k < std::min<int>(n, TS_ARENA_INFO_N); k++) out[k] = v[k];
  return TS_ARENA_INFO_N;
}
// debugging hook (not part of include/trafficsim.h): the quads' walks back along found paths over this engine's quad passes, as
// int64 - [0] walks, [1] cells written, [2] HBM round trips (two cells each, the last one of an odd walk one), [3] walks of odd
// length (they ended on the first cell of a pair), [4] walks of one cell, [5] walks of two.  Returns TS_QUAD_WALK_N.
constexpr int TS_QUAD_WALK_N = 6;
int ts_debug_quad_walks(ts_handle e, int64_t* out, int32_t n) {
  if (!e || (!out && n > 0) || n < 0) return TS_E_INVALID;
  const long long* qs = e->quad_stats;
  const long long v[TS_QUAD_WALK_N] = {qs[QST_WALKS], qs[QST_WALK_CELLS], qs[QST_WALK_TRIPS], qs[QST_WALK_ODD], qs[QST_WALK_LEN1], qs[QST_WALK_LEN2]};
  for (int k = 0; k < std::min<int>(n, TS_QUAD_WALK_N); k++) out[k] = v[k];
  return TS_QUAD_WALK_N;
}

int ts_set_device(int32_t device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return TS_E_DEVICE;
  g_device = device;
  return hipSetDevice(device) == hipSuccess ? TS_OK : TS_E_DEVICE;
}
int ts_profile_enable(ts_handle e, int32_t on) {
  if (!e) return TS_E_INVALID;
  e->prof = on != 0;
  if (on) { memset(e->prof_ms, 0, sizeof(e->prof_ms)); memset(e->prof_launches, 0, sizeof(e->prof_launches));
            memset(e->prof_items, 0, sizeof(e->prof_items)); }
  return TS_OK;
}
int ts_profile_count(void) { return PK_COUNT; }
const char* ts_profile_name(int32_t id) { return id >= 0 && id < PK_COUNT ? PK_NAMES[id] : ""; }
int ts_profile_get(ts_handle e, int32_t id, double* total_ms, int64_t* launches, int64_t* items) {
  if (!e || id < 0 || id >= PK_COUNT) return TS_E_INVALID;
  if (total_ms) *total_ms = e->prof_ms[id];
  if (launches) *launches = e->prof_launches[id];
  if (items) *items = e->prof_items[id];
  return TS_OK;
}

// debugging hook (not part of include/trafficsim.h; profiles/tail_probe.py): n searches (start cell, goal cell, soft; no step limit,
// on the flow) on `threads` threads of the host tail's pool (0: all), on a fresh copy of the A* snapshot of the engine's current
// maps.  Per search its path length, its expansions and the milliseconds it took; *wall_ms: the whole batch.  Nothing is counted
// or committed.  TS_E_UNSUPPORTED where the host searcher does not apply (fractional penalties, field-of-view masking).
int ts_debug_tail_probe(ts_handle e, int32_t n, const int32_t* start, const int32_t* goal, const int32_t* soft, int32_t threads,
                        int32_t* out_len, int32_t* out_exp, double* out_ms, double* wall_ms) {
  if (!e || n < 0 || (n > 0 && (!start || !goal || !soft || !out_len || !out_exp || !out_ms)) || !wall_ms) return TS_E_INVALID;
  for (int k = 0; k < n; k++) if (start[k] < 0 || start[k] >= e->N || goal[k] < 0 || goal[k] >= e->N) return fail(e, TS_E_INVALID, "probe endpoints out of bounds");
  if (!astar_half_units(e->P) || e->P.respect_awareness) return fail(e, TS_E_UNSUPPORTED, "the host searcher carries half-unit costs without a field-of-view mask");
  TRY(search_maps_now(e));
  TRY(tail_snapshot_begin(e));
  TRY(tail_snapshot_wait(e));
  const ahost::Map map = tail_map(e);
  const ahost::Costs costs = ahost::costs_of(e->P);
  const int cap = e->slots.cap;
  const double t0 = now_ms();
  e->tail.pool->run(n, [&](ahost::Searcher& s, int k) {
    thread_local std::vector<int32_t> cells;
    cells.resize((size_t)cap);
    const double t = now_ms();
    const ahost::Result r = s.run(map, costs, ahost::Query{start[k], goal[k], soft[k] != 0, false, 0x7FFFFFFF}, cells.data(), cap);
    out_ms[k] = now_ms() - t; out_len[k] = r.len; out_exp[k] = r.n_exp;
  }, threads);
  *wall_ms = now_ms() - t0;
  return TS_OK;
}

int ts_astar(ts_handle e, int32_t sx, int32_t sy, int32_t gx, int32_t gy, int32_t soft, int32_t ignore_flow,
             int32_t maximum_steps, int32_t* out_xy, int32_t cap_cells) {
  if (!e) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (sx < 0 || sx >= e->W || sy < 0 || sy >= e->H || gx < 0 || gx >= e->W || gy < 0 || gy >= e->H)
    return fail(e, TS_E_INVALID, "astar endpoints out of bounds");
  if (maximum_steps < e->N && maximum_steps > A_STEPS_MAX)
    return fail(e, TS_E_UNSUPPORTED, "a binding maximum_steps above 4094 is not carried (use >= width * height for 'unlimited')");
  TRY(search_maps_now(e));  // "evaluated on the engine's current maps"
  if (e->tail.astar_host) {   // TS_ASTAR_HOST (a test hook): the host searcher on a fresh copy of the snapshot
    TRY(tail_snapshot_begin(e));
    TRY(tail_snapshot_wait(e));
    std::vector<int32_t> cells((size_t)e->slots.cap);
    ahost::Result r{};
    const ahost::Map map = tail_map(e);
    const ahost::Costs costs = ahost::costs_of(e->P);
    const ahost::Query q{sy * e->W + sx, gy * e->W + gx, soft != 0, ignore_flow != 0, maximum_steps};
    e->tail.pool->run(1, [&](ahost::Searcher& s, int) { r = s.run(map, costs, q, cells.data(), (int)cells.size()); });
    if (r.len < 0) return fail(e, TS_E_CAPACITY, "an A* search exceeded its heap or path buffers");
    hipLaunchKernelGGL(k_searcher_account, dim3(1), dim3(1), 0, e->stream, e->d, 1ll, (long long)r.n_exp, (long long)r.n_relax);
    HIPOK(hipStreamSynchronize(e->stream));
    if (r.len > cap_cells) return TS_E_CAPACITY;
    for (int k = 0; k < r.len; k++) { out_xy[2 * k] = cells[(size_t)k] % e->W; out_xy[2 * k + 1] = cells[(size_t)k] / e->W; }
    return r.len;
  }
  hipLaunchKernelGGL(k_astar_single, dim3(1), dim3(64), 0, e->stream, e->d, e->P, e->slots, sy * e->W + sx, gy * e->W + gx, soft,
                     ignore_flow, maximum_steps, e->d_status);
  TRY(read_back(e, &e->hm->scratch, e->d_status, sizeof(int)));
  const int len = e->hm->scratch;
  if (len < 0) return fail(e, TS_E_CAPACITY, "an A* search exceeded its heap or path buffers");
  if (len > cap_cells) return TS_E_CAPACITY;
  if (len > 0) {
    std::vector<int32_t> cells(len);
    HIPOK(hipMemcpy(cells.data(), e->slots.cells, (size_t)len * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < len; k++) { out_xy[2 * k] = cells[k] % e->W; out_xy[2 * k + 1] = cells[k] / e->W; }
  }
  return len;
}

}  // extern "C"
