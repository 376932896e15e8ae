// tick.h - the tick driver: one stretch of the decide order (decide_range), what the phases of a tick share (TickState), the
// decide phase's stretches and arrivals, the move phase (host work in rank order between the device's rounds) and tick().
// Part of the single translation unit engine.hip (included from there, in order).
#pragma once

namespace {

// One stretch [lo, hi) of the decide order, start to finish: draws, step_decide, the searches it asks for.  A tick
// is one stretch unless a vehicle may despawn inside the decide phase (decide_stretches) or vehicles decide one at a time
// (decide_point).  nA = the tick's decide population: the stretch that ends it prefetches the next tick's words.
int decide_range(E* e, const int lo, const int hi, const int nA) {
  Dev& d = e->d;
  const TsParams& P = e->P;
  hipStream_t st = e->stream;
  HIPOK(hipMemsetAsync(&d.cnt->replan, 0, sizeof(ReplanCtl), st));
  const Roll rl = roll_of(P);
  MTPipe& r = e->rng_global;
  // vehicles per pass (bounds the look-ahead into the word ring); TS_DEBUG_SEG shrinks it so that tests can walk
  // the multi-pass path on small worlds
  static const int SEG = getenv("TS_DEBUG_SEG") ? std::max(64, atoi(getenv("TS_DEBUG_SEG"))) : SEG_VEHICLES;
  int start = lo;
  bool main_done = false;
  LAUNCH(e, PK_DECIDE_PRE, hi - lo, k_decide_pre, dim3(nblk(hi - lo)), dim3(BLK), d, P, lo, hi);
  while (start < hi) {
    const int seg_end = std::min(hi, start + SEG), n = seg_end - start;
    TRY(rng_pass1(e, start, n));
    const uint64_t base = r.pos();
    size_t n_take = 0, toff = 0;
    TRY(take_table(e, rl, base, &n_take, &toff));
    int cnt = 0;
    uint64_t taken = 0;
    TRY(roll_chain(e, rl, base, e->h_take + toff, n_take, n, &cnt, &taken));
    const uint64_t final_pos = base + taken;
    e->take_guess = taken + taken / 8 + (1u << 16);
    // the words this pass reads must be on the device (usually prefetched during the previous tick)
    const double t_wu = now_ms();
    TRY(words_upload(e, final_pos + 8));
    host_prof(e, PH_WORDS, now_ms() - t_wu, n);
    HIPOK(hipStreamWaitEvent(st, e->words_ev, 0));
    HIPOK(hipMemcpyAsync(d.Tcum, e->h_Tcum, ((size_t)cnt + 1) * 4, hipMemcpyHostToDevice, st));
    // pass 3 (device): every vehicle reads its words: malfunction / sideswipe tests, rolled speeds
    {
      int tok = prof_begin(e, PK_RNG, n);
      hipLaunchKernelGGL(k_rng_apply, dim3(nblk(n)), dim3(BLK), 0, st, d, start, n, (unsigned long long)base,
                         thr53(P.malfunction_chance), thr53(P.sideswipe_chance), rl.span, rl.rshift, P.vehicle_min_speed);
      prof_end(e, tok);
    }
    if (seg_end == hi) {  // k_decide_main returns at once if a draw fired (the fix-up below re-runs it)
      LAUNCH(e, PK_DECIDE_MAIN, hi - lo, k_decide_main, dim3(nblk(hi - lo)), dim3(BLK), d, P, lo, hi, e->class_list);
      HIPOK(hipMemcpyAsync(&e->hm->replan, &d.cnt->replan, sizeof(ReplanCtl), hipMemcpyDeviceToHost, st));
    }
    HIPOK(hipMemcpyAsync(&e->hm->rng_event, &d.cnt->rng_event, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    const double t_w3 = now_ms();
    HIPOK(hipStreamSynchronize(st));
    host_prof(e, PH_WAIT3, now_ms() - t_w3, n);
    const unsigned int evk = e->hm->rng_event;
    if (evk == 0xFFFFFFFFu) {
      r.advance_to(final_pos);
      start = seg_end;
      main_done = seg_end == hi;
      continue;
    }
    TRY(draw_event(e, evk, base, hi, &start));
  }
  if (!main_done) {  // the last pass ended with an event at the very last vehicle (or there was no pass left)
    HIPOK(hipMemsetAsync(&d.cnt->rng_event, 0xFF, sizeof(unsigned int), st));
    LAUNCH(e, PK_DECIDE_MAIN, hi - lo, k_decide_main, dim3(nblk(hi - lo)), dim3(BLK), d, P, lo, hi, e->class_list);
    TRY(read_back(e, &e->hm->replan, &d.cnt->replan, sizeof(ReplanCtl)));
  }
  if (hi == nA) TRY(prefetch_next_tick(e, rl, nA));
  return dispatch_replans(e);
}

// What the phases of one tick share on the host
struct HostEv { uint32_t rank; int hid; int slot; };            // a host agent's step: rain manager (hid 0) or cloud
struct Point { uint32_t rank; int kind; int ref; int slot; };   // the device's rounds stop in front of it: kind 0 = the clock agent,
                                                                // 1 = finishing service vehicle, 2 = a vehicle's own step_decide
struct HostStep { uint32_t rank; int kind; int ref; };          // kind 0 rain (ref: index into host_events), 1 CityBlock,
                                                                // 2 service start, 3 service despawn
struct TickState {
  bool seq = false, svc_on = false;
  int nA = 0, nS = 0;
  int arr_read = 0;                    // service records of this tick consumed so far
  std::vector<int32_t> recs;           // the records fetch_records read last
  std::vector<HostEv> host_events;
  std::vector<HostStep> static_events;   // kinds 0 and 1, known before the rounds
  size_t se_cur = 0;                   // static events handled so far
  std::vector<Point> points;
  RainDiscs discs{-1, {}, {}, {}};     // discs.n = -1: the manager has not stepped in this tick
  int host_deaths = 0;
  uint32_t rank_clock = 0;
  double elapsed0 = 0;
  int done = 0;                        // agents stepped so far in the move phase
  int dev_deaths = 0, dev_arr = 0, dev_error = 0;   // the device's deaths / arr_n / error as the last rounds left them
};

// fetch service records [arr_read, upto) from the device
int fetch_records(E* e, TickState& ts, int upto) {
  ts.recs.clear();
  if (upto > e->d.arr_cap) return fail(e, TS_E_CAPACITY, "more service records in one tick than the record buffer holds");
  if (upto <= ts.arr_read) return TS_OK;
  ts.recs.resize((size_t)(upto - ts.arr_read) * 3);
  TRY(read_back(e, ts.recs.data(), e->d.arr + 3 * (size_t)ts.arr_read, ts.recs.size() * 4));
  ts.arr_read = upto;
  return TS_OK;
}

// Vehicles that stand on their target (a trip that ends where it starts) despawn inside the decide phase
// (vehicle_base.py:657-661) - and leave the schedule before it is shuffled.  `standing` = their decide indices.
int find_standing(E* e, int nA, std::vector<int32_t>& standing) {
  if (!e->d_standing) HIPOK(dalloc(e, &e->d_standing, (size_t)E::STANDING_CAP + 1));
  HIPOK(hipMemsetAsync(e->d_standing, 0, sizeof(int32_t), e->stream));
  hipLaunchKernelGGL(k_find_standing, dim3(nblk(nA)), dim3(BLK), 0, e->stream, e->d, nA, e->d_standing, (int)E::STANDING_CAP);
  int32_t n_st = 0;
  TRY(read_back(e, &n_st, e->d_standing, sizeof(int32_t)));
  if (n_st > E::STANDING_CAP) return fail(e, TS_E_CAPACITY, "more than 4096 vehicles stand on their own target");
  standing.resize((size_t)n_st);
  if (n_st > 0) HIPOK(hipMemcpy(standing.data(), e->d_standing + 1, (size_t)n_st * 4, hipMemcpyDeviceToHost));
  std::sort(standing.begin(), standing.end());
  if (n_st == 0) e->standing_possible = false;
  return TS_OK;
}

// A stretch [lo, hi) whose last vehicle may despawn inside it: decide_range with Dev::dec_expect = hi, so that the vehicle
// tells whether it arrived.  *arrived <- DevCnt::dec_arrived (hi: it did, and the caller takes it off the maps)
int decide_to_candidate(E* e, int lo, int hi, int nA, int* arrived) {
  e->d.dec_expect = hi;
  HIPOK(hipMemsetAsync(&e->d.cnt->dec_arrived, 0, sizeof(int), e->stream));
  const int rc = decide_range(e, lo, hi, nA);
  e->d.dec_expect = 0;
  TRY(rc);
  return read_back(e, arrived, &e->d.cnt->dec_arrived, sizeof(int));
}

// Stretch by stretch, each ending at a vehicle that may despawn: everybody up to and including it decides (draws,
// searches and all), then it leaves the maps and the vehicle behind it loses its turn (k_decide_despawn) - the
// later stretches see exactly what the reference's sequential loop would show them.
int decide_stretches(E* e, TickState& ts, const std::vector<int32_t>& standing) {
  Dev& d = e->d;
  const int nA = ts.nA;
  int lo = 0, removed = 0;
  size_t ci = 0;
  while (lo < nA) {
    while (ci < standing.size() && standing[ci] < lo) ci++;   // (it was the one that lost its turn)
    const bool at_candidate = ci < standing.size();
    const int hi = at_candidate ? standing[ci] + 1 : nA;
    int arrived = 0;
    if (at_candidate) TRY(decide_to_candidate(e, lo, hi, nA, &arrived));
    else TRY(decide_range(e, lo, hi, nA));
    lo = hi;
    if (at_candidate) {
      if (arrived == hi) {
        hipLaunchKernelGGL(k_decide_despawn, dim3(1), dim3(64), 0, e->stream, d, e->P, hi - 1, hi < nA ? hi : -1);
        e->amap_valid = false;
        removed++;
        lo = hi + 1;
      }
      ci++;
    }
  }
  e->tl_pending += removed;
  if (removed > 0) {   // the schedule is shuffled without them (RandomActivation.step takes the live keys)
    TRY(compact_lists(e, removed));
    ts.nA = e->n_active; ts.nS = e->n_sched;
  }
  return TS_OK;
}

// on_target_reached inside step_decide for vehicles that stay on the grid (vehicle_base.py:657-661): apply the
// flag changes now that no decider can see them half-way, then the host part in decide order
int decide_arrivals(E* e, TickState& ts) {
  TRY(read_back(e, &e->hm->arr_n, &e->d.cnt->arr_n, sizeof(int)));
  const int n_rec = e->hm->arr_n;
  if (n_rec <= 0) return TS_OK;
  TRY(fetch_records(e, ts, n_rec));
  hipLaunchKernelGGL(k_decide_arrive, dim3(nblk(n_rec)), dim3(BLK), 0, e->stream, e->d, 0, n_rec);
  std::vector<std::pair<int, int>> order;   // (decide index, vehicle)
  for (int k = 0; k < n_rec; k++) if (ts.recs[3 * k + 2] == AR_DECIDE) order.push_back({ts.recs[3 * k], ts.recs[3 * k + 1]});
  std::sort(order.begin(), order.end());
  for (auto& o : order) { int k = svc_find(e, o.second); if (k >= 0) svc_start(e, e->svc[k]); }
  return TS_OK;
}

// The host's part of the move phase, in rank order.  Host-side agents (rain manager, rain clouds) step at their ranks: they only
// touch host state and the global stream, so they need no device synchronisation of their own (clouds created during this tick
// do not step).  CityBlocks step on the host at their ranks too.  The device's rounds stop in front of the points: the traffic
// generator's own step (`split`: spawns plan on the maps as they are at that point), service vehicles whose load timer runs out
// in this tick (_finish_service plans a path there too) and, without pathfinding batching, every vehicle's step_decide.
int collect_host_work(E* e, TickState& ts, bool split) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  if (e->rain_manager) {
    const int nh = e->n_host_agents;
    std::vector<int32_t> slots(nh);
    TRY(read_back(e, slots.data(), d.hslot, (size_t)nh * 4));
    std::vector<uint32_t> ranks(nh);
    for (int hdx = 0; hdx < nh; hdx++) {
      if (hdx > 0 && !e->rains_all[(size_t)hdx - 1].alive) continue;
      HIPOK(hipMemcpyAsync(&ranks[hdx], d.rank + slots[hdx], 4, hipMemcpyDeviceToHost, st));
    }
    HIPOK(hipStreamSynchronize(st));
    for (int hdx = 0; hdx < nh; hdx++) {
      if (hdx > 0 && !e->rains_all[(size_t)hdx - 1].alive) continue;
      ts.host_events.push_back(HostEv{ranks[hdx], hdx, slots[hdx]});
    }
    std::sort(ts.host_events.begin(), ts.host_events.end(), [](const HostEv& a, const HostEv& b) { return a.rank < b.rank; });
  }
  for (size_t k = 0; k < ts.host_events.size(); k++) ts.static_events.push_back(HostStep{ts.host_events[k].rank, 0, (int)k});
  if (split) ts.points.push_back(Point{ts.rank_clock, 0, 0, e->clock_slot});
  std::vector<int32_t> ids;
  const int nb = std::min((int)e->blocks.size(), e->blocks_scheduled);
  for (int b = 0; b < nb; b++) ids.push_back(b);
  std::vector<int> fin;   // indices into e->svc
  for (size_t k = 0; k < e->svc.size(); k++) {
    auto& v = e->svc[k];
    if (v.phase != 1) continue;
    if (v.ticks <= 1) { fin.push_back((int)k); ids.push_back(v.vid); }   // service_ticks -= 1; <= 0 -> _finish_service
    else v.ticks -= 1;
  }
  if (!ids.empty()) {
    if ((int)ids.size() > e->cap_ids) {
      const int nc = (int)ids.size() * 2 + 64;
      TRY(regrow(e, &e->d_ids, 0, (size_t)nc));
      TRY(regrow(e, &e->d_sr, 0, (size_t)nc * 2));
      e->cap_ids = nc;
    }
    std::vector<int32_t> sr(ids.size() * 2);
    HIPOK(hipMemcpyAsync(e->d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, st));
    if (nb > 0) hipLaunchKernelGGL(k_gather_ranks, dim3(nblk(nb)), dim3(BLK), 0, st, d, e->d_ids, nb, 0, e->d_sr);
    if (!fin.empty())
      hipLaunchKernelGGL(k_gather_ranks, dim3(nblk((long long)fin.size())), dim3(BLK), 0, st, d, e->d_ids + nb, (int)fin.size(), 1,
                         e->d_sr + 2 * nb);
    TRY(read_back(e, sr.data(), e->d_sr, sr.size() * 4));
    for (int b = 0; b < nb; b++) ts.static_events.push_back(HostStep{(uint32_t)sr[2 * b + 1], 1, b});
    for (size_t q = 0; q < fin.size(); q++)
      ts.points.push_back(Point{(uint32_t)sr[2 * (nb + q) + 1], 1, e->svc[fin[q]].vid, sr[2 * (nb + q)]});
  }
  if (ts.seq && ts.nA > 0) {
    // kind 2 = a vehicle about to step: its step_decide runs first (ServiceVehicleAgent.step returns before it while servicing,
    // vehicle_service.py:43-49).  ref = its index in the decide order.
    const int nS = ts.nS;
    std::vector<uint32_t> rk((size_t)nS);
    std::vector<int8_t> kinds((size_t)nS);
    std::vector<int32_t> refs((size_t)nS), aidx((size_t)e->n_vehicles_total);
    std::vector<uint16_t> fl((size_t)e->n_vehicles_total);
    HIPOK(hipMemcpyAsync(rk.data(), d.rank, (size_t)nS * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(kinds.data(), d.sched_kind, (size_t)nS, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(refs.data(), d.sched_ref, (size_t)nS * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(aidx.data(), d.active_idx, (size_t)e->n_vehicles_total * 4, hipMemcpyDeviceToHost, st));
    TRY(read_back(e, fl.data(), d.flags, (size_t)e->n_vehicles_total * 2));
    for (int q = 0; q < nS; q++) {
      if (kinds[q] != K_VEHICLE) continue;
      const int vid = refs[q];
      if (fl[vid] & VF_SERVICING) continue;
      ts.points.push_back(Point{rk[q], 2, aidx[vid], q});
    }
  }
  std::sort(ts.static_events.begin(), ts.static_events.end(), [](const HostStep& a, const HostStep& b) { return a.rank < b.rank; });
  std::sort(ts.points.begin(), ts.points.end(), [](const Point& a, const Point& b) { return a.rank < b.rank; });
  return TS_OK;
}

// host-side work of every agent ranked below `hi`, in rank order: rain, CityBlocks, and what the device reported
// about service vehicles (arrivals -> _start_service, despawns)
int run_window(E* e, TickState& ts, uint32_t hi) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  std::vector<HostStep> evs;
  while (ts.se_cur < ts.static_events.size() && ts.static_events[ts.se_cur].rank < hi) evs.push_back(ts.static_events[ts.se_cur++]);
  if (ts.svc_on) {
    TRY(fetch_records(e, ts, ts.dev_arr));
    for (size_t k = 0; k + 2 < ts.recs.size(); k += 3) {
      if (ts.recs[k + 2] == AR_START) evs.push_back(HostStep{(uint32_t)ts.recs[k], 2, ts.recs[k + 1]});
      else if (ts.recs[k + 2] == AR_DESPAWN) evs.push_back(HostStep{(uint32_t)ts.recs[k], 3, ts.recs[k + 1]});
    }
  }
  std::stable_sort(evs.begin(), evs.end(), [](const HostStep& a, const HostStep& b) { return a.rank < b.rank; });
  if (getenv("TS_DEBUG_EVENTS"))
    for (const HostStep& ev : evs)
      fprintf(stderr, "[events] tick %lld rank %u kind %d ref %d%s\n", (long long)e->C.step_count, ev.rank, ev.kind, ev.ref,
              ev.kind == 0 ? (ts.host_events[ev.ref].hid == 0 ? " (rain manager)" : " (cloud)") : "");
  for (const HostStep& ev : evs) {
    if (ev.kind == 0) {
      const HostEv& h = ts.host_events[ev.ref];
      if (h.hid == 0) {
        TRY(rain_manager_step(e, ts.discs));
        if (ts.seq && ts.discs.n >= 0) {   // the vehicles that decide after the manager in this tick read the new rain_map (vehicle_base.py:104)
          hipLaunchKernelGGL(k_rain_map, dim3(nblk((long long)e->N)), dim3(BLK), 0, st, d.rain, e->W, e->H, e->prev_discs, ts.discs);
          e->prev_discs = ts.discs;
          ts.discs.n = -1;
        }
      }
      else if (rain_agent_step(e, h.hid)) {
        const int8_t dead = K_DEAD;   // schedule.remove(self)
        HIPOK(hipMemcpyAsync(d.sched_kind + h.slot, &dead, 1, hipMemcpyHostToDevice, st));
        HIPOK(hipStreamSynchronize(st));
        ts.host_deaths++;
      }
    } else if (ev.kind == 1) {
      block_step(e, ev.ref);
    } else {
      const int k = svc_find(e, ev.ref);
      if (k < 0) continue;
      if (ev.kind == 2) svc_start(e, e->svc[k]);
      else {
        auto& v = e->svc[k];
        if (v.id >= 0) e->sv_live[(size_t)(v.type == TS_TRIP_SERVICE_FOOD ? 0 : e->gen.T.total_service_vehicles_food) + v.id] = 0;
        if (v.type == TS_TRIP_SERVICE_FOOD) e->C.live_service_food--; else e->C.live_service_waste--;
        e->svc.erase(e->svc.begin() + k);
      }
    }
  }
  return TS_OK;
}

// Rounds of claims and resolves until `target` agents have stepped (nobody ranked at or beyond `rank_limit` moves).  Round 1
// covers every slot; later rounds only the slots that were still blocked (ping-pong lists).
int run_rounds(E* e, TickState& ts, int target, uint32_t rank_limit) {
  Dev& d = e->d;
  const TsParams& P = e->P;
  hipStream_t st = e->stream;
  const int nS = ts.nS;
  int round_no = 0, pending_bound = nS;
  HIPOK(hipMemsetAsync(d.cnt->pend_n, 0, sizeof(int) * 2, st));
  while (ts.done < target) {
    const int chunk = round_no == 0 ? 1 : 4;
    e->amap_valid = false;   // the rounds below move vehicles and switch lights
    for (int rr = 0; rr < chunk; rr++, round_no++) {
      if ((e->epoch % EPOCHS) == 0) {  // epoch prefix wrapped: stale keys would win again -> clear once
        size_t n = (size_t)e->N;
        hipLaunchKernelGGL(k_claims_reset, dim3(nblk((long long)n)), dim3(BLK), 0, st, d.cell, (int)n);
        HIPOK(hipMemsetAsync(d.gclaim_r, 0xFF, (size_t)std::max(d.G, 1) * 4, st));
      }
      const uint32_t prefix = (EPOCHS - 1) - (e->epoch % EPOCHS);
      e->epoch++;
      const int in = round_no & 1, out = in ^ 1;   // round r reads list[r & 1] (none in round 0), writes the other
      const int32_t* in_list = round_no == 0 ? nullptr : e->pend_list[in];
      const int grid_items = round_no == 0 ? nS : pending_bound;
      HIPOK(hipMemsetAsync(&d.cnt->pend_n[out], 0, sizeof(int), st));
      const int flat = round_no == 0 && d.gc_n > 0 && e->groups_scheduled == d.G && P.light_algorithm != TS_LIGHTS_DISABLED;
      LAUNCH(e, PK_MOVE_CLAIM, grid_items, k_move_claim, dim3(nblk(grid_items)), dim3(BLK), d, P, nS, prefix, in_list,
             &d.cnt->pend_n[in], rank_limit, flat);
      if (flat) LAUNCH(e, PK_MOVE_CLAIM, d.gc_n, k_move_claim_groups, dim3(nblk(d.gc_n)), dim3(BLK), d, prefix, rank_limit);
      LAUNCH(e, PK_MOVE_RESOLVE, grid_items, k_move_resolve, dim3(nblk(grid_items)), dim3(BLK), d, P, nS, prefix,
             ts.rank_clock, ts.elapsed0, in_list, &d.cnt->pend_n[in], e->pend_list[out], &d.cnt->pend_n[out], rank_limit);
      e->C.move_rounds++;
    }
    HostMirror& hm = *e->hm;
    TRY(read_back(e, &hm.resolved, &d.cnt->resolved, sizeof(int) * 4));   // resolved .. error
    if (hm.resolved == ts.done && hm.resolved < target) return fail(e, TS_E_DEVICE, "move phase made no progress (internal error)");
    ts.done = hm.resolved;
    ts.dev_deaths = hm.deaths; ts.dev_arr = hm.arr_n; ts.dev_error = hm.error;
    pending_bound = std::max(1, target - ts.done);
  }
  return TS_OK;
}

// step_decide of the vehicle whose turn it is (decide index i, vehicle_base.py:669-670), alone: draws from the stream where it
// stands, searches on the maps as they are, flags / parking / despawn applied before anybody else looks
int decide_point(E* e, TickState& ts, int i) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  d.elapsed = e->C.elapsed;
  e->amap_valid = false;
  int arrived = 0, arr_n = 0;
  TRY(decide_to_candidate(e, i, i + 1, ts.nA, &arrived));
  TRY(read_back(e, &arr_n, &d.cnt->arr_n, sizeof(int)));
  if (arrived == i + 1) hipLaunchKernelGGL(k_decide_despawn, dim3(1), dim3(64), 0, st, d, e->P, i, -1);
  if (ts.svc_on && arr_n > ts.arr_read) {
    const int first = ts.arr_read;
    TRY(fetch_records(e, ts, arr_n));
    hipLaunchKernelGGL(k_decide_arrive, dim3(nblk(arr_n - first)), dim3(BLK), 0, st, d, first, arr_n);
    for (size_t k = 0; k + 2 < ts.recs.size(); k += 3)
      if (ts.recs[k + 2] == AR_DECIDE) { int q = svc_find(e, ts.recs[k + 1]); if (q >= 0) svc_start(e, e->svc[q]); }
  }
  e->amap_valid = false;
  return TS_OK;
}

// schedule.step: the device's rounds up to every point, the host's work in rank order between them
int move_phase(E* e, TickState& ts) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  ts.rank_clock = e->rank_clock_host;
  ts.elapsed0 = e->C.elapsed;
  const int sched_vehicles_at_shuffle = e->n_sched_vehicles;
  if (e->sh_err) return fail(e, TS_E_DEVICE, "the shuffle thread could not send the permutation to the device");
  HIPOK(hipStreamWaitEvent(st, e->perm_ev, 0));   // the permutation went up on its own stream while the decide phase ran
  hipLaunchKernelGGL(k_rank_invert, dim3(nblk(ts.nS)), dim3(BLK), 0, st, e->d_perm, d.rank, ts.nS);
  HIPOK(hipMemsetAsync(d.resolved, 0, (size_t)ts.nS, st));
  HIPOK(hipMemsetAsync(&d.cnt->resolved, 0, sizeof(int) * 2, st));  // resolved, deaths
  // With an armed traffic generator the phase runs in two parts: first every agent ranked before it, then the
  // generator's own step on the host (spawns plan on the maps as they are at that point), then the rest.
  const bool split = e->gen.armed && e->clock_slot >= 0;
  TRY(collect_host_work(e, ts, split));
  ts.dev_arr = ts.arr_read;
  for (size_t pi = 0; pi <= ts.points.size(); pi++) {
    const bool last = pi == ts.points.size();
    const uint32_t rank_limit = last ? NO_RANK : ts.points[pi].rank;
    TRY(run_rounds(e, ts, last ? ts.nS : (int)rank_limit, rank_limit));
    TRY(run_window(e, ts, rank_limit));
    if (last) break;
    const Point& pt = ts.points[pi];
    if (pt.kind == 2) {
      TRY(decide_point(e, ts, pt.ref));
      continue;      // (its movement belongs to the rounds in front of the next point)
    }
    if (pt.kind == 0) TRY(generator_step(e));   // the generator's turn: DynamicTrafficAgent.step on the host
    else { const int k = svc_find(e, pt.ref); if (k >= 0) TRY(svc_finish(e, e->svc[k])); }
    // mark the agent's slot as stepped
    const uint8_t one = 1;
    HIPOK(hipMemcpyAsync(d.resolved + pt.slot, &one, 1, hipMemcpyHostToDevice, st));
    ts.done += 1;
    HIPOK(hipMemcpyAsync(&d.cnt->resolved, &ts.done, sizeof(int), hipMemcpyHostToDevice, st));
    HIPOK(hipStreamSynchronize(st));
  }
  if (ts.dev_error) return fail(e, ts.dev_error, "device-side error: a vehicle despawned inside the decide phase without the host expecting it (internal error)");
  if (ts.discs.n >= 0) {   // RainManager.step ran: rain_map is exactly the union of the discs it saw
    hipLaunchKernelGGL(k_rain_map, dim3(nblk((long long)e->N)), dim3(BLK), 0, st, d.rain, e->W, e->H, e->prev_discs, ts.discs);
    e->prev_discs = ts.discs;
  }
  e->C.agent_steps += sched_vehicles_at_shuffle;
  e->tl_pending += ts.dev_deaths;
  if (ts.dev_deaths + ts.host_deaths > 0) return compact_lists(e, ts.dev_deaths);   // spawns of this tick are part of the lists by now
  return TS_OK;
}

int tick(E* e) {
  Dev& d = e->d;
  const TsParams& P = e->P;
  hipStream_t st = e->stream;
  TickState ts;
  if (getenv("TS_DEBUG_POOL_GC")) TRY(pool_make_room(e, 0));   // (tests: a collection per tick on traces that never replan, too)
  ts.nA = e->n_active; ts.nS = e->n_sched;
  // PATHFINDING_BATCHING=False (vehicle_base.py:669-670): no decide phase - every vehicle runs step_decide at the top of its own
  // step(), in the shuffled order.  Here: the move phase below stops in front of every vehicle (a "point", like the traffic
  // generator's), runs the decide machinery for that one vehicle on the maps and the stream as they are, and goes on.  One
  // vehicle at a time is the reference's own speed limit for this switch; nothing about it is parallel.
  ts.seq = !P.pathfinding_batching;
  d.seq = ts.seq ? 1 : 0;
  d.tl_step = (int)e->C.step_count;
  e->le.observed = false;   // (lights_ext_api.h: the maps move, a cached state vector ends here)
  if (ts.seq && e->dist_world > 1) return fail(e, TS_E_UNSUPPORTED, "PATHFINDING_BATCHING=False has no sharded form (its decisions are sequential)");
  std::vector<int32_t> standing;
  if (e->standing_possible && ts.nA > 0 && !ts.seq) TRY(find_standing(e, ts.nA, standing));
  const bool careful = !standing.empty();
  // the scheduler stream is independent of everything the decide phase does: shuffle on a host thread (unless the decide
  // phase may still change the schedule)
  struct Joiner { E* e; bool done = false; ~Joiner() { if (!done) shuffle_wait(e); } } joiner{e};
  if (!careful) shuffle_start(e, ts.nS); else joiner.done = true;
  const double t_tick0 = now_ms();

  // density_map is a function of the occupancy at this point (city_model.py:1853)
  HIPOK(hipMemcpyAsync(d.occ_snap, d.occ, (size_t)e->N, hipMemcpyDeviceToDevice, st));
  e->density_valid = false;
  e->amap_valid = false;   // the A* snapshot is rebuilt from the cell records when the first search of the tick needs it
  d.elapsed = e->C.elapsed;
  ts.svc_on = !e->svc.empty();
  if (ts.svc_on) HIPOK(hipMemsetAsync(&d.cnt->arr_n, 0, sizeof(int), st));
  // ---------------- decide ----------------
  if (ts.nA > 0) HIPOK(hipMemsetAsync(d.ev, 0, (size_t)e->n_vehicles_total, st));
  if (ts.nA > 0 && !ts.seq) {
    TRY(careful ? decide_stretches(e, ts, standing) : decide_range(e, 0, ts.nA, ts.nA));
    if (ts.svc_on) TRY(decide_arrivals(e, ts));
  }
  if (careful) { shuffle_start(e, ts.nS); joiner.done = false; }
  // ---------------- move (schedule.step) ----------------
  const double t_dec1 = now_ms();
  host_prof(e, PH_DECIDE_WALL, t_dec1 - t_tick0, ts.nA);
  shuffle_wait(e);
  joiner.done = true;
  host_prof(e, PH_SHUFFLE_WAIT, now_ms() - t_dec1, ts.nS);
  host_prof(e, PH_SHUFFLE, e->shuffle_ms, ts.nS);
  const double t_move0 = now_ms();
  if (ts.nS > 0) TRY(move_phase(e, ts));
  host_prof(e, PH_MOVE_WALL, now_ms() - t_move0, ts.nS);
  if (e->clock_slot >= 0 && !e->gen.armed) e->C.elapsed += P.time_per_step_seconds;  // an armed generator did it in its step
  e->C.step_count++;
  // the trip log (triplog.h): this tick's removals become one group of records, in ascending vehicle id
  if (d.tlog && e->tl_pending > 0) TRY(tl_seal(e));
  e->tl_pending = 0;
  // traffic observation (observe.h): the tick's ENTER increments were made by the move kernel; sample the live vehicles where
  // they stand now (the lists are compacted: exactly the rows ts_download_vehicles would return)
  if (e->obs_mask) {
    if ((e->obs_mask & OBS_SAMPLED) && e->n_active > 0)
      hipLaunchKernelGGL(k_obs_sample, dim3(nblk(e->n_active)), dim3(BLK), 0, st, d, e->n_active);
    e->obs_ticks++;
  }
  if (e->prof) { HIPOK(hipStreamSynchronize(st)); prof_collect(e); }
  return TS_OK;
}

}  // namespace
