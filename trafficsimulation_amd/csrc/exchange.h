// exchange.h - replicated-state multi-GPU mode: a rank's share of the replans as a payload, the exchange through the caller's
// collective, the import of the other ranks' results; and dispatch_replans (a tick's queue goes this way or straight to run_replans).
// Part of the single translation unit engine.hip (included from there, in order).
#pragma once

namespace {

// Replicated-state multi-GPU mode: after this rank's share of the replans, trade results with the other ranks.
// The counters a rank's replans move, traded as deltas since the replanning phase began (XHeader::delta / ddelta, in this order)
constexpr long long DevCnt::*X_LONG[] = {&DevCnt::stuck, &DevCnt::collisions, &DevCnt::malfunctions, &DevCnt::overtaking,
                                         &DevCnt::in_stuck_detour, &DevCnt::parked, &DevCnt::completed_internal,
                                         &DevCnt::completed_through, &DevCnt::dist_internal, &DevCnt::dist_through,
                                         &DevCnt::astar_calls, &DevCnt::astar_exp, &DevCnt::astar_relax};
constexpr double DevCnt::*X_DOUBLE[] = {&DevCnt::dur_internal, &DevCnt::dur_through};
// A rank's payload: this header | n_recs records | n_words path words | n_arr service records (12 bytes each)
struct XHeader {
  int64_t n_recs, n_words, n_arr, error;   // error: the rank's sticky device error (DevCnt::error)
  int64_t delta[std::size(X_LONG)];
  int64_t dec_arrived;                      // DevCnt::dec_arrived after the rank's replans (the ranks keep the largest)
  int64_t rank_error;                       // != 0: the rank failed before the exchange, with this code, and sent the header alone
  int64_t unused_;
  double ddelta[std::size(X_DOUBLE)];
};
static_assert(sizeof(XHeader) == 176, "the header's size is part of every payload (exchange_bytes)");
inline size_t payload_bytes(const XHeader& h) {
  return sizeof(XHeader) + (size_t)h.n_recs * sizeof(ReplanRec) + (size_t)h.n_words * 4 + (size_t)std::max<int64_t>(h.n_arr, 0) * 12;
}

// This rank's share of the replans as exchange records and path words (d_recs, d_xwords), and the header that describes them;
// `after` = the device counters once they were planned
int export_replans(E* e, const DevCnt& before, XHeader& hd, DevCnt& after) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  const int n_owned = e->hm->replan.owned_n;
  TRY(grow(e, &e->d_recs, e->cap_recs, (size_t)std::max(n_owned, 1), (size_t)n_owned * 2 + 1024));
  if (!e->d_xwords_n) HIPOK(dalloc(e, &e->d_xwords_n, 1));
  // the words this rank's replans rewrote, counted first (the pool's growth over the phase is no bound: pool_make_room may
  // have garbage-collected inside it), then exported into a buffer that holds them
  HIPOK(hipMemcpyAsync(e->hcnt, d.cnt, sizeof(DevCnt), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemsetAsync(e->d_xwords_n, 0, sizeof(unsigned long long), st));
  if (n_owned > 0)
    hipLaunchKernelGGL(k_replan_export, dim3(nblk(n_owned)), dim3(BLK), 0, st, d, e->owned_list, n_owned, e->d_recs, e->d_xwords, e->d_xwords_n, 1);
  unsigned long long need_words = 0;
  TRY(read_back(e, &need_words, e->d_xwords_n, sizeof(need_words)));
  after = *e->hcnt;
  TRY(grow(e, &e->d_xwords, e->cap_xwords, (size_t)need_words + 16, (size_t)need_words * 2 + 4096));
  HIPOK(hipMemsetAsync(e->d_xwords_n, 0, sizeof(unsigned long long), st));
  if (n_owned > 0)
    hipLaunchKernelGGL(k_replan_export, dim3(nblk(n_owned)), dim3(BLK), 0, st, d, e->owned_list, n_owned, e->d_recs, e->d_xwords, e->d_xwords_n, 0);
  unsigned long long n_words = 0;
  TRY(read_back(e, &n_words, e->d_xwords_n, sizeof(n_words)));
  if (n_words != need_words) return fail(e, TS_E_DEVICE, "replan export wrote a different number of words than it counted (internal error)");
  hd.n_recs = n_owned; hd.n_words = (int64_t)n_words; hd.n_arr = after.arr_n - before.arr_n; hd.error = after.error;
  for (size_t q = 0; q < std::size(X_LONG); q++) hd.delta[q] = after.*X_LONG[q] - before.*X_LONG[q];
  for (size_t q = 0; q < std::size(X_DOUBLE); q++) hd.ddelta[q] = after.*X_DOUBLE[q] - before.*X_DOUBLE[q];
  hd.dec_arrived = after.dec_arrived;
  return TS_OK;
}

// Pack a payload where the exchange callback reads it: into the device send buffer (device-direct: gathered between device
// buffers) or into send_buf (host-staged).  The service records are d.arr[arr_from, arr_from + n_arr).
int stage_payload(E* e, const XHeader& hd, int arr_from, const void** sendp) {
  const bool dev = e->dist_dev;
  const size_t bytes = payload_bytes(hd), rec_b = (size_t)hd.n_recs * sizeof(ReplanRec), word_b = (size_t)hd.n_words * 4;
  if (dev) TRY(grow(e, &e->d_send, e->cap_send, bytes, bytes * 2 + 4096));
  if (!dev) e->send_buf.resize(bytes);
  uint8_t* p = dev ? e->d_send : e->send_buf.data();
  *sendp = p;
  if (dev) HIPOK(hipMemcpyAsync(p, &hd, sizeof(hd), hipMemcpyHostToDevice, e->stream));
  else memcpy(p, &hd, sizeof(hd));
  p += sizeof(hd);
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (rec_b > 0) HIPOK(hipMemcpyAsync(p, e->d_recs, rec_b, kind, e->stream));
  if (word_b > 0) HIPOK(hipMemcpyAsync(p + rec_b, e->d_xwords, word_b, kind, e->stream));
  if (hd.n_arr > 0) HIPOK(hipMemcpyAsync(p + rec_b + word_b, e->d.arr + 3 * (size_t)arr_from, (size_t)hd.n_arr * 12, kind, e->stream));
  if (dev || bytes > sizeof(hd)) HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

// `before` = the device counters as they were when the replanning phase began.  `local_rc` != 0: this rank failed on the host
// side before the exchange (capacity, a device error).  It still joins the collective, with a header that says so, and every
// rank fails the tick together instead of waiting in the all-gather until the process group times out; so does every failure
// here before the collective.  A failure after the gather (pool_make_room for the others' words, an import) leaves this rank
// part-way through the others' results and out of step with them: it is fatal for the whole group.
int exchange_replans(E* e, const DevCnt& before, int local_rc) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  const double t0 = now_ms();
  XHeader hd;
  memset(&hd, 0, sizeof(hd));
  DevCnt after = before;
  const void* sendp = nullptr;
  if (!local_rc) local_rc = export_replans(e, before, hd, after);
  if (!local_rc) local_rc = stage_payload(e, hd, before.arr_n, &sendp);
  if (local_rc) {
    memset(&hd, 0, sizeof(hd));
    hd.rank_error = local_rc;
    const std::string why = e->err;
    const int staged = stage_payload(e, hd, 0, &sendp);
    e->err = why;
    if (staged != TS_OK) return local_rc;   // (no device memory left even for a header: the other ranks run into their collective's time-out)
  }
  const int64_t bytes = (int64_t)payload_bytes(hd);
  void* recv = nullptr;
  int64_t* sizes = nullptr;
  int64_t stride = 0;
  const int xrc = e->dist_fn(e->dist_user, sendp, bytes, &recv, &sizes, &stride);
  if (local_rc) return local_rc;
  if (xrc != 0 || !recv || !sizes) return fail(e, TS_E_DEVICE, "the replan exchange callback failed");
  // the other ranks' headers (in the gathered device slots, or the gathered host buffer), checked, and their counters merged
  // into this rank's: the device copy moves on only in pool_used (imports), everything else is after + the others' deltas
  auto slot = [&](int r) { return (const uint8_t*)recv + (size_t)r * (size_t)stride; };
  std::vector<XHeader> hs((size_t)e->dist_world);
  for (int r = 0; r < e->dist_world; r++) {
    if (r == e->dist_rank) continue;
    if ((size_t)sizes[r] < sizeof(XHeader)) return fail(e, TS_E_DEVICE, "short replan exchange buffer");
    if (e->dist_dev) HIPOK(hipMemcpyAsync(&hs[r], slot(r), sizeof(XHeader), hipMemcpyDeviceToHost, st));
    else memcpy(&hs[r], slot(r), sizeof(XHeader));
  }
  if (e->dist_dev) HIPOK(hipStreamSynchronize(st));
  DevCnt merged = after;
  long long in_words = 0, in_arr = 0;
  for (int r = 0; r < e->dist_world; r++) {
    if (r == e->dist_rank) continue;
    const XHeader& h = hs[r];
    if (h.rank_error) return fail(e, (int)h.rank_error, "rank " + std::to_string(r) + " failed in its share of the replans (error " + std::to_string((long long)h.rank_error) + ")");
    if ((size_t)sizes[r] != payload_bytes(h)) return fail(e, TS_E_DEVICE, "replan exchange buffer size mismatch");
    in_words += h.n_words; in_arr += h.n_arr;
    for (size_t q = 0; q < std::size(X_LONG); q++) merged.*X_LONG[q] += h.delta[q];
    for (size_t q = 0; q < std::size(X_DOUBLE); q++) merged.*X_DOUBLE[q] += h.ddelta[q];
    if (h.error && !merged.error) merged.error = (int)h.error;
    if ((int)h.dec_arrived > merged.dec_arrived) merged.dec_arrived = (int)h.dec_arrived;
  }
  if (in_words > 0) TRY(pool_make_room(e, (size_t)in_words + 64));
  if (in_arr > 0 && (long long)after.arr_n + in_arr > d.arr_cap) return fail(e, TS_E_CAPACITY, "more service records in one tick than the record buffer holds");
  e->exchange_bytes += bytes;
  int arr_at = after.arr_n;
  for (int r = 0; r < e->dist_world; r++) {
    if (r == e->dist_rank) continue;
    const XHeader& h = hs[r];
    const uint8_t* recs = slot(r) + sizeof(XHeader);
    const uint8_t* words = recs + (size_t)h.n_recs * sizeof(ReplanRec);
    if (h.n_recs > 0 && e->dist_dev) {   // imported straight out of the gathered slot
      hipLaunchKernelGGL(k_replan_import, dim3(nblk((long long)h.n_recs)), dim3(BLK), 0, st, d, (const ReplanRec*)recs, (int)h.n_recs,
                         (const uint32_t*)words);
    } else if (h.n_recs > 0) {           // staged through d_recs / d_xwords
      TRY(grow(e, &e->d_recs, e->cap_recs, (size_t)h.n_recs, (size_t)h.n_recs * 2));
      TRY(grow(e, &e->d_xwords, e->cap_xwords, (size_t)h.n_words + 16, (size_t)h.n_words * 2 + 4096));
      HIPOK(hipMemcpyAsync(e->d_recs, recs, (size_t)h.n_recs * sizeof(ReplanRec), hipMemcpyHostToDevice, st));
      if (h.n_words > 0) HIPOK(hipMemcpyAsync(e->d_xwords, words, (size_t)h.n_words * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_replan_import, dim3(nblk((long long)h.n_recs)), dim3(BLK), 0, st, d, e->d_recs, (int)h.n_recs, e->d_xwords);
      HIPOK(hipStreamSynchronize(st));   // (the staging buffers are reused for the next rank)
    }
    if (h.n_arr > 0) {
      HIPOK(hipMemcpyAsync(d.arr + 3 * (size_t)arr_at, words + (size_t)h.n_words * 4, (size_t)h.n_arr * 12,
                           e->dist_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
      arr_at += (int)h.n_arr;
    }
  }
  unsigned long long pool_now = 0;
  TRY(read_back(e, &pool_now, &d.cnt->pool_used, sizeof(pool_now)));     // (device-direct: the gathered slots are the callee's again after this tick's imports)
  merged.pool_used = pool_now; merged.arr_n = arr_at;
  *e->hcnt = merged;
  HIPOK(hipMemcpyAsync(d.cnt, e->hcnt, sizeof(DevCnt), hipMemcpyHostToDevice, st));
  HIPOK(hipStreamSynchronize(st));
  e->exchange_ms += now_ms() - t0;
  return TS_OK;
}

// The searches the decide phase queued: sharded, this rank's share and the exchange; all of them otherwise
int dispatch_replans(E* e) {
  const int n_all = replan_pending(e->hm->replan);
  if (e->dist_world <= 1) return n_all > 0 ? run_replans(e) : TS_OK;
  // every rank sees the same work lists (as sets): plan this rank's share, then trade results - also when this
  // rank has nothing to plan, the exchange is collective
  TRY(read_back(e, e->hcnt, e->d.cnt, sizeof(DevCnt)));
  const DevCnt before = *e->hcnt;
  int rc_local = grow(e, &e->owned_list, e->cap_owned, (size_t)n_all, (size_t)n_all * 2 + 1024);
  if (!rc_local && n_all > 0) rc_local = run_replans(e);
  return exchange_replans(e, before, rc_local);
}

}  // namespace
