// rng_host.h - the MT19937 draw passes of the decide phase on the host: the upload of the global stream's words, pass 1, the take
// table, the serial chain over the speed rolls, the fix-up after a draw that fired, the prefetch for the next tick.
// Part of the single translation unit engine.hip (included from there, in order).
#pragma once

namespace {

constexpr int SEG_VEHICLES = 1 << 20;   // vehicles per decide pass (bounds one pass' look-ahead into the MT19937 word ring)

// mirror the global stream's tempered words [uploaded, upto) into the device ring (copy stream + event)
int words_upload(E* e, uint64_t upto) {
  MTPipe& r = e->rng_global;
  if (e->words_uploaded < r.pos()) e->words_uploaded = r.pos();
  if (upto <= e->words_uploaded) return TS_OK;
  if (upto - r.pos() > MTPipe::MAX_AHEAD_BLOCKS * 600ull)
    return fail(e, TS_E_CAPACITY, "one decide pass would read more of the MT19937 stream than the ring holds");
  const double t0 = now_ms();
  r.need(upto - r.pos());
  host_prof(e, PH_NEED, now_ms() - t0, 0);
  uint64_t a = e->words_uploaded;
  while (a < upto) {
    const uint64_t off = a & (MTPipe::TW_CAP - 1);
    const uint64_t len = std::min<uint64_t>(upto - a, MTPipe::TW_CAP - off);
    HIPOK(hipMemcpyAsync(e->d.words + off, e->h_words + off, len * 4, hipMemcpyHostToDevice, e->copy_stream));
    a += len;
  }
  HIPOK(hipEventRecord(e->words_ev, e->copy_stream));
  e->words_uploaded = upto;
  return TS_OK;
}

// random() < c  <=>  the 53-bit integer (a << 26 | b) < ceil(c * 2^53)   (exact: power-of-two scaling)
inline unsigned long long thr53(double c) {
  if (!(c > 0.0)) return 0;
  if (c >= 1.0) return 1ull << 53;
  return (unsigned long long)std::ceil(std::ldexp(c, 53));
}
// the speed roll: getrandbits(span.bit_length()) = a word >> rshift, until it is below span
struct Roll { uint32_t span; int rshift; };
inline Roll roll_of(const TsParams& P) {
  const uint32_t span = (uint32_t)(P.vehicle_max_speed - P.vehicle_min_speed + 1);
  return Roll{span, __builtin_clz(span)};
}

// Pass 1 (device) of the vehicles [start, start + n): fixed-word prefix sums, roll ranks, roll start offsets
int rng_pass1(E* e, int start, int n) {
  Dev& d = e->d;
  hipStream_t st = e->stream;
  const int nb = nblk(n, BLK * RS_ITEMS);
  HIPOK(hipMemsetAsync(&d.cnt->rng_event, 0xFF, sizeof(unsigned int), st));
  int tok = prof_begin(e, PK_RNG, n);
  hipLaunchKernelGGL(k_rng_blocksum, dim3(nb), dim3(BLK), 0, st, d.F, start, n, e->rng_blocks);
  hipLaunchKernelGGL(k_rng_scanblocks, dim3(1), dim3(1024), 0, st, e->rng_blocks, nb, d.cnt->rng_tot);
  hipLaunchKernelGGL(k_rng_final, dim3(nb), dim3(BLK), 0, st, d, start, n, e->rng_blocks);
  prof_end(e, tok);
  return TS_OK;
}

// Entries of a take table from `base` on: what the last pass' estimate, the table's room and the words on the device allow
size_t take_len(const E* e, uint64_t base) {
  const size_t nt = (size_t)std::min<uint64_t>(e->cap_take, e->take_guess);
  if (e->words_uploaded >= base + nt + 64) return nt;
  return e->words_uploaded > base + 64 ? (size_t)(e->words_uploaded - base - 64) : 0;
}
// ... and the table itself, queued on `st`: k_rng_take and its download to h_take (the caller orders `st` and records what it needs)
int take_queue(E* e, Roll rl, uint64_t base, size_t nt, hipStream_t st) {
  hipLaunchKernelGGL(k_rng_take, dim3(nblk((long long)nt)), dim3(BLK), 0, st, e->d.words, (unsigned long long)base,
                     (int)nt, rl.span, rl.rshift, e->d_take);
  HIPOK(hipMemcpyAsync(e->h_take, e->d_take, nt, hipMemcpyDeviceToHost, st));
  return TS_OK;
}

// The take table for the stretch of the stream a pass that starts at `base` will most likely walk: the one built ahead of
// time covers [take_base, take_base + take_n) (`*toff` = where this pass starts in it); otherwise one is built now, from the
// estimate of the last pass (positions beyond it fall back to the accept bitmask on the host), valid once the stream syncs
int take_table(E* e, Roll rl, uint64_t base, size_t* n_take, size_t* toff) {
  hipStream_t st = e->stream;
  if (e->take_n > 0 && base >= e->take_base && base - e->take_base + 4096 < e->take_n) {
    *toff = (size_t)(base - e->take_base);
    *n_take = e->take_n - *toff;
    HIPOK(hipEventSynchronize(e->take_ev));
    return TS_OK;
  }
  const size_t nt = take_len(e, base);
  if (nt > 0) {
    HIPOK(hipStreamWaitEvent(st, e->words_ev, 0));
    if (e->take_ev_recorded) HIPOK(hipEventSynchronize(e->take_ev));   // the table built ahead still owns d_take / h_take
    TRY(take_queue(e, rl, base, nt, st));
  }
  e->take_base = base; e->take_n = nt;
  *toff = 0; *n_take = nt;
  return TS_OK;
}

// Pass 2 (host): pass 1's totals and roll start offsets read back, then the serial chain over the speed rolls.  Roll k starts
// at base + rollD[k] + (words taken by the rolls before it); the producer thread tabulated how many words a roll takes from any
// position.  Fills h_Tcum[0..*cnt]; *taken = the words the pass takes (fixed words and rolls).
int roll_chain(E* e, Roll rl, uint64_t base, const uint8_t* take_tab, size_t n_take, int n, int* cnt_out, uint64_t* taken) {
  Dev& d = e->d;
  const int guess = std::min(n, e->roll_guess);
  HIPOK(hipMemcpyAsync(e->hm->rng_tot, d.cnt->rng_tot, sizeof(unsigned int) * 2, hipMemcpyDeviceToHost, e->stream));
  if (guess > 0) HIPOK(hipMemcpyAsync(e->h_rollD, d.rollD, (size_t)guess * 4, hipMemcpyDeviceToHost, e->stream));
  const double t_w1 = now_ms();
  HIPOK(hipStreamSynchronize(e->stream));
  host_prof(e, PH_WAIT1, now_ms() - t_w1, n);
  const uint32_t Ctot = e->hm->rng_tot[0];
  const int cnt = (int)e->hm->rng_tot[1];
  if (cnt > guess) TRY(read_back(e, e->h_rollD + guess, d.rollD + guess, (size_t)(cnt - guess) * 4));
  e->roll_guess = cnt + cnt / 8 + 1024;
  const double t_scan0 = now_ms();
  MTPipe& r = e->rng_global;
  const uint32_t span = rl.span;
  const int rshift = rl.rshift;
  uint32_t* Tcum = e->h_Tcum;
  const uint32_t* rollD = e->h_rollD;
  Tcum[0] = 0;
  uint64_t T = 0, ensured = 0;
  int k0 = 0;
  {
    // fast path while the walk stays inside the device-built table: nothing but the dependent chain
    // T -> address -> byte load -> T (32-bit arithmetic, four rolls per trip)
    uint32_t T32 = 0;
    const uint32_t lim = (uint32_t)std::min<size_t>(n_take, 0x7FFFFFFFu);
    int k = 0;
    for (; k + 4 <= cnt; k += 4) {
      const uint32_t r0 = rollD[k], r1 = rollD[k + 1], r2 = rollD[k + 2], r3 = rollD[k + 3];
      if ((uint64_t)r3 + T32 + 256 >= lim) break;
      const uint32_t t0 = take_tab[r0 + T32]; const uint32_t a0 = T32 + t0;
      const uint32_t t1 = take_tab[r1 + a0]; const uint32_t a1 = a0 + t1;
      const uint32_t t2 = take_tab[r2 + a1]; const uint32_t a2 = a1 + t2;
      const uint32_t t3 = take_tab[r3 + a2]; const uint32_t a3 = a2 + t3;
      if (__builtin_expect((t0 == 0) | (t1 == 0) | (t2 == 0) | (t3 == 0), 0)) break;   // a run the table does not record
      Tcum[k + 1] = a0; Tcum[k + 2] = a1; Tcum[k + 3] = a2; Tcum[k + 4] = a3;
      T32 = a3;
    }
    k0 = k; T = T32;
  }
  for (int k = k0; k < cnt; k++) {
    const uint64_t pos = base + rollD[k] + T;
    if (__builtin_expect(pos + 8 >= ensured, 0)) {
      const uint64_t want = (pos - r.pos()) + (1u << 18);
      r.need(want + 1248);
      ensured = pos + (1u << 18) - 64;
    }
    const uint64_t rel = pos - base;
    uint32_t t = rel < n_take ? take_tab[rel] : r.take(pos);
    if (__builtin_expect(t == 0, 0)) {  // run longer than the table records: count it here
      uint64_t q = pos;
      for (;;) {
        r.need((q - r.pos()) + 8);
        if ((r.at(q++) >> rshift) < span) break;
      }
      t = (uint32_t)(q - pos);
    }
    T += t;
    Tcum[k + 1] = (uint32_t)T;
  }
  host_prof(e, PH_SCAN, now_ms() - t_scan0, n);
  *cnt_out = cnt;
  *taken = Ctot + T;
  return TS_OK;
}

// Rare: a malfunction / sideswipe fired at the vehicle `evk` names (index * 2 + is_collision).  Everything before it stands;
// apply the event, move the stream to just behind its draws and re-derive the draw bytes of the suffix, which the next pass
// starts at (*start)
int draw_event(E* e, unsigned int evk, uint64_t base, int hi, int* start) {
  Dev& d = e->d;
  const TsParams& P = e->P;
  hipStream_t st = e->stream;
  HostMirror& hm = *e->hm;
  e->C.rng_fixups++;
  const int ev_at = (int)(evk >> 1), ev_coll = (int)(evk & 1u);
  uint32_t cx = 0, rr = 0;
  uint8_t fbyte = 0;
  HIPOK(hipMemcpyAsync(&hm.ev_vid, d.active + ev_at, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&hm.ev_partner, d.cand + ev_at, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&cx, d.Cx + ev_at, 4, hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&rr, d.rollrank + ev_at, 4, hipMemcpyDeviceToHost, st));
  TRY(read_back(e, &fbyte, d.F + ev_at, 1));
  const uint64_t after = base + cx + e->h_Tcum[rr] + (ev_coll ? ((fbyte & F_DRAW_MALF) ? 4u : 2u) : 2u);
  e->rng_global.advance_to(after);
  LAUNCH(e, PK_EVENT, 1, k_apply_event, dim3(1), dim3(64), d, P, hm.ev_vid, ev_coll, hm.ev_partner, ev_at);
  *start = ev_at + 1;
  if (*start < hi) LAUNCH(e, PK_DECIDE_PRE, hi - *start, k_decide_pre, dim3(nblk(hi - *start)), dim3(BLK), d, P, *start, hi);
  return TS_OK;
}

// Prefetch the part of the stream the next tick will most likely read (at most one pass' worth - the ring holds
// MAX_AHEAD_BLOCKS blocks; populations above SEG vehicles decide in passes) ...
int prefetch_next_tick(E* e, Roll rl, int nA) {
  MTPipe& r = e->rng_global;
  { const double t_wu = now_ms();
    const uint64_t ahead = std::min<uint64_t>((uint64_t)std::min(nA, SEG_VEHICLES) * 4 + (1u << 16), MTPipe::MAX_AHEAD_BLOCKS * 600ull - (1u << 16));
    TRY(words_upload(e, r.pos() + ahead));
    host_prof(e, PH_WORDS, now_ms() - t_wu, nA); }
  // ... and build the next tick's take table behind that upload, on the copy stream: kernel and download
  // overlap the move phase instead of sitting in front of the next host chain
  const uint64_t nb = r.pos();
  const size_t nt = take_len(e, nb);
  e->take_n = 0;
  static const bool ahead = !getenv("TS_NO_TAKE_AHEAD");
  if (nt > 0 && ahead) {
    TRY(take_queue(e, rl, nb, nt, e->copy_stream));
    HIPOK(hipEventRecord(e->take_ev, e->copy_stream));
    e->take_ev_recorded = true;
    e->take_base = nb; e->take_n = nt;
  }
  return TS_OK;
}

}  // namespace
