// The epoch ranges of the two searchers' table records (trafficsimulation_amd/csrc/arena_epochs.h), checked on the host,
// exhaustively over the top byte of a word: no record of one kernel is ever live for the other, zero is live for neither, the
// stamps stay inside their ranges and wrap where they should.  Built and run by tests/test_arena_epochs_native.py
// (-fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "arena_epochs.h"

static long long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the low bits a word is tried with under every top byte: the corners and a few patterns
static const uint32_t LOW24[] = {0u, 1u, 0x3FFFu, 0x4000u, 0x3FFFFFu, 0x400000u, 0x555555u, 0xAAAAAAu, 0xC00000u, 0xFFFFFFu};

int main() {
  // ---- k_replan's stamps: start, stay in range, wrap after exactly `span` searches, for the spans in use and the corners
  const uint32_t spans[] = {1u, 2u, 300u, 0xFFFFu, 0x3FFFFu, 0xFFFFFFFFu};
  for (uint32_t span : spans) {
    const uint32_t eff = span < W_EPOCH_SPAN_MAX ? span : W_EPOCH_SPAN_MAX;
    bool wrap = true;
    uint32_t e = wave_epoch_next(0u, span, wrap);       // a fresh slot: no clear, the first stamp of the range
    CHECK(!wrap && e == W_EPOCH_LO + 1u);
    uint32_t between = 1;
    for (uint32_t k = 0; k < 2u * eff + 5u; k++) {
      CHECK(e > W_EPOCH_LO && e <= W_EPOCH_LO + eff && (e >> 18) == 0u);
      CHECK(((e << W_STAMP_SHIFT) >> 24) >= 0xC0u);     // the top byte of every meta word it stamps
      const uint32_t n = wave_epoch_next(e, span, wrap);
      if (wrap) { CHECK(between == eff && n == W_EPOCH_LO + 1u); between = 1; }
      else { CHECK(n == e + 1u); between++; }
      e = n;
    }
    // anything below the range counts as fresh, anything at or beyond its end wraps
    for (uint32_t junk : {1u, 255u, 300u, W_EPOCH_LO - 1u}) { CHECK(wave_epoch_next(junk, span, wrap) == W_EPOCH_LO + 1u && !wrap); }
    for (uint32_t junk : {W_EPOCH_LO + eff, 0x3FFFFu, 0xFFFFFFFFu}) { CHECK(wave_epoch_next(junk, span, wrap) == W_EPOCH_LO + 1u && wrap); }
  }
  // ---- the quads' epochs: 1 .. emax, wrap after emax searches; the debug limit never widens the range
  for (uint32_t emax = 1; emax <= Q_EPOCH_MAX; emax++) {
    bool wrap = true;
    uint32_t e = quad_epoch_next(0u, emax, wrap);
    CHECK(!wrap && e == 1u);
    for (uint32_t k = 1; k < emax; k++) { e = quad_epoch_next(e, emax, wrap); CHECK(!wrap && e == k + 1u); }
    CHECK(e == emax);
    e = quad_epoch_next(e, emax, wrap);
    CHECK(wrap && e == 1u);
  }
  for (long long asked = -3; asked <= 300; asked++) {
    const uint32_t lim = quad_epoch_limit(asked);
    CHECK(lim >= 1u && lim <= Q_EPOCH_MAX && (asked < 1 || asked >= (long long)Q_EPOCH_MAX || lim == (uint32_t)asked));
  }
  // ---- liveness across the kernels, over every top byte
  for (uint32_t top = 0; top < 256u; top++)
    for (uint32_t low : LOW24) {
      const uint32_t w = (top << 24) | low;
      const bool quad_record = top >= 1u && top <= Q_EPOCH_MAX;                // a word a quad may have written (any epoch, any dist / direction)
      const bool wave_meta = (w >> W_STAMP_SHIFT) > W_EPOCH_LO && (w >> W_STAMP_SHIFT) <= W_EPOCH_LO + W_EPOCH_SPAN_MAX;   // ... k_replan, as a meta word
      const bool wave_dist = w < ARENA_BIGDIST;                                // ... k_replan, as a dist word it need not report
      CHECK(!(quad_record && wave_meta));
      if (w == 0u) CHECK(!quad_record && !wave_meta);
      // no quad's word and no zero is a live meta word for any k_replan epoch (all 65 535 of them)
      if (quad_record || w == 0u)
        for (uint32_t e = W_EPOCH_LO + 1u; e <= W_EPOCH_LO + W_EPOCH_SPAN_MAX; e++) CHECK(!wave_meta_live(w, e));
      // no k_replan meta word, no dist word below the threshold and no zero is a live record for any quad epoch
      if (wave_meta || wave_dist)
        for (uint32_t q = 1; q <= Q_EPOCH_MAX; q++) CHECK(!quad_word_live(w, q));
      // (what the threshold is for: a dist word from 2^24 on CAN be one)
      if (!wave_dist && quad_record) CHECK(quad_word_live(w, top));
      // and each kernel still knows its own
      if (quad_record) CHECK(quad_word_live(w, top) && (top == Q_EPOCH_MAX || !quad_word_live(w, top + 1u)));
      if (wave_meta) CHECK(wave_meta_live(w, w >> W_STAMP_SHIFT) && !wave_meta_live(w, (w >> W_STAMP_SHIFT) ^ 1u));
    }
  // every stamp of k_replan's range, with any steps / direction bits, has its top byte at 0xC0 or above
  for (uint32_t e = W_EPOCH_LO + 1u; e <= W_EPOCH_LO + W_EPOCH_SPAN_MAX; e++)
    for (uint32_t low : {0u, 0x3FFFu, 0x1555u}) CHECK((((e << W_STAMP_SHIFT) | low) >> 24) >= 0xC0u);
  printf("arena epochs ok: %lld checks\n", g_checks);
  return 0;
}
