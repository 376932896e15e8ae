// arena_epochs.h - the epoch stamps of the two searchers' table records, kept apart so that the table arena they share
// (replan_host.h) can change hands without a clear.
//   k_replan (astar.h):      8-byte record, word 0 = dist, word 1 = meta = 18-bit stamp << 14 | steps << 2 | direction
//   the quads (astar_quad.h): 4-byte record = 8-bit stamp << 24 | direction << 22 | 22-bit dist
// A quad's word can lie on either word of a k_replan record.  The stamps are disjoint in the top byte of a word and zero is
// no stamp of either: the quads' run over 1 .. Q_EPOCH_MAX (< 0xC0), k_replan's over W_EPOCH_LO + 1 .. W_EPOCH_LO + span with
// W_EPOCH_LO = 0x30000 (the top byte of every meta word they stamp is >= 0xC0).  So a quad's record, live or stale, is never a
// live meta word to k_replan; a meta word and a dist word below 2^24 are never a live record to a quad.  What is left, a dist
// of 2^24 or more, is watched for where it is stored (astar_loop) and answered with a clear at the next hand-over.
// Plain C++ as well as HIP: tests/native/arena_epochs_test.cpp runs these functions on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS_EPOCH_FN __host__ __device__ inline
#else
#define TS_EPOCH_FN inline
#endif

constexpr uint32_t W_STAMP_SHIFT = 14, Q_EPOCH_SHIFT = 24;
constexpr uint32_t W_EPOCH_LO = 0x30000u, W_EPOCH_SPAN_MAX = 0xFFFFu;   // 65 535 searches between two wraps of a k_replan table
constexpr uint32_t Q_EPOCH_MAX = 191u;                                  // 191 searches between two wraps of a quad's table
constexpr uint32_t ARENA_BIGDIST = 1u << 24;                            // a k_replan dist word from here on has a top byte
static_assert(Q_EPOCH_MAX < 0xC0u && (W_EPOCH_LO << W_STAMP_SHIFT) >> Q_EPOCH_SHIFT == 0xC0u, "the two stamp ranges are disjoint in the top byte");
static_assert(((W_EPOCH_LO + W_EPOCH_SPAN_MAX) >> (32 - W_STAMP_SHIFT)) == 0u, "k_replan's stamps fit 18 bits");

// k_replan's next stamp after `epoch` (a slot's first: anything below the range, the zero of a fresh or cleared slot included).
// `span` = searches between wraps; `wrap`: the table must be cleared before the stamp is used.
TS_EPOCH_FN uint32_t wave_epoch_next(uint32_t epoch, uint32_t span, bool& wrap) {
  const uint32_t hi = W_EPOCH_LO + (span < W_EPOCH_SPAN_MAX ? (span ? span : 1u) : W_EPOCH_SPAN_MAX);
  const uint32_t e = epoch < W_EPOCH_LO ? W_EPOCH_LO : epoch;
  wrap = e >= hi;
  return (wrap ? W_EPOCH_LO : e) + 1u;
}
// the quads' next epoch after `epoch` (0: a fresh or cleared slot), over 1 .. emax
TS_EPOCH_FN uint32_t quad_epoch_next(uint32_t epoch, uint32_t emax, bool& wrap) {
  wrap = epoch >= emax;
  return (wrap ? 0u : epoch) + 1u;
}
// the epoch limit a quad uses: Q_EPOCH_MAX unless a debug value (TS_DEBUG_QUAD_EPOCH_MAX) asks for earlier wraps
TS_EPOCH_FN uint32_t quad_epoch_limit(long long asked) { return asked >= 1 && asked < (long long)Q_EPOCH_MAX ? (uint32_t)asked : Q_EPOCH_MAX; }
// is this 32-bit word a live record / meta word for a search with this epoch?
TS_EPOCH_FN bool wave_meta_live(uint32_t word, uint32_t epoch) { return (word >> W_STAMP_SHIFT) == epoch; }
TS_EPOCH_FN bool quad_word_live(uint32_t word, uint32_t epoch) { return (word >> Q_EPOCH_SHIFT) == epoch; }
