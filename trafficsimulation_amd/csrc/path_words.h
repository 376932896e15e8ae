// path_words.h - the vehicle paths in the pool (Dev::pool), in one place: the format of a direction string, the window and the
// walk that read it, the encoder's word, and which words of a vehicle's strings are live.  Plain C++17 as well as HIP:
// tests/native/path_words_check.cpp runs these functions on the host.
//
// A path is a string of 2-bit directions (N 0, E 1, S 2, W 3 = +y, +x, -y, -x), sixteen per 32-bit pool word, step k in bits
// 2 (k & 15) .. 2 (k & 15) + 1 of word k >> 4; the bits of the last word beyond the string's length mean nothing.  A string says
// where it goes, not where it starts: the cell in front of its first step is kept beside it.  A vehicle holds five strings:
//   the main path  path_off / path_len / path_cur: steps [path_cur, path_len) are still to drive, from Dev::pos on.  The words
//                  before the one holding path_cur are dead: a collection or a checkpoint drops them (path_live below) and
//                  path_cur, path_len shrink by sixteen per dropped word.
//   four aux paths ax_start / ax_off / ax_len (dev.h: which four): whole strings from the cell ax_start on, ax_len <= 0 = none.
//
// In the kernels that bound a tick (k_decide_main, k_move_claim, k_move_resolve and whatever instantiates decide_vehicle /
// commit_paths) a helper is used where it leaves the instruction stream as it was (profiles/device_code_diff.py): PathWalk in
// k_move_claim, k_move_resolve's slow claim test and AxReader; path_dir, step_cell and path_words everywhere.
// Where it does not, the site keeps its expression, written with the constants and functions below:
//   scan_ahead_dev (decide.h) and k_move_resolve's fast arm (kernels.h) load the window's two words themselves: path_window's
//       test of the first word costs instructions there, and they hold a vehicle with steps left, whose first word exists;
//   vw_path_cell, ax_contains without scratch (decide.h) and vehicle_step_dev's slow arm (kernels.h) step with path_dir and
//       step_cell on their own counter: a PathWalk beside it changes registers and loop shape (vehicle_step_dev also needs
//       the next cell before it decides to enter it);
//   encode_cells (decide.h) gathers a word in a register and stores it whole: path_put's shift, no read-modify-write of the pool;
//   vehicle_step_dev's fast arm (kernels.h) compares the two cells where dir_of_delta compares their difference.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS_WORDS_FN __host__ __device__ __forceinline__
#else
#define TS_WORDS_FN inline
#endif

// ---- the format -------------------------------------------------------------------------------------------------------------------
constexpr int PATH_DIR_BITS = 2, PATH_STEPS_PER_WORD = 16;
constexpr int PATH_STEP_SHIFT = 4, PATH_STEP_MASK = PATH_STEPS_PER_WORD - 1;     // step k: word k >> SHIFT, place k & MASK
constexpr uint32_t PATH_DIR_MASK = (1u << PATH_DIR_BITS) - 1u;
static_assert((1 << PATH_STEP_SHIFT) == PATH_STEPS_PER_WORD && PATH_STEPS_PER_WORD * PATH_DIR_BITS == 32, "sixteen directions fill a pool word");

// pool words of a string of `len` steps (the host sums them beyond 2^31)
TS_WORDS_FN int path_words(int len) { return (len + PATH_STEP_MASK) >> PATH_STEP_SHIFT; }
TS_WORDS_FN size_t path_words(size_t len) { return (len + (size_t)PATH_STEP_MASK) >> PATH_STEP_SHIFT; }
TS_WORDS_FN int path_dir(const uint32_t* pool, uint32_t off, int k) {
  return (pool[off + ((uint32_t)k >> PATH_STEP_SHIFT)] >> ((k & PATH_STEP_MASK) * PATH_DIR_BITS)) & PATH_DIR_MASK;
}
// step k of the string in `words` becomes `dir`.  Steps are put in ascending order: the first step of a word sets the word, so
// the words need not be zero beforehand
TS_WORDS_FN void path_put(uint32_t* words, int k, int dir) {
  uint32_t& w = words[(uint32_t)k >> PATH_STEP_SHIFT];
  w = ((k & PATH_STEP_MASK) ? w : 0u) | ((uint32_t)dir << ((k & PATH_STEP_MASK) * PATH_DIR_BITS));
}

// directions and cells: a cell index is y * W + x, so N is + W and E is + 1
TS_WORDS_FN int dir_dx(int dd) { return (dd == 1) - (dd == 3); }
TS_WORDS_FN int dir_dy(int dd) { return (dd == 0) - (dd == 2); }
TS_WORDS_FN int dir_delta(int dir, int W) { return dir == 0 ? W : dir == 1 ? 1 : dir == 2 ? -W : -1; }
TS_WORDS_FN int step_cell(int cell, int dir, int W) {
  return dir == 0 ? cell + W : dir == 1 ? cell + 1 : dir == 2 ? cell - W : cell - 1;
}
// the direction of a step between two cells known to be 4-adjacent, from the difference of their indices ...
TS_WORDS_FN int dir_of_delta(int delta, int W) { return delta == W ? 0 : delta == 1 ? 1 : delta == -W ? 2 : 3; }
// ... and of a step that has to be checked: -1 unless (dx, dy) is one of the four
TS_WORDS_FN int dir_of_step(int dx, int dy) {
  return dx == 0 && dy == 1 ? 0 : dx == 1 && dy == 0 ? 1 : dx == 0 && dy == -1 ? 2 : dx == -1 && dy == 0 ? 3 : -1;
}

// ---- the window: the next up-to-32 steps from step `cur` of a string of len_total steps, step cur + k in bits 2k .. 2k + 1 --------
// Two words at the most, and never one at or beyond path_words(len_total): steps beyond the string read as whatever its last
// word holds, or 0.
TS_WORDS_FN uint64_t path_window(const uint32_t* pool, uint32_t off, int cur, int len_total) {
  const uint32_t wi = (uint32_t)cur >> PATH_STEP_SHIFT, nwords = (uint32_t)path_words(len_total);
  uint64_t bits = 0;
  if (wi < nwords) bits = pool[off + wi];
  if (wi + 1 < nwords) bits |= (uint64_t)pool[off + wi + 1] << 32;
  return bits >> ((cur & PATH_STEP_MASK) * PATH_DIR_BITS);
}

// ---- the walk: a string read step by step - PathWalk{pool, off, first step, the cell in front of it, W}, next() = the next cell -------
struct PathWalk {
  const uint32_t* pool;
  uint32_t off;
  int idx, cell, W;
  TS_WORDS_FN int next() {
    cell = step_cell(cell, path_dir(pool, off, idx++), W);
    return cell;
  }
};

// ---- the live words of a vehicle ----------------------------------------------------------------------------------------------------
// The main path keeps whole words from the one holding the cursor on: `words` of them from word w0 of the string, against which
// the cursor and the length read `cur` and `len`.  (k_pool_gc, the checkpoint's pack kernel and its validation of a blob,
// k_replan_export over paths just written: cursor 0.)  An aux path keeps all its words if it exists.
struct PathLive { int w0, words, cur, len; };
TS_WORDS_FN PathLive path_live(int cur, int len) {
  PathLive l;
  l.w0 = cur >> PATH_STEP_SHIFT;
  l.words = path_words(len) - l.w0;
  if (l.words < 0) l.words = 0;
  l.cur = cur & PATH_STEP_MASK;
  l.len = len - (l.w0 << PATH_STEP_SHIFT);
  return l;
}
TS_WORDS_FN int aux_words(int len) { return len > 0 ? path_words(len) : 0; }
