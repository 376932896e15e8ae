// astar_quad.h - the replanning searches, sixteen to a wavefront (k_replan_quad).
//
// k_replan (replan.h) spreads ONE search over the 64 lanes of a wave: 138 vector + 151 scalar instructions per expansion,
// issued for one expansion's worth of work (profiles/r03_sq_replan_4096.json).  Here a search owns a QUAD of four lanes -
// lane j of the quad is direction j of astar_numba.py's neighbour loop (N, E, S, W) - and the sixteen quads of a wave run
// sixteen independent searches through one branch-light loop in lockstep: every instruction issued serves sixteen
// expansions, nothing is wave-uniform (no scalar unit work beyond loop control), and the cross-lane traffic is quad_perm
// DPP, which is free.  The algorithm is astar_core's, slot for slot and compare for compare:
//   * heap: the reference's binary heap as 8-byte (f, cell) entries, the first TS_QUAD_LCAP slots of every search in LDS
//     (16 x 156 x 8 B = 19.5 KB per wave: seven waves per CU beside k_replan's side waves), deeper slots in the search's
//     HBM spill.  Sift-down, two levels per LDS round trip: lanes 0 / 1 of the quad fetch the hole's two children, the four
//     lanes its four grandchildren, one DPP swap shows each its sibling's key, "my entry moves up" is one compare (strict
//     '<', ties to the parent, then to the left child: astar_numba.py:67-85).  Beyond LDS the first step takes three
//     levels in one HBM round trip - with the children and grandchildren every lane requests the two children of its
//     own grandchild, and the lane whose grandchild the hole moves to decides that level from its registers - so the
//     blocking loads start three levels below the LDS share (heaps beyond 1 022 entries), two per round trip.  Sixteen
//     searches in lockstep wait for every round trip any one of them needs: one a quad takes on 18 % of its turns is on
//     96 % of the wave's.  Sift-up: the four lanes fetch the twelve ancestors a slot can have in one LDS round trip (52-65);
//   * dir_arr (indexed by heap SLOT, never moved by the sifts: the stale-slot quirk) is only ever read at the heap's
//     last slot and written at the slots behind it - a stack.  Two bits per slot, the 32 slots around the heap's end in
//     a register pair, the rest in HBM; slot 0 in a register of its own;
//   * dist / came_from: one 4-byte record per CELL (dist 22 bits | direction 2 | epoch stamp 8: epochs 1 .. 191, kept apart from
//     k_replan's stamps so that the two kernels can share table memory without clearing it between them, arena_epochs.h) in a table that is a
//     1152 x 1152-cell window centred on the search's start (8 x 8-tiled, addressed by the cell's offset in it): the record's address
//     does not depend on the map entry, so both loads of an expansion leave together (k_replan's node-numbered table costs
//     a dependent second round trip), and a searcher costs 5.3 MB instead of 8 bytes per road cell of the whole map.  A
//     search that reaches a cell 576 or more columns / rows away from its start, whose g reaches 2^22, whose heap outgrows
//     the spill or whose path outgrows the buffers is abandoned, and its vehicle goes to k_replan's queue (nothing of it
//     has been committed: step_decide is a pure function of the tick-start state until its last lines);
//   * half-unit integer costs only (astar_half_units: the reference's defaults), no step limit, no contraflow, no
//     field-of-view mask: the searches that need those (bypasses: a few hundred expansions each, rare) take the vehicle to
//     k_replan as well.
// The policy around the searches (decide_vehicle<DM_QUAD>: step_decide with _compute_path_internal's phases) is run by the
// quad like k_replan runs it by the wave - every lane the same code on the same values - but it cannot keep a search on its
// call stack while fifteen other quads advance theirs.  It is re-run from the top after every search instead: finished
// searches are taken from a log (length + counters; their paths already sit in the buffers the policy handed out), the
// first unfinished one suspends the pass (DV_SUSPEND) and becomes the quad's search.
// Measured: 86 instructions per expansion against k_replan's 289, but only ~50 heaps of this workload
// fit the LDS of a CU whatever the kernel, so the quads run at one to two waves per SIMD with half of each heap in HBM: worth
// 25-30 % on a replanning wave (and 7 % more since the sifts' round trips above: DESIGN.md section 5), and slower than
// k_replan on a queue that is bounded by its longest search - run_replans (engine.hip) sends them queues of
// TS_QUAD_MIN = 262 144 entries and more.
#pragma once
#include "replan.h"

namespace {

#ifndef TS_QUAD_LCAP
#define TS_QUAD_LCAP 156
#endif
#ifndef TS_QUAD_WAVES_PER_CU
#define TS_QUAD_WAVES_PER_CU 7
#endif
constexpr int QL = TS_QUAD_LCAP;            // heap slots per search in LDS (and the stride between two searches' heaps)
// (bank spread: the 8-byte slots of the eight quads of a half-wave at the same heap index must fall into different banks)
static_assert(QL % 8 == 4, "TS_QUAD_LCAP must be 4 mod 8 (LDS bank spread between the quads of a wave)");
static_assert(((size_t)16 * QL + 64) * 8 * TS_QUAD_WAVES_PER_CU <= 160 * 1024 - 512, "the LDS heaps of TS_QUAD_WAVES_PER_CU waves must fit a CU");
static_assert(((size_t)16 * QL + 64) * 8 * TS_QUAD_WAVES_PER_CU + 2 * REPLAN_LDS_BYTES <= 160 * 1024,
              "two side waves of k_replan must fit a CU beside the quads' waves");
#ifndef TS_QUAD_WINDOW
#define TS_QUAD_WINDOW 1152
#endif
constexpr int QT_MAX = TS_QUAD_WINDOW;       // table window: at most 1152 x 1152 cells around the search's start (a multiple of 8)
static_assert(QT_MAX % 8 == 0, "the table window is 8 x 8-tiled");
#ifndef TS_QUAD_CELLS
#define TS_QUAD_CELLS 4096
#endif
constexpr int Q_CELLS = TS_QUAD_CELLS;      // path buffer capacity per search (cells)
#ifndef TS_QUAD_SPILL
#define TS_QUAD_SPILL 7936
#endif
constexpr int Q_SPILL = TS_QUAD_SPILL;      // heap slots per search beyond LDS (HBM)
#ifndef TS_QUAD_MAX_EXP
#define TS_QUAD_MAX_EXP (1 << 17)
#endif
constexpr int Q_MAX_EXP = TS_QUAD_MAX_EXP;  // expansions after which a quad hands its search (and vehicle) to k_replan
constexpr uint32_t Q_DIST_MASK = (1u << 22) - 1, Q_STAMP_SHIFT = Q_EPOCH_SHIFT, Q_DIR_SHIFT = 22;
enum { QS_NEEDJOB = 0, QS_POLICY = 1, QS_SEARCH = 2, QS_FOUND = 3, QS_EMPTY = 4, QS_ABANDON = 5, QS_IDLE = 6, QS_WRAP = 7, QS_START = 8 };
// the quads' own diagnostics (QSlots::stats, added up per engine by run_quad_pass, read by ts_debug_quad_stats): hand-backs
// to k_replan by reason, searches started, table-epoch wraps, and the sift-down's steps beyond LDS: those that consulted the
// third level fetched ahead (QST_STEP3) and the blocking steps below it (QST_DEEP).  Not simulation state: never exchanged,
// never checkpointed.
enum { QST_WINDOW = 1, QST_HEAP = 2, QST_BUDGET = 3, QST_PATHBUF = 4, QST_BAIL = 5, QST_OVERFLOW = 6, QST_SEARCHES = 7, QST_WRAPS = 8,
       QST_STEP3 = 9, QST_DEEP = 10,
       // the walks back along found paths: cells written, HBM round trips they took (two cells per trip), walks, walks of odd length
       // (they end on the first cell of a pair), walks of one cell and of two
       QST_WALK_CELLS = 11, QST_WALK_TRIPS = 12, QST_WALKS = 13, QST_WALK_ODD = 14, QST_WALK_LEN1 = 15, QST_WALK_LEN2 = 16,
       // (TS_QUAD_PROF builds: wave cycles the quads spent outside the lockstep loop, by segment - policy passes, search set-up,
       // path walk, the shift copy behind it; each quad stamps its own, the rest is what the wave's total leaves)
       QST_PROF = 20, QST_N = 24 };

struct QSlots {
  int n_slots;            // searches = quads: sixteen per wave
  int tw, th;             // table window in cells, multiples of 8 (the whole map when it is smaller)
  int chk_x, chk_y;       // the map is wider / taller than the window: it is centred on the search's start and relaxations are bounded to it
  size_t tab_entries;     // per slot
  uint32_t* tab;
  unsigned long long* gq; // per slot Q_SPILL entries
  uint32_t* gdw;          // per slot (QL + Q_SPILL) / 16 + 4 words of 2-bit directions
  int32_t* cells;         // per slot slot_cell_ints(Q_CELLS)
  int32_t* log;           // per slot SLOG_INTS
  uint32_t* slot_epoch;        // per slot, over 1 .. epoch_max (0: fresh or cleared); kept from launch to launch and across hand-overs of the arena
  uint32_t epoch_max;          // Q_EPOCH_MAX (arena_epochs.h; TS_DEBUG_QUAD_EPOCH_MAX: earlier wraps for tests)
  unsigned long long* stats;   // QST_N counters (QST_*)
};
constexpr int Q_DWORDS = (QL + Q_SPILL) / 16 + 4;
constexpr int Q_HEAP_MAX = (QL + Q_SPILL) < (32 * QL - 2) ? (QL + Q_SPILL) : (32 * QL - 2);   // largest heap a quad carries

static_assert(Q_HEAP_MAX < (1 << 13), "a push fetches the twelve ancestors a slot can have at once (quad_turn's sift-up)");
__shared__ unsigned long long q_lds[16 * QL + 64];     // (the last 64 entries: one scratch slot per lane, see q_lput_if)

// what a quad keeps about its search while the lockstep loop runs (every lane of the quad holds the same values)
struct QState {
  int hs;                   // heap_size
  int dir0;                 // dir_arr[0]
  int wb;                   // first slot of the direction window (a multiple of 16)
  unsigned long long dwin;  // dir_arr[wb .. wb + 32), two bits per slot
  int gx, gy, sx, sy;
  int ox, oy;               // origin of the table window
  uint32_t goal_xy;         // x | y << 16
  uint32_t stamp;           // epoch << 24
  int soft;
  int n_exp, n_relax;
  unsigned long long xpre;  // heap entry hs - 1 when it lies beyond LDS (requested at the end of the previous turn)
  int why;                  // why the search was abandoned (QST_WINDOW / g, QST_HEAP, QST_BUDGET, QST_PATHBUF): QSlots::stats
  unsigned n_step3, n_deep; // QST_STEP3 / QST_DEEP of this quad over the kernel's lifetime (counted out once, at its end)
#ifdef TS_QUAD_PROF
  long long pf[10], pt;   // (8: delivery of xpre; 9: the deep sift's first step, before its blocking levels)
#endif
};
#ifdef TS_QUAD_PROF
#define QP(k) do { const long long _t = clock64(); s.pf[k] += _t - s.pt; s.pt = _t; } while (0)
// (outside the lockstep loop: QSEG_BEGIN where a segment starts, QSEG(k) where it ends - QST_PROF + k)
#define QSEG_BEGIN() do { pf_mark = clock64(); } while (0)
#define QSEG(k) do { const long long _t = clock64(); pf_seg[k] += _t - pf_mark; pf_mark = _t; } while (0)
#else
#define QP(k) do { } while (0)
#define QSEG_BEGIN() do { } while (0)
#define QSEG(k) do { } while (0)
#endif
struct QConst {   // per quad, fixed for the kernel's lifetime
  TS_GLOBAL uint32_t* tab;
  gu64p gq;
  TS_GLOBAL uint32_t* gdw;
  int lbase;                // first slot of this quad's heap in q_lds
  int j;                    // lane of the quad = neighbour direction
  int dx, dy;
  // wave-uniform
  const TS_GLOBAL u64* amap;
  int W, H, W8, tw, th, tw8, chk_x, chk_y;
  HalfCosts hc;             // (contra2 and veh2 go unused: no contraflow here, the vehicle penalty rides in the snapshot word)
  bool turn_on, rt_on;
};

// the table record of cell (x, y): the window's origin (ox, oy) is the search's start minus half a window when the map is
// larger than the window, (0, 0) otherwise
__device__ __forceinline__ uint32_t q_tix(const QConst& K, int ox, int oy, int x, int y) { return tix(K.tw8, x - ox, y - oy); }
__device__ __forceinline__ uint32_t q_aix(const QConst& K, int x, int y) { return tix(K.W8, x, y); }
// heap slot k of the quad's search: LDS below QL, the search's HBM spill above.  The turn's hot path uses the LDS forms
// only (no branch around a memory operation, no wait for the expansion's loads in flight); slots that may lie beyond QL
// are touched in blocks of their own, which only run for quads whose heap has outgrown LDS.
__device__ __forceinline__ u64 q_lget(const QConst& K, int k) { return q_lds[K.lbase + k]; }
__device__ __forceinline__ void q_lput(const QConst& K, int k, u64 v) { q_lds[K.lbase + k] = v; }
// A store some lanes make and others do not, without a branch: the others write their own scratch slot behind the heaps.  (A
// predicated store costs the wave an exec-mask bracket and a branch - three scalar instructions and a pipeline bubble; the
// turn has a dozen of them, and at one or two waves per SIMD nothing hides them.)
__device__ __forceinline__ void q_lput_if(const QConst& K, bool on, int k, u64 v) { q_lds[on ? K.lbase + k : 16 * QL + (int)threadIdx.x] = v; }
// heap slot k for the lanes that want it (on) and whose slot lies in LDS; the store of a slot beyond LDS stays behind a branch
// (one, and only quads whose heap has outgrown LDS take it)
__device__ __forceinline__ void q_hput_if(const QConst& K, bool on, int k, u64 v) {
  q_lput_if(K, on & (k < QL), k, v);
  if (on & (k >= QL)) K.gq[k - QL] = v;
}
// A load from the HBM spill in one of the turn's rare side paths, waited for on the spot and kept out of the compiler's
// bookkeeping of outstanding memory operations: a load it can see behind a branch costs an unconditional
// `s_waitcnt vmcnt(0)` where the branch rejoins - for every quad of the wave, on every turn, and with the turn's stores
// (table records, heap entries) in flight that is a wait of microseconds.
__device__ __forceinline__ u64 q_gload_now(const TS_GLOBAL u64* p) {
  u64 v;
  asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// (two of them on their way together, one wait)
__device__ __forceinline__ void q_gload2_now(const TS_GLOBAL u64* pa, const TS_GLOBAL u64* pb, u64& a, u64& b) {
  asm volatile("global_load_dwordx2 %0, %2, off\n\tglobal_load_dwordx2 %1, %3, off\n\ts_waitcnt vmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(pa), "v"(pb) : "memory");
}
__device__ __forceinline__ void q_hput(const QConst& K, int k, u64 v) {
  if (k < QL) q_lds[K.lbase + k] = v; else K.gq[k - QL] = v;
}

// Two levels of heap_sift_down (astar_numba.py:67-85) below the hole at slot p: lanes 0 / 1 of the quad fetch the hole's
// children (2 / 3 mirror them), the four lanes its four grandchildren (quad_sift2_load); every lane decides with its
// sibling's key (one DPP swap) whether its entry would move up if its parent were the hole - smallest of (x, left, right),
// ties to x, then to the left - and one OR over the quad tells every lane the path (quad_sift2_apply).  apply returns
// true when x has found its place (p).  `wr0` / `wr1`: the slots it wrote (-1: none), for whoever holds copies of them.
struct QPair { u64 ce, ge; bool cv, gv; };
template <bool DEEP>
__device__ __forceinline__ QPair quad_sift2_load(const QConst& K, int p, int size) {
  const int j = K.j, side = j & 1;
  const int c = 2 * p + 1 + side, gc = 4 * p + 3 + j;
  QPair r;
  r.cv = c < size; r.gv = gc < size;
  r.ce = 0; r.ge = 0;
  if (DEEP) {    // (the blocking levels: both entries requested together and waited for once; LDS and HBM both read, clamped)
    const u64 cl = q_lget(K, min(c, QL - 1)), gl = q_lget(K, min(gc, QL - 1));
    u64 cg, gg;
    q_gload2_now(K.gq + ((r.cv & (c >= QL)) ? c - QL : 0), K.gq + ((r.gv & (gc >= QL)) ? gc - QL : 0), cg, gg);
    r.ce = c < QL ? cl : cg;
    r.ge = gc < QL ? gl : gg;
  } else {       // (no branch around the reads: a slot that does not exist is read at the root and not used)
    r.ce = q_lget(K, r.cv ? c : 0);
    r.ge = q_lget(K, r.gv ? gc : 0);
  }
  return r;
}
// The same fetch with nothing conditional about it: an LDS read and an HBM load per entry, both always issued (clamped to
// a valid address when the slot lies on the other side or does not exist), the right one picked afterwards.  A load the
// compiler can count is a load it can wait for precisely: behind a branch it would make every later wait for an older
// load (the expansion's map entries and table records) a wait for all of them.
// With them travels a third level: each lane requests the two children of its grandchild (h0 / h1: slots 2 gc + 1, 2 gc + 2),
// so the lane whose grandchild the hole moves to decides the next level from its own registers (quad_sift1_apply) and the
// blocking loads only start three levels below the LDS share.  This step runs where 4 p + 6 >= QL, so those slots
// (8 p + 7 and up) always lie in the spill.  A slot that does not exist is requested at the spill's first entry (a line the
// quad keeps hitting) and not used.
struct QBoth { u64 cl, cg, gl, gg, h0, h1; int c, gc; bool cv, gv; };
__device__ __forceinline__ QBoth quad_sift2_load_both(const QConst& K, int p, int size) {
  const int j = K.j, side = j & 1;
  QBoth r;
  r.c = 2 * p + 1 + side; r.gc = 4 * p + 3 + j;
  const int hc = 2 * r.gc + 1;
  r.cv = r.c < size; r.gv = r.gc < size;
  r.cl = q_lget(K, min(r.c, QL - 1)); r.gl = q_lget(K, min(r.gc, QL - 1));
  r.cg = K.gq[r.cv ? max(r.c - QL, 0) : 0]; r.gg = K.gq[r.gv ? max(r.gc - QL, 0) : 0];
  r.h0 = K.gq[hc < size ? max(hc - QL, 0) : 0]; r.h1 = K.gq[hc + 1 < size ? max(hc + 1 - QL, 0) : 0];
  return r;
}
template <bool DEEP>
__device__ __forceinline__ bool quad_sift2_apply(const QConst& K, int& p, int xf, const QPair& r, int& wr0, int& wr1) {
  const int j = K.j, side = j & 1;
  const int cf = r.cv ? hq_f(r.ce) : 0x7FFFFFFF, gf = r.gv ? hq_f(r.ge) : 0x7FFFFFFF;
  const int csf = qperm<QP_SWAP1>(cf), gsf = qperm<QP_SWAP1>(gf);
  const unsigned adj = (unsigned)(side ^ 1);
  const bool cw = (unsigned)cf < min((unsigned)xf, (unsigned)csf + adj);
  const bool gw = (unsigned)gf < min((unsigned)xf, (unsigned)gsf + adj);
  const int bits = quad_or((cw ? (1 << j) : 0) | (gw ? (16 << j) : 0));
  const int w1 = bits & 3;
  wr0 = -1; wr1 = -1;
  if (w1 == 0) return true;
  const int sdn = w1 >> 1;                              // the hole moves to the left (0) / right (1) child
  const int pc = 2 * p + 1 + sdn;
  const int w2 = (bits >> (4 + 2 * sdn)) & 3;
  const int t = 2 * sdn + (w2 >> 1);                    // ... and on to grandchild t (if w2)
  if (DEEP) {
    q_hput_if(K, cw & (j < 2), p, r.ce);
    q_hput_if(K, (w2 != 0) & (j == t), pc, r.ge);
  } else {
    q_lput_if(K, cw & (j < 2), p, r.ce);
    q_lput_if(K, (w2 != 0) & (j == t), pc, r.ge);
  }
  wr0 = p;
  if (w2 == 0) { p = pc; return true; }
  wr1 = pc;
  p = 4 * p + 3 + t;
  return false;
}

// One level more below the hole at slot p, a grandchild of the step before: lane t = (p + 1) & 3 of the quad fetched that
// slot and, with it, both of its children (QBoth::h0 / h1).  It decides alone - smallest of (x, left, right), ties to x, then
// to the left - and one OR over the quad tells the others.  Returns true when x has found its place (p); `wr`: the slot written.
__device__ __forceinline__ bool quad_sift1_apply(const QConst& K, int& p, int xf, u64 h0, u64 h1, int size, int& wr) {
  const int c0 = 2 * p + 1;
  const bool mine = K.j == ((p + 1) & 3);
  const int f0 = c0 < size ? hq_f(h0) : 0x7FFFFFFF, f1 = c0 + 1 < size ? hq_f(h1) : 0x7FFFFFFF;
  const bool lw = (unsigned)f0 < min((unsigned)xf, (unsigned)f1 + 1u);
  const bool rw = (unsigned)f1 < min((unsigned)xf, (unsigned)f0);
  const int bits = quad_or(mine ? (lw ? 1 : 0) | (rw ? 2 : 0) : 0);
  wr = -1;
  if (bits == 0) return true;
  const int sdn = bits >> 1;
  q_hput_if(K, mine, p, sdn ? h1 : h0);
  wr = p;
  p = c0 + sdn;
  return false;
}

// One turn of astar_core's main loop (astar_numba.py:136-237) for every quad whose search is on.  Returns the quad's
// new state: QS_SEARCH, QS_FOUND (the goal was popped), QS_EMPTY (heap empty: `return []`) or QS_ABANDON.
// Order of the turn (what the reference does one after the other is only reordered where the results cannot tell):
//   pop -> the expansion's loads leave (map entries, table records; the parents of the next two heap slots when they lie
//   beyond LDS) -> sift-down through the levels in LDS -> the loads of its first three levels beyond LDS leave -> the popped
//   cell's neighbours are evaluated (registers only) while those travel -> the sift-down finishes -> table records, pushes.
__device__ __forceinline__ int quad_turn(const QConst& K, QState& s) {
  if (s.hs <= 0) return QS_EMPTY;
  const int j = K.j;
  QP(7);
  // ---- the direction window follows the heap's end: slots hs - 1 (read by this pop) .. hs + 2 (written by its pushes)
  if (s.hs + 2 > s.wb + 31) {
    K.gdw[s.wb >> 4] = (uint32_t)s.dwin;
    s.dwin = (s.dwin >> 32) | ((u64)K.gdw[(s.wb >> 4) + 2] << 32);
    s.wb += 16;
  } else if (s.hs - 1 < s.wb) {
    K.gdw[(s.wb >> 4) + 1] = (uint32_t)(s.dwin >> 32);
    s.dwin = (s.dwin << 32) | (u64)K.gdw[(s.wb >> 4) - 1];
    s.wb -= 16;
  }
  // ---- pop (138-148).  The last entry (it takes the root's place) was requested at the end of the previous turn when it
  // lies beyond LDS
  const u64 root = q_lget(K, 0);
  const int last_i = s.hs - 1;
  const int f_top = hq_f(root);
  const uint32_t cxy = (uint32_t)hq_i(root);
  int cx, cy; xy_unpack(cxy, cx, cy);
  const int prev_dir = s.dir0;
  const int xd = (int)((s.dwin >> (2 * ((last_i - s.wb) & 31))) & 3ull);
  s.hs = last_i;
  // everything the expansion reads from HBM leaves now and travels while the sift-down works: lane j the map entry and
  // the table record of neighbour j, every lane (one request) the popped cell's own
  const int nx = cx + K.dx, ny = cy + K.dy;
  const bool inb = (unsigned)nx < (unsigned)K.W && (unsigned)ny < (unsigned)K.H;
  const uint32_t a_ixc = q_aix(K, cx, cy), t_ixc = q_tix(K, s.ox, s.oy, cx, cy);
  const uint32_t a_ix = inb ? q_aix(K, nx, ny) : a_ixc;
  const bool inw = inb & ((unsigned)(nx - s.ox) < (unsigned)K.tw) & ((unsigned)(ny - s.oy) < (unsigned)K.th);
  const uint32_t t_ix = inw ? q_tix(K, s.ox, s.oy, nx, ny) : t_ixc;
  const u64 am_l = ld8(K.amap, a_ix);
  const uint32_t t_l = K.tab[t_ix];
  const uint32_t am_c = *(const TS_GLOBAL uint32_t*)((const TS_GLOBAL char*)K.amap + (uint32_t)(a_ixc << 3));
  const uint32_t t_c = K.tab[t_ixc];
  // the pushes of this turn go to slots last_i, last_i + 1, ...: lane j will want ancestor 1 + j of each, ((i + 1) >> (1 + j)) - 1.
  // Those that lie beyond LDS are requested now, each lane its own two (pa0 / pa1: the slots, -1 = not held or in LDS)
  int pa0 = (int)(((unsigned)(last_i + 1) >> (1 + j)) - 1u), pa1 = (int)(((unsigned)(last_i + 2) >> (1 + j)) - 1u);
  pa0 = pa0 >= QL ? pa0 : -1;
  pa1 = pa1 >= QL ? pa1 : -1;
  // (both loads always leave - of the spill's first entry when there is nothing to fetch: see quad_sift2_load_both)
  const u64 pv0 = K.gq[max(pa0 - QL, 0)], pv1 = K.gq[max(pa1 - QL, 0)];
  QP(0);
#ifdef TS_QUAD_PROF
  asm volatile("" : : "v"(s.xpre));     // (the stamp takes delivery of the entry requested at the end of the previous turn)
  QP(8);
#endif
  int p = 0;
  bool sinking = false;
  u64 x = 0;
  int xf = 0;
  if (last_i > 0) {
    s.dir0 = xd;
    const u64 xl = q_lget(K, min(last_i, QL - 1));
    x = last_i < QL ? xl : s.xpre;
    xf = hq_f(x);
    bool done = false;
    int w0, w1;
    // (a step reads slots up to 4 p + 6: LDS-only code while those that exist all lie below QL)
    while (!done && (last_i <= QL || 4 * p + 6 < QL)) {
      const QPair r = quad_sift2_load<false>(K, p, last_i);
      done = quad_sift2_apply<false>(K, p, xf, r, w0, w1);
    }
    sinking = !done;
  }
  const QBoth db = quad_sift2_load_both(K, sinking ? p : 0, sinking ? last_i : 0);     // (on their way while the neighbours are evaluated)
  QP(1);
  // ---- lane j evaluates neighbour j (171-225) in half units, exactly as astar_loop<HALF> does: registers only
  const bool is_goal = cxy == s.goal_xy;                        // (151: before the staleness test)
  const int g = f_top - (abs(cx - s.gx) + abs(cy - s.gy));
  const int dist_c = ((t_c ^ s.stamp) >> Q_STAMP_SHIFT) == 0u ? (int)(t_c & Q_DIST_MASK) : A_INF;
  const bool stale = g > dist_c;                                // (165)
  const uint32_t a_l = (uint32_t)am_l;
  const bool node_l = (uint32_t)(am_l >> 32) != AM_NO_NODE;
  const int dist_l = ((t_l ^ s.stamp) >> Q_STAMP_SHIFT) == 0u ? (int)(t_l & Q_DIST_MASK) : A_INF;
  const bool n_occ = ((a_l >> AM_OCC_BIT) & 1u) != 0u, n_stop = ((a_l >> AM_RED_BIT) & 1u) != 0u, n_road = ((a_l >> AM_ROAD_BIT) & 1u) != 0u;
  const uint32_t rt = (a_l >> AM_RT_SHIFT) & AM_RT_MASK;
  const bool flow = ((am_c >> j) & 1u) != 0u;
  const bool turn = K.turn_on & (prev_dir != -1) & (j != prev_dir);
  int n2 = 2 * (g + 1);
  n2 += turn ? K.hc.turn2 : 0;
  n2 += n_occ ? (int)(a_l >> AM_PEN_SHIFT) : 0;
  n2 += n_stop ? K.hc.stop2 : 0;
  const int rtp = rt == 1u ? K.hc.rt2_1 : rt == 2u ? K.hc.rt2_2 : rt == 3u ? K.hc.rt2_3 : 0;
  n2 += (K.rt_on & n_road) ? rtp : 0;
  const bool cand = !is_goal & !stale & inb & node_l & flow & ((s.soft != 0) | !(n_occ | n_stop));
  const bool ok = cand & inw & (n2 < 2 * dist_l);
  const int ngi = n2 >> 1;
  // what this searcher cannot carry: a g beyond the record's 22 bits, a neighbour outside the table window (its record
  // cannot be consulted: whether it would be relaxed is unknowable here)
  const bool bad = (ok & (ngi > (int)Q_DIST_MASK)) | (cand & !inw);
  int relax = quad_or((ok ? (1 << j) : 0) | (bad ? 16 : 0));
  const int nf_l = ngi + abs(nx - s.gx) + abs(ny - s.gy);
  const int nxy_l = xy_pack(nx, ny);
  QP(3);
  // ---- the sift-down finishes beyond LDS.  (Every path takes delivery of the two entries here, before the turn's stores
  // leave: a load still pending on some path would be waited for behind them - stores included - where its register is
  // next written.)
  asm volatile("" : : "v"(relax), "v"(nf_l), "v"(nxy_l), "v"(ngi));   // (the evaluation first ...)
  asm volatile("" : : "v"(db.cg), "v"(db.gg), "v"(db.h0), "v"(db.h1), "v"(pv0), "v"(pv1));
  QPair dp;
  dp.cv = db.cv; dp.gv = db.gv;
  dp.ce = db.c < QL ? db.cl : db.cg;
  dp.ge = db.gc < QL ? db.gl : db.gg;
  bool deep = false;                    // the hole sinks on below the entries that were fetched ahead
  if (sinking) {
    int w0, w1;
    deep = !quad_sift2_apply<true>(K, p, xf, dp, w0, w1);
    if ((w0 >= 0) & ((w0 == pa0) | (w0 == pa1))) { if (w0 == pa0) pa0 = -1; if (w0 == pa1) pa1 = -1; }
    if ((w1 >= 0) & ((w1 == pa0) | (w1 == pa1))) { if (w1 == pa0) pa0 = -1; if (w1 == pa1) pa1 = -1; }
    // (the third level that travelled with the two: the lane that holds the hole's new slot holds its children)
    deep = deep & (2 * p + 1 < last_i);
    if (deep) {
      s.n_step3++;
      deep = !quad_sift1_apply(K, p, xf, db.h0, db.h1, last_i, w0);
      if ((w0 >= 0) & ((w0 == pa0) | (w0 == pa1))) { if (w0 == pa0) pa0 = -1; if (w0 == pa1) pa1 = -1; }
      deep = deep & (2 * p + 1 < last_i);
    }
  }
  QP(9);
  while (deep) {    // (the blocking levels: a hole that still has children three levels below the LDS share)
    int w0, w1;
    s.n_deep++;
    const QPair r = quad_sift2_load<true>(K, p, last_i);
    deep = !quad_sift2_apply<true>(K, p, xf, r, w0, w1);
    if ((w0 >= 0) & ((w0 == pa0) | (w0 == pa1))) { if (w0 == pa0) pa0 = -1; if (w0 == pa1) pa1 = -1; }
    if ((w1 >= 0) & ((w1 == pa0) | (w1 == pa1))) { if (w1 == pa0) pa0 = -1; if (w1 == pa1) pa1 = -1; }
    deep = deep & (2 * p + 1 < last_i);
  }
  if (last_i > 0) {
    q_hput_if(K, j == 0, p, x);
    if (p == pa0) pa0 = -1;
    if (p == pa1) pa1 = -1;
  }
  wave_mem_sync();
  QP(2);
  int st = QS_SEARCH;
  do {
    if (is_goal) { st = QS_FOUND; break; }
    if (stale) break;
    s.n_exp++;
    if (s.n_exp > Q_MAX_EXP) { st = QS_ABANDON; s.why = QST_BUDGET; break; }   // a long search: k_replan's single search is the faster one
    if (relax & 16) { st = QS_ABANDON; s.why = QST_WINDOW; break; }
    if (relax == 0) break;
    const int n_new = __builtin_popcount((unsigned)relax);
    // (a heap the spill holds and whose slots' ancestors 5 and up all lie in LDS: (i + 1) / 32 - 1 < QL)
    if (s.hs + n_new > Q_HEAP_MAX) { st = QS_ABANDON; s.why = QST_HEAP; break; }
    s.n_relax += n_new;
    if (ok) K.tab[t_ix] = (uint32_t)ngi | ((uint32_t)j << Q_DIR_SHIFT) | s.stamp;   // dist / came_from (226-227)
    const int nf0 = qperm<QP_B0>(nf_l), nf1 = qperm<QP_B1>(nf_l), nf2 = qperm<QP_B2>(nf_l), nf3 = qperm<QP_B3>(nf_l);
    const int nc0 = qperm<QP_B0>(nxy_l), nc1 = qperm<QP_B1>(nxy_l), nc2 = qperm<QP_B2>(nxy_l), nc3 = qperm<QP_B3>(nxy_l);
    QP(4);
    // ---- heap pushes in the reference's order N, E, S, W (229-237)
    int npush = 0;
    while (relax) {
      const int dd = __builtin_ctz((unsigned)relax);
      relax &= relax - 1;
      const int nf = dd == 0 ? nf0 : dd == 1 ? nf1 : dd == 2 ? nf2 : nf3;
      const int nxy = dd == 0 ? nc0 : dd == 1 ? nc1 : dd == 2 ? nc2 : nc3;
      const int i = s.hs;
      if (i == 0) s.dir0 = dd;
      else {
        const int sh = 2 * ((i - s.wb) & 31);
        s.dwin = (s.dwin & ~(3ull << sh)) | ((u64)(unsigned)dd << sh);
      }
      // heap_sift_up (52-65): ancestor k of slot i is slot ((i + 1) >> k) - 1, and a heap of Q_HEAP_MAX entries has at most
      // twelve levels above a slot: lane j of the quad fetches ancestors 1 + j, 5 + j and 9 + j in ONE LDS round trip (a
      // wave's sixteen pushes rise 0 to 12 levels: fetched four at a time, the wave paid three round trips for the one
      // that rises furthest).  No store of this push lies between the reads: reading them first changes nothing.
      // (ancestors 1-4 of a slot beyond 2 QL can lie beyond LDS: those of the first two pushes of a turn were requested at
      // the pop, unless something has written to them since; the rest are fetched like any slot)
      const int depth = 31 - __builtin_clz((unsigned)(i + 1));
      const int pa = npush == 0 ? pa0 : npush == 1 ? pa1 : -1;
      const u64 pv = npush == 0 ? pv0 : pv1;
      const int k0 = 1 + j, k1 = 5 + j, k2 = 9 + j;
      const bool has0 = k0 <= depth, has1 = k1 <= depth, has2 = k2 <= depth;
      const int a0 = (int)(((unsigned)(i + 1) >> k0) - 1u), a1 = (int)(((unsigned)(i + 1) >> k1) - 1u), a2 = (int)(((unsigned)(i + 1) >> k2) - 1u);
      // (the reads are unconditional - of the root for a lane without an ancestor, or whose ancestor lies beyond LDS: that
      // entry was requested at the pop or is fetched behind one branch)
      u64 anc0 = q_lget(K, (has0 & (a0 < QL)) ? a0 : 0);
      const u64 anc1 = q_lget(K, (has1 & (a1 < QL)) ? a1 : 0), anc2 = q_lget(K, (has2 & (a2 < QL)) ? a2 : 0);
      if (i > 2 * QL) {
        if (has0 & (a0 >= QL)) { if (a0 == pa) anc0 = pv; else anc0 = q_gload_now(K.gq + (a0 - QL)); }
      }
      const bool up0 = has0 & (nf < hq_f(anc0)), up1 = has1 & (nf < hq_f(anc1)), up2 = has2 & (nf < hq_f(anc2));
      const int um = quad_or((up0 ? (1 << j) : 0) | (up1 ? (16 << j) : 0) | (up2 ? (256 << j) : 0));
      const int rise = __builtin_ctz(~(unsigned)um);       // the entry passes a PREFIX of its ancestors (heap order)
      // ancestor k moves to where k - 1 was
      q_hput_if(K, up0, (int)(((unsigned)(i + 1) >> (k0 - 1)) - 1u), anc0);
      q_hput_if(K, up1, (int)(((unsigned)(i + 1) >> (k1 - 1)) - 1u), anc1);
      q_hput_if(K, up2, (int)(((unsigned)(i + 1) >> (k2 - 1)) - 1u), anc2);
      const int fin = (int)(((unsigned)(i + 1) >> (rise & 31)) - 1u);
      q_hput_if(K, j == 0, fin, hq_pack(nf, nxy));
      // (this push wrote ancestors 0 .. rise of slot i: a lane's copy for the next push is stale if its slot is one of them -
      // on the copy's level that can only be ancestor 1 + j, or j where slot i + 1 opens a new level)
      {
        const int w_a = (int)(((unsigned)(i + 1) >> (1 + j)) - 1u), w_b = (int)(((unsigned)(i + 1) >> j) - 1u);
        if (((pa1 == w_a) & (1 + j <= rise)) | ((pa1 == w_b) & (j <= rise))) pa1 = -1;
      }
      s.hs = i + 1;
      npush++;
      wave_mem_sync();
    }
  } while (0);
  QP(5);
  // the entry the next pop moves to the root, if it lies beyond LDS: on its way while this turn ends and the next begins
  s.xpre = K.gq[max(s.hs - 1 - QL, 0)];
  QP(6);
  return st;
}

struct QReq { int start, goal, soft, cap; int32_t* out; };

__device__ __forceinline__ void quad_scratch_bind(const QSlots& qs, int slot, AScratch& S) {
  S.tab = nullptr; S.gq = nullptr; S.gd = nullptr; S.heap_cap = 0; S.epoch = 0;
  int32_t* c = qs.cells + (size_t)slot * slot_cell_ints(Q_CELLS);
  S.A = c; S.P = c + Q_CELLS; S.T = c + 2 * Q_CELLS; S.PO = c + 3 * Q_CELLS; S.PD = c + 4 * Q_CELLS;
  S.BYP = c + 5 * Q_CELLS; S.OV = S.BYP + MAXB; S.DV = S.OV + MAXB;
  S.cap = Q_CELLS;
  S.use_reach = 0;
  S.big_thr = ~0u; S.big_flag = nullptr;      // (the quads' records carry 22-bit dists: nothing to watch)
  S.calls = 0; S.expansions = 0; S.relaxations = 0;
  S.q_log = qs.log + (size_t)slot * SLOG_INTS;
  S.q_status = DV_BAIL; S.q_replay = 0; S.q_done = 0;
  S.q_start = 0; S.q_goal = 0; S.q_soft = 0; S.q_cap = 0; S.q_out = nullptr;
}

// One pass of vehicle i's step_decide by the quad (see the header: re-run from the top after every search).  Kept out of
// line like replan_turn.
__device__ __attribute__((noinline)) int quad_policy(const Dev& d, const TsParams& P, const QSlots& qs, const RQueue& q, int slot, int i,
                                                     int n_done, QReq& req) {
  AScratch S;
  quad_scratch_bind(qs, slot, S);
  S.q_done = n_done;
  const int r = decide_vehicle<DM_QUAD>(d, P, i, &S);
  const bool one = (threadIdx.x & 3) == 0;
  if (r == DV_SUSPEND) {
    req.start = S.q_start; req.goal = S.q_goal; req.soft = S.q_soft; req.cap = S.q_cap; req.out = S.q_out;
  } else if (one) {
    if (r == DV_DONE || r == DV_POOL_FULL) replan_settle(d, q, i, r, S.calls, S.expansions, S.relaxations);
    else { atomicAdd(&qs.stats[r == DV_BAIL ? QST_BAIL : QST_OVERFLOW], 1ull); __hip_atomic_store(&q.handback_list[atomicAdd(&d.cnt->handback_n, 1)], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }     // DV_BAIL, DV_OVERFLOW: k_replan takes the vehicle
  }
  return r;
}

// Replanning vehicles, sixteen per wave: every quad takes the next entry of the queue (RQueue, replan.h) until it is empty;
// vehicles this searcher cannot carry are handed back to k_replan.
__global__ void __launch_bounds__(64) k_replan_quad(Dev d, TsParams P, QSlots qs, RQueueArgs qa) {
  const int lane = (int)threadIdx.x, j = lane & 3;
  const int slot = (int)blockIdx.x * 16 + (lane >> 2);
  const bool one = j == 0;
  const RQueue q = rqueue_open(d, qa);
  const int n_all = q.n[3] + q.n[2] + q.n[1] + q.n[0];
  QConst K;
  K.tab = (TS_GLOBAL uint32_t*)(uintptr_t)(qs.tab + (size_t)slot * qs.tab_entries);
  K.gq = (gu64p)(uintptr_t)(qs.gq + (size_t)slot * Q_SPILL);
  K.gdw = (TS_GLOBAL uint32_t*)(uintptr_t)(qs.gdw + (size_t)slot * Q_DWORDS);
  K.lbase = (lane >> 2) * QL;
  K.j = j;
  K.dx = (j == 1) - (j == 3); K.dy = (j == 0) - (j == 2);
  K.amap = (const TS_GLOBAL u64*)(uintptr_t)uni64((u64)(uintptr_t)d.amap);
  K.W = uni(d.W); K.H = uni(d.H); K.W8 = uni(d.W8);
  K.tw = qs.tw; K.th = qs.th; K.tw8 = qs.tw >> 3;
  K.chk_x = qs.chk_x; K.chk_y = qs.chk_y;
  K.turn_on = P.turn_penalty_enabled != 0; K.rt_on = P.road_type_penalties_enabled != 0;
  K.hc = half_costs(P);
  uint32_t epoch = qs.slot_epoch[slot];
  QState s;
  s.hs = 0; s.dir0 = -1; s.wb = 0; s.dwin = 0; s.xpre = 0; s.why = 0; s.n_step3 = 0; s.n_deep = 0; s.gx = s.gy = s.sx = s.sy = 0; s.ox = s.oy = 0; s.goal_xy = 0; s.stamp = 0; s.soft = 0; s.n_exp = 0; s.n_relax = 0;
  QReq req;
  req.start = req.goal = req.soft = req.cap = 0; req.out = nullptr;
  int st = QS_NEEDJOB, job = -1, n_done = 0;
  unsigned n_started = 0, n_wraps = 0;      // (QST_SEARCHES / QST_WRAPS of this quad: counted out once, at the end)
  unsigned n_walks = 0, n_cells = 0, n_odd = 0, n_trips = 0;     // (QST_WALKS, QST_WALK_CELLS / _ODD / _TRIPS likewise)
#ifdef TS_QUAD_PROF
  long long pf_t0 = clock64(), pf_search = 0, pf_turns = 0, pf_quadturns = 0;
  for (int k = 0; k < 10; k++) s.pf[k] = 0;
  s.pt = clock64();
  long long pf_seg[4] = {0, 0, 0, 0}, pf_mark = 0;
#endif
  for (;;) {
    // ---------------- per quad: everything that is not a search turn ----------------
    while (st != QS_SEARCH && st != QS_IDLE) {
      if (st == QS_FOUND || st == QS_EMPTY) {
        // the search the policy waited for is over: its path (start excluded, goal included: 151-162) goes where the
        // policy asked for it, its length and counters into the log
        int len = 0;
        if (st == QS_FOUND) {
          const TS_GLOBAL uint32_t* tab = K.tab;
          gi32p outg = (gi32p)(uintptr_t)req.out;
          int px, py; xy_unpack(s.goal_xy, px, py);
          unsigned trips = 0;
          QSEG_BEGIN();
          // Two cells per HBM round trip (the fifteen other quads of the wave wait for this chain of dependent loads): with the
          // record of the current cell c, lane j requests the record of c minus direction j - the four cells c can have come
          // from (the load is clamped to c's own record where that cell lies outside the window or the map).  c's record names
          // the direction d0 it was reached by, lane d0's record is that of the cell before it.  Only records on the path are
          // ever interpreted: the three others may be stale or another epoch's and are dropped unread.  (The tables start on
          // 256-byte boundaries, an 8 x 8 tile of records is two 128-byte lines: most of the extra loads ride on the line of c's own.
          // Measured on the first replanning wave of the bench workload, wave cycles in this loop: 266.5e9 one cell per trip, 186.3e9
          // so, 193.8e9 when lanes only ask for records in c's own line - profiles/r15_quad_prof.json.)
          while (px != s.sx || py != s.sy) {
            const int qx = px - K.dx, qy = py - K.dy;
            const bool qin = ((unsigned)qx < (unsigned)K.W) & ((unsigned)qy < (unsigned)K.H) &
                             ((unsigned)(qx - s.ox) < (unsigned)K.tw) & ((unsigned)(qy - s.oy) < (unsigned)K.th);
            const uint32_t ixc = q_tix(K, s.ox, s.oy, px, py);
            const uint32_t rc = tab[ixc], rq = tab[qin ? q_tix(K, s.ox, s.oy, qx, qy) : ixc];
            trips++;
            if (len >= req.cap) { len = -1; break; }
            outg[req.cap - 1 - len] = py * K.W + px;
            len++;
            const int d0 = (int)((rc >> Q_DIR_SHIFT) & 3u);
            px -= (d0 == 1) - (d0 == 3); py -= (d0 == 0) - (d0 == 2);
            if (px == s.sx && py == s.sy) break;      // (the start was reached at the first cell of the pair)
            const int r0 = qperm<QP_B0>((int)rq), r1 = qperm<QP_B1>((int)rq), r2 = qperm<QP_B2>((int)rq), r3 = qperm<QP_B3>((int)rq);
            const int d1 = (int)(((uint32_t)(d0 == 0 ? r0 : d0 == 1 ? r1 : d0 == 2 ? r2 : r3) >> Q_DIR_SHIFT) & 3u);
            if (len >= req.cap) { len = -1; break; }
            outg[req.cap - 1 - len] = py * K.W + px;
            len++;
            px -= (d1 == 1) - (d1 == 3); py -= (d1 == 0) - (d1 == 2);
          }
          wave_mem_sync();
          QSEG(2);
          if (len > 0) {
            n_walks++; n_cells += (unsigned)len; n_odd += (unsigned)(len & 1); n_trips += trips;
            if ((len <= 2) & one) atomicAdd(&qs.stats[len == 1 ? QST_WALK_LEN1 : QST_WALK_LEN2], 1ull);
          }
          // the path slides to the front of its buffer, sixteen cells per step: every lane loads its four before it stores them
          // (a store writes below everything still to be read: shift > 0)
          const int shift = req.cap - len;
          if (len > 0 && shift > 0)
            for (int k0 = 0; k0 < len; k0 += 16) {
              const int ka = k0 + j, kb = ka + 4, kc = ka + 8, kd = ka + 12;
              const int va = ka < len ? outg[shift + ka] : 0, vb = kb < len ? outg[shift + kb] : 0;
              const int vc = kc < len ? outg[shift + kc] : 0, vd = kd < len ? outg[shift + kd] : 0;
              if (ka < len) outg[ka] = va;
              if (kb < len) outg[kb] = vb;
              if (kc < len) outg[kc] = vc;
              if (kd < len) outg[kd] = vd;
            }
          wave_mem_sync();
          QSEG(3);
        }
        if (len < 0) { st = QS_ABANDON; s.why = QST_PATHBUF; }
        else {
          int32_t* lg = qs.log + (size_t)slot * SLOG_INTS + 3 * n_done;
          lg[0] = len; lg[1] = s.n_exp; lg[2] = s.n_relax;
          n_done++;
          st = QS_POLICY;
        }
      }
      if (st == QS_ABANDON) {
        if (one) atomicAdd(&qs.stats[s.why & 7], 1ull);
        if (one) __hip_atomic_store(&q.handback_list[atomicAdd(&d.cnt->handback_n, 1)], job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st = QS_NEEDJOB;
      }
      if (st == QS_NEEDJOB) {
        int t = 0;
        if (one) t = atomicAdd(&d.cnt->quad_cursor, 1);
        t = quad_first(t);
        if (t >= n_all) { st = QS_IDLE; break; }
        int i, pos;
        if (!rqueue_entry(q, t, i, pos)) continue;
        job = i; n_done = 0;
        st = QS_POLICY;
      }
      if (st == QS_POLICY) {
        QSEG_BEGIN();
        const int r = quad_policy(d, P, qs, q, slot, job, n_done, req);
        QSEG(0);
        if (r != DV_SUSPEND) { st = QS_NEEDJOB; continue; }
        // (a table whose epochs are used up is cleared by the whole wave, below: the quad waits there for the others to come out)
        if (epoch >= qs.epoch_max) { st = QS_WRAP; break; }
        st = QS_START;
      }
      if (st == QS_START) {
        // ---- a fresh search (113-128): new epoch for the table, start record, one-entry heap
        QSEG_BEGIN();
        bool wrap;
        epoch = quad_epoch_next(epoch, qs.epoch_max, wrap);
        n_started++;
        int gxx, gyy, sxx, syy;
        cell_xy(d, req.goal, gxx, gyy); cell_xy(d, req.start, sxx, syy);
        s.gx = gxx; s.gy = gyy; s.sx = sxx; s.sy = syy;
        s.ox = K.chk_x ? sxx - (K.tw >> 1) : 0; s.oy = K.chk_y ? syy - (K.th >> 1) : 0;
        s.goal_xy = (uint32_t)xy_pack(gxx, gyy);
        s.stamp = epoch << Q_STAMP_SHIFT;
        s.soft = req.soft;
        s.n_exp = 0; s.n_relax = 0;
        s.dir0 = -1; s.wb = 0; s.dwin = 0;
        if (one) {
          K.tab[q_tix(K, s.ox, s.oy, sxx, syy)] = s.stamp;    // dist 0
          q_lds[K.lbase] = hq_pack(abs(sxx - gxx) + abs(syy - gyy), xy_pack(sxx, syy));
        }
        s.hs = 1;
        wave_mem_sync();
        QSEG(1);
        st = QS_SEARCH;
      }
    }
    // ---------------- tables whose epochs are used up: the whole wave clears them, one after the other ----------------
    // (191 searches per slot between two of these, kept across launches: an ordinary event, not a rare one - 64 lanes with
    // 8-byte stores take tens of microseconds for the 5.3 MB where the quad's own four lanes, a word each, took a millisecond)
    if (unsigned long long wr = ballot(st == QS_WRAP)) {
      const size_t n2 = qs.tab_entries >> 1;      // (a multiple of 64 words: whole 8 x 8 tiles)
      do {
        const int src = __builtin_ctzll(wr);
        wr &= ~(0xFull << src);
        gu64p t8 = (gu64p)(uintptr_t)rl((u64)(uintptr_t)K.tab, src);
        for (size_t t = (size_t)lane; t < n2; t += 64) t8[t] = 0ull;
      } while (wr);
      wave_mem_sync();
      if (st == QS_WRAP) { n_wraps++; st = QS_START; }     // (quad_epoch_next starts over at 1: epoch >= epoch_max)
      continue;
    }
    const unsigned long long act = ballot(st == QS_SEARCH);
    if (act == 0ull) break;
    // ---------------- the searches of the wave advance in lockstep until one of them ends ----------------
#ifdef TS_QUAD_PROF
    const long long pf_a = clock64();
#endif
    do {
#ifdef TS_QUAD_PROF
      pf_turns++; pf_quadturns += __builtin_popcountll(act) >> 2;
#endif
      if (st == QS_SEARCH) st = quad_turn(K, s);
    } while (ballot(st == QS_SEARCH) == act);
#ifdef TS_QUAD_PROF
    pf_search += clock64() - pf_a;
#endif
  }
#ifdef TS_QUAD_PROF
  if (lane == 0) {   // wave cycles in all / in the lockstep loop, turns of the wave, quad-turns
    atomicAdd((unsigned long long*)&d.cnt->prof[0], (unsigned long long)(clock64() - pf_t0));
    atomicAdd((unsigned long long*)&d.cnt->prof[1], (unsigned long long)pf_search);
    atomicAdd((unsigned long long*)&d.cnt->prof[2], (unsigned long long)pf_turns);
    atomicAdd((unsigned long long*)&d.cnt->prof[3], (unsigned long long)pf_quadturns);
    for (int k = 0; k < 8; k++) atomicAdd((unsigned long long*)&d.cnt->qprof[k], (unsigned long long)s.pf[k]);
    for (int k = 8; k < 10; k++) atomicAdd((unsigned long long*)&d.cnt->prof[k - 4], (unsigned long long)s.pf[k]);   // (prof[4..5]: DevCnt keeps its layout)
  }
  if (one) for (int k = 0; k < 4; k++) atomicAdd(&qs.stats[QST_PROF + k], (unsigned long long)pf_seg[k]);
#endif
  if (one) {
    qs.slot_epoch[slot] = epoch;
    if (n_started) atomicAdd(&qs.stats[QST_SEARCHES], (unsigned long long)n_started);
    if (n_wraps) atomicAdd(&qs.stats[QST_WRAPS], (unsigned long long)n_wraps);
    if (n_walks) {
      atomicAdd(&qs.stats[QST_WALKS], (unsigned long long)n_walks); atomicAdd(&qs.stats[QST_WALK_CELLS], (unsigned long long)n_cells);
      atomicAdd(&qs.stats[QST_WALK_TRIPS], (unsigned long long)n_trips);
      if (n_odd) atomicAdd(&qs.stats[QST_WALK_ODD], (unsigned long long)n_odd);
    }
    if (s.n_step3) atomicAdd(&qs.stats[QST_STEP3], (unsigned long long)s.n_step3);
    if (s.n_deep) atomicAdd(&qs.stats[QST_DEEP], (unsigned long long)s.n_deep);
  }
  // every hand-back of this wave is published before the wave counts itself out (k_replan's replan_turn waits on both)
  __threadfence();
  if (lane == 0) atomicAdd(&d.cnt->quad_waves_done, 1);
}

}  // namespace
