// astar.h - GPU A* (one search per wavefront, heap in LDS): the wave searcher, astar_wave.  The policy that calls it is
// decide.h (decide_vehicle), the work queue that feeds it replan.h (k_replan).
// Also here, because every kernel that runs a searcher wave uses them without the queue (k_astar_single below, k_astar_batch in
// astar_batch.h): wave_pop, a wave's draw from a work cursor through g_job, and searcher_account, a search's counters into the model's.
//
// astar_wave restates astar_numba.py:87-239 verbatim, quirks included:
//   * binary heap keyed on f only, strict '<' in both sift routines (52-85);
//   * dir_arr lives in heap-SLOT order and is NOT swapped by the sifts, so prev_dir = dir_arr[0] is a
//     stale slot value (139, 147, 235);
//   * `ng` is a double (R1 penalty 0.5) that truncates when stored into the int32 arrays (226-232);
//   * soft-obstacle penalty int(1000 * (1 + 4 * density)) in double arithmetic on the float32 density.
// What is laid out for the machine instead of restated:
//   * one wavefront = one search; the heap's first LDS_HEAP slots (f, cell: 8 bytes) and their dir bytes live in
//     LDS, deeper levels spill to the searcher's HBM scratch.  g and steps are not carried in the heap: g = f - h(cell)
//     exactly (h is an integer, ng >= 0), and the steps of a non-stale entry are those of the relaxation that wrote the
//     table entry (every relaxation strictly lowers dist, so the entry with g == dist is the last one pushed);
//   * dist / came_from / steps are one 8-byte record per cell in a table indexed DIRECTLY by the cell's position in an
//     8 x 8-tiled order (no hashing, no probing, never outgrown), stamped with the searcher's epoch instead of the
//     reference's O(W*H) initialisation per call (119-122).  A searcher's table is N x 8 bytes; the 288 GB of HBM
//     hold several hundred of them even at 4096^2;
//   * the maps a search reads are a per-tick snapshot in the same tiled order (Dev::amap; the word, the record and the
//     half-unit costs: astar_words.h), so the neighbours of a cell usually share its line;
//   * everything an expansion needs from HBM (5 map entries, 5 table records, 4 densities) is requested as soon as
//     the popped cell is known and travels while the sift-down works in LDS: one memory round trip per expansion.
//
#pragma once
#include <type_traits>
#include "dev.h"
#include "astar_words.h"

namespace {

constexpr int MAXB = 64;  // longest contraflow bypass (VEHICLE_MAX_CONTRAFLOW_*_STEPS <= 64)

// heap slots (and dir bytes) a searcher keeps in LDS: 6.2 KB, twenty-four searchers per CU (736 entries already cost occupancy) (the deepest heap seen on
// 1024^2 - 4096^2 runs is ~2100 entries; what does not fit spills to the searcher's HBM scratch)
#ifndef TS_LDS_HEAP
#define TS_LDS_HEAP 704
#endif
constexpr int LDS_HEAP = TS_LDS_HEAP;
// register budget of the replanning kernels and (propagated by the compiler) of the functions they call: at least this
// many waves per SIMD.  Four searchers per SIMD keep its vector ALU ~70 % busy (profiles/r02_sq_replan_2048.json); six
// (the search loop needs 72 vector registers then, spills stay outside it) are 11 % faster at 4096^2 / 10^6 vehicles once
// the queue is ordered in space
#ifndef TS_REPLAN_WAVES
#define TS_REPLAN_WAVES 6
#endif
#define TS_REPLAN_OCC __attribute__((amdgpu_waves_per_eu(TS_REPLAN_WAVES, 8)))
struct __attribute__((aligned(8))) HQ { int32_t f, i; };             // heap entry: f_arr, i_arr (g_arr / s_arr: see above)
struct __attribute__((aligned(8))) TEnt { int32_t dist; uint32_t meta; };   // k_replan's table record (astar_words.h)
// The stamps run over W_EPOCH_LO + 1 .. W_EPOCH_LO + T_STAMP_MAX (arena_epochs.h: a range the quads' records, which can lie in the
// same memory, never look live in); T_STAMP_MAX = searches between two wraps.
// (TS_DEBUG_STAMP_MAX: a test build that wraps the searcher tables' epochs every few hundred searches instead of every 65 535)
#ifndef TS_DEBUG_STAMP_MAX
#define TS_DEBUG_STAMP_MAX 0xFFFFu
#endif
constexpr uint32_t T_STAMP_SHIFT = W_STAMP_SHIFT, T_STAMP_MAX = TS_DEBUG_STAMP_MAX;
constexpr int A_STEPS_MAX = (int)T_STEPS_MASK - 1;   // largest binding step limit a search can carry (a limit >= N never binds)

// (slot LDS_HEAP of both arrays is a spare no search reads: a lane-predicated store sends its idle lanes there instead of
// switching them off, which would cost an exec-mask bracket - two scalar instructions and a branch - per store)
__shared__ unsigned long long g_lq[LDS_HEAP + 1];   // packed HQ: f in the low word, cell (y << 16 | x) in the high word
__shared__ int8_t g_ld[LDS_HEAP + 1];
__shared__ int g_job;   // the work-queue entry the wave is on (wave_pop)
// a workgroup's LDS, rounded up to 1 280-byte allocation granules: twenty-four searchers must fit the 160 KB of a CU
// (astar_quad.h checks the mix of a replanning wave: the quads' waves with two side waves of k_replan beside them)
constexpr size_t REPLAN_LDS_BYTES = ((LDS_HEAP + 1) * (sizeof(unsigned long long) + 1) + sizeof(int) + 16 + 1279) / 1280 * 1280;
static_assert(REPLAN_LDS_BYTES * 4 * TS_REPLAN_WAVES <= 160 * 1024, "the LDS heaps of TS_REPLAN_WAVES searchers per SIMD must fit a CU");
// heap entries carry the cell as packed coordinates: 16 bits each (ts_create refuses wider / taller maps)
constexpr int A_XY_MAX = 0xFFFF;
__device__ __forceinline__ int xy_pack(int x, int y) { return (int)(((uint32_t)y << 16) | (uint32_t)x); }
__device__ __forceinline__ void xy_unpack(uint32_t xy, int& x, int& y) { x = (int)(xy & 0xFFFFu); y = (int)(xy >> 16); }

// One searcher's scratch: LDS heap (above) + its slot of the HBM arena.
struct AScratch {
  HQ* gq;        // heap slots [LDS_HEAP, heap_cap), indexed by slot - LDS_HEAP
  int8_t* gd;    // dir_arr for the same slots: indexed by heap SLOT and deliberately not moved by the sift routines
  int heap_cap;
  TEnt* tab;     // one record per search node (Dev::n_nodes), nodes numbered in tiled order, and one spare behind them
  uint32_t epoch;
  uint32_t big_thr;    // a dist from here on could pass for a quad's live record (ASlots::big_thr) ...
  uint32_t* big_flag;  // ... and a search that stored one says so here (ASlots::big_flag)
  int32_t *A, *P, *T, *PO, *PD;  // cap cells each: A* result, current new path, splice target, staged pre-paths
  int32_t *BYP, *OV, *DV;        // MAXB cells each: bypass result, staged overtake / detour paths
  int cap;        // capacity of the cell buffers
  int use_reach;  // phase 1 asks reach_strict_wave before it searches (off: TS_NO_REACH, a debugging switch)
  long long calls, expansions, relaxations;
  // DM_QUAD only (astar_quad.h): the policy code is re-run from the top after every search (it is a pure function of the
  // tick-start state and of its searches' results until the final commit), taking finished searches from this log and
  // suspending at the first one that is not in it
  int q_status, q_replay, q_done;          // DV_SUSPEND / DV_BAIL when a planner returns false; searches replayed / finished
  int32_t* q_log;                          // per finished search: path length, expansions, relaxations
  int q_start, q_goal, q_soft, q_cap;      // the search the policy is waiting for
  int32_t* q_out;
  // DM_WAVE with a tail control block (k_replan's plain passes, replan.h RTail): the same log, kept by astar_any<DM_WAVE> for the
  // searches without a step limit and on the flow, so that a step_decide whose search was handed to the host (DV_HANDOFF) can be
  // re-run from the top with that search's result in the log.  t_ctl == nullptr: no search of this wave is ever handed over.
  struct TailCtl* t_ctl;
  int t_thr, t_floor, t_first;             // hand over when t_ctl->idle >= t_thr and the search has made t_floor expansions; first look at t_first
};
// The tail control block of a k_replan pass (device memory; the host zeroes idle and n before the launch and reads n and the
// entries after the pass' stream has drained): waves that found the queue empty, searches handed to the host, and for each the
// queue entry, the searcher slot, its ordinal among the logged searches of this step_decide, its arguments and where its path goes.
struct TailEnt { int32_t i, slot, ord, start, goal, soft, out_off, out_cap; };   // out_off: ints from ASlots::cells
struct TailCtl { int idle, n, cap, pad_; };     // TailEnt list[cap] follows
constexpr int TAIL_PERIOD = 4096;     // fresh expansions between two looks at TailCtl::idle
constexpr int TAIL_GAVE_UP = -1;      // astar_loop's heap size once the search has given up

// ints in a searcher slot's cell buffers (scratch_bind, quad_scratch_bind): A, P, T, PO, PD of `cap` cells each, then BYP, OV, DV of MAXB
__host__ __device__ constexpr size_t slot_cell_ints(size_t cap) { return 5 * cap + 3 * MAXB; }

struct ASlots {
  int n_slots, heap_cap, cap, use_reach;
  size_t tab_entries;    // per slot: max(n_nodes, 1) + 1 (the last one is the spare that idle lanes' stores go to)
  TEnt* tab;
  HQ* gq;
  int8_t* gd;
  int32_t* cells;        // per slot: slot_cell_ints(cap)
  uint32_t* slot_epoch;
  // the one way a record of these tables could pass for a quad's live one once the arena changes hands without a clear: a dist
  // word of big_thr (2^24; TS_DEBUG_ARENA_BIGDIST) or more.  A search that stores one sets *big_flag, and the next hand-over clears.
  uint32_t big_thr;
  uint32_t* big_flag;
};

__device__ __forceinline__ void scratch_bind(const ASlots& t, int slot, AScratch& S) {
  S.tab = t.tab + (size_t)slot * t.tab_entries;
  S.gq = t.gq + (size_t)slot * (size_t)(t.heap_cap - LDS_HEAP);
  S.gd = t.gd + (size_t)slot * (size_t)(t.heap_cap - LDS_HEAP);
  S.heap_cap = t.heap_cap;
  int32_t* c = t.cells + (size_t)slot * slot_cell_ints((size_t)t.cap);
  S.A = c; S.P = c + t.cap; S.T = c + 2 * (size_t)t.cap; S.PO = c + 3 * (size_t)t.cap; S.PD = c + 4 * (size_t)t.cap;
  S.BYP = c + 5 * (size_t)t.cap; S.OV = S.BYP + MAXB; S.DV = S.OV + MAXB;
  S.cap = t.cap;
  S.use_reach = t.use_reach;
  S.epoch = t.slot_epoch[slot];
  S.big_thr = t.big_thr; S.big_flag = t.big_flag;
  S.calls = 0; S.expansions = 0; S.relaxations = 0;
  S.q_status = 0; S.q_replay = 0; S.q_done = 0; S.q_log = nullptr; S.q_start = 0; S.q_goal = 0; S.q_soft = 0; S.q_cap = 0; S.q_out = nullptr;
  S.t_ctl = nullptr; S.t_thr = 0; S.t_floor = 0; S.t_first = -1;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ void wave_mem_sync() { __builtin_amdgcn_wave_barrier(); }
// values every lane holds alike: tell the compiler (scalar registers, scalar branches) / read one lane's copy
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// __ballot() takes an int: a lane predicate would be turned into 0 / 1 and compared against 0 again (two vector
// instructions and a hazard nop per ballot); this form hands the compare's own lane mask over
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double rl(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// quad_perm DPP: lane j of every quad reads lane P[j] of its quad
template <int CTRL> __device__ __forceinline__ int qperm(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }
constexpr int QP_SWAP1 = 0xB1;   // [1,0,3,2]
constexpr int QP_SWAP2 = 0x4E;   // [2,3,0,1]
constexpr int QP_B0 = 0x00, QP_B1 = 0x55, QP_B2 = 0xAA, QP_B3 = 0xFF;   // broadcasts of lane 0 .. 3
__device__ __forceinline__ int quad_or(int v) {   // OR over the four lanes of the quad, in every lane
  v |= qperm<QP_SWAP1>(v);
  v |= qperm<QP_SWAP2>(v);
  return v;
}
// (quad_perm [0,0,0,0]: every lane of a quad reads its lane 0)
__device__ __forceinline__ int quad_first(int v) { return qperm<QP_B0>(v); }

// Heap entries and table records travel as packed 64-bit words (HQ: f low, cell high; TEnt: dist low, meta high), and
// the searcher's HBM arrays are addressed through global-address-space pointers: pointers that reach a function inside
// a struct are generic to the compiler, and generic ("flat") loads count against the LDS wait counter as well, which
// would make every LDS wait of the sift-down also wait for the expansion's loads in flight.
#define TS_GLOBAL __attribute__((address_space(1)))
typedef unsigned long long u64;
typedef TS_GLOBAL u64* gu64p;
typedef TS_GLOBAL int8_t* gi8p;
typedef TS_GLOBAL int32_t* gi32p;
__device__ __forceinline__ u64 hq_pack(int f, int i) { return (u64)(uint32_t)f | ((u64)(uint32_t)i << 32); }
__device__ __forceinline__ int hq_f(u64 e) { return (int)(uint32_t)e; }
__device__ __forceinline__ int hq_i(u64 e) { return (int)(uint32_t)(e >> 32); }
__device__ __forceinline__ u64 rl(u64 v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 uni64(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}
// Element `idx` of an array of 8-byte records whose byte size stays below 4 GiB (map snapshot, searcher tables: at most
// 2^26 records): the 32-bit byte offset lets the access use its scalar-base + 32-bit-offset form instead of 64-bit
// vector address arithmetic.
__device__ __forceinline__ u64 ld8(const TS_GLOBAL u64* base, uint32_t idx) {
  return *(const TS_GLOBAL u64*)((const TS_GLOBAL char*)base + (uint32_t)(idx << 3));
}
__device__ __forceinline__ void st8(TS_GLOBAL u64* base, uint32_t idx, u64 v) {
  *(TS_GLOBAL u64*)((TS_GLOBAL char*)base + (uint32_t)(idx << 3)) = v;
}
// heap slot k / its dir byte: LDS below LDS_HEAP, the searcher's HBM spill above (gq / gd are the slot's spill arrays).
// SPILL = false: the caller guarantees k < LDS_HEAP - straight LDS accesses, no branch (and with it no conservative
// wait for the expansion's loads in flight) in the hot loop.
template <bool SPILL> __device__ __forceinline__ u64 hq_get(gu64p gq, int k) {
  if constexpr (SPILL) return k < LDS_HEAP ? g_lq[k] : gq[k - LDS_HEAP];
  else return g_lq[k];
}
template <bool SPILL> __device__ __forceinline__ void hq_put(gu64p gq, int k, u64 v) {
  if constexpr (SPILL) { if (k < LDS_HEAP) g_lq[k] = v; else gq[k - LDS_HEAP] = v; }
  else g_lq[k] = v;
}
template <bool SPILL> __device__ __forceinline__ int hd_get(gi8p gd, int k) {
  if constexpr (SPILL) return k < LDS_HEAP ? (int)g_ld[k] : (int)gd[k - LDS_HEAP];
  else return (int)g_ld[k];
}
template <bool SPILL> __device__ __forceinline__ void hd_put(gi8p gd, int k, int v) {
  if constexpr (SPILL) { if (k < LDS_HEAP) g_ld[k] = (int8_t)v; else gd[k - LDS_HEAP] = (int8_t)v; }
  else g_ld[k] = (int8_t)v;
}
// the same for the lanes with `p` only, without switching the others off: every lane stores to LDS, an idle lane (and, in
// the spill form, one whose slot lies in HBM) to the spare slot; only the HBM part of the spill form keeps its branch
template <bool SPILL> __device__ __forceinline__ void hq_put_if(gu64p gq, bool p, int k, u64 v) {
  if constexpr (SPILL) {
    const bool lo = p & (k < LDS_HEAP);
    g_lq[lo ? k : LDS_HEAP] = v;
    if (p & !lo) gq[k - LDS_HEAP] = v;
  } else g_lq[p ? k : LDS_HEAP] = v;
}
template <bool SPILL> __device__ __forceinline__ void hd_put_if(gi8p gd, bool p, int k, int v) {
  if constexpr (SPILL) {
    const bool lo = p & (k < LDS_HEAP);
    g_ld[lo ? k : LDS_HEAP] = (int8_t)v;
    if (p & !lo) gd[k - LDS_HEAP] = (int8_t)v;
  } else g_ld[p ? k : LDS_HEAP] = (int8_t)v;
}

// a fresh epoch for the searcher's table (cleared by the wave when the stamp reaches the end of its range: wave_epoch_next)
__device__ __forceinline__ uint32_t next_epoch(const Dev& d, AScratch& S) {
  bool wrap;
  const uint32_t e = wave_epoch_next(S.epoch, T_STAMP_MAX, wrap);
  if (wrap) {
    const size_t n = (size_t)max(d.n_nodes, 1);     // (the spare record behind them is never read)
    for (size_t q = lane_id(); q < n; q += 64) S.tab[q] = TEnt{0, 0u};
    __syncthreads();
  }
  S.epoch = e;
  return e;
}

// obstacle penalty of an occupied cell under VEHICLE_DYNAMIC_PENALTIES (astar_numba.py:203-206): int(veh_pen * (1 + scale * density))
__device__ __forceinline__ double occ_penalty_dyn(double veh_pen, double dyn_scale, float dens) {
#pragma clang fp contract(off)
  return __builtin_trunc(veh_pen * (1.0 + dyn_scale * (double)dens));
}

// what a search keeps in registers while its loop runs (d, P and S themselves live in scratch memory behind references)
struct ACtx {
  int W, H, W8, N, lane;
  u64 w_magic;
  gu64p gq, tab;
  gi8p gd;
  const TS_GLOBAL u64* amap;
  const TS_GLOBAL u64* fovrun;
  const TS_GLOBAL float* density;
  gi32p outg;
  int heap_cap, out_cap, start_idx, goal_idx, gx, gy, maximum_steps, sx, sy, aw;
  int goal_xy;            // the goal as a heap entry carries it (xy_pack)
  uint32_t tab_spare;     // the table record no search reads
  bool fov;
  uint32_t epoch;
  bool soft, ignore_flow, limited, turn_on, rt_on, dens_on;
  double turn_pen, contra_pen, veh_pen, stop_pen, dyn_scale, rt1, rt2, rt3;
  HalfCosts hc;           // the same in half units (valid when `half`)
  bool half;
  // per search, 32 bits (n_exp <= n_relax + 1: every pop but the first was pushed by a relaxation; the loop gives up with
  // AL_OVERFLOW before n_relax can wrap); n_exp_spill: expansions made while part of the heap sat in HBM
  int n_exp, n_relax, n_exp_spill;
  int max_heap;
  uint32_t big;           // per lane: the largest dist word a table store of this search carried (ASlots::big_thr)
  // the tail rule (AScratch::t_ctl; `tail`: this search follows it): n_exp then counts up to zero, the expansions made are
  // n_exp + n_exp_base (exp_made), and at zero the search looks at the idle counter
  int n_exp_base, tail_thr, tail_floor;
  bool tail;
  const TS_GLOBAL int* tail_idle;
  __device__ __forceinline__ int exp_made() const { return n_exp + n_exp_base; }
  long long prof[8], pt;
  __device__ __forceinline__ void xy_of(int cell, int& x, int& y) const { cell_xy(W, w_magic, cell, x, y); }
  __device__ __forceinline__ uint32_t tile_ix(int x, int y) const { return tix(W8, x, y); }
};
#ifdef TS_KPROF
#define KP(k) do { const long long _t = clock64(); C.prof[k] += _t - C.pt; C.pt = _t; } while (0)
#else
#define KP(k) do { } while (0)
#endif
enum { AL_EMPTY = -2, AL_OVERFLOW = -1, AL_SWITCH = -3, AL_HANDOFF = -4 };   // astar_loop results besides a path length >= 0
constexpr int AW_HANDOFF = -2;   // astar_wave: the search was abandoned for the host to run (besides a length >= 0 and -1 = capacity)

// ---------------------------------------------------------------------------------------------
// astar_core's main loop, one search spread over one wavefront.  The algorithm is the sequential one - same heap
// layout, same comparisons, same order of relaxations - only its work is organised by lanes:
//   * everything the expansion of the popped cell reads from HBM is requested as soon as the cell is known (lanes
//     0-3: map entry, table record and density of neighbour `lane`; the other lanes: the cell's own) and travels while
//     the sift-down works on the heap;
//   * sift-down: lanes 2..63 fetch the 62 entries of the five levels below the hole at once (lane L's children sit
//     on lanes 2L and 2L + 1, siblings on an even / odd lane pair); every lane decides with its sibling's key (one DPP
//     swap) whether its entry would move up if its parent were the hole, one ballot collects that, the walk down
//     the five levels is scalar bit tests on the ballot, and the entries on the path move up with one masked write;
//   * sift-up of a push: the ancestors of the new slot are fetched at once, a ballot finds how far the entry rises,
//     the lanes holding ancestors write them one level down in parallel;
//   * the four neighbours are evaluated on lanes 0-3, then committed in the reference's order N, E, S, W.
// SPILL = false runs while the whole heap fits LDS (straight LDS accesses); SPILL = true is the general form.  Either
// returns AL_SWITCH when the other one should take over.
// ---------------------------------------------------------------------------------------------
// TAIL: the loop carries the tail rule's test (searches of a wave with a tail control block, half units, no field of view);
// without it the loop is instruction for instruction what it was before the rule existed.
template <bool SPILL, bool HALF, bool FOV, bool TAIL = false>
__device__ __forceinline__ int astar_loop(ACtx& C, int& heap_size) {
  // A lone wave issues one instruction every four cycles whatever its kind, so this loop is written for instruction
  // count: lane-parallel vector work and one ballot in place of scalar walks, no scalar <-> vector round trips that
  // can be avoided.
  const int lane = C.lane;
  const int W = C.W, H = C.H;
  const gu64p gq = C.gq;
  const gi8p gd = C.gd;
  const gu64p tab = C.tab;
  const uint32_t epoch = C.epoch, stamp = C.epoch << T_STAMP_SHIFT;
  const int gx = C.gx, gy = C.gy, goal_xy = C.goal_xy;
  const uint32_t tab_spare = C.tab_spare;
  // window geometry of this lane (lanes 2..63 = the 62 entries of five levels below a hole that sits on "lane 1")
  const int wlvl = 31 - __builtin_clz((unsigned)max(lane, 1));   // 1 for lanes 2-3, ... 5 for 32-63
  const int woff = lane - (1 << wlvl);
  const bool wlane = lane >= 2;
  const int wadj = (lane & 1) == 0 ? 1 : 0;                       // left children (even lanes) win ties against their sibling
  unsigned long long wanc = 0;                                     // this lane's ancestors-or-self inside the window
  for (int j = 0; j < wlvl; j++) wanc |= 1ull << (lane >> j);
  if (!wlane) wanc = ~0ull;                                        // lanes 0-1 hold no entry: their path test can never pass (bits 0-1 of a winner mask are never set)
  {  // pin the mask in registers: left alone, the compiler re-derives it (a six-step loop) in every turn of the main loop
    unsigned lo = (unsigned)wanc, hi = (unsigned)(wanc >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    wanc = ((unsigned long long)hi << 32) | lo;
  }
  const int dd_l = lane & 3;
  const int dx_l = lane < 4 ? (dd_l == 1) - (dd_l == 3) : 0, dy_l = lane < 4 ? (dd_l == 0) - (dd_l == 2) : 0;
  const int dxy_l = dx_l + dy_l * 65536;                           // the same step on packed coordinates
  const unsigned below_l = (1u << lane) - 1u;                      // (lanes 0-3 use it)
  // One back edge: a stale pop runs the evaluation with every neighbour killed (a few per cent of the pops: cheaper than a
  // second path to the loop's head with its copies of the loop-carried state), and a turn without relaxations skips
  // the commit block only.
  while (heap_size > 0) {
    if (!SPILL && heap_size > LDS_HEAP - 4) return AL_SWITCH;        // this turn's pushes might not fit LDS
    if (SPILL && heap_size < LDS_HEAP - 96) return AL_SWITCH;      // (heaps breathe by a few entries per turn: a band of ~90 keeps the switches rare)
    KP(7);
    // one LDS read serves the root (lane 0; every lane gets it through readfirstlane) and the first sift-down window
    // (lanes 2..63: slots 1..62 - the window below a hole at the root): nothing has written to them in this turn yet
    const u64 w0 = g_lq[max(lane - 1, 0)];
    const int prev_dir = uni((int)g_ld[0]);
    const u64 x = uni64(hq_get<SPILL>(gq, heap_size - 1));            // the last entry: it takes the root's place
    const int xd = uni(hd_get<SPILL>(gd, heap_size - 1));
    const int f_top = uni(hq_f(w0)), cur = uni(hq_i(w0));     // (readfirstlane: lane 0's word, the root; cur = y << 16 | x)
    heap_size--;
    KP(0);
    const int cx = cur & A_XY_MAX, cy = (int)((unsigned)cur >> 16);
    const int nx_l = cx + dx_l, ny_l = cy + dy_l;
    const bool inb_l = (unsigned)nx_l < (unsigned)W && (unsigned)ny_l < (unsigned)H;
    const int nidx_l = inb_l ? (int)((uint32_t)cur + (uint32_t)dxy_l) : cur;
    const uint32_t t_l = C.tile_ix(inb_l ? nx_l : cx, inb_l ? ny_l : cy);    // (the coordinates are selected, not the results: no branch)
    // round 1: the map entries (flags + search-node number); round 2, issued half-way through the sift-down: the table
    // records of those nodes
    const u64 am_l = ld8(C.amap, t_l);
    float dens_l = 0.0f;      // (HALF searches find the cell's vehicle penalty in the map entry itself)
    if constexpr (!HALF) dens_l = C.density[inb_l ? ny_l * W + nx_l : cy * W + cx];      // (read whether or not the search is soft: no branch around a load)
    u64 fr_l = 0;
    if constexpr (FOV) fr_l = ld8(C.fovrun, t_l);
    u64 e_l = 0;
    bool e_loaded = false;
    KP(1);
    if (heap_size > 0) {
      const int xf = hq_f(x);
      wave_mem_sync();                     // every lane has read slot 0 before it is overwritten
      g_ld[lane == 0 ? 0 : LDS_HEAP] = (int8_t)xd;
      int idx = 0;                         // the hole; x keeps sinking
      for (;;) {
        const int abs_l = ((idx + 1) << wlvl) + woff - 1;
        const bool valid = wlane & (abs_l < heap_size);
        const u64 mine = idx == 0 ? w0 : hq_get<SPILL>(gq, valid ? abs_l : 0);   // (idx == 0: abs_l = lane - 1, read above)
        const int mf = valid ? hq_f(mine) : 0x7FFFFFFF;
        const int sf = __builtin_amdgcn_mov_dpp(mf, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]: the sibling's key
        // smallest of (x, left, right) with ties going to x, then left (heap_sift_down, astar_numba.py:67-85):
        // "my entry moves up if my parent is the hole" - at most one of two siblings.  Left: mine <= sibling's, right:
        // mine < sibling's; keys are >= 0, so mine <= s is (mine - 1) < s.
        // (one compare per ballot: the backend hands a compare's lane mask over as it is, anything else is turned into
        // 0 / 1 and compared again.)  mf < xf and mf - wadj < sf  <=>  mf < min(xf, sf + wadj), in unsigned arithmetic
        // (keys are >= 0, an empty slot is 0x7FFFFFFF: the sum cannot wrap)
        const unsigned long long wmask = ballot((unsigned)mf < min((unsigned)xf, (unsigned)sf + (unsigned)wadj));
        // A lane's entry is on the sift path iff it and all its ancestors inside the window are winners: one mask
        // test per lane (wanc = the lane's ancestors-or-self).  Exactly one lane per level can pass, so a second
        // ballot yields both the number of levels the hole sinks (k) and where it ends up (L).
        const bool onp = (wmask & wanc) == wanc;
        const unsigned long long pmask = ballot(onp);
        const int k = __builtin_popcountll(pmask);
        const int L = 63 - __builtin_clzll(pmask | 2ull);             // deepest lane on the path; the hole itself (1) if none
        const int abs_end = uni(((idx + 1) << k) + (L - (1 << k)) - 1);
        const bool done = k < 5;
        // the entries on the path move up one level, and x settles where the hole ends up: one store (lane 0 holds no
        // entry and is never on the path - it carries x)
        const bool put_x = done & (lane == 0);
        hq_put_if<SPILL>(gq, onp | put_x, put_x ? abs_end : (abs_l - 1) >> 1, put_x ? x : mine);
        if (!e_loaded) {                   // the first window is done: the map entries have had time to arrive
          const uint32_t r_l = (uint32_t)(am_l >> 32);
          e_l = ld8(tab, r_l != AM_NO_NODE ? r_l : 0u);
          e_loaded = true;
        }
        if (done) break;
        idx = abs_end;                     // five levels down and still sinking: next window
      }
    }
    wave_mem_sync();
    KP(2);
    const uint32_t a_l = (uint32_t)am_l, r_l = (uint32_t)(am_l >> 32);
    const bool node_l = r_l != AM_NO_NODE;
    if (!e_loaded) e_l = ld8(tab, node_l ? r_l : 0u);     // (the heap held a single entry: no sift-down happened)
    if (cur == goal_xy) {
      // walk came_from back to the start, filling the output from its far end, then slide it to the front
      const gi32p outg = C.outg;
      const int out_cap = C.out_cap;
      int len = 0, px = cx, py = cy;
      for (int c = cy * W + cx; c != C.start_idx;) {
        if (len >= out_cap) return AL_OVERFLOW;
        if (lane == 0) outg[out_cap - 1 - len] = c;
        len++;
        const uint32_t pr = (uint32_t)(C.amap[C.tile_ix(px, py)] >> 32);
        const int dd = (int)((tab[pr] >> 32) & T_DIR_MASK);
        px -= (dd == 1) - (dd == 3); py -= (dd == 0) - (dd == 2);
        c = py * W + px;
      }
      __syncthreads();
      const int shift = out_cap - len;
      if (shift > 0)
        for (int k0 = 0; k0 < len; k0 += 64) {
          const int k = k0 + lane;
          const int v = k < len ? outg[shift + k] : 0;
          if (k < len) outg[k] = v;
        }
      __syncthreads();
      return len;
    }
    const int g = f_top - (abs(cx - gx) + abs(cy - gy));
    const u64 e_c = rl(e_l, 4);
    const bool node_c = rl((int)node_l, 4) != 0;     // (only a start cell can be off the node set: dist 0, no steps)
    const uint32_t m_c = node_c ? (uint32_t)(e_c >> 32) : (epoch << T_STAMP_SHIFT);
    const int dist_c = !node_c ? 0 : (m_c >> T_STAMP_SHIFT) == epoch ? (int)(uint32_t)e_c : A_INF;
    bool fresh = g <= dist_c;      // (a stale pop relaxes nothing)
    KP(3);
    C.n_exp += fresh ? 1 : 0;
    // the tail rule: one scalar compare per turn; every TAIL_PERIOD fresh expansions a look at the idle counter.  The search is
    // abandoned (nothing of it is kept) once all but t_max waves of the launch have found the queue empty.
    // (A search under the rule counts its expansions from minus the number still to go until the next look - the count itself is
    // n_exp + n_exp_base -, so the test is a compare with zero.  Giving up is no exit of its own - that would stage the loop's
    // results on every turn: the heap size goes to TAIL_GAVE_UP and the pop counts as stale, so the turn relaxes nothing and the
    // loop ends as if the heap were empty; astar_wave reads the heap size.)
    if constexpr (TAIL) if (__builtin_expect(C.n_exp == 0, 0)) {
      const int made = C.n_exp_base;
      C.n_exp_base = made + TAIL_PERIOD; C.n_exp = -TAIL_PERIOD;
      const int idle = uni(__hip_atomic_load(C.tail_idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if ((idle >= C.tail_thr) & (made >= C.tail_floor)) { heap_size = TAIL_GAVE_UP; fresh = false; }
    }
    const int steps = C.limited ? (int)((m_c >> T_STEPS_SHIFT) & T_STEPS_MASK) : 0;
    const uint32_t bits = (uint32_t)rl((int)a_l, 4) & AM_DIRS_MASK;
    // ---- lane dd < 4 evaluates neighbour dd from what was fetched before the sift-down -------------------------
    // HALF: every penalty is a non-negative multiple of 0.5 (the reference's defaults are), so the reference's float `ng`
    // is carried exactly as an integer count of half units: ng < dist  <=>  ng2 < 2 dist, int(ng) = ng2 >> 1,
    // int(ng + h) = (ng2 >> 1) + h.  Otherwise the same in doubles.
    double ng_l = 0.0;
    int ng2_l = 0;
    bool ok_l;
    {
      const uint32_t m_l = (uint32_t)(e_l >> 32);
      const int dist_l = (m_l >> T_STAMP_SHIFT) == epoch ? (int)(uint32_t)e_l : A_INF;
      bool n_occ = ((a_l >> AM_OCC_BIT) & 1u) != 0u, n_stop = ((a_l >> AM_RED_BIT) & 1u) != 0u;
      const bool n_road = ((a_l >> AM_ROAD_BIT) & 1u) != 0u;
      if constexpr (FOV) {
        // compute_fov_inplace (astar_numba.py:29-50): the neighbour is seen iff a straight run of road cells joins it to
        // the line of 2 * awareness - 1 cells through the START cell perpendicular to that run's direction
        const int dxs = nx_l - C.sx, dys = ny_l - C.sy, aw = C.aw;
        const int run_dn = (int)(fr_l & 0xFFFF), run_up = (int)((fr_l >> 16) & 0xFFFF), run_lf = (int)((fr_l >> 32) & 0xFFFF), run_rt = (int)(fr_l >> 48);
        const bool band_x = (dxs < aw) & (dxs > -aw), band_y = (dys < aw) & (dys > -aw);
        const bool seen = (band_x & (dys >= 0) & (run_dn > dys)) | (band_x & (dys <= 0) & (run_up > -dys)) |
                          (band_y & (dxs >= 0) & (run_lf > dxs)) | (band_y & (dxs <= 0) & (run_rt > -dxs));
        n_occ &= seen; n_stop &= seen;
      }
      const uint32_t rt = (a_l >> AM_RT_SHIFT) & AM_RT_MASK;
      const bool flow = ((bits >> dd_l) & 1u) != 0u;
      const bool turn = C.turn_on & (prev_dir != -1) & (dd_l != prev_dir);
      bool cheaper;
      // (selects, not branches: a killed neighbour's cost is simply not used)
      if constexpr (HALF) {
        int n2 = 2 * (g + 1);
        n2 += turn ? C.hc.turn2 : 0;
        n2 += flow ? 0 : C.hc.contra2;
        const int occ2 = (int)(a_l >> AM_PEN_SHIFT);     // k_amap_build: veh2, or the density-dependent penalty of this cell
        n2 += n_occ ? occ2 : 0;
        n2 += n_stop ? C.hc.stop2 : 0;
        const int rtp = (rt == 1u ? C.hc.rt2_1 : 0) | (rt == 2u ? C.hc.rt2_2 : 0) | (rt == 3u ? C.hc.rt2_3 : 0);   // (a chain of ?: becomes nested branches)
        n2 += (C.rt_on & n_road) ? rtp : 0;
        ng2_l = n2;
        cheaper = n2 < 2 * dist_l;
      } else {
        ng_l = (double)(g + 1);
        ng_l += turn ? C.turn_pen : 0.0;
        ng_l += flow ? 0.0 : C.contra_pen;
        const double occ_pen = C.dens_on ? occ_penalty_dyn(C.veh_pen, C.dyn_scale, dens_l) : C.veh_pen;
        ng_l += n_occ ? occ_pen : 0.0;
        ng_l += n_stop ? C.stop_pen : 0.0;
        ng_l += (C.rt_on & n_road) ? ((rt == 1u ? C.rt1 : 0.0) + (rt == 2u ? C.rt2 : 0.0) + (rt == 3u ? C.rt3 : 0.0)) : 0.0;   // (one term at most is not + 0.0: exact)
        cheaper = ng_l < (double)dist_l;
      }
      ok_l = fresh & (lane < 4) & inb_l & node_l & (steps + 1 <= C.maximum_steps) & (flow | (C.ignore_flow & n_road)) & (C.soft | !(n_occ | n_stop)) & cheaper;
    }
    // ---- commit.  The four neighbours are distinct cells, so no relaxation changes another one's test: the table
    // records and the dir bytes of all of them go out with one masked store each; only the heap pushes are made one
    // after the other, in the reference's order N, E, S, W.
    unsigned relax = (unsigned)(ballot(ok_l) & 15ull);
    KP(4);
    // (the counters move on both paths alike - nothing to copy where they join; heap_size + 0 never exceeds the deepest heap)
    const int n_new = __builtin_popcount(relax);
    C.n_relax += n_new;
    C.max_heap = max(C.max_heap, heap_size + n_new);
    if (relax != 0u) {
      if ((heap_size + n_new > C.heap_cap) | (C.n_relax > 0x7FFFFFF0)) return AL_OVERFLOW;
      const int h_l = abs(nx_l - gx) + abs(ny_l - gy);
      const int ngi_l = HALF ? (ng2_l >> 1) : (int)ng_l;
      const u64 ent_l = hq_pack(HALF ? ngi_l + h_l : (int)(ng_l + (double)h_l), nidx_l);
      // (every lane stores: the idle ones to the table's spare record and the spare dir byte - their dist words count for
      // `big` like any other: the spare record lies in the arena too)
      C.big = max(C.big, (uint32_t)ngi_l);
      st8(tab, ok_l ? r_l : tab_spare, (u64)(uint32_t)ngi_l | ((u64)(stamp | (C.limited ? (uint32_t)(steps + 1) << T_STEPS_SHIFT : 0u) | (uint32_t)dd_l) << 32));
      hd_put_if<SPILL>(gd, ok_l, heap_size + __builtin_popcount(relax & below_l), dd_l);
      KP(5);
      do {
        const int dd = __builtin_ctz(relax);
        relax &= relax - 1;
        const u64 nx64 = rl(ent_l, dd);
        const int nf = hq_f(nx64);
        const int i = heap_size;
        // ancestors of slot i: a_k = ((i + 1) >> k) - 1, k = 1 .. depth; lane k - 1 fetches a_k
        const int depth = 31 - __builtin_clz((unsigned)(i + 1));
        const bool has = lane < depth;                                  // depth <= 31: lanes beyond it fetch nothing
        const int a_mine = (int)(((unsigned)(i + 1) >> ((lane + 1) & 31)) - 1u) & (has ? -1 : 0);
        const u64 anc = hq_get<SPILL>(gq, a_mine);
        const unsigned long long rises = ballot(has & (nf < hq_f(anc)));
        const int r = __builtin_ctzll(~rises);                          // leading ancestors the entry passes (lanes >= 31 never rise: r <= depth)
        // ancestor k moves to where k - 1 was (lanes < r), the new entry to where ancestor r was (lane r): slot
        // ((i + 1) >> lane) - 1 for both - one store
        hq_put_if<SPILL>(gq, lane <= r, (int)((unsigned)(i + 1) >> (lane & 31)) - 1, lane == r ? nx64 : anc);
        heap_size++;
        wave_mem_sync();
      } while (relax);
    }
    KP(6);
  }
  return AL_EMPTY;
}

// astar_core (astar_numba.py:87-239).  All 64 lanes call it with identical arguments and get the same return value.
// Writes the path (start excluded, goal included) to out[0..len); returns len >= 0, or -1 when the heap or the output
// buffer is too small.
// may_hand_off (astar_any<DM_WAVE> for a logged search of a wave with a tail control block): the search follows the tail rule and
// returns AW_HANDOFF, counted nowhere, when it gives up for the host.
__device__ int astar_wave(const Dev& d, const TsParams& P, AScratch& S, int start_idx, int goal_idx, bool soft,
                          bool ignore_flow, int maximum_steps, int32_t* out, int out_cap, bool may_hand_off = false) {
  ACtx C;
  C.lane = lane_id();
  // the arguments arrive in vector registers: tell the compiler they are wave-uniform (scalar loop control)
  C.start_idx = uni(start_idx); C.goal_idx = uni(goal_idx); C.maximum_steps = uni(maximum_steps); C.out_cap = uni(out_cap);
  C.soft = uni((int)soft) != 0; C.ignore_flow = uni((int)ignore_flow) != 0;
  S.calls++;
  C.epoch = (uint32_t)uni((int)next_epoch(d, S));
  C.W = uni(d.W); C.H = uni(d.H); C.W8 = uni(d.W8); C.N = uni(d.N);
  C.w_magic = uni64(d.w_magic);
  C.gq = (gu64p)(uintptr_t)uni64((u64)(uintptr_t)S.gq);
  C.gd = (gi8p)(uintptr_t)uni64((u64)(uintptr_t)S.gd);
  C.tab = (gu64p)(uintptr_t)uni64((u64)(uintptr_t)S.tab);
  C.amap = (const TS_GLOBAL u64*)(uintptr_t)uni64((u64)(uintptr_t)d.amap);
  C.fovrun = (const TS_GLOBAL u64*)(uintptr_t)uni64((u64)(uintptr_t)d.fovrun);
  C.fov = P.respect_awareness != 0 && d.fovrun != nullptr;
  C.aw = uni(P.vehicle_awareness_range);
  C.density = (const TS_GLOBAL float*)(uintptr_t)uni64((u64)(uintptr_t)d.density);
  C.outg = (gi32p)(uintptr_t)uni64((u64)(uintptr_t)out);
  C.heap_cap = uni(S.heap_cap);
  C.turn_on = P.turn_penalty_enabled != 0; C.rt_on = P.road_type_penalties_enabled != 0;
  C.dens_on = C.soft && P.dynamic_penalties_enabled;
  C.turn_pen = P.turn_penalty; C.contra_pen = P.contraflow_penalty; C.veh_pen = P.obstacle_penalty_vehicle;
  C.stop_pen = P.obstacle_penalty_stop; C.dyn_scale = P.dynamic_penalty_scale; C.rt1 = P.road_type_penalty_r1;
  C.rt2 = P.road_type_penalty_r2; C.rt3 = P.road_type_penalty_r3;
  {
    // half units carry the costs exactly iff every penalty is a non-negative multiple of 0.5 of moderate size
    C.half = astar_half_units(P);
    C.hc = half_costs(P);
  }
  C.n_relax = 0; C.n_exp_spill = 0; C.max_heap = 0; C.big = 0;     // (n_exp: with the tail rule's switches below)
  C.tab_spare = (uint32_t)uni(max(d.n_nodes, 1));
  for (int k = 0; k < 8; k++) C.prof[k] = 0;
  C.pt = clock64();
  // the chain of relaxations behind a heap entry never revisits a cell (dist strictly falls), so it is shorter than
  // N: a limit of N or more never binds and the steps need not be carried
  C.limited = C.maximum_steps < C.N;
  {
    const bool tail = may_hand_off && S.t_ctl != nullptr && !C.limited && !C.ignore_flow && C.half && !C.fov;
    C.tail = uni((int)tail) != 0;
    C.n_exp_base = uni(tail ? S.t_first : 0); C.n_exp = -C.n_exp_base;
    C.tail_thr = uni(S.t_thr); C.tail_floor = uni(max(S.t_floor, 1));
    C.tail_idle = (const TS_GLOBAL int*)(uintptr_t)uni64((u64)(uintptr_t)(tail ? &S.t_ctl->idle : nullptr));
  }
  C.xy_of(C.goal_idx, C.gx, C.gy);
  C.xy_of(C.start_idx, C.sx, C.sy);
  C.goal_xy = xy_pack(C.gx, C.gy);
  const int sx = C.sx, sy = C.sy;
  if (C.lane == 0) {
    const uint32_t sr = (uint32_t)(C.amap[C.tile_ix(sx, sy)] >> 32);
    if (sr != AM_NO_NODE) C.tab[sr] = (u64)0u | ((u64)(C.epoch << T_STAMP_SHIFT) << 32);    // dist 0, steps 0
    g_lq[0] = hq_pack(abs(sx - C.gx) + abs(sy - C.gy), xy_pack(sx, sy));
    g_ld[0] = -1;
  }
  int heap_size = 1;
  wave_mem_sync();
  int r;
  // (the default policy is the <HALF, no FOV> pair; the other instantiations serve fractional penalties and
  // VEHICLE_RESPECT_AWARENESS)
  auto run = [&](auto half_c, auto fov_c, auto tail_c) {
    constexpr bool HF = decltype(half_c)::value, FV = decltype(fov_c)::value, TL = decltype(tail_c)::value;
    for (;;) {
      int q = astar_loop<false, HF, FV, TL>(C, heap_size);
      if (q != AL_SWITCH) return q;
      const int exp0 = C.exp_made();
      q = astar_loop<true, HF, FV, TL>(C, heap_size);
      C.n_exp_spill += C.exp_made() - exp0;
      if (q != AL_SWITCH) return q;
    }
  };
  if (C.tail && C.half && !C.fov) r = run(std::true_type{}, std::false_type{}, std::true_type{});
  else if (!C.fov) r = C.half ? run(std::true_type{}, std::false_type{}, std::false_type{}) : run(std::false_type{}, std::false_type{}, std::false_type{});
  else r = C.half ? run(std::true_type{}, std::true_type{}, std::false_type{}) : run(std::false_type{}, std::true_type{}, std::false_type{});
  if (heap_size == TAIL_GAVE_UP) r = AL_HANDOFF;
  if (r == AL_HANDOFF) S.calls--;     // (the abandoned part is not counted: the host's search is)
  else { S.expansions += C.exp_made(); S.relaxations += C.n_relax; }
  // (once per search: a dist word that a quad could take for a live record went into this slot's table)
  if (ballot(C.big >= S.big_thr) != 0ull && C.lane == 0) __hip_atomic_store(S.big_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (C.lane == 0) {   // profiling aid: deepest heap / longest search any searcher has seen (ts_debug_read words 4, 5)
    atomicMax(&d.cnt->max_heap, C.max_heap);
    if (r != AL_HANDOFF) atomicMax(&d.cnt->max_search_exp, C.exp_made());
    if (C.n_exp_spill) atomicAdd((unsigned long long*)&d.cnt->spill_exp, (unsigned long long)C.n_exp_spill);
#ifdef TS_KPROF
    for (int k = 0; k < 8; k++) d.cnt->prof[k] = C.prof[k];
#endif
  }
  return r == AL_EMPTY ? 0 : r == AL_HANDOFF ? AW_HANDOFF : r;
}

// Strict reachability of `goal` from `start`: a frontier BFS by the wave over the same edges the strict A* relaxes
// (flow bit set, neighbour in bounds, neither occupied nor red), 64 cells per step.  Unreachable targets are by far
// the most expensive searches (the sequential search floods the whole component before returning []); knowing the
// answer lets phase 1 skip them.  Visited marks are stamps of a fresh epoch in the searcher's own table, the queue is
// a ring in its heap spill area.  Returns 1 reachable, 2 not, 0 unknown (ring overflow).
__device__ int reach_strict_wave(const Dev& d, AScratch& S, int start, int goal) {
  const int lane = lane_id();
  start = uni(start); goal = uni(goal);
  const uint32_t stamp = (uint32_t)uni((int)next_epoch(d, S)) << T_STAMP_SHIFT;
  const int W = uni(d.W), H = uni(d.H), W8 = uni(d.W8);
  const u64 w_magic = uni64(d.w_magic);
  const gi32p ring = (gi32p)(uintptr_t)uni64((u64)(uintptr_t)S.gq);
  TS_GLOBAL uint32_t* const tabw = (TS_GLOBAL uint32_t*)(uintptr_t)uni64((u64)(uintptr_t)S.tab);   // record t: dist at 2t, meta at 2t + 1
  const TS_GLOBAL u64* amap = (const TS_GLOBAL u64*)(uintptr_t)uni64((u64)(uintptr_t)d.amap);
  const unsigned qcap = (unsigned)uni(S.heap_cap - LDS_HEAP) * 2u;
  if (qcap < 256u) return 0;
  if (lane == 0) {
    int sx, sy;
    cell_xy(W, w_magic, start, sx, sy);
    ring[0] = start;
    const uint32_t sr = (uint32_t)(amap[tix(W8, sx, sy)] >> 32);
    if (sr != AM_NO_NODE) tabw[2 * (size_t)sr + 1] = stamp;
  }
  __syncthreads();
  unsigned head = 0, tail = 1;
  bool found = false;
  while (head < tail && !found) {
    const unsigned idx = head + (unsigned)lane;
    const int c = idx < tail ? ring[idx % qcap] : -1;
    head = min(tail, head + 64u);
    int cx = 0, cy = 0;
    if (c >= 0) cell_xy(W, w_magic, c, cx, cy);
    const uint32_t bits = c >= 0 ? (uint32_t)amap[tix(W8, cx, cy)] & AM_DIRS_MASK : 0u;
    for (int dd = 0; dd < 4; dd++) {
      int n = -1;
      if (bits & (1u << dd)) {
        const int nx = cx + (dd == 1) - (dd == 3), ny = cy + (dd == 0) - (dd == 2);
        if (nx >= 0 && nx < W && ny >= 0 && ny < H) {
          const u64 an = amap[tix(W8, nx, ny)];
          const uint32_t rn = (uint32_t)(an >> 32);
          if (((uint32_t)an & AM_BLOCKED) == 0u && rn != AM_NO_NODE &&
              __hip_atomic_exchange(&tabw[2 * (size_t)rn + 1], stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != stamp)
            n = ny * W + nx;
        }
      }
      const unsigned long long m = __ballot(n >= 0);
      const unsigned cnt = (unsigned)__popcll(m);
      if (tail + cnt - head > qcap) return 0;
      if (n >= 0) ring[(tail + (unsigned)__popcll(m & ((1ULL << lane) - 1))) % qcap] = n;
      if (__ballot(n == goal && n >= 0)) found = true;
      tail += cnt;
    }
    __syncthreads();  // ring writes of this step are read by the next one
  }
  return found ? 1 : 2;
}

// lane 0 draws the next value of a queue cursor for the whole wave
__device__ __forceinline__ int wave_pop(int* cursor) {
  if (threadIdx.x == 0) g_job = atomicAdd(cursor, 1);
  __syncthreads();
  const int j = uni(g_job);
  __syncthreads(); return j;
}
// searches that ended in a committed result, into the model's counters
__device__ __forceinline__ void searcher_account(const Dev& d, long long calls, long long exp, long long relax) {
  atomicAdd((unsigned long long*)&d.cnt->astar_calls, (unsigned long long)calls);
  atomicAdd((unsigned long long*)&d.cnt->astar_exp, (unsigned long long)exp);
  atomicAdd((unsigned long long*)&d.cnt->astar_relax, (unsigned long long)relax);
}

// one search on the current maps (the `astar(...)` operator seam, ts_astar) - searcher slot 0
TS_REPLAN_OCC __global__ void __launch_bounds__(64) k_astar_single(Dev d, TsParams P, ASlots sl, int start_idx, int goal_idx, int soft,
                                                      int ignore_flow, int maximum_steps, int32_t* out_len) {
  if (blockIdx.x) return;
  AScratch S;
  scratch_bind(sl, 0, S);
  const long long c0 = clock64(), w0 = wall_clock64();
  int len = astar_wave(d, P, S, start_idx, goal_idx, soft != 0, ignore_flow != 0, maximum_steps, S.A, S.cap);
  if (threadIdx.x) return;
  {  // probe figures (profiles/astar_probe.py): shader cycles and 100 MHz wall ticks the search took
    const long long dc = clock64() - c0, dw = wall_clock64() - w0;
    d.cnt->probe_cycles = dc; d.cnt->probe_wall = dw;
  }
  sl.slot_epoch[0] = S.epoch;
  if (len >= 0) searcher_account(d, S.calls, S.expansions, S.relaxations);
  *out_len = len;  // -1 = heap / output capacity exceeded; the path cells are in the slot's A buffer
}

}  // namespace
