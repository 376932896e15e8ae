// decide.h - the replanning policy of VehicleAgent (decide_vehicle) and the path pool its plans are committed to.
//
// decide_vehicle restates step_decide (vehicle_base.py:616-663) with _recompute_path_on_stuck 506-517,
// _recompute_path_on_obstacle 454-504, _compute_path 143-167 and _compute_path_internal 199-420
// (phases 0-4).  It is a pure function of the tick-start state until its final commit, so the same code
// runs in k_decide_main (one vehicle per lane, no scratch: bails out as soon as a search is needed) and in
// k_replan (one vehicle per wave, every lane executing the same code on the same values).
#pragma once
#include "astar.h"

namespace {

// (DV_HANDOFF: DM_WAVE under the tail rule - a search was abandoned for the host to run, nothing is committed; replan.h)
enum { DV_DONE = 0, DV_DEFER = 1, DV_OVERFLOW = 2, DV_POOL_FULL = 3, DV_SUSPEND = 4, DV_BAIL = 5, DV_HANDOFF = 6 };
// Who runs a vehicle's step_decide: one lane without scratch (k_decide_main: bails out as soon as a search is needed), one
// wavefront (k_replan: every lane the same code on the same values, searches spread over the wave), or one quad of four
// lanes (k_replan_quad, astar_quad.h: sixteen vehicles per wave, their searches advancing in lockstep)
enum { DM_LANE = 0, DM_WAVE = 1, DM_QUAD = 2 };

// ---------------------------------------------------------------------------------------------
// vehicle working state for one step_decide
// ---------------------------------------------------------------------------------------------
struct VW {
  int vid, i, pos, target;
  uint16_t f;
  int base, cur, cooldown, over_dur, det_dur, stuck_ticks;
  // current path: pool-resident direction string, or cells in S.P
  bool newpath;
  int plen, pcur;
  uint32_t off;
  // aux paths k: 0 overtake_path, 1 pre_overtake_path, 2 stuck_detour_path, 3 pre_stuck_detour_path
  bool ax_staged[4];
  int ax_len[4];  // -1 = None
  int d_overtaking, d_detour;
  bool reach_known;  // a replan inside the decide phase: phase 1 asks reach_strict_wave first
};

__device__ __forceinline__ int32_t* ax_buf(const AScratch& S, int k) { return k == 0 ? S.OV : k == 1 ? S.PO : k == 2 ? S.DV : S.PD; }

// sequential reader over an aux path (staged cells or pool-resident directions)
struct AxReader {
  const int32_t* cells;
  PathWalk walk;   // (walk.idx counts the staged cells too)
  __device__ void init(const Dev& d, const AScratch& S, const VW& v, int k) {
    walk.idx = 0; walk.W = d.W; walk.pool = d.pool;
    if (v.ax_staged[k]) { cells = ax_buf(S, k); }
    else { cells = nullptr; walk.off = d.ax_off[k][v.vid]; walk.cell = d.ax_start[k][v.vid]; }
  }
  __device__ __forceinline__ int next() { return cells ? cells[walk.idx++] : walk.next(); }
};

__device__ __forceinline__ int vw_path_cell(const Dev& d, const AScratch* S, const VW& v, int k, int& walk) {
  // k-th remaining cell; `walk` carries the running cell for pool-resident paths (call with k ascending)
  if (v.newpath) return S->P[k];
  walk = step_cell(walk, path_dir(d.pool, v.off, v.pcur + k), d.W);
  return walk;
}

// _scan_ahead_for_obstacles (vehicle_base.py:422-452).  The cells are decoded first and their records loaded
// together (independent loads, one memory round trip); the reference's early exit at index 0 only shortens the
// evaluation.
constexpr int SCAN_MAX = 16;
__device__ void scan_ahead_dev(const Dev& d, const TsParams& P, const AScratch* S, const VW& v, int& idx_stop,
                               int& idx_veh, int& first_cell) {
  idx_stop = -1; idx_veh = -1; first_cell = -1;
  const int look = min(P.vehicle_awareness_range, v.plen);
  int walk = v.pos;
  if (look <= SCAN_MAX && !v.newpath) {
    int cells[SCAN_MAX];
    uint32_t dyn[SCAN_MAX];   // the dword holding occ / stop / stuck / stat
    // the next 16 steps are at most 32 bits of the direction string: two pool words, decoded in registers
    // (path_window without its test of the first word: path_words.h)
    const uint32_t wi = (uint32_t)v.pcur >> PATH_STEP_SHIFT, nwords = (uint32_t)path_words(v.pcur + v.plen);
    uint64_t bits = d.pool[v.off + wi];
    if (wi + 1 < nwords) bits |= (uint64_t)d.pool[v.off + wi + 1] << 32;
    bits >>= (v.pcur & PATH_STEP_MASK) * PATH_DIR_BITS;
    {
      int c = v.pos;
#pragma unroll
      for (int k = 0; k < SCAN_MAX; k++) {
        if (k < look) c = step_cell(c, (int)((bits >> (PATH_DIR_BITS * k)) & PATH_DIR_MASK), d.W);
        cells[k] = c;
      }
    }
    if (look > 0) first_cell = cells[0];
    // an obstacle at index 0 ends the scan (the reference's break can only fire there) - and in dense traffic that
    // is the common case, so the first record is fetched alone and the other nine only if it is clear
    dyn[0] = look > 0 ? *reinterpret_cast<const uint32_t*>(&d.cell[cells[0]].occ) : 0u;
    if (look > 0 && (int8_t)((dyn[0] >> 8) & 0xFF) == 1) idx_stop = 0;
    if (look > 0 && (int8_t)(dyn[0] & 0xFF) == 1) idx_veh = 0;
    if (idx_stop == 0 || idx_veh == 0) return;
#pragma unroll
    for (int k = 1; k < SCAN_MAX; k++) dyn[k] = k < look ? *reinterpret_cast<const uint32_t*>(&d.cell[cells[k]].occ) : 0u;
#pragma unroll
    for (int k = 1; k < SCAN_MAX; k++) {
      const bool in = k < look;
      const int occ = (int8_t)(dyn[k] & 0xFF), stop = (int8_t)((dyn[k] >> 8) & 0xFF);
      if (in && idx_stop < 0 && stop == 1) idx_stop = k;
      if (in && idx_veh < 0 && occ == 1) idx_veh = k;
    }
    return;
  }
  for (int k = 0; k < look; k++) {
    int c = vw_path_cell(d, S, v, k, walk);
    if (k == 0) first_cell = c;
    const Cell cc = d.cell[c];
    if (idx_stop < 0 && cc.stop == 1) idx_stop = k;
    if (idx_veh < 0 && cc.occ == 1) idx_veh = k;
    if (idx_stop == 0 || idx_veh == 0) break;
  }
}

__device__ __forceinline__ void swap_ptr(int32_t*& a, int32_t*& b) { int32_t* t = a; a = b; b = t; }

// _compute_path_internal (vehicle_base.py:199-420).  On success the result is in S.P[0..*out_len) (possibly
// empty).  Returns false on tier overflow.
// DM_WAVE: the caller runs with all 64 lanes of its wave executing the same code on the same values (one vehicle per
// wave); plain stores are then harmless duplicates, atomics are issued by lane 0 only, and the searches use
// astar_wave.  DM_QUAD: the same with the four lanes of a quad.  DM_LANE: one vehicle per lane (k_decide_main), nothing is shared.
constexpr int QLOG = 8;   // searches one step_decide can make in quad mode (beyond that the vehicle goes to k_replan)
constexpr int SLOG_INTS = 3 * QLOG;   // ints in a searcher slot's log (AScratch::q_log): length, expansions, relaxations per search
template <int MODE>
__device__ __forceinline__ int astar_any(const Dev& d, const TsParams& P, AScratch& S, int start_idx, int goal_idx, bool soft,
                                         bool ignore_flow, int maximum_steps, int32_t* out, int out_cap) {
  if constexpr (MODE == DM_WAVE) {
    // With a log (a k_replan pass that carries a tail control block, and its re-run): the quads' scheme for the searches the tail
    // rule applies to - no step limit, on the flow; the bypass searches always run.  Such a search is replayed from the log when an
    // earlier pass finished it (the host's among them; its path sits in `out`), may be abandoned for the host, and is logged.  Two
    // of them share an `out` buffer only when the first came back empty, so a replayed path is always intact.
    if (S.q_log == nullptr || maximum_steps < d.N || ignore_flow)
      return astar_wave(d, P, S, start_idx, goal_idx, soft, ignore_flow, maximum_steps, out, out_cap);
    const int k = S.q_replay++;
    if (k < S.q_done) {
      S.calls++; S.expansions += S.q_log[3 * k + 1]; S.relaxations += S.q_log[3 * k + 2];
      return S.q_log[3 * k];
    }
    const long long e0 = S.expansions, r0 = S.relaxations;
    const int r = astar_wave(d, P, S, start_idx, goal_idx, soft, ignore_flow, maximum_steps, out, out_cap, k < QLOG);
    if (r == AW_HANDOFF) {
      S.q_start = start_idx; S.q_goal = goal_idx; S.q_soft = soft ? 1 : 0; S.q_out = out; S.q_cap = out_cap;
      S.q_status = DV_HANDOFF;
      return -1;
    }
    if (k < QLOG && lane_id() == 0) { S.q_log[3 * k] = r; S.q_log[3 * k + 1] = (int)(S.expansions - e0); S.q_log[3 * k + 2] = (int)(S.relaxations - r0); }
    return r;
  }
  else if constexpr (MODE == DM_QUAD) {
    const int k = S.q_replay++;
    if (k < S.q_done) {   // finished in an earlier pass: its path already sits in `out`
      S.calls++; S.expansions += S.q_log[3 * k + 1]; S.relaxations += S.q_log[3 * k + 2];
      return S.q_log[3 * k];
    }
    // the quad searcher carries neither step limits nor contraflow (bypass searches are rare and small): such a vehicle is
    // handed to k_replan, as is one that searches more often than the log is long
    if (maximum_steps < d.N || ignore_flow || k >= QLOG) { S.q_status = DV_BAIL; return -1; }
    S.q_start = start_idx; S.q_goal = goal_idx; S.q_soft = soft ? 1 : 0; S.q_out = out; S.q_cap = out_cap;
    S.q_status = DV_SUSPEND;
    return -1;
  }
  else return -1;   // (one vehicle per lane never searches: decide_vehicle<DM_LANE> defers before it gets here)
}
// reach_strict_wave with its answer in the same log (an entry of its own: a re-run does not flood the component again)
__device__ __forceinline__ int reach_logged(const Dev& d, AScratch& S, int start, int goal) {
  if (S.q_log == nullptr) return reach_strict_wave(d, S, start, goal);
  const int k = S.q_replay++;
  if (k < S.q_done) return S.q_log[3 * k];
  const int r = reach_strict_wave(d, S, start, goal);
  if (k < QLOG && lane_id() == 0) { S.q_log[3 * k] = r; S.q_log[3 * k + 1] = 0; S.q_log[3 * k + 2] = 0; }
  return r;
}
// Phases 3 and 4, once a bypass of `bl` cells (S.BYP) ends on cell `merge_idx` of the path found (S.A[0..la)): the new path is
// the bypass and what follows that cell (built in S.T, then swapped in as S.P), the path as it was and the bypass are staged
// as aux paths kb + 1 and kb, in their buffers `pre` and `byp` (= ax_buf(S, kb + 1), ax_buf(S, kb): named by the caller, because
// ax_buf's selects in here cost the quads' policy four vector registers in the windowed test build).  false: the new path
// outgrows the buffers.
__device__ __forceinline__ bool splice_bypass(AScratch& S, VW& v, int kb, int32_t* pre, int32_t* byp, int bl, int la, int merge_idx, int& out_len) {
  int n = 0;
  for (int q = 0; q < bl; q++) S.T[n++] = S.BYP[q];
  if (n + (la - merge_idx - 1) > S.cap) return false;
  for (int q = merge_idx + 1; q < la; q++) S.T[n++] = S.A[q];
  for (int q = 0; q < la; q++) pre[q] = S.A[q];
  v.ax_staged[kb + 1] = true; v.ax_len[kb + 1] = la;
  for (int q = 0; q < bl; q++) byp[q] = S.BYP[q];
  v.ax_staged[kb] = true; v.ax_len[kb] = bl;
  swap_ptr(S.P, S.T);
  out_len = n;
  return true;
}
template <int MODE>
__device__ bool compute_path_internal_dev(const Dev& d, const TsParams& P, AScratch& S, VW& v, int& out_len) {
  // ---- phase 0: re-merge with the saved original path (219-277) ----
  for (int which = 0; which < 2; which++) {
    const int kb = which == 0 ? 0 : 2, kp = kb + 1;  // bypass slot, pre-path slot
    const bool active = which == 0 ? (v.f & VF_OVER) != 0 : (v.f & VF_DETOUR) != 0;
    if (!active || v.ax_len[kp] <= 0) continue;
    AxReader r;
    r.init(d, S, v, kp);
    int merge_idx = -1, b = -1;
    for (int q = 0; q < v.ax_len[kp]; q++) {
      int c = r.next();
      if (d.cell[c].occ == 0) { merge_idx = q; b = c; break; }
    }
    if (merge_idx < 0) continue;
    int bl = astar_any<MODE>(d, P, S, v.pos, b, false, true, P.max_contraflow_overtake_steps, S.BYP, MAXB);
    if (bl < 0) return false;
    if (bl > 0 && S.BYP[bl - 1] == b) {
      int n = 0;
      for (int q = 0; q < bl; q++) S.T[n++] = S.BYP[q];
      int rest = v.ax_len[kp] - (merge_idx + 1);
      if (n + rest > S.cap) return false;
      for (int q = 0; q < rest; q++) S.T[n++] = r.next();
      int32_t* dst = ax_buf(S, kb);
      for (int q = 0; q < bl; q++) dst[q] = S.BYP[q];
      v.ax_staged[kb] = true; v.ax_len[kb] = bl;
      swap_ptr(S.P, S.T);
      out_len = n;
      return true;
    }
  }
  // ---- phase 1: strict; phase 2: soft obstacles (280-306) ----
  const int sx_goal = v.target;
  int la;
  bool unreachable = false;
  if constexpr (MODE == DM_WAVE) unreachable = v.reach_known && reach_logged(d, S, v.pos, sx_goal) == 2;
  if (unreachable) {
    // the frontier BFS proved the target unreachable under the strict rules: the search would flood its whole
    // component and return [] (astar_numba.py:239).  Same result, without the flood.
    S.calls++;
    la = 0;
  } else {
    la = astar_any<MODE>(d, P, S, v.pos, sx_goal, false, false, 0x7FFFFFFF, S.A, S.cap);
    if (la < 0) return false;
  }
  if (la == 0) {
    la = astar_any<MODE>(d, P, S, v.pos, sx_goal, true, false, 0x7FFFFFFF, S.A, S.cap);
    if (la < 0) return false;
  }
  // ---- phase 3: contraflow overtake of a stranded / parked blocker (309-366) ----
  if (P.contraflow_overtake_active && la > 0) {
    int idx_stop = -1, idx_veh = -1;
    int look = min(P.vehicle_awareness_range, la);
    for (int q = 0; q < look; q++) {
      if (idx_stop < 0 && d.cell[S.A[q]].stop == 1) idx_stop = q;
      if (idx_veh < 0 && d.cell[S.A[q]].occ == 1) idx_veh = q;
      if (idx_stop >= 0 && idx_veh >= 0) break;
    }
    if (idx_veh == 0) {
      int bk = d.cell[S.A[0]].veh;
      if (bk >= 0 && (seen_stranded(d, bk, v.i) || seen_parked(d, bk, v.i))) {
        int bt = -1, idx_bp = -1;
        for (int q = 0; q < la; q++) if (d.cell[S.A[q]].occ == 0) { bt = S.A[q]; idx_bp = q; break; }
        if (bt >= 0) {
          int bl = astar_any<MODE>(d, P, S, v.pos, bt, false, true, P.max_contraflow_overtake_steps, S.BYP, MAXB);
          if (bl < 0) return false;
          if (bl > 1 && S.BYP[bl - 1] == bt) {
            // idx_bp = first index of bt in path = the index found above (first free cell)
            // pre_overtake_path = path, overtake_path = bypass
            if (!splice_bypass(S, v, 0, S.PO, S.OV, bl, la, idx_bp, out_len)) return false;
            v.f |= VF_OVER;
            v.d_overtaking++;
            v.over_dur = 0;
            return true;
          }
        }
      }
    }
  }
  // ---- phase 4: stuck detour (369-418) ----
  if (P.stuck_contraflow_enabled && la > 0) {
    int threshold = st_inter(d.cell[v.pos].stat) == 1 ? P.stuck_contraflow_threshold_intersection : P.stuck_contraflow_threshold;
    if (v.stuck_ticks >= threshold) {
      int bt = -1, merge_idx = -1;
      for (int q = 0; q < la; q++) if (d.cell[S.A[q]].occ == 0) { bt = S.A[q]; merge_idx = q; break; }
      if (bt >= 0) {
        int bl = astar_any<MODE>(d, P, S, v.pos, bt, true, true, P.max_contraflow_stuck_detour_steps, S.BYP, MAXB);
        if (bl < 0) return false;
        if (bl > 1 && S.BYP[bl - 1] == bt) {
          // pre_stuck_detour_path = path.copy(), stuck_detour_path = bypass
          if (!splice_bypass(S, v, 2, S.PD, S.DV, bl, la, merge_idx, out_len)) return false;
          v.d_detour++;
          v.f |= VF_DETOUR;
          v.det_dur = 0;
          return true;
        }
      }
    }
  }
  swap_ptr(S.P, S.A);
  out_len = la;
  return true;
}

// `pos not in aux path k`
__device__ bool ax_contains(const Dev& d, const AScratch* S, const VW& v, int k, int cell) {
  if (v.ax_len[k] <= 0) return false;
  if (!S) {  // no scratch: only pool-resident paths can exist
    int c = d.ax_start[k][v.vid];
    uint32_t off = d.ax_off[k][v.vid];
    for (int q = 0; q < v.ax_len[k]; q++) { c = step_cell(c, path_dir(d.pool, off, q), d.W); if (c == cell) return true; }
    return false;
  }
  AxReader r;
  r.init(d, *S, v, k);
  for (int q = 0; q < v.ax_len[k]; q++) if (r.next() == cell) return true;
  return false;
}

// device-side bump allocation in the path pool; returns false when the pool is exhausted
template <int MODE>
__device__ __forceinline__ bool pool_alloc(const Dev& d, int words, uint32_t& off) {
  unsigned long long o = 0;
  const bool one = MODE == DM_LANE || (MODE == DM_WAVE ? lane_id() == 0 : (lane_id() & 3) == 0);
  if (one) o = atomicAdd((unsigned long long*)&d.cnt->pool_used, (unsigned long long)words);
  if (MODE == DM_WAVE) o = ((unsigned long long)(unsigned)__shfl((int)(o >> 32), 0) << 32) | (unsigned)__shfl((int)(unsigned)o, 0);
  if (MODE == DM_QUAD) o = ((unsigned long long)(unsigned)quad_first((int)(o >> 32)) << 32) | (unsigned)quad_first((int)(unsigned)o);
  if (o + (unsigned long long)words > (unsigned long long)d.pool_cap_words) return false;
  off = (uint32_t)o;
  return true;
}
__device__ void encode_cells(const Dev& d, uint32_t off, int start_cell, const int32_t* cells, int len) {
  int prev = start_cell;
  uint32_t word = 0;
  for (int k = 0; k < len; k++) {
    int c = cells[k];
    int dir = dir_of_delta(c - prev, d.W);
    word |= (uint32_t)dir << ((k & PATH_STEP_MASK) * PATH_DIR_BITS);   // (path_put's place, in a register: path_words.h)
    if ((k & PATH_STEP_MASK) == PATH_STEP_MASK) { d.pool[off + (k >> PATH_STEP_SHIFT)] = word; word = 0; }
    prev = c;
  }
  if (len & PATH_STEP_MASK) d.pool[off + (len >> PATH_STEP_SHIFT)] = word;
}
// A plan into the pool, in one allocation: the new path (S.P[0..v.plen), if `path`) and the staged aux paths, from v.pos on;
// the vehicle's path and aux records then point at them.  Returns what was rewritten as Dev::chg counts it (bit 0 path,
// bits 1-4 aux paths), or CP_POOL_FULL with nothing written.
constexpr int CP_POOL_FULL = -1;
template <int MODE>
__device__ int commit_paths(const Dev& d, const AScratch& S, const VW& v, bool path) {
  int words = path ? path_words(v.plen) : 0;
  for (int k = 0; k < 4; k++) if (v.ax_staged[k]) words += path_words(v.ax_len[k]);
  uint32_t off = 0;
  if (words > 0 && !pool_alloc<MODE>(d, words, off)) return CP_POOL_FULL;
  int chg = 0;
  if (path) {
    encode_cells(d, off, v.pos, S.P, v.plen);
    d.path_off[v.vid] = off; d.path_len[v.vid] = v.plen; d.path_cur[v.vid] = 0;
    off += path_words(v.plen);
    chg |= 1;
  }
  for (int k = 0; k < 4; k++) {
    if (!v.ax_staged[k]) continue;
    encode_cells(d, off, v.pos, ax_buf(S, k), v.ax_len[k]);
    d.ax_start[k][v.vid] = v.pos; d.ax_off[k][v.vid] = off; d.ax_len[k][v.vid] = v.ax_len[k];
    off += path_words(v.ax_len[k]);
    chg |= 2 << k;
  }
  return chg;
}
// a direction string of nw words copied to the next free words of `dst` (the bump counter `used` hands them out); returns where it went
__device__ __forceinline__ unsigned long long move_words(uint32_t* dst, unsigned long long* used, const uint32_t* src, int nw) {
  const unsigned long long o = atomicAdd(used, (unsigned long long)nw);
  for (int q = 0; q < nw; q++) dst[o + q] = src[q];
  return o;
}

// step_decide for vehicle number i of active_vehicle_agents.  S == nullptr: run until a search is needed
// (returns DV_DEFER without side effects).  Otherwise completes, unless the tier overflows or the pool is full.
template <int MODE>
__device__ int decide_vehicle(const Dev& d, const TsParams& P, int i, AScratch* S) {
  const bool one = MODE == DM_LANE || (MODE == DM_WAVE ? lane_id() == 0 : (lane_id() & 3) == 0);   // the lane that issues this vehicle's atomics
  const int vid = d.active[i];
  if (vid < 0) return DV_DONE;
  VW v;
  v.vid = vid; v.i = i; v.pos = d.pos[vid]; v.target = d.target[vid];
  v.reach_known = S != nullptr && S->use_reach;
  v.f = d.flags[vid] & ~VF_EARLY;
  const uint8_t ev = d.ev[vid];
  v.base = d.base_speed[vid]; v.cur = d.cur_speed[vid];
  bool early = false;
  int stranded_left = d.stranded_left[vid];
  bool write_stranded = false;
  int dc_coll = 0, dc_malf = 0;
  if (ev == 1) {  // became stranded at its own decide point: state already written by k_apply_event
    v.base = 0; v.cur = 0; early = true;
  } else {
    if (ev != 2 && (v.f & (VF_COLL | VF_MALF))) {  // _tick_stranded (552-565)
      stranded_left -= 1;
      if (stranded_left <= 0) {
        if (v.f & VF_COLL) dc_coll--;
        if (v.f & VF_MALF) dc_malf--;
        v.f &= ~(VF_COLL | VF_MALF);
        stranded_left = 0;
      }
      write_stranded = true;
      if (v.f & (VF_COLL | VF_MALF)) { v.base = 0; v.cur = 0; early = true; }
    }
    if (!early && !P.malfunction_active) {  // `not ACTIVE or ...` (609): malfunction without a draw
      v.f = (v.f | VF_MALF) & ~VF_COLL;
      stranded_left = P.malfunction_duration; write_stranded = true;
      dc_malf++;
      v.base = 0; v.cur = 0; early = true;
    }
    if (!early && d.cell[v.pos].stop == 1) { v.base = 0; v.cur = 0; early = true; }
  }
  int max_steps = d.max_steps[vid];
  bool path_changed = false, reached_body = false, arrived = false;
  v.newpath = false;
  v.d_overtaking = 0; v.d_detour = 0;
  for (int k = 0; k < 4; k++) { v.ax_staged[k] = false; v.ax_len[k] = 0; }
  bool ax_none_set[2] = {false, false};
  if (!early) {
    if (v.base == 0) v.base = d.R[i];  // _choose_new_speed: rolled by the host scan
    int speed = v.base;
    if (P.rain_enabled && d.rain[v.pos] == 1) speed = max(1, speed - P.rain_speed_reduction);
    v.cur = speed;
    v.off = d.path_off[vid]; v.pcur = d.path_cur[vid]; v.plen = d.path_len[vid] - v.pcur;
    v.cooldown = d.cooldown[vid]; v.over_dur = d.over_dur[vid]; v.det_dur = d.det_dur[vid];
    v.stuck_ticks = d.stuck_ticks[vid];
    for (int k = 0; k < 4; k++) { v.ax_staged[k] = false; v.ax_len[k] = d.ax_len[k][vid]; }
    // _recompute_path_on_stuck (506-517): self.path = self._compute_path(use_cache=False)
    const int thresh = st_inter(d.cell[v.pos].stat) == 1 ? P.stuck_recompute_threshold_intersection : P.stuck_recompute_threshold;
    if (v.stuck_ticks >= thresh) {
      if (!S) return DV_DEFER;
      v.cooldown = P.pathfinding_cooldown;
      int len;
      if (!compute_path_internal_dev<MODE>(d, P, *S, v, len)) return MODE == DM_QUAD || (MODE == DM_WAVE && S->q_status == DV_HANDOFF) ? S->q_status : DV_OVERFLOW;
      v.newpath = true; v.plen = len; path_changed = true;
    }
    // _recompute_path_on_obstacle (454-504)
    if ((v.f & VF_OVER) && (v.ax_len[0] <= 0 || !ax_contains(d, S, v, 0, v.pos))) {
      v.ax_len[0] = -1; v.ax_staged[0] = false; ax_none_set[0] = true; v.f &= ~VF_OVER;
    }
    if ((v.f & VF_DETOUR) && (v.ax_len[2] <= 0 || !ax_contains(d, S, v, 2, v.pos))) {
      v.ax_len[2] = -1; v.ax_staged[2] = false; ax_none_set[1] = true; v.f &= ~VF_DETOUR;
    }
    int idx_stop, idx_veh, first_cell;
    scan_ahead_dev(d, P, S, v, idx_stop, idx_veh, first_cell);
    bool done_obst = false;
    if (v.f & VF_OVER) {
      v.over_dur += 1;
      if (v.over_dur <= P.contraflow_overtake_duration) done_obst = true;
    }
    if (!done_obst && (v.f & VF_DETOUR)) {
      v.det_dur += 1;
      if (v.det_dur <= P.contraflow_stuck_detour_duration) done_obst = true;
    }
    if (!done_obst && v.cooldown > 0) {
      if (idx_veh == 0) {
        int b = d.cell[first_cell].veh;
        if (b >= 0 && (seen_stranded(d, b, i) || seen_parked(d, b, i))) {
          // immediate pathfinding
        } else { v.cooldown -= 1; done_obst = true; }
      } else { v.cooldown -= 1; done_obst = true; }
    }
    if (!done_obst && (idx_stop >= 0 || idx_veh >= 0)) {
      if (!S) return DV_DEFER;
      // path = self._compute_path(use_cache=False); adopted only when non-empty (498-502).  The planner
      // never writes through S->P, it only swaps buffer pointers at the end, so a previous result of this
      // tick (stuck replan) survives an empty answer and is swapped back.
      v.cooldown = P.pathfinding_cooldown;
      const bool keep_new = v.newpath;
      int len;
      if (!compute_path_internal_dev<MODE>(d, P, *S, v, len)) return MODE == DM_QUAD || (MODE == DM_WAVE && S->q_status == DV_HANDOFF) ? S->q_status : DV_OVERFLOW;
      if (len > 0) {
        v.newpath = true; v.plen = len; path_changed = true;
        scan_ahead_dev(d, P, S, v, idx_stop, idx_veh, first_cell);
      } else if (keep_new) {
        swap_ptr(S->P, S->A);  // undo the final swap of the empty result
      }
    }
    // _determine_max_steps (719-731)
    int ms = min(v.cur, v.plen);
    bool blocked = false;
    if (idx_stop >= 0) ms = min(ms, idx_stop);
    if (idx_veh >= 0) { if (idx_veh == 0) blocked = true; ms = min(ms, idx_veh); }
    max_steps = ms;
    v.f = blocked ? (v.f | VF_BLOCKED) : (v.f & ~VF_BLOCKED);
    if (ms <= 0) {
      v.base = 0;
      if (v.pos == v.target) arrived = true;   // on_target_reached() inside step_decide (657-661)
      early = true;
    }
    reached_body = true;
  }
  if (ev == 2) { v.base = 0; v.cur = 0; }  // collision inflicted after this vehicle had decided
  // ---------------- commit (first the allocation that can fail, then everything else) ----------------
  if (reached_body && S) {
    const int chg = commit_paths<MODE>(d, *S, v, path_changed);
    if (chg == CP_POOL_FULL) return DV_POOL_FULL;
    if (chg) d.chg[vid] = (uint8_t)chg;
  }
  if (reached_body) {
    if (ax_none_set[0] && !v.ax_staged[0]) d.ax_len[0][vid] = -1;
    if (ax_none_set[1] && !v.ax_staged[2]) d.ax_len[2][vid] = -1;
    d.cooldown[vid] = v.cooldown; d.over_dur[vid] = v.over_dur; d.det_dur[vid] = v.det_dur;
    if (one && v.d_overtaking) atomicAdd((unsigned long long*)&d.cnt->overtaking, (unsigned long long)v.d_overtaking);
    if (one && v.d_detour) atomicAdd((unsigned long long*)&d.cnt->in_stuck_detour, (unsigned long long)v.d_detour);
  }
  if (write_stranded) d.stranded_left[vid] = stranded_left;
  if (one && dc_coll) atomicAdd((unsigned long long*)&d.cnt->collisions, (unsigned long long)(long long)dc_coll);
  if (one && dc_malf) atomicAdd((unsigned long long*)&d.cnt->malfunctions, (unsigned long long)(long long)dc_malf);
  d.max_steps[vid] = (int8_t)max_steps;
  d.base_speed[vid] = (int8_t)v.base;
  d.cur_speed[vid] = (int8_t)v.cur;
  d.flags[vid] = early ? (v.f | VF_EARLY) : v.f;
  if (arrived && one) {
    if (!(v.f & VF_KEEP)) {   // a trip that ends where it starts: _despawn inside step_decide.  The host ends the stretch of
      // the decide order at such a vehicle and takes it off the maps once everybody before it is through (tick())
      if (d.dec_expect == i + 1) atomicExch(&d.cnt->dec_arrived, i + 1);
      else atomicExch(&d.cnt->error, TS_E_DEVICE);
    }
    else if (v.f & VF_TOBLOCK) svc_record(d, i, vid, AR_DECIDE);        // ServiceVehicleAgent._start_service
    else {   // base on_target_reached of a vehicle that stays: trip statistics once more, then _park()
      if (P.enable_traffic && d.pop[vid] == TS_POP_THROUGH) {
        atomicAdd(&d.cnt->dur_through, d.elapsed - d.depart[vid]);
        atomicAdd((unsigned long long*)&d.cnt->dist_through, (unsigned long long)d.steps[vid]);
        atomicAdd((unsigned long long*)&d.cnt->completed_through, 1ULL);
      } else if (P.enable_traffic && d.pop[vid] == TS_POP_INTERNAL) {
        atomicAdd(&d.cnt->dur_internal, d.elapsed - d.depart[vid]);
        atomicAdd((unsigned long long*)&d.cnt->dist_internal, (unsigned long long)d.steps[vid]);
        atomicAdd((unsigned long long*)&d.cnt->completed_internal, 1ULL);
      }
      if (!(v.f & VF_PARKED)) svc_record(d, i, vid, AR_DECIDE);
    }
  }
  return DV_DONE;
}

// VehicleAgent.__init__ -> self.path = self._compute_path() on a cache miss (vehicle_base.py:80-81, 143-167):
// the phase 0-4 planner for a freshly placed vehicle.  status: path length, or -1 overflow / -2 pool full.
TS_REPLAN_OCC __global__ void __launch_bounds__(64) k_spawn_plan(Dev d, TsParams P, ASlots sl, int vid, int32_t* status) {
  if (blockIdx.x) return;
  const bool one = threadIdx.x == 0;
  AScratch S;
  scratch_bind(sl, 0, S);
  VW v;
  v.vid = vid; v.i = LAST_IDX; v.pos = d.pos[vid]; v.target = d.target[vid];
  v.f = d.flags[vid]; v.base = 0; v.cur = 0; v.cooldown = P.pathfinding_cooldown;
  v.over_dur = d.over_dur[vid]; v.det_dur = d.det_dur[vid]; v.stuck_ticks = d.stuck_ticks[vid];
  v.newpath = false; v.plen = 0; v.pcur = 0; v.off = 0; v.d_overtaking = 0; v.d_detour = 0;
  v.reach_known = false;
  for (int k = 0; k < 4; k++) { v.ax_staged[k] = false; v.ax_len[k] = d.ax_len[k][vid]; }
  int len;
  bool ok = compute_path_internal_dev<DM_WAVE>(d, P, S, v, len);
  if (one) sl.slot_epoch[0] = S.epoch;
  if (!ok) { if (one) *status = -1; return; }
  v.plen = len;
  if (commit_paths<DM_WAVE>(d, S, v, true) == CP_POOL_FULL) { if (one) *status = -2; return; }
  if (one) searcher_account(d, S.calls, S.expansions, S.relaxations);
  d.flags[vid] = v.f; d.over_dur[vid] = v.over_dur; d.det_dur[vid] = v.det_dur;
  if (one && v.d_overtaking) atomicAdd((unsigned long long*)&d.cnt->overtaking, (unsigned long long)v.d_overtaking);
  if (one && v.d_detour) atomicAdd((unsigned long long*)&d.cnt->in_stuck_detour, (unsigned long long)v.d_detour);
  if (one) *status = len;
}

// path-pool garbage collection: every live vehicle copies the words it still needs (path_words.h: path_live) into a fresh pool
__global__ void k_pool_gc(Dev d, int n_active, uint32_t* new_pool, unsigned long long* new_used) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_active) return;
  int vid = d.active[i];
  if (vid < 0) return;
  {
    const PathLive l = path_live(d.path_cur[vid], d.path_len[vid]);
    d.path_off[vid] = l.words > 0 ? (uint32_t)move_words(new_pool, new_used, d.pool + d.path_off[vid] + l.w0, l.words) : 0u;
    d.path_cur[vid] = l.cur; d.path_len[vid] = l.len;
  }
  for (int k = 0; k < 4; k++) {
    const int words = aux_words(d.ax_len[k][vid]);
    if (words > 0) d.ax_off[k][vid] = (uint32_t)move_words(new_pool, new_used, d.pool + d.ax_off[k][vid], words);
  }
}

}  // namespace
