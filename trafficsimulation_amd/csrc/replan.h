// replan.h - the replanning work queue (RQueue: k_decide_main files the vehicles whose step_decide needs a search, k_replan and
// k_replan_quad serve them) and the records the ranks of a multi-GPU run exchange about what they planned.
#pragma once
#include "decide.h"

namespace {

struct RLists { int32_t* l[4]; };       // the replanning queue's class lists (RQueue)
// expected cost of a vehicle's replan (cost_bits, dev.h): what its last one took, or what a search over this distance is likely to
__device__ __forceinline__ int replan_cost_bits(const Dev& d, int vid) {
  int x0, y0, x1, y1;
  cell_xy(d, d.pos[vid], x0, y0); cell_xy(d, d.target[vid], x1, y1);
  return max((int)d.tier_hint[vid], cost_bits_of_distance(abs(x0 - x1) + abs(y0 - y1)));
}

// sort key of a replanning entry (run_replans): expected cost, largest first (bit length of the expansions, see cost_bits),
// then the Morton index of the 32 x 32-cell block its vehicle stands in
constexpr int REPLAN_KEY_BITS = 21;
__device__ __forceinline__ uint32_t replan_key(const Dev& d, int i) {
  const int vid = d.active[i];
  int x = 0, y = 0, bits = 0;
  if (vid >= 0) { cell_xy(d, d.pos[vid], x, y); bits = min(replan_cost_bits(d, vid), 31); }
  // (only the long searches are ordered by cost - 65 536 expansions and more, bit by bit; the bulk stays in plain spatial order)
  return ((uint32_t)(31 - max(bits, 16)) << 16) | morton_block_key(x, y);
}
// The same with the entry itself (its decide-order index) below the key: a total order, the same on every rank of a sharded
// run whatever order k_decide_main's atomics left the list in, so that ranks can split the queue by POSITION (entry j of
// the sorted queue belongs to rank j % world: every rank gets every world-th search of every cost class and every
// neighbourhood - the longest searches are dealt out one by one instead of falling where index % world puts them).
__global__ void k_replan_keys64(Dev d, const int32_t* list, int n, unsigned long long* keys) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  keys[j] = ((unsigned long long)replan_key(d, list[j]) << 32) | (unsigned long long)(uint32_t)list[j];
}
__global__ void k_replan_unkey64(const unsigned long long* keys, int n, int32_t* list) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) list[j] = (int32_t)(uint32_t)keys[j];
}
__global__ void k_replan_keys(Dev d, const int32_t* list, int n, uint32_t* keys) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  keys[j] = replan_key(d, list[j]);
}

// ---- the replanning work queue ---------------------------------------------------------------------------------------
// Vehicles whose step_decide needs a search wait in four class lists, by expected cost (k_decide_main files them, run_replans
// sorts each).  The queue is classes 3, 2, 1, 0 in turn: a tick's replanning time is bounded below by its longest search, so
// those start first and the short ones fill in behind.  Its counters are DevCnt::replan and the four words after it.  k_replan
// (one wave per search) and k_replan_quad (astar_quad.h, sixteen per wave) serve it, each the classes of its `class_mask` with
// a cursor of its own; pool-full entries go to retry_list for the host to run again.
// Ownership by position (`world` > 1, the replicated-state multi-GPU mode): the queue is in the same total order on every
// rank (run_replans sorts by (key, index)) and the entry at position pos of the WHOLE queue - every class counted, whichever
// kernel serves it - is rank pos % world's.  What a rank plans goes to owned_list for ts_replan_export / ts_replan_import.
// Hand-backs: a vehicle the quads cannot carry goes to handback_list - counted in handback_n, then stored (-1 = not yet
// written).  k_replan's waves beside the quads (fb_waves = the quads' grid, 0 = none) serve that list once their own classes
// are done: a ticket from handback_claimed, never beyond handback_n, so what is left when they stop is a suffix the host can
// queue again; hand-backs of this rank's quads are this rank's.  They give up when all fb_waves quad waves have counted
// themselves out in quad_waves_done and nothing more was produced, or when no counter has moved for about three seconds
// (the kernels were not run side by side - a profiler or debugger serialising launches; k_replan_quad is then yet to run).
// The host's part, one kernel argument.  fb_waves: k_replan only, the quads' grid (0: no quads beside it).
struct RQueueArgs { RLists lists; int class_mask; int32_t *retry_list, *handback_list; int rank, world; int32_t* owned_list /* nullptr unless sharded */; int fb_waves; };
struct RQueue {         // what a turn at the queue reads: the host's part + what rqueue_open fills on the device
  RLists lists;
  int n[4], pos0[4];    // class list lengths (0: not served by this launch); position of each class' first entry in the whole queue
  int32_t *retry_list, *handback_list, *owned_list; int rank, world;
};
// k_replan's: + the quads beside it.  Apart from RQueue for the compiler's sake only: the queue goes to the turn functions through the stack, and fb_waves inside RQueue (or as a parameter) changes k_replan_quad's (k_replan's) scratch size
struct RQueueFb : RQueue { int fb_waves; };
__device__ __forceinline__ RQueue rqueue_open(const Dev& d, const RQueueArgs& a) {
  RQueue q; const int* cn = d.cnt->replan.class_n;
  q.lists = a.lists;
  for (int c = 0; c < 4; c++) q.n[c] = ((a.class_mask >> c) & 1) ? cn[c] : 0;
  q.pos0[3] = 0; q.pos0[2] = cn[3]; q.pos0[1] = cn[3] + cn[2]; q.pos0[0] = cn[3] + cn[2] + cn[1];
  q.retry_list = a.retry_list; q.handback_list = a.handback_list; q.owned_list = a.owned_list; q.rank = a.rank; q.world = a.world;
  return q;
}
// cursor value j (below the launch's total) -> the entry i and its position in the whole queue; false: another rank's
__device__ __forceinline__ bool rqueue_entry(const RQueue& q, int j, int& i, int& pos) {
  const int n3 = q.n[3], n2 = q.n[2], n1 = q.n[1];
  if (j < n3) { i = q.lists.l[3][j]; pos = q.pos0[3] + j; }
  else if (j < n3 + n2) { i = q.lists.l[2][j - n3]; pos = q.pos0[2] + j - n3; }
  else if (j < n3 + n2 + n1) { i = q.lists.l[1][j - n3 - n2]; pos = q.pos0[1] + j - n3 - n2; }
  else { i = q.lists.l[0][j - n3 - n2 - n1]; pos = q.pos0[0] + j - n3 - n2 - n1; }
  return q.world <= 1 || (pos % q.world) == q.rank;
}

// every live vehicle: the part of step_decide that needs no search; the others go to the replan list
__global__ void k_decide_main(Dev d, TsParams P, int lo, int n_active, RLists lists) {
  int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_active) return;
  if (d.cnt->rng_event != 0xFFFFFFFFu) return;  // a malfunction / sideswipe fired: the host re-runs this after the fix-up
  if (decide_vehicle<DM_LANE>(d, P, i, nullptr) == DV_DEFER) {
    // work-queue class (largest first): what the vehicle's last replan cost, or what a search over this distance is
    // likely to cost
    const int h = cost_class_of_bits(replan_cost_bits(d, d.active[i]));
    lists.l[h][atomicAdd(&d.cnt->replan.class_n[h], 1)] = i;
  }
}

// One turn of a searcher wave at the replanning work queue: take the next entry, run the vehicle's step_decide with
// all 64 lanes, account for it.  Returns 0 once the queue is empty.  Kept out of line on purpose: inlined into
// k_replan's loop, hipcc 7.2 threaded the lane-0-only parts (queue pop, accounting) of consecutive turns together and
// let lane 0 run the loop on a path of its own, apart from the other 63 lanes - wrong for code whose lanes cooperate
// through readlane / ballot.  A call boundary is a point where the wave is whole again.
#ifdef TS_TRACE_REPLAN
// profiling builds (profiles/replan_trace.py): per queue entry (start, end: low words of the 100 MHz clock; expansions;
// predicted cost bits | searcher slot << 8)
__device__ int4* g_rtrace = nullptr;
__device__ int g_rtrace_cap = 0;
#endif
// A vehicle's step_decide has ended with r (the lane that issues its atomics calls this, with what its searches came to): a
// committed result is accounted for and the entry goes to owned_list, one that found the pool full goes to retry_list
__device__ __forceinline__ void replan_settle(const Dev& d, const RQueue& q, int i, int r, long long calls, long long exp, long long relax) {
  if (r == DV_DONE) {  // work of attempts that are re-run after pool growth is not counted twice
    const int vid = d.active[i];
    if (calls > 0) d.tier_hint[vid] = (uint8_t)cost_bits(exp);
    searcher_account(d, calls, exp, relax);
    if (q.owned_list) q.owned_list[atomicAdd(&d.cnt->replan.owned_n, 1)] = i;
  } else if (r == DV_POOL_FULL) q.retry_list[atomicAdd(&d.cnt->replan.retry_n, 1)] = i;
}
// The host tail.  A plain pass of run_replans can carry a tail control block (RTail: AScratch::t_ctl
// and the slot's log): a wave that finds the queue empty counts itself in TailCtl::idle, and a search that sees all but t_max waves
// of the launch idle (astar_loop's tail rule) is abandoned - decide_vehicle returns DV_HANDOFF without a commit, the wave files
// the entry, its slot and the search's arguments in the list behind TailCtl and ends, leaving the slot as it is: the paths of the
// searches this step_decide finished before are in its buffers, their results in its log.  Once the pass has drained, the host
// runs the listed searches on its own threads (astar_host.h), puts each path where the search would have put it and its result
// in the log, and k_replan_tail runs those step_decides again from the top on the same slots, replaying the log.  No kernel
// waits for the host or reads what the host writes while it runs.
struct RTail { TailCtl* ctl; int32_t* log; int t_max, floor, force, pad_; };   // ctl == nullptr: off; log: SLOG_INTS ints per searcher slot
__device__ __forceinline__ void tail_bind(const RTail& t, int slot, int grid, AScratch& S) {
  if (!t.ctl) return;
  S.q_log = t.log + (size_t)slot * SLOG_INTS;
  S.t_ctl = t.ctl;
  // (TS_TAIL_FORCE: every search the rule applies to gives up when it has made `force` expansions, whatever the other waves do)
  S.t_thr = t.force > 0 ? (int)0x80000000 : grid - t.t_max;
  S.t_floor = t.force > 0 ? t.force : t.floor;
  S.t_first = t.force > 0 ? t.force : TAIL_PERIOD;
}
// step_decide of queue entry i on this wave's slot, and what follows from its result; false: the wave ends here (a hand-off)
__device__ __forceinline__ bool replan_entry(const Dev& d, const TsParams& P, AScratch* S, const RQueue& q, int i, int done) {
  const long long c0 = S->calls, e0 = S->expansions, r0 = S->relaxations;
  S->q_status = 0; S->q_replay = 0; S->q_done = done;
  if (S->q_log) {
    // the policy swaps S->A / S->P / S->T as it goes, and a wave keeps them from entry to entry: with a log every step_decide starts
    // from the slot's own assignment, so that the re-run finds each replayed path in the buffer its search wrote
    int32_t* const c = S->BYP - (size_t)5 * S->cap;
    S->A = c; S->P = c + S->cap; S->T = c + 2 * (size_t)S->cap;
  }
  const int r = uni(decide_vehicle<DM_WAVE>(d, P, i, S));
  if (threadIdx.x == 0) {
    if (r == DV_HANDOFF) {
      TailCtl* const t = S->t_ctl;
      const int k = atomicAdd(&t->n, 1);     // (at most one per wave: the list has a place for every wave of the launch)
      if (k < t->cap)
        ((TailEnt*)(t + 1))[k] = TailEnt{i, (int)blockIdx.x, S->q_replay - 1, S->q_start, S->q_goal, S->q_soft,
                                         (int)(S->q_out - (S->BYP - (size_t)5 * S->cap)), S->q_cap};   // (BYP: the one cell buffer the policy never swaps)
    }
    replan_settle(d, q, i, r, S->calls - c0, S->expansions - e0, S->relaxations - r0);
    if (r == DV_OVERFLOW) atomicExch(&d.cnt->error, TS_E_CAPACITY);
  }
  return r != DV_HANDOFF;
}
__device__ __attribute__((noinline)) int replan_turn(const Dev& d, const TsParams& P, AScratch* S, const RQueueFb& q) {
  const int n3 = uni(q.n[3]), n2 = uni(q.n[2]), n1 = uni(q.n[1]), n0 = uni(q.n[0]);
  const int j = wave_pop(&d.cnt->replan.cursor);
  int i, pos = j;
  bool mine = true;
  if (j >= n3 + n2 + n1 + n0) {
    if (q.fb_waves == 0) {
      if (S->t_ctl && threadIdx.x == 0) atomicAdd(&S->t_ctl->idle, 1);
      return 0;
    }
    // this launch's own lists are done: serve the hand-back list (the protocol and its give-up rule: see RQueue)
    if (threadIdx.x == 0) {
      int job = -1;
      long long t_last = wall_clock64();
      int seen = -1;
      for (;;) {
        const int produced = __hip_atomic_load(&d.cnt->handback_n, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        int claimed = __hip_atomic_load(&d.cnt->handback_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (claimed < produced) {
          if (__hip_atomic_compare_exchange_strong(&d.cnt->handback_claimed, &claimed, claimed + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            // (the producer stores the entry right after counting it: a running wave, a few hundred cycles at most)
            do job = __hip_atomic_load(&q.handback_list[claimed], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); while (job < 0);
            break;
          }
          continue;
        }
        const int done = __hip_atomic_load(&d.cnt->quad_waves_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (done >= q.fb_waves) {
          if (__hip_atomic_load(&d.cnt->handback_n, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == produced) break;   // nothing more can come
          continue;
        }
        const int mark = produced + done + __hip_atomic_load(&d.cnt->quad_cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long now = wall_clock64();
        if (mark != seen) { seen = mark; t_last = now; }
        else if (now - t_last > 300000000ll) break;          // 3 s of the 100 MHz clock
        __builtin_amdgcn_s_sleep(64);
      }
      g_job = job;
    }
    __syncthreads();
    i = uni(g_job);
    __syncthreads();
    if (i < 0) return 0;
  }
  else mine = rqueue_entry(q, j, i, pos);
  i = uni(i);
  if (!mine) return 1;
  // the most expensive classes are a tick's critical path (its longest search bounds it): their waves take the issue slots
  // of their SIMD first, the five waves beside them fill in behind (`s_setprio`; TS_NO_PRIO: a build without it)
#ifndef TS_NO_PRIO
  if (j < n3) __builtin_amdgcn_s_setprio(3);
  else if (j < n3 + n2) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(0);
#endif
#ifdef TS_TRACE_REPLAN
  const long long tr0 = wall_clock64(), tr_e0 = S->expansions;
  const int tr_bits = replan_cost_bits(d, max(d.active[i], 0));
#endif
  const bool go_on = replan_entry(d, P, S, q, i, 0);
#ifdef TS_TRACE_REPLAN
  if (threadIdx.x == 0 && g_rtrace && j < g_rtrace_cap && j < n3 + n2 + n1 + n0)
    g_rtrace[j] = make_int4((int)(unsigned)tr0, (int)(unsigned)wall_clock64(), (int)(S->expansions - tr_e0), tr_bits | ((int)blockIdx.x << 8));
#endif
  return go_on ? 1 : 0;
}

// Replanning vehicles, one wave per searcher slot: every wave takes the next entry of the queue (RQueue) until it is empty;
// all 64 lanes run the vehicle's step_decide together and share the work inside the searches.
TS_REPLAN_OCC __global__ void __launch_bounds__(64) k_replan(Dev d, TsParams P, ASlots sl, RQueueArgs qa, RTail tl) {
  AScratch S;
  scratch_bind(sl, blockIdx.x, S);
  tail_bind(tl, blockIdx.x, gridDim.x, S);
  const RQueueFb q = {rqueue_open(d, qa), qa.fb_waves};
  while (uni(replan_turn(d, P, &S, q))) {}
  if (threadIdx.x == 0) sl.slot_epoch[blockIdx.x] = S.epoch;
}
// The step_decides whose search the host finished (tl.ctl's list, n entries; see RTail), one per wave, each on the slot it was
// abandoned on: re-run from the top with the log replayed as far as the host's search, the tail rule off.
__device__ __attribute__((noinline)) void replan_rerun(const Dev& d, const TsParams& P, AScratch* S, const RQueue& q, int i, int done) {
  replan_entry(d, P, S, q, i, done);
}
TS_REPLAN_OCC __global__ void __launch_bounds__(64) k_replan_tail(Dev d, TsParams P, ASlots sl, RQueueArgs qa, RTail tl, int n) {
  if ((int)blockIdx.x >= n) return;
  const TailEnt t = ((const TailEnt*)(tl.ctl + 1))[blockIdx.x];
  AScratch S;
  scratch_bind(sl, t.slot, S);
  S.q_log = tl.log + (size_t)t.slot * SLOG_INTS;
  const RQueue q = rqueue_open(d, qa);
  replan_rerun(d, P, &S, q, t.i, t.ord + 1);
  if (threadIdx.x == 0) sl.slot_epoch[t.slot] = S.epoch;
}
// What a pass left unserved because its waves ended on hand-offs (TS_TAIL_FORCE, or fewer waves than t_max): the entries at cursor
// values [from, total) that are this rank's, appended to `out` (the order of the queue does not touch any result)
__global__ void k_tail_unserved(Dev d, RQueueArgs qa, int from, int total, int32_t* out, int* out_n) {
  const int j = from + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  const RQueue q = rqueue_open(d, qa);
  int i, pos;
  if (rqueue_entry(q, j, i, pos)) out[atomicAdd(out_n, 1)] = i;
}
// searches the host ran for a caller of its own (ts_astar under TS_ASTAR_HOST), into the model's counters
__global__ void k_searcher_account(Dev d, long long calls, long long exp, long long relax) { searcher_account(d, calls, exp, relax); }

// ---- replicated-state multi-GPU mode (ts_set_replan_sharding) ------------------------------------------------------
// What step_decide changed about a vehicle this rank planned, for the ranks that did not: one fixed record plus the
// 2-bit direction words of whatever paths the replan rewrote.
struct ReplanRec {
  int32_t i, vid, flags, base, cur, max_steps, cooldown, over_dur, det_dur, stranded_left, hint;
  int32_t path_len, path_woff;          // path_woff < 0: the path was left as it is
  int32_t ax_len[4], ax_start[4], ax_woff[4];
  int32_t pad_[3];
};
static_assert(sizeof(ReplanRec) == 112, "ReplanRec is exchanged as 28 ints");
// `count_only`: add up the words the export will need and touch nothing else (the host sizes the word buffer with it: the
// pool's growth over the phase is no bound once a garbage collection ran inside it).
__global__ void k_replan_export(Dev d, const int32_t* owned, int n, ReplanRec* recs, uint32_t* words, unsigned long long* words_n,
                                int count_only) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = owned[t];
  const int vid = d.active[i];
  if (count_only) {
    if (vid < 0) return;
    const uint8_t chg = d.chg[vid];
    // (the live words of what was rewritten, path_words.h: a path just committed has its cursor at 0)
    unsigned long long nw = (chg & 1) ? (unsigned long long)path_live(0, d.path_len[vid]).words : 0ull;
    for (int k = 0; k < 4; k++) if ((chg >> (1 + k)) & 1) nw += (unsigned long long)aux_words(d.ax_len[k][vid]);
    if (nw) atomicAdd(words_n, nw);
    return;
  }
  ReplanRec r;
  r.i = i; r.vid = vid;
  r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
  if (vid < 0) { recs[t] = r; return; }
  r.flags = d.flags[vid]; r.base = d.base_speed[vid]; r.cur = d.cur_speed[vid]; r.max_steps = d.max_steps[vid];
  r.cooldown = d.cooldown[vid]; r.over_dur = d.over_dur[vid]; r.det_dur = d.det_dur[vid];
  r.stranded_left = d.stranded_left[vid]; r.hint = d.tier_hint[vid];
  const uint8_t chg = d.chg[vid];
  d.chg[vid] = 0;
  r.path_len = d.path_len[vid]; r.path_woff = -1;
  if (chg & 1) r.path_woff = (int32_t)move_words(words, words_n, d.pool + d.path_off[vid], path_live(0, r.path_len).words);
  for (int k = 0; k < 4; k++) {
    r.ax_len[k] = d.ax_len[k][vid]; r.ax_start[k] = d.ax_start[k][vid]; r.ax_woff[k] = -1;
    if ((chg >> (1 + k)) & 1) r.ax_woff[k] = (int32_t)move_words(words, words_n, d.pool + d.ax_off[k][vid], aux_words(r.ax_len[k]));
  }
  recs[t] = r;
}
// the same in the other direction: records of vehicles another rank planned (pool capacity ensured by the host)
__global__ void k_replan_import(Dev d, const ReplanRec* __restrict__ recs, int n, const uint32_t* __restrict__ words) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const ReplanRec r = recs[t];
  const int vid = r.vid;
  if (vid < 0) return;
  d.flags[vid] = (uint16_t)r.flags; d.base_speed[vid] = (int8_t)r.base; d.cur_speed[vid] = (int8_t)r.cur;
  d.max_steps[vid] = (int8_t)r.max_steps; d.cooldown[vid] = r.cooldown; d.over_dur[vid] = r.over_dur; d.det_dur[vid] = r.det_dur;
  d.stranded_left[vid] = r.stranded_left; d.tier_hint[vid] = (uint8_t)r.hint;
  if (r.path_woff >= 0) {
    d.path_off[vid] = (uint32_t)move_words(d.pool, &d.cnt->pool_used, words + r.path_woff, path_live(0, r.path_len).words);
    d.path_len[vid] = r.path_len; d.path_cur[vid] = 0;
  }
  for (int k = 0; k < 4; k++) {
    d.ax_len[k][vid] = r.ax_len[k];
    if (r.ax_woff[k] >= 0) {
      d.ax_start[k][vid] = r.ax_start[k];
      d.ax_off[k][vid] = (uint32_t)move_words(d.pool, &d.cnt->pool_used, words + r.ax_woff[k], aux_words(r.ax_len[k]));
    }
  }
}

}  // namespace
