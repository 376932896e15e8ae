// astar_batch.h - the kernels behind ts_astar_batch (include/trafficsim_astar_batch.h): many A* queries on the current maps in
// one launch.  k_astar_batch is k_replan's loop with a query in place of a vehicle: one wavefront per searcher slot takes
// queries off a device-side cursor and runs astar_wave (astar.h) on each.  Path lengths are only known after a search and the
// waves finish in no fixed order, so a wave first copies its path into a bump-allocated staging arena and records where;
// a scan of the lengths then gives the CSR offsets and k_batch_gather writes the (x, y) pairs in query order.  Nothing of
// the result depends on the order of service.  The host side is astar_batch_api.h.
#pragma once
#include "astar.h"   // (the order helpers - cost classes, morton_block_key - are dev.h's: no policy, no replanning queue here)

namespace {

// Dev-side bookkeeping of one launch
struct BatchCtl {
  int cursor;       // queue position the next free wave takes
  int n_retry;      // queries whose path found the staging arena full (BatchQ::retry)
  int first_bad;    // lowest query index whose search outgrew its heap or path buffer (INT_MAX: none)
  int pad_;
  unsigned long long stage_used;   // cells handed out from the staging arena (may run past its capacity: the host sizes the next one by it)
};
enum { BQ_OVERFLOW = -1, BQ_NOFIT = -2 };   // BatchQ::len besides a path length >= 0
struct BatchQ {
  const int32_t* q;        // n x 7: sx, sy, gx, gy, soft, ignore_flow, maximum_steps
  const int32_t* order;    // n_run query indices in the order of service
  int n_run;
  int32_t* len;            // per query: path length / BQ_*
  unsigned long long* soff;   // per query: its path's first cell in `stage`
  int32_t* stage;
  unsigned long long stage_cap;
  int32_t* retry;
  BatchCtl* ctl;
};

__shared__ unsigned long long g_boff;   // k_astar_batch: the staging offset lane 0 drew

// Order of service, longest first by the only cost hint a bare query has - the Manhattan distance of its endpoints, in the
// classes cost_bits_of_distance gives a vehicle without history - and inside a class in space (Morton index of the 32 x 32-cell
// block of the start, as run_replans orders vehicles): searches that run side by side read the same part of the snapshot.
constexpr int BATCH_KEY_BITS = 18;
__global__ void k_batch_keys(const int32_t* __restrict__ q, int n, uint32_t* __restrict__ keys, int32_t* __restrict__ ident) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t* a = q + (size_t)i * 7;
  const int cls = cost_class_of_bits(cost_bits_of_distance(abs(a[0] - a[2]) + abs(a[1] - a[3])));
  keys[i] = ((uint32_t)(3 - cls) << 16) | morton_block_key(a[0], a[1]);
  ident[i] = i;
}

// short queues are served as they come
__global__ void k_batch_iota(int32_t* __restrict__ order, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) order[i] = i;
}

// One turn of a searcher wave at the query queue.  Returns 0 once the queue is empty.  Out of line for the reason replan_turn
// is: inlined into the kernel's loop, the lane-0-only parts of consecutive turns (queue pop, bookkeeping) are threaded together
// and lane 0 leaves the other 63 lanes; a call boundary is a point where the wave is whole again.
__device__ __attribute__((noinline)) int batch_turn(const Dev& d, const TsParams& P, AScratch* S, const BatchQ& q) {
  const int j = wave_pop(&q.ctl->cursor);
  if (j >= q.n_run) return 0;
  const int qi = uni(q.order[j]);
  const int32_t* a = q.q + (size_t)qi * 7;
  const int sx = uni(a[0]), sy = uni(a[1]), gx = uni(a[2]), gy = uni(a[3]);
  const int soft = uni(a[4]), ign = uni(a[5]), max_steps = uni(a[6]);
  const long long c0 = S->calls, e0 = S->expansions, r0 = S->relaxations;
  const int len = uni(astar_wave(d, P, *S, sy * d.W + sx, gy * d.W + gx, soft != 0, ign != 0, max_steps, S->A, S->cap));
  if (len < 0) {   // heap or path buffer outgrown: the call fails as ts_astar does; this search is not counted (the others that finished are)
    if (threadIdx.x == 0) { q.len[qi] = BQ_OVERFLOW; atomicMin(&q.ctl->first_bad, qi); }
    return 1;
  }
  unsigned long long so = 0;
  if (len > 0) {
    if (threadIdx.x == 0) g_boff = atomicAdd(&q.ctl->stage_used, (unsigned long long)len);
    __syncthreads();
    so = uni64(g_boff);
    __syncthreads();
    if (so + (unsigned long long)len > q.stage_cap) {
      // the arena is full: the host grows it and queues this query again (its search is counted then, not now)
      if (threadIdx.x == 0) { q.len[qi] = BQ_NOFIT; q.retry[atomicAdd(&q.ctl->n_retry, 1)] = qi; }
      return 1;
    }
    int32_t* dst = q.stage + so;
    for (int k = lane_id(); k < len; k += 64) dst[k] = S->A[k];
  }
  if (threadIdx.x == 0) {
    q.soff[qi] = so; q.len[qi] = len;
    searcher_account(d, S->calls - c0, S->expansions - e0, S->relaxations - r0);
  }
  return 1;
}

// One wave per searcher slot in use (the grid is min(queries, usable slots)); every wave binds its slot once and serves the
// queue until it is empty, then hands the slot's epoch back for the slot's next user.
TS_REPLAN_OCC __global__ void __launch_bounds__(64) k_astar_batch(Dev d, TsParams P, ASlots sl, BatchQ q) {
  AScratch S;
  scratch_bind(sl, blockIdx.x, S);
  while (uni(batch_turn(d, P, &S, q))) {}
  if (threadIdx.x == 0) sl.slot_epoch[blockIdx.x] = S.epoch;
}

// lengths as the scan's input: len64[i] = cells of query i, len64[n] = 0 (its exclusive sum is the total)
__global__ void k_batch_lens(const int32_t* __restrict__ len, int n, long long* __restrict__ len64) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) len64[i] = i < n ? (long long)max(len[i], 0) : 0ll;
}

// staging arena -> xy in query order: one wave per query, consecutive lanes write consecutive (x, y) pairs
__global__ void k_batch_gather(Dev d, int n, const int32_t* __restrict__ len, const unsigned long long* __restrict__ soff,
                               const int32_t* __restrict__ stage, const long long* __restrict__ off, int32_t* __restrict__ xy) {
  const int qi = (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 6);
  if (qi >= n) return;
  const int l = len[qi];
  if (l <= 0) return;
  const int32_t* src = stage + soff[qi];
  int2* dst = reinterpret_cast<int2*>(xy) + off[qi];
  for (int k = (int)(threadIdx.x & 63); k < l; k += 64) {
    int x, y;
    cell_xy(d, src[k], x, y);
    dst[k] = make_int2(x, y);
  }
}

}  // namespace
