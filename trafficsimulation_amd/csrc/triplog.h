// triplog.h - the trip log (include/trafficsim_triplog.h): what k_spawn and remove_vehicle_dev note about a vehicle, the
// seal that turns a tick's removals into records in canonical order, and the OD reduction over the log.
// Part of the single translation unit engine.hip (included from there, in front of kernels.h).
//
// State.  Everything lives in one device struct, TripLog, reached through Dev::tlog (nullptr = the log is off: the one test
// the two hooks make).  Per vehicle (indexed by vehicle id like Dev's own arrays, regrown with them): where and when it was
// placed, its service type, and - written by the removal - why, when and at which `elapsed` it left.  Vehicle ids are never
// reused, so all of Dev's per-vehicle arrays (pos, target, steps, ...) of a removed vehicle stay as the removal left them.
//
// Order.  A removal pushes the vehicle id onto the staging list (one atomic per wave).  The list's order depends on
// scheduling, the log's must not: the seal (end of every tick that removed anything, and right after a host removal) marks
// the staged ids in a bitmap, counts the bits per block, scans the block counts and emits the records in ascending id behind
// the records already kept.  Group sizes from 1 to every live vehicle take the same path; its cost follows the number of
// vehicle ids handed out (one bit each), not the group.
//
// Capacity.  Position count + k of the group's k-th record is either below the capacity (kept) or not (dropped, counted):
// the kept set is canonical as well.
#pragma once

namespace {

struct TripLog {
  // ---- pointers and sizes: written by the host only (tl_upload copies this part) ----
  int32_t *origin, *spawn_step, *end_step;   // per vehicle; origin = cell, -1 = unknown
  double* end_elapsed;                       // per vehicle
  int8_t *vtype, *end_reason;                // per vehicle
  int32_t* staged;                           // vehicle ids removed since the last seal, in any order
  uint32_t* bitmap;                          // one bit per vehicle id, all zero between seals
  TsTripRecord* rec;
  const int32_t* zone;                       // ts_triplog_set_zones' plane (nullptr: none)
  long long capacity;
  int staged_cap, n_zones;
  // ---- counters: written by the device (tl_finish, the hooks) ----
  long long count, dropped, groups;
  int staged_n, pad_;
};
constexpr size_t TL_HOST_PART = offsetof(TripLog, count);

// Bitmap words per block of k_tl_count / k_tl_emit, one per thread: BLK (8192 vehicle ids per block), or fewer with
// TS_DEBUG_TRIPLOG_BLOCK=n (read by ts_triplog_start), so that a small test runs the seal over many blocks.
constexpr int TL_WORDS = BLK;

// k_spawn's hook.  The caller has tested d.tlog.
__device__ __forceinline__ void tl_spawn_dev(const Dev& d, int vid, int pos) {
  TripLog* t = d.tlog;
  t->origin[vid] = pos; t->spawn_step[vid] = d.tl_step; t->vtype[vid] = 0;
}

// remove_vehicle_dev's hook.  The caller has tested d.tlog.  The lanes of the wave that remove a vehicle right now share
// one atomic: the first of them reserves a run of the staging list for all.
__device__ __forceinline__ void tl_remove_dev(const Dev& d, int vid, int reason, double elapsed) {
  TripLog* t = d.tlog;
  t->end_reason[vid] = (int8_t)reason; t->end_elapsed[vid] = elapsed; t->end_step[vid] = d.tl_step;
  const unsigned long long m = __ballot(1);
  const int lane = (int)(threadIdx.x & 63);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  int base = 0;
  if (before == 0) base = atomicAdd(&t->staged_n, __popcll(m));
  base = __builtin_amdgcn_readfirstlane(base);   // (the first active lane is the one that reserved)
  const int k = base + before;
  if (k < t->staged_cap) t->staged[k] = vid;
}

__global__ void k_tl_mark(TripLog* t) {
  const int n = min(t->staged_n, t->staged_cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int vid = t->staged[i];
    atomicOr(&t->bitmap[vid >> 5], 1u << (vid & 31));
  }
}

// block sum of an int over BLK threads; valid in every thread
__device__ __forceinline__ int tl_block_sum(int v, int* wsum) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < BLK / 64; w++) s += wsum[w];
  return s;
}

__global__ void k_tl_count(const TripLog* t, int n_words, int wpb, int* block_counts) {
  __shared__ int wsum[BLK / 64];
  const int w = blockIdx.x * wpb + threadIdx.x;
  const int c = ((int)threadIdx.x < wpb && w < n_words) ? __popc(t->bitmap[w]) : 0;
  const int s = tl_block_sum(c, wsum);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s;
}

__device__ __forceinline__ void tl_write_record(const Dev& d, const TripLog* t, int vid, TsTripRecord* r) {
  TsTripRecord o;
  o.spawn_idx = vid; o.population = d.pop[vid]; o.vehicle_type = t->vtype[vid]; o.end_reason = t->end_reason[vid];
  const int org = t->origin[vid], tgt = d.target[vid], pos = d.pos[vid];
  int x, y;
  if (org >= 0) { cell_xy(d, org, x, y); o.origin_x = x; o.origin_y = y; } else { o.origin_x = -1; o.origin_y = -1; }
  cell_xy(d, tgt, x, y); o.dest_x = x; o.dest_y = y;
  cell_xy(d, pos, x, y); o.end_x = x; o.end_y = y;
  o.spawn_step = t->spawn_step[vid]; o.end_step = t->end_step[vid];
  o.distance = d.steps[vid]; o.stuck_ticks = d.stuck_ticks[vid];
  o.depart_elapsed = d.depart[vid]; o.end_elapsed = t->end_elapsed[vid];
  *r = o;
}

// block_off = the exclusive scan of k_tl_count's counts (k_scan_blocks).  One bitmap word per thread: its records go
// behind those of the words before it, in ascending bit order; the word is cleared for the next seal.
__global__ void k_tl_emit(Dev d, int n_words, int wpb, const int* block_off) {
  __shared__ int wcnt[BLK / 64];
  TripLog* t = d.tlog;
  const int w = blockIdx.x * wpb + threadIdx.x;
  uint32_t bits = ((int)threadIdx.x < wpb && w < n_words) ? t->bitmap[w] : 0u;
  const int c = __popc(bits);
  // exclusive prefix of c inside the block: inside the wave by shuffles, across the waves through LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
  if (lane == 63) wcnt[wave] = incl;
  __syncthreads();
  int before = incl - c;
  for (int q = 0; q < wave; q++) before += wcnt[q];
  if (!bits) return;
  t->bitmap[w] = 0u;
  long long k = t->count + block_off[blockIdx.x] + before;   // (count is only advanced by k_tl_finish, after this kernel)
  while (bits) {
    const int b = __ffs(bits) - 1;
    bits &= bits - 1;
    if (k < t->capacity) tl_write_record(d, t, (w << 5) + b, &t->rec[k]);
    k++;
  }
}

__global__ void k_tl_finish(TripLog* t) {
  if (threadIdx.x || blockIdx.x) return;
  const long long n = min(t->staged_n, t->staged_cap);
  const long long kept = max(0ll, min(n, t->capacity - t->count));
  t->count += kept; t->dropped += n - kept;
  if (n > 0) t->groups += 1;
  t->staged_n = 0;
}

// One lane per record: both zones looked up, three global atomics into the [n_zones][n_zones] matrices (any of them may be
// nullptr).  Durations are integer-valued doubles (multiples of the tick length, see k_live_stats), so the double adds are
// exact and their order cannot show.  The records that fall outside are counted per wave.
__global__ void k_triplog_od(Dev d, long long n, uint32_t reason_mask, unsigned long long* cnt, double* dur,
                             unsigned long long* dist, unsigned long long* unzoned) {
  const TripLog* t = d.tlog;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (i < n) {
    const TsTripRecord r = t->rec[i];
    if ((reason_mask >> r.end_reason) & 1u) {
      int zo = -1, zd = -1;
      if (r.origin_x >= 0) zo = t->zone[(size_t)r.origin_y * d.W + r.origin_x];
      zd = t->zone[(size_t)r.dest_y * d.W + r.dest_x];
      if (zo < 0 || zd < 0 || zo >= t->n_zones || zd >= t->n_zones) out = true;
      else {
        const size_t k = (size_t)zo * t->n_zones + zd;
        if (cnt) atomicAdd(&cnt[k], 1ull);
        if (dur) atomicAdd(&dur[k], r.end_elapsed - r.depart_elapsed);
        if (dist) atomicAdd(&dist[k], (unsigned long long)r.distance);
      }
    }
  }
  const unsigned long long m = __ballot(out);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(unzoned, (unsigned long long)__popcll(m));
}

}  // namespace
