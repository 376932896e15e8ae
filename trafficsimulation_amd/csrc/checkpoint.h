// checkpoint.h - ts_checkpoint_size / _save / _load (include/trafficsim_checkpoint.h): every piece of dynamic state of an
// engine as one canonical blob, and back.  DESIGN.md "Checkpoints" has the member-by-member classification (saved / rebuilt
// on load / reset on load) this file implements, and the blob layout.
// Part of the single translation unit engine.hip (included at its end, after the C-ABI entries it reuses).
#pragma once
#include "../../include/trafficsim_checkpoint.h"

namespace {

constexpr uint64_t CK_MAGIC = 0x31544B4354535254ull;   // "TRSTCKT1" little-endian
constexpr uint32_t CK_VERSION = 1;

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// cell records -> dense dynamic planes: veh (int32), occ, stop, stuck (int8).  One thread per cell reads the record's
// dynamic dword pair (veh | occ stop stuck stat) with one 8-byte load: consecutive lanes read consecutive records.
__global__ void k_ckpt_pack_cells(const Cell* __restrict__ cell, int n, int32_t* __restrict__ veh, int8_t* __restrict__ occ,
                                  int8_t* __restrict__ stop, int8_t* __restrict__ stuck) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const uint2 w = *reinterpret_cast<const uint2*>(&cell[c].veh);
  veh[c] = (int32_t)w.x;
  occ[c] = (int8_t)(w.y & 0xFF); stop[c] = (int8_t)((w.y >> 8) & 0xFF); stuck[c] = (int8_t)((w.y >> 16) & 0xFF);
}
// dense planes -> the target's records.  The static byte (and the node number behind it) stays: the fingerprint has proved
// that the target was built from the same world.  The claim words are cleared (epoch-tagged scratch: the target's epoch
// restarts at 0), occupancy and stop are written through to their byte planes.
__global__ void k_ckpt_unpack_cells(Cell* __restrict__ cell, int n, const int32_t* __restrict__ veh, const int8_t* __restrict__ occ,
                                    const int8_t* __restrict__ stop, const int8_t* __restrict__ stuck, int8_t* __restrict__ occ_plane,
                                    int8_t* __restrict__ stop_plane) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const uint32_t stat = (uint32_t)cell[c].stat;
  const int8_t o = occ[c], s = stop[c];
  *reinterpret_cast<uint4*>(&cell[c].claim[0]) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  *reinterpret_cast<uint2*>(&cell[c].veh) =
      make_uint2((uint32_t)veh[c], (uint32_t)(uint8_t)o | ((uint32_t)(uint8_t)s << 8) | ((uint32_t)(uint8_t)stuck[c] << 16) | (stat << 24));
  occ_plane[c] = o;
  stop_plane[c] = s;
}

// words a vehicle's paths take in a blob: the live words of its main path and of its four aux paths (path_words.h: path_live,
// aux_words - what k_pool_gc keeps); 0 for a vehicle that is gone
__device__ __forceinline__ void ck_path_words(const Dev& d, int v, int& w0, int& main_w, int (&ax_w)[4]) {
  w0 = 0; main_w = 0;
  for (int k = 0; k < 4; k++) ax_w[k] = 0;
  if (!(d.flags[v] & VF_ALIVE)) return;
  const PathLive l = path_live(d.path_cur[v], d.path_len[v]);
  w0 = l.w0; main_w = l.words;
  for (int k = 0; k < 4; k++) ax_w[k] = aux_words(d.ax_len[k][v]);
}
__device__ __forceinline__ int ck_total(int main_w, const int (&ax_w)[4]) { return main_w + ax_w[0] + ax_w[1] + ax_w[2] + ax_w[3]; }

// per block of BLK vehicles: the words they take (k_scan_blocks turns the sums into block offsets)
__global__ void k_ckpt_count_paths(Dev d, int nv, int* block_sums) {
  __shared__ int wsum[BLK / 64];
  const int v = blockIdx.x * BLK + threadIdx.x;
  int c = 0;
  if (v < nv) { int w0, mw, aw[4]; ck_path_words(d, v, w0, mw, aw); c = ck_total(mw, aw); }
  for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < BLK / 64; w++) t += wsum[w]; block_sums[blockIdx.x] = t; }
}
// exclusive offset of this thread's `c` inside its block (waves in order, lanes in order)
__device__ __forceinline__ int ck_block_excl(int c) {
  __shared__ int wtot[BLK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  int base = 0;
  for (int q = 0; q < w; q++) base += wtot[q];
  return base + incl - c;
}
// every vehicle's words at its place in vehicle-id order (offsets from the block scan, never from arrival order), and its
// main path's cursor and length as they read against the packed words (path_live's)
__global__ void k_ckpt_pack_paths(Dev d, int nv, const int* __restrict__ block_off, uint32_t* __restrict__ out,
                                  int32_t* __restrict__ out_cur, int32_t* __restrict__ out_len) {
  const int v = blockIdx.x * BLK + threadIdx.x;
  int w0 = 0, mw = 0, aw[4] = {0, 0, 0, 0};
  if (v < nv) ck_path_words(d, v, w0, mw, aw);
  const int off = block_off[blockIdx.x] + ck_block_excl(ck_total(mw, aw));
  if (v >= nv) return;
  const PathLive l = path_live(d.path_cur[v], d.path_len[v]);
  out_cur[v] = l.cur;                   // (gone vehicles too: their cursors are canonical after a load as well)
  out_len[v] = l.len;
  uint32_t o = (uint32_t)off;
  const uint32_t src = d.path_off[v] + (uint32_t)w0;
  for (int q = 0; q < mw; q++) out[o + q] = d.pool[src + q];
  o += (uint32_t)mw;
  for (int k = 0; k < 4; k++) {
    const uint32_t s = d.ax_off[k][v];
    for (int q = 0; q < aw[k]; q++) out[o + q] = d.pool[s + q];
    o += (uint32_t)aw[k];
  }
}
// the packed words -> pool[0, used), path_off / ax_off rewritten (path_cur / path_len / ax_len / flags are already the blob's)
__global__ void k_ckpt_unpack_paths(Dev d, int nv, const int* __restrict__ block_off, const uint32_t* __restrict__ in) {
  const int v = blockIdx.x * BLK + threadIdx.x;
  int w0 = 0, mw = 0, aw[4] = {0, 0, 0, 0};
  if (v < nv) ck_path_words(d, v, w0, mw, aw);   // (w0 = 0: the blob's cursors are packed)
  const int off = block_off[blockIdx.x] + ck_block_excl(ck_total(mw, aw));
  if (v >= nv) return;
  uint32_t o = (uint32_t)off;
  d.path_off[v] = o;
  for (int q = 0; q < mw; q++) d.pool[o + q] = in[o + q];
  o += (uint32_t)mw;
  for (int k = 0; k < 4; k++) {
    d.ax_off[k][v] = o;
    for (int q = 0; q < aw[k]; q++) d.pool[o + q] = in[o + q];
    o += (uint32_t)aw[k];
  }
}

// ---------------------------------------------------------------------------------------------
// blob writer / reader
// ---------------------------------------------------------------------------------------------
struct CkHeader {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t fp_world, fp_params, fp_lights, fp_traffic;
  int32_t width, height;
};
static_assert(sizeof(CkHeader) == 64, "checkpoint header layout");

// the host scalars (fixed size, no padding: every field 8 bytes or in pairs of 4)
struct CkScalars {
  int32_t n_vehicles_total, n_active, n_sched, n_sched_vehicles;
  int32_t clock_slot, mixed_order, groups_scheduled, blocks_scheduled;
  int32_t n_host_agents, rain_manager, rain_counter, rain_cooldown_left;
  int32_t standing_possible, G, gen_armed, gen_current_day;
  int64_t gen_completed_at_day_start;
  int32_t gen_ticks_since_stats, n_blocks;
  uint64_t path_words;
  uint32_t mt_global[624], idx_global, mt_sched[624], idx_sched;
  RainDiscs prev_discs;
  int32_t pad_;
  TsCounters C;
  TsCachedStats cs;
  DevCnt cnt;
};

// Writes into dst (or only counts when dst is null).  Device ranges are queued as copies on the engine's stream.
struct CkSink {
  uint8_t* dst; size_t pos = 0; hipStream_t st; hipError_t err = hipSuccess;
  void put(const void* p, size_t n) { if (dst && n) memcpy(dst + pos, p, n); pos += n; }
  template <typename T> void val(const T& v) { put(&v, sizeof(T)); }
  template <typename T> void vec(const std::vector<T>& v) { val<uint64_t>(v.size()); put(v.data(), v.size() * sizeof(T)); }
  void dev(const void* p, size_t n) {
    if (dst && n && err == hipSuccess) err = hipMemcpyAsync(dst + pos, p, n, hipMemcpyDeviceToHost, st);
    pos += n;
  }
};
struct CkSrc {
  const uint8_t* p; size_t n, pos = 0; bool ok = true;
  const uint8_t* take(size_t k) { if (!ok || k > n - pos) { ok = false; return nullptr; } const uint8_t* r = p + pos; pos += k; return r; }
  template <typename T> bool val(T& v) { const uint8_t* r = take(sizeof(T)); if (r) memcpy(&v, r, sizeof(T)); return r != nullptr; }
  // a length-prefixed vector, at most `max_n` elements
  template <typename T> bool vec(std::vector<T>& v, uint64_t max_n) {
    uint64_t k = 0;
    if (!val(k) || k > max_n || k > (n - pos) / sizeof(T)) { ok = false; return false; }
    v.resize((size_t)k);
    const uint8_t* r = take((size_t)k * sizeof(T));
    if (r && k) memcpy(v.data(), r, (size_t)k * sizeof(T));
    return r != nullptr;
  }
};

// the vehicle columns a blob carries as they are, [0, n_vehicles_total) each (path_cur / path_len travel packed, path_off /
// ax_off are rewritten on load; ev / ev_idx are one decide phase's scratch - tick() clears ev first - and are cleared on load)
std::vector<std::pair<void**, size_t>> ck_vehicle_columns(Dev& d) {
  std::vector<std::pair<void**, size_t>> c;
#define CKC(f) c.push_back({(void**)&d.f, sizeof(*d.f)});
  CKC(pos) CKC(target) CKC(stuck_ticks) CKC(cooldown) CKC(stranded_left) CKC(steps) CKC(over_dur) CKC(det_dur)
  CKC(next_in_cell) CKC(active_idx) CKC(sched_slot) CKC(base_speed) CKC(cur_speed) CKC(max_steps) CKC(dir) CKC(pop)
  CKC(flags) CKC(depart) CKC(st_before) CKC(st_after) CKC(tier_hint) CKC(chg)
  for (int k = 0; k < 4; k++) { CKC(ax_start[k]) CKC(ax_len[k]) }
#undef CKC
  return c;
}
// light-group state, G entries each
std::vector<int32_t**> ck_group_columns(Dev& d) {
  return {&d.gs_cur, &d.gs_pend, &d.gs_trans, &d.gs_clear, &d.gs_ftphase, &d.gs_fttimer, &d.gs_qtimer, &d.gs_gap,
          &d.gs_last, &d.gs_nsp, &d.gs_ewp, &d.gs_repop, &d.g_slot};
}

// The external light control (lights_ext_api.h): a trailing section, written only under TS_LIGHTS_EXTERNAL - blobs of every
// other algorithm are what they were.  The scalars, then the controller columns [G][2], the stored pressures [G][2] and the
// cached state vector [G][dim] (meaningful while `observed` is set).
struct CkLightsExt {
  uint32_t magic;
  int32_t dim, min_green, observed;
  int64_t calls;
};
constexpr uint32_t CK_LE_MAGIC = 0x3154584Cu;   // "LXT1"
static_assert(sizeof(CkLightsExt) == 24, "checkpoint: external light control section");
// The A2C / GAT-DQN protocols (lights_proto_api.h): a second trailing section behind it, written only once a protocol is
// configured - every other blob is what it was.  The scalars, then epsilon [G] as doubles.
struct CkLightsProto {
  uint32_t magic;
  int32_t protocol, min_green, pad_;
  double eps_min, eps_decay;
  int64_t calls;
};
constexpr uint32_t CK_LP_MAGIC = 0x3152504Cu;   // "LPR1"
static_assert(sizeof(CkLightsProto) == 40, "checkpoint: light protocol section");

// what is in flight between two ticks: the shuffle pipeline (idle once tick() returned), the take-ahead table on the copy
// stream, the permutation copies, the quad searcher's stream and the main stream
int ck_drain(E* e) {
  if (e->sh_thread.joinable()) shuffle_wait(e);
  if (e->take_ev_recorded) HIPOK(hipEventSynchronize(e->take_ev));
  if (e->copy_stream) HIPOK(hipStreamSynchronize(e->copy_stream));
  if (e->perm_stream) HIPOK(hipStreamSynchronize(e->perm_stream));
  if (e->quad_stream) HIPOK(hipStreamSynchronize(e->quad_stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}
int ck_stage(E* e, size_t bytes) {
  if (bytes <= e->cap_ck_stage) return TS_OK;
  dfree(e, e->ck_stage);
  e->ck_stage = nullptr; e->cap_ck_stage = 0;
  HIPOK(dalloc(e, &e->ck_stage, bytes));
  e->cap_ck_stage = bytes;
  return TS_OK;
}
// the path words of [0, nv) vehicles as they stand on the device: block offsets into e->ck_bsum, the total into *words
int ck_count_paths(E* e, int nv, uint64_t* words) {
  *words = 0;
  if (nv == 0) return TS_OK;
  const int nb = nblk(nv);
  if (nb + 1 > e->cap_ck_bsum) {
    dfree(e, e->ck_bsum); e->ck_bsum = nullptr; e->cap_ck_bsum = 0;
    HIPOK(dalloc(e, &e->ck_bsum, (size_t)nb + 1));
    e->cap_ck_bsum = nb + 1;
  }
  hipLaunchKernelGGL(k_ckpt_count_paths, dim3(nb), dim3(BLK), 0, e->stream, e->d, nv, e->ck_bsum);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, e->stream, e->ck_bsum, nb, e->ck_bsum + nb);
  int total = 0;
  TRY(read_back(e, &total, e->ck_bsum + nb, sizeof(int)));
  if (total < 0) return fail(e, TS_E_CAPACITY, "checkpoint: more than 2^31 live path words");
  *words = (uint64_t)total;
  return TS_OK;
}

// Everything but the header's size field, in blob order.  `stage` is true when the device staging holds the packed cell
// planes and paths (a real save); a size query only counts.
int ck_write(E* e, CkSink& s, uint64_t path_words, bool stage) {
  Dev& d = e->d;
  const size_t N = (size_t)e->N, nv = (size_t)e->n_vehicles_total;
  CkHeader h{};
  h.magic = CK_MAGIC; h.version = CK_VERSION; h.header_bytes = sizeof(CkHeader);
  h.fp_world = e->fp_world; h.fp_params = e->fp_params; h.fp_lights = e->fp_lights; h.fp_traffic = e->gen.armed ? e->fp_traffic : 0;
  h.width = e->W; h.height = e->H;
  s.val(h);
  // --- host scalars
  CkScalars S;
  memset(&S, 0, sizeof(S));
  S.n_vehicles_total = e->n_vehicles_total; S.n_active = e->n_active; S.n_sched = e->n_sched; S.n_sched_vehicles = e->n_sched_vehicles;
  S.clock_slot = e->clock_slot; S.mixed_order = e->mixed_order; S.groups_scheduled = e->groups_scheduled;
  S.blocks_scheduled = e->blocks_scheduled; S.n_host_agents = e->n_host_agents; S.rain_manager = e->rain_manager;
  S.rain_counter = e->rain_counter; S.rain_cooldown_left = e->rain_cooldown_left; S.standing_possible = e->standing_possible;
  S.G = d.G; S.gen_armed = e->gen.armed; S.gen_current_day = e->gen.current_day;
  S.gen_completed_at_day_start = e->gen.completed_at_day_start; S.gen_ticks_since_stats = e->gen.ticks_since_stats;
  S.n_blocks = (int32_t)e->blocks.size();
  S.path_words = path_words;
  e->rng_global.state(S.mt_global, &S.idx_global);
  e->rng_sched.state(S.mt_sched, &S.idx_sched);
  S.prev_discs = e->prev_discs;
  S.C = e->C;
  S.cs = e->gen.cs;
  if (s.dst) {
    memcpy(&S.cnt, e->hcnt, sizeof(DevCnt));   // (sync_counters has just read it)
    // the bump allocator's position depends on the pool's layout, the profiling / debugging words are not state
    S.cnt.pool_used = 0;
    memset(S.cnt.qprof, 0, sizeof(S.cnt.qprof)); memset(S.cnt.prof, 0, sizeof(S.cnt.prof));
    S.cnt.probe_cycles = S.cnt.probe_wall = S.cnt.spill_exp = 0; S.cnt.max_heap = S.cnt.max_search_exp = 0;
  }
  s.val(S);
  // --- host containers (unordered ones in key order)
  s.val<uint64_t>(e->rains_all.size());
  for (const auto& r : e->rains_all) {
    s.val(r.x); s.val(r.y); s.val(r.dx); s.val(r.dy);
    const int32_t q[6] = {r.radius, r.stepped, r.alive, r.cx, r.cy, 0};
    s.put(q, sizeof(q));
  }
  { std::vector<int32_t> v(e->rains.begin(), e->rains.end()); s.vec(v); }
  s.val<uint64_t>(e->gen.pending.size());
  for (const auto& t : e->gen.pending) { const int32_t q[4] = {t.origin, t.dest, t.kind, t.day}; s.put(q, sizeof(q)); s.val(t.depart); }
  { std::vector<int64_t> v(e->gen.daily_difference_history.begin(), e->gen.daily_difference_history.end()); s.vec(v); }
  for (const auto& b : e->blocks) {
    const double q[4] = {b.food, b.waste, b.food_rem, b.waste_rem};
    const int32_t t[2] = {b.ticks_since_food, b.ticks_since_waste};
    s.put(q, sizeof(q)); s.put(t, sizeof(t));
  }
  s.val<uint64_t>(e->svc.size());
  for (const auto& v : e->svc) {
    const int32_t q[8] = {v.vid, v.type, v.id, v.block, v.phase, v.ticks, v.pos, v.target};
    s.put(q, sizeof(q)); s.val(v.load); s.val(v.max_load);
  }
  {
    std::vector<std::pair<int32_t, int32_t>> pc(e->parked_cells.begin(), e->parked_cells.end());
    std::sort(pc.begin(), pc.end());
    s.val<uint64_t>(pc.size());
    for (const auto& p : pc) { s.val(p.first); s.val(p.second); }
  }
  { std::vector<uint8_t> v(e->sv_live.begin(), e->sv_live.end()); s.vec(v); }
  {
    std::vector<uint64_t> keys;
    keys.reserve(e->path_cache.size());
    for (const auto& kv : e->path_cache) keys.push_back(kv.first);
    std::sort(keys.begin(), keys.end());
    s.val<uint64_t>(keys.size());
    for (uint64_t k : keys) { const auto& cp = e->path_cache.at(k); s.val(k); s.val<int32_t>(cp.len); s.vec(cp.words); }
  }
  // --- device sections: cell planes, rain and tick-start occupancy, vehicles, paths, lists, light groups
  uint8_t* stg = e->ck_stage;
  if (stage) s.dev(stg, N * 7); else s.pos += N * 7;
  s.dev(d.rain, N);
  s.dev(d.occ_snap, N);
  for (auto& c : ck_vehicle_columns(d)) s.dev(*c.first, nv * c.second);
  const size_t paths_at = N * 7;   // staging: [cell planes][path_cur][path_len][words]
  if (stage) { s.dev(stg + paths_at, nv * 4); s.dev(stg + paths_at + nv * 4, nv * 4); s.dev(stg + paths_at + nv * 8, path_words * 4); }
  else s.pos += nv * 8 + path_words * 4;
  s.dev(d.active, (size_t)e->n_active * 4);
  s.dev(d.sched_kind, (size_t)e->n_sched);
  s.dev(d.sched_ref, (size_t)e->n_sched * 4);
  s.dev(d.hslot, (size_t)e->n_host_agents * 4);
  s.dev(d.bslot, (size_t)e->blocks_scheduled * 4);
  for (int32_t** g : ck_group_columns(d)) s.dev(*g, (size_t)d.G * 4);
  if (e->P.light_algorithm == TS_LIGHTS_EXTERNAL && e->le.ready) {
    const LightsExt& x = e->le.x;
    const CkLightsExt L{CK_LE_MAGIC, x.dim, x.min_green, e->le.observed ? 1 : 0, e->le.calls};
    s.val(L);
    s.dev(x.ctrl, (size_t)x.G * 8);
    s.dev(x.stored, (size_t)x.G * 8);
    s.dev(x.state, (size_t)x.G * x.dim * 4);
    if (e->lp.protocol) {
      const CkLightsProto Q{CK_LP_MAGIC, e->lp.protocol, e->lp.min_green, 0, e->lp.eps_min, e->lp.eps_decay, e->lp.calls};
      s.val(Q);
      s.put(e->lp.eps.data(), (size_t)x.G * 8);
    }
  }
  return TS_OK;
}

// everything a save reads, drained and packed; *size = the blob's size
int ck_prepare(E* e, bool stage, uint64_t* path_words, uint64_t* size) {
  if (e->fatal) return fail(e, TS_E_STATE, "checkpoint: the run ended with an error (model.step() raised)");
  if (!e->rng_global.seeded() || !e->rng_sched.seeded()) return fail(e, TS_E_STATE, "checkpoint: seed both RNG streams first");
  TRY(ck_drain(e));
  TRY(ck_count_paths(e, e->n_vehicles_total, path_words));
  TRY(sync_counters(e));
  const size_t N = (size_t)e->N, nv = (size_t)e->n_vehicles_total;
  if (stage) {
    TRY(ck_stage(e, N * 7 + nv * 8 + *path_words * 4));
    uint8_t* stg = e->ck_stage;
    hipLaunchKernelGGL(k_ckpt_pack_cells, dim3(nblk((long long)N)), dim3(BLK), 0, e->stream, e->d.cell, (int)N, (int32_t*)stg,
                       (int8_t*)(stg + N * 4), (int8_t*)(stg + N * 5), (int8_t*)(stg + N * 6));
    if (nv)
      hipLaunchKernelGGL(k_ckpt_pack_paths, dim3(nblk((long long)nv)), dim3(BLK), 0, e->stream, e->d, (int)nv, e->ck_bsum,
                         (uint32_t*)(stg + N * 7 + nv * 8), (int32_t*)(stg + N * 7), (int32_t*)(stg + N * 7 + nv * 4));
    HIPOK(hipGetLastError());
  }
  CkSink cnt{nullptr, 0, e->stream};
  TRY(ck_write(e, cnt, *path_words, false));
  *size = cnt.pos;
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_checkpoint_size(ts_handle e, uint64_t* bytes) {
  if (!e || !bytes) return TS_E_INVALID;
  uint64_t words = 0;
  TRY(ck_prepare(e, false, &words, bytes));
  return TS_OK;
}

int ts_checkpoint_save(ts_handle e, void* dst, uint64_t cap, uint64_t* written) {
  if (!e || !dst || !written) return TS_E_INVALID;
  uint64_t words = 0, size = 0;
  TRY(ck_prepare(e, true, &words, &size));
  if (size > cap) { *written = size; return fail(e, TS_E_CAPACITY, "checkpoint: the buffer is smaller than ts_checkpoint_size"); }
  CkSink s{(uint8_t*)dst, 0, e->stream};
  TRY(ck_write(e, s, words, true));
  if (s.err != hipSuccess) return fail(e, TS_E_DEVICE, std::string("checkpoint copy: ") + hipGetErrorString(s.err));
  HIPOK(hipStreamSynchronize(e->stream));
  ((CkHeader*)dst)->total_bytes = size;
  *written = size;
  return TS_OK;
}

int ts_checkpoint_load(ts_handle e, const void* src, uint64_t n) {
  if (!e) return TS_E_INVALID;
  e->batch.valid = false;   // (astar_batch_api.h: the last query batch's result ends here)
  if (!src && n) return fail(e, TS_E_INVALID, "checkpoint: null blob");
  if (e->dist_world > 1) return fail(e, TS_E_STATE, "checkpoint: loading onto a handle with replan sharding is not supported");
  Dev& d = e->d;
  const size_t N = (size_t)e->N;
  // ---------------- validation: nothing in the target changes before it has passed ----------------
  CkSrc r{(const uint8_t*)src, (size_t)n};
  CkHeader h;
  if (!r.val(h)) return fail(e, TS_E_INVALID, "checkpoint: shorter than its header");
  if (h.magic != CK_MAGIC) return fail(e, TS_E_INVALID, "checkpoint: bad magic (not a checkpoint blob)");
  if (h.version != CK_VERSION || h.header_bytes != sizeof(CkHeader))
    return fail(e, TS_E_INVALID, "checkpoint: format version " + std::to_string(h.version) + ", this build reads " + std::to_string(CK_VERSION));
  if (h.total_bytes != n) return fail(e, TS_E_INVALID, "checkpoint: truncated or padded (" + std::to_string(n) + " bytes, header says " + std::to_string(h.total_bytes) + ")");
  if (h.width != e->W || h.height != e->H || h.fp_world != e->fp_world) return fail(e, TS_E_INVALID, "checkpoint: fingerprint mismatch: world");
  if (h.fp_params != e->fp_params) return fail(e, TS_E_INVALID, "checkpoint: fingerprint mismatch: params");
  if (h.fp_lights != e->fp_lights) return fail(e, TS_E_INVALID, "checkpoint: fingerprint mismatch: light tables");
  if (h.fp_traffic != (e->gen.armed ? e->fp_traffic : 0)) return fail(e, TS_E_INVALID, "checkpoint: fingerprint mismatch: traffic tables");
  CkScalars S;
  if (!r.val(S)) return fail(e, TS_E_INVALID, "checkpoint: truncated (scalars)");
  auto bad = [&](const char* what) { return fail(e, TS_E_INVALID, std::string("checkpoint: section size: ") + what); };
  if (S.n_vehicles_total < 0 || S.n_active < 0 || S.n_active > S.n_vehicles_total || S.n_sched < 0 ||
      (long long)S.n_sched >= (long long)RANK_MASK || S.n_sched_vehicles < 0 || S.n_sched_vehicles > S.n_sched)
    return bad("vehicle / schedule counts");
  if (S.G != d.G || S.groups_scheduled < 0 || S.groups_scheduled > d.G) return bad("light groups");
  if (S.n_blocks != (int32_t)e->blocks.size() || S.blocks_scheduled < 0 || S.blocks_scheduled > S.n_sched) return bad("city blocks");
  if (S.n_host_agents < 0) return bad("host agents");
  if (S.clock_slot < -1 || S.clock_slot >= std::max(S.n_sched, 1)) return bad("clock slot");
  if (S.idx_global > 624 || S.idx_sched > 624) return bad("RNG index");
  if (S.prev_discs.n < 0 || S.prev_discs.n > 16) return bad("rain discs");
  if (S.path_words >= (1ull << 31)) return bad("path words");
  std::vector<ts_engine::Rain> rains_all;
  {
    uint64_t k = 0;
    if (!r.val(k) || k > (uint64_t)S.n_host_agents) return bad("rain clouds");
    rains_all.resize((size_t)k);
    for (auto& c : rains_all) {
      int32_t q[6];
      if (!r.val(c.x) || !r.val(c.y) || !r.val(c.dx) || !r.val(c.dy) || !r.val(q)) return bad("rain clouds");
      c.radius = q[0]; c.stepped = q[1] != 0; c.alive = q[2] != 0; c.cx = q[3]; c.cy = q[4];
    }
  }
  std::vector<int32_t> rains;
  if (!r.vec(rains, rains_all.size())) return bad("rain list");
  for (int32_t id : rains) if (id < 1 || (size_t)id > rains_all.size()) return bad("rain list");
  std::vector<ts_engine::Trip> pending;
  {
    uint64_t k = 0;
    if (!r.val(k) || k > n / 24) return bad("trips");
    pending.resize((size_t)k);
    for (auto& t : pending) {
      int32_t q[4];
      if (!r.val(q) || !r.val(t.depart)) return bad("trips");
      t.origin = q[0]; t.dest = q[1]; t.kind = q[2]; t.day = q[3];   // (service trips carry no cells: not range-checked)
    }
  }
  std::vector<int64_t> hist;
  if (!r.vec(hist, n / 8)) return bad("daily history");
  std::vector<ts_engine::Block> blocks_dyn(e->blocks.size());
  for (auto& b : blocks_dyn) {
    double q[4]; int32_t t[2];
    if (!r.val(q) || !r.val(t)) return bad("city blocks");
    b.food = q[0]; b.waste = q[1]; b.food_rem = q[2]; b.waste_rem = q[3]; b.ticks_since_food = t[0]; b.ticks_since_waste = t[1];
  }
  std::vector<ts_engine::SvcVeh> svc;
  {
    uint64_t k = 0;
    if (!r.val(k) || k > (uint64_t)S.n_vehicles_total) return bad("service vehicles");
    svc.resize((size_t)k);
    for (auto& v : svc) {
      int32_t q[8];
      if (!r.val(q) || !r.val(v.load) || !r.val(v.max_load)) return bad("service vehicles");
      v.vid = q[0]; v.type = q[1]; v.id = q[2]; v.block = q[3]; v.phase = q[4]; v.ticks = q[5]; v.pos = q[6]; v.target = q[7];
      if (v.vid < 0 || v.vid >= S.n_vehicles_total || v.block < -1 || v.block >= (int)e->blocks.size()) return bad("service vehicles");
    }
  }
  std::vector<std::pair<int32_t, int32_t>> parked;
  {
    uint64_t k = 0;
    if (!r.val(k) || k > N) return bad("parked cells");
    parked.resize((size_t)k);
    for (auto& p : parked) if (!r.val(p.first) || !r.val(p.second)) return bad("parked cells");
  }
  std::vector<uint8_t> sv_live;
  if (!r.vec(sv_live, e->sv_live.size()) || sv_live.size() != e->sv_live.size()) return bad("service fleet ids");
  std::vector<std::pair<uint64_t, ts_engine::CachedPath>> cache;
  {
    uint64_t k = 0;
    if (!r.val(k) || k > n / 20) return bad("path cache");
    cache.resize((size_t)k);
    for (auto& c : cache) {
      int32_t len = 0;
      if (!r.val(c.first) || !r.val(len) || !r.vec(c.second.words, n / 4)) return bad("path cache");
      c.second.len = len;
    }
  }
  const size_t nv = (size_t)S.n_vehicles_total;
  const uint8_t* cells_p = r.take(N * 7);
  const uint8_t* rain_p = r.take(N);
  const uint8_t* snap_p = r.take(N);
  auto cols = ck_vehicle_columns(d);
  std::vector<const uint8_t*> col_p;
  for (auto& c : cols) col_p.push_back(r.take(nv * c.second));
  const uint8_t* paths_p = r.take(nv * 8 + (size_t)S.path_words * 4);
  const uint8_t* active_p = r.take((size_t)S.n_active * 4);
  const uint8_t* kind_p = r.take((size_t)S.n_sched);
  const uint8_t* ref_p = r.take((size_t)S.n_sched * 4);
  const uint8_t* hslot_p = r.take((size_t)S.n_host_agents * 4);
  const uint8_t* bslot_p = r.take((size_t)S.blocks_scheduled * 4);
  auto gcols = ck_group_columns(d);
  std::vector<const uint8_t*> g_p;
  for (size_t k = 0; k < gcols.size(); k++) g_p.push_back(r.take((size_t)d.G * 4));
  const bool le_on = e->P.light_algorithm == TS_LIGHTS_EXTERNAL && e->le.ready;
  CkLightsExt L{};
  const uint8_t *le_ctrl_p = nullptr, *le_stored_p = nullptr, *le_state_p = nullptr;
  if (le_on) {
    if (!r.val(L) || L.magic != CK_LE_MAGIC) return bad("external light control");
    if (L.dim != e->le.x.dim || L.min_green != e->le.x.min_green)
      return fail(e, TS_E_INVALID, "checkpoint: the blob's external light control has dimension " + std::to_string(L.dim) + " and min-green " +
                  std::to_string(L.min_green) + ", the handle is configured with " + std::to_string(e->le.x.dim) + " and " + std::to_string(e->le.x.min_green));
    if (L.calls < 0 || (L.observed != 0 && L.observed != 1) || (L.observed && L.calls == 0)) return bad("external light control");
    le_ctrl_p = r.take((size_t)d.G * 8);
    le_stored_p = r.take((size_t)d.G * 8);
    le_state_p = r.take((size_t)d.G * L.dim * 4);
  }
  CkLightsProto Q{};
  const uint8_t* lp_eps_p = nullptr;
  if (le_on && r.ok && (e->lp.protocol || r.pos != n)) {
    // (a blob without the section on a handle with a protocol, or the other way round, is another configuration too)
    const bool have = r.pos != n;
    if (have && (!r.val(Q) || Q.magic != CK_LP_MAGIC)) return bad("light protocol");
    if (!have || Q.protocol != e->lp.protocol || Q.min_green != e->lp.min_green || Q.eps_min != e->lp.eps_min || Q.eps_decay != e->lp.eps_decay)
      return fail(e, TS_E_INVALID, "checkpoint: the blob's light protocol is " + std::to_string(have ? Q.protocol : 0) + " (min-green " +
                  std::to_string(have ? Q.min_green : 0) + "), the handle is configured with protocol " + std::to_string(e->lp.protocol) +
                  " (min-green " + std::to_string(e->lp.min_green) + ") or other epsilon settings");
    if (Q.calls < 0) return bad("light protocol");
    lp_eps_p = r.take((size_t)d.G * 8);
    for (int g = 0; lp_eps_p && g < d.G; g++) {
      double v;
      memcpy(&v, lp_eps_p + (size_t)g * 8, 8);
      if (!(v >= 0.0 && v <= 1.0)) return bad("light protocol: epsilon outside [0, 1]");
    }
  }
  if (!r.ok) return bad("device sections truncated");
  if (r.pos != n) return bad("trailing bytes");
  {
    // the packed paths must match the counts the columns imply (k_ckpt_unpack_paths trusts them)
    const int32_t* cur = (const int32_t*)paths_p;
    const int32_t* len = cur + nv;
    const uint16_t* fl = nullptr;
    const int32_t* axl[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t k = 0; k < cols.size(); k++) {
      if (cols[k].first == (void**)&d.flags) fl = (const uint16_t*)col_p[k];
      for (int a = 0; a < 4; a++) if (cols[k].first == (void**)&d.ax_len[a]) axl[a] = (const int32_t*)col_p[k];
    }
    uint64_t want = 0;
    for (size_t v = 0; v < nv; v++) {
      int32_t c0, l0, la; uint16_t f;
      memcpy(&f, fl + v, 2);
      if (!(f & VF_ALIVE)) continue;
      memcpy(&c0, cur + v, 4); memcpy(&l0, len + v, 4);
      if (c0 < 0 || c0 > PATH_STEP_MASK) return bad("path cursor");
      want += (uint64_t)path_live(c0, l0).words;
      for (int a = 0; a < 4; a++) { memcpy(&la, axl[a] + v, 4); want += (uint64_t)aux_words(la); }
    }
    if (want != S.path_words) return bad("path words");
  }
  // ---------------- apply ----------------
  TRY(ck_drain(e));
  e->pool_used = 0;
  TRY(ensure_vehicle_capacity(e, (int)nv, S.n_sched));
  TRY(ensure_pool(e, (size_t)S.path_words + 1));
  if (S.n_host_agents > e->cap_hslot) {
    const int nc = std::max(64, S.n_host_agents * 2);
    TRY(regrow(e, &d.hslot, 0, (size_t)nc));
    e->cap_hslot = nc;
  }
  if (S.blocks_scheduled > e->cap_bslot) {
    const int nc = S.blocks_scheduled * 2 + 64;
    TRY(regrow(e, &d.bslot, 0, (size_t)nc));
    e->cap_bslot = nc;
  }
  TRY(ck_stage(e, N * 7 + (size_t)S.path_words * 4 + 4));
  hipStream_t st = e->stream;
  uint8_t* stg = e->ck_stage;
  HIPOK(hipMemcpyAsync(stg, cells_p, N * 7, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ckpt_unpack_cells, dim3(nblk((long long)N)), dim3(BLK), 0, st, d.cell, (int)N, (const int32_t*)stg,
                     (const int8_t*)(stg + N * 4), (const int8_t*)(stg + N * 5), (const int8_t*)(stg + N * 6), d.occ, d.stop);
  HIPOK(hipStreamSynchronize(st));   // (the staging is reused for the paths below)
  HIPOK(hipMemcpyAsync(d.rain, rain_p, N, hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(d.occ_snap, snap_p, N, hipMemcpyHostToDevice, st));
  for (size_t k = 0; k < cols.size(); k++) if (nv) HIPOK(hipMemcpyAsync(*cols[k].first, col_p[k], nv * cols[k].second, hipMemcpyHostToDevice, st));
  if (nv) {
    HIPOK(hipMemsetAsync(d.ev, 0, nv, st));
    HIPOK(hipMemsetAsync(d.ev_idx, 0, nv * 4, st));
    HIPOK(hipMemcpyAsync(d.path_cur, paths_p, nv * 4, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d.path_len, paths_p + nv * 4, nv * 4, hipMemcpyHostToDevice, st));
    if (S.path_words) HIPOK(hipMemcpyAsync(stg, paths_p + nv * 8, (size_t)S.path_words * 4, hipMemcpyHostToDevice, st));
    uint64_t words = 0;
    TRY(ck_count_paths(e, (int)nv, &words));   // (the same block offsets the source packed with)
    if (words != S.path_words) return fail(e, TS_E_DEVICE, "checkpoint: path words differ after upload (internal error)");
    hipLaunchKernelGGL(k_ckpt_unpack_paths, dim3(nblk((long long)nv)), dim3(BLK), 0, st, d, (int)nv, e->ck_bsum, (const uint32_t*)stg);
  }
  if (S.n_active) HIPOK(hipMemcpyAsync(d.active, active_p, (size_t)S.n_active * 4, hipMemcpyHostToDevice, st));
  if (S.n_sched) {
    HIPOK(hipMemcpyAsync(d.sched_kind, kind_p, (size_t)S.n_sched, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d.sched_ref, ref_p, (size_t)S.n_sched * 4, hipMemcpyHostToDevice, st));
  }
  if (S.n_host_agents) HIPOK(hipMemcpyAsync(d.hslot, hslot_p, (size_t)S.n_host_agents * 4, hipMemcpyHostToDevice, st));
  if (S.blocks_scheduled) HIPOK(hipMemcpyAsync(d.bslot, bslot_p, (size_t)S.blocks_scheduled * 4, hipMemcpyHostToDevice, st));
  if (d.G) {
    for (size_t k = 0; k < gcols.size(); k++) HIPOK(hipMemcpyAsync(*gcols[k], g_p[k], (size_t)d.G * 4, hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(d.gclaim_r, 0xFF, (size_t)d.G * 4, st));
  }
  if (le_on && d.G) {
    HIPOK(hipMemcpyAsync(e->le.x.ctrl, le_ctrl_p, (size_t)d.G * 8, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(e->le.x.stored, le_stored_p, (size_t)d.G * 8, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(e->le.x.state, le_state_p, (size_t)d.G * L.dim * 4, hipMemcpyHostToDevice, st));
  }
  // counters: the device block with the bump allocator at the packed pool's end
  S.cnt.pool_used = S.path_words;
  *e->hcnt = S.cnt;
  HIPOK(hipMemcpyAsync(d.cnt, e->hcnt, sizeof(DevCnt), hipMemcpyHostToDevice, st));
  HIPOK(hipGetLastError());
  HIPOK(hipStreamSynchronize(st));
  // host state
  e->n_vehicles_total = S.n_vehicles_total; e->n_active = S.n_active; e->n_sched = S.n_sched; e->n_sched_vehicles = S.n_sched_vehicles;
  e->clock_slot = S.clock_slot; e->mixed_order = S.mixed_order != 0; e->groups_scheduled = S.groups_scheduled;
  e->blocks_scheduled = S.blocks_scheduled; e->n_host_agents = S.n_host_agents; e->rain_manager = S.rain_manager != 0;
  e->rain_counter = S.rain_counter; e->rain_cooldown_left = S.rain_cooldown_left; e->standing_possible = S.standing_possible != 0;
  e->prev_discs = S.prev_discs;
  e->rains_all = std::move(rains_all);
  e->rains.assign(rains.begin(), rains.end());
  e->gen.armed = S.gen_armed != 0; e->gen.current_day = S.gen_current_day;
  e->gen.completed_at_day_start = S.gen_completed_at_day_start; e->gen.ticks_since_stats = S.gen_ticks_since_stats;
  e->gen.pending = std::move(pending);
  e->gen.daily_difference_history.assign(hist.begin(), hist.end());
  e->gen.cs = S.cs;
  for (size_t b = 0; b < blocks_dyn.size(); b++) {
    auto& B = e->blocks[b]; const auto& X = blocks_dyn[b];
    B.food = X.food; B.waste = X.waste; B.food_rem = X.food_rem; B.waste_rem = X.waste_rem;
    B.ticks_since_food = X.ticks_since_food; B.ticks_since_waste = X.ticks_since_waste;
  }
  e->svc = std::move(svc);
  e->parked_cells.clear();
  for (const auto& p : parked) e->parked_cells[p.first] = p.second;
  e->sv_live.assign(sv_live.begin(), sv_live.end());
  e->path_cache.clear();
  for (auto& c : cache) e->path_cache[c.first] = std::move(c.second);
  e->pool_used = (size_t)S.path_words;
  e->C = S.C;
  // the MT pipes restart at the saved logical positions (ts_seed: words_uploaded and the take-ahead table follow)
  TRY(ts_seed(e, TS_RNG_GLOBAL, S.mt_global, S.idx_global));
  TRY(ts_seed(e, TS_RNG_SCHEDULER, S.mt_sched, S.idx_sched));
  // rebuilt on demand / reset
  e->amap_valid = false; e->density_valid = false;
  e->epoch = 0;
  e->rank_clock_host = 0xFFFFFFFFu;
  e->roll_guess = 0; e->take_guess = 0; e->take_n = 0;
  e->quad_last_fb = -1;
  e->prof_pending.clear(); e->ev_used = 0;
  // the trip log keeps its records; it did not see any of these vehicles being placed
  e->tl_pending = 0;
  if (e->tl_on) TRY(tl_forget_origins(e));
  if (le_on) { e->le.calls = L.calls; e->le.observed = L.observed != 0; }
  if (lp_eps_p) {
    e->lp.calls = Q.calls;
    if (d.G) memcpy(e->lp.eps.data(), lp_eps_p, (size_t)d.G * 8);
    if (d.G && e->lp.d_eps) {
      HIPOK(hipMemcpyAsync(e->lp.d_eps, e->lp.eps.data(), (size_t)d.G * 8, hipMemcpyHostToDevice, e->stream));
      HIPOK(hipStreamSynchronize(e->stream));
    }
  }
  return TS_OK;
}

}  // extern "C"
