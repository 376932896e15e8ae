// lights_ext.h - kernels of the external light control (include/trafficsim_lights_ext.h has the semantics and the
// reference lines): the per-group sums, the state vector, the commit of the stored pressures, the action protocol and the
// phase requests.  Host side: lights_ext_api.h.  Part of the single translation unit engine.hip.
//
// No kernel here uses an atomic or depends on its launch geometry: every output word has one writer, and a group's sums
// are integers (any lane split gives the same total).
#pragma once

namespace {

// What the kernels need, by value (Dev stays as it is: its size is part of the A* kernels' resource budget).
struct LightsExt {
  int G, dim, min_green;
  const Cell* cell;
  const int32_t *nsin_off, *nsin, *ewin_off, *ewin, *nsout_off, *nsout, *ewout_off, *ewout;
  const int32_t *nb, *nb_ctor, *repop;
  int32_t *gs_cur, *gs_pend;
  int32_t* sums;     // [G][4] this call's local sums: occupancy N-S, E-W, stuck N-S, E-W
  int32_t* stored;   // [G][2] pressure_ns, pressure_ew as the last control call left them
  int32_t* ctrl;     // [G][2] _rl_phase, rl_timer
  double *size, *pen;   // [G] intersection_size, penalty_score
  float *state, *next;  // [G][dim]
  int* bad;          // one word: an action / phase outside its range was seen
};

// Sums pass: a team of TEAM adjacent lanes per group strides over the group's two approach lists and reads each cell's
// dynamic dword once (occ | stop << 8 | stuck << 16 | stat << 24, as k_move_resolve's dyn[k].y); the four partial sums
// meet in a butterfly of log2(TEAM) __shfl_xor steps that stays inside the team.  Lists are a handful to a few tens of
// cells: with TEAM = 8 most lists take one to three strides and a wavefront serves 8 groups.
template <int TEAM>
__global__ void k_le_sums(LightsExt x) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = t / TEAM, l = t % TEAM;
  const bool live = g < x.G;   // (a whole team is live or not; dead teams run the butterfly on zeros)
  int on = 0, oe = 0, sn = 0, se = 0;
  if (live) {
    for (int k = x.nsin_off[g] + l; k < x.nsin_off[g + 1]; k += TEAM) {
      const uint32_t dw = *reinterpret_cast<const uint32_t*>(&x.cell[x.nsin[k]].occ);
      on += (int8_t)(dw & 0xFF); sn += (int8_t)((dw >> 16) & 0xFF);
    }
    for (int k = x.ewin_off[g] + l; k < x.ewin_off[g + 1]; k += TEAM) {
      const uint32_t dw = *reinterpret_cast<const uint32_t*>(&x.cell[x.ewin[k]].occ);
      oe += (int8_t)(dw & 0xFF); se += (int8_t)((dw >> 16) & 0xFF);
    }
  }
#pragma unroll
  for (int o = TEAM / 2; o; o >>= 1) {
    on += __shfl_xor(on, o, TEAM); oe += __shfl_xor(oe, o, TEAM);
    sn += __shfl_xor(sn, o, TEAM); se += __shfl_xor(se, o, TEAM);
  }
  if (live && l == 0) *reinterpret_cast<int4*>(x.sums + 4 * (size_t)g) = make_int4(on, oe, sn, se);
}

// penalty_score from the cell records' road types (intersection_light_group.py:156-165): the mean of the R1 / R2 / R3
// penalties over the four coordinate lists, duplicates counted; intersection_size is 0 (see the header)
__global__ void k_le_static(LightsExt x, double r1, double r2, double r3) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  const double w[4] = {0.0, r1, r2, r3};
  const int32_t* offs[4] = {x.nsin_off, x.nsout_off, x.ewin_off, x.ewout_off};
  const int32_t* lists[4] = {x.nsin, x.nsout, x.ewin, x.ewout};
  double total = 0.0;
  int n = 0;
  for (int q = 0; q < 4; q++)
    for (int k = offs[q][g]; k < offs[q][g + 1]; k++) { total += w[st_road_type(x.cell[lists[q][k]].stat)]; n++; }
  x.size[g] = 0.0;
  x.pen[g] = n ? total / (double)n : 0.0;
}

// pressure_ns a group's own get_rl_state leaves behind in this call: its last compute_pressure is on the stuck map above 13
// dimensions (rl_simple.py:133-137), on the occupancy map otherwise
__device__ __forceinline__ int le_this_call(const LightsExt& x, int j) {
  const int32_t* s = x.sums + 4 * (size_t)j + (x.dim > 13 ? 2 : 0);
  return s[0] - s[1];
}

// get_rl_state (rl_simple.py:95-143) of group g with controller state (phase, timer).  all_current: every neighbour holds
// this call's value (phase B); otherwise neighbour j < g does and j > g holds the stored one - which in the very first call
// (`first`) is its occupancy pressure, computed on the spot (rl_simple.py:70-72).  Doubles, rounded to float32 once.
__device__ __forceinline__ void le_vector(const LightsExt& x, int g, int phase, int timer, bool all_current, bool first, float* out) {
  const int4 s = *reinterpret_cast<const int4*>(x.sums + 4 * (size_t)g);
  const int32_t* nb = (x.repop[g] ? x.nb : x.nb_ctor) + (size_t)g * 8;
  int cnt = 0;
  long long p_sum = 0;
  double size_sum = 0.0, pen_sum = 0.0;
  for (int k = 0; k < 4; k++) {
    const int nd = nb[2 * k], n = nb[2 * k + 1];
    if (nd < 0 || n < 0) continue;
    cnt++;
    size_sum += x.size[n]; pen_sum += x.pen[n];
    int p;
    if (all_current || n < g) p = le_this_call(x, n);
    else if (first) p = x.sums[4 * (size_t)n] - x.sums[4 * (size_t)n + 1];
    else p = x.stored[2 * (size_t)n];
    p_sum += p;
  }
  const double c = (double)max(cnt, 1);
  float* o = out + (size_t)g * x.dim;
  o[0] = (float)s.x; o[1] = (float)s.y; o[2] = (float)(s.x - s.y); o[3] = (float)(s.y - s.x);
  o[4] = phase == 0 ? 1.f : 0.f; o[5] = phase == 0 ? 0.f : 1.f;
  o[6] = (float)((double)timer / 30.0);
  if (x.dim > 7) { o[7] = (float)x.size[g]; o[8] = (float)x.pen[g]; o[9] = (float)(size_sum / c); o[10] = (float)(pen_sum / c); }
  // (pressure_ew = -pressure_ns for every group, so the two sums are exact negatives of each other)
  if (x.dim > 11) { o[11] = (float)((double)p_sum / c); o[12] = (float)((double)(-p_sum) / c); }
  if (x.dim > 13) { o[13] = (float)s.z; o[14] = (float)s.w; o[15] = (float)(s.z - s.w); o[16] = (float)(s.w - s.z); }
  if (x.dim > 17) { o[17] = (float)((double)p_sum / c); o[18] = (float)((double)(-p_sum) / c); }
}

// State-vector pass of phase A: parallel over the groups, because "this call's" and "stored" both exist after the sums pass.
__global__ void k_le_state(LightsExt x, int first) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  le_vector(x, g, x.ctrl[2 * (size_t)g], x.ctrl[2 * (size_t)g + 1], false, first != 0, x.state);
}

// Commit pass of phase A: every group now holds this call's value.
__global__ void k_le_commit(LightsExt x) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  const int p = le_this_call(x, g);
  *reinterpret_cast<int2*>(x.stored + 2 * (size_t)g) = make_int2(p, -p);
}

// any entry outside [lo, 1] sets *bad (every offender stores the same 1)
__global__ void k_le_check(const int8_t* v, int n, int lo, int* bad) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n && (v[g] < lo || v[g] > 1)) *bad = 1;
}

// Phase B (rl_simple.py:226-252): the controller's timer and phase, apply_phase, then next_state.
__global__ void k_le_act(LightsExt x, const int8_t* __restrict__ actions) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  int phase = x.ctrl[2 * (size_t)g], timer = x.ctrl[2 * (size_t)g + 1] + 1;
  if (timer == 1) {
    int cur = x.gs_cur[g], pend = x.gs_pend[g];
    apply_phase(cur, pend, phase);
    x.gs_pend[g] = pend;
  }
  if (actions[g] == 1 && timer >= x.min_green) { phase = 1 - phase; timer = 0; }
  *reinterpret_cast<int2*>(x.ctrl + 2 * (size_t)g) = make_int2(phase, timer);
  le_vector(x, g, phase, timer, true, false, x.next);
}

// ts_lights_ext_request: apply_phase(phases[g]) where it is 0 or 1
__global__ void k_le_request(LightsExt x, const int8_t* __restrict__ phases) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  const int ph = phases[g];
  if (ph < 0) return;
  int cur = x.gs_cur[g], pend = x.gs_pend[g];
  apply_phase(cur, pend, ph);
  x.gs_pend[g] = pend;
}

}  // namespace
