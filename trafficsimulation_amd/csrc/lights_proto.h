// lights_proto.h - kernels of the A2C and GAT-DQN batched light protocols (include/trafficsim_lights_proto.h has the semantics
// and the reference lines): the A2C vector, the graph state with its direction look-up, the action step with both rewards,
// the next graph state and the greedy byte of a q row.  Host side: lights_proto_api.h.  Part of the single translation unit
// engine.hip.  The per-group sums are k_le_sums' (lights_ext.h).
//
// Like lights_ext.h: no atomics, one writer per output word, results independent of the launch geometry.
#pragma once

namespace {

struct LightsProto {
  LightsExt x;           // the tables, the sums, the shared controller columns and the static features (lights_ext.h)
  int protocol, min_green;
  float *state, *mask, *next;   // [G][13] or [G][5][9]; [G][5]; [G][5][9]
  double* reward;        // [G]
  int32_t* prev_phase;   // [G] _rl_phase as it was before the last action step
  int8_t* applied;       // [G] the actions of the last action step
  uint8_t* greedy;       // [G] argmax of a q row (a tie is 0); 2 = the row is not finite
};

// the table a group's get_neighbor_groups() reads (group.py:293-296)
__device__ __forceinline__ const int32_t* lp_nb(const LightsExt& x, int g) { return (x.repop[g] ? x.nb : x.nb_ctor) + (size_t)g * 8; }

// get_rl_state of rl_a2c.py:41-70
__global__ void k_lp_a2c_state(LightsProto p) {
  const LightsExt& x = p.x;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  const int4 s = *reinterpret_cast<const int4*>(x.sums + 4 * (size_t)g);
  const int32_t* nb = lp_nb(x, g);
  int cnt = 0;
  double pen_sum = 0.0;
  for (int k = 0; k < 4; k++) {
    const int nd = nb[2 * k], n = nb[2 * k + 1];
    if (nd < 0 || n < 0) continue;
    cnt++;
    pen_sum += x.pen[n];
  }
  const int phase = x.ctrl[2 * (size_t)g], timer = x.ctrl[2 * (size_t)g + 1];
  float* o = p.state + (size_t)g * 13;
  o[0] = (float)s.x; o[1] = (float)s.y; o[2] = (float)(s.x - s.y); o[3] = (float)(s.y - s.x);
  o[4] = 0.f; o[5] = 0.f;   // _pressure_ns / _pressure_ew: attributes nothing sets
  o[6] = phase == 0 ? 1.f : 0.f; o[7] = phase == 0 ? 0.f : 1.f;
  o[8] = (float)((double)timer / 30.0);
  o[9] = (float)x.size[g]; o[10] = (float)x.pen[g];
  o[11] = 0.f;              // intersection_size_factor: never set
  o[12] = (float)(pen_sum / (double)max(cnt, 1));
}

// the nine figures of one node (rl_gatdqn.py:128-134, 158-164)
__device__ __forceinline__ void lp_node(const LightsExt& x, int j, int phase, double t_norm, float* o) {
  const int ns = x.sums[4 * (size_t)j], ew = x.sums[4 * (size_t)j + 1];
  o[0] = (float)ns; o[1] = (float)ew; o[2] = (float)(ns - ew); o[3] = (float)(ew - ns);
  o[4] = phase == 0 ? 1.f : 0.f; o[5] = phase == 0 ? 0.f : 1.f;
  o[6] = (float)t_norm;
  o[7] = (float)x.size[j]; o[8] = (float)x.pen[j];
}

// get_gat_state (rl_gatdqn.py:105-173) of group g whose own controller state is (phase, timer).  after: the call comes from
// inside the action loop, so a neighbour j < g shows its new phase and j > g the one it had before the step.
__device__ __forceinline__ void lp_graph(const LightsProto& p, int g, int phase, int timer, bool after, float* feat, float* mask) {
  const LightsExt& x = p.x;
  float* o = feat + (size_t)g * 45;
  lp_node(x, g, phase, (double)timer / 30.0, o);
  const int32_t* nb = lp_nb(x, g);
  const int order[4] = {0, 2, 1, 3};   // N, S, E, W as direction codes
  if (mask) mask[(size_t)g * 5] = 1.f;
  for (int d = 0; d < 4; d++) {
    int n = -1;
    for (int k = 0; k < 4; k++)
      if (nb[2 * k] == order[d] && nb[2 * k + 1] >= 0) n = nb[2 * k + 1];   // (dict semantics: a later entry of the same key wins)
    float* q = o + 9 * (d + 1);
    if (n < 0) {
#pragma unroll
      for (int c = 0; c < 9; c++) q[c] = 0.f;
    } else {
      const int ph = (after && n > g) ? p.prev_phase[n] : x.ctrl[2 * (size_t)n];
      lp_node(x, n, ph, 0.0, q);   // (`_rl_timer`: an attribute nothing sets)
    }
    if (mask) mask[(size_t)g * 5 + d + 1] = n < 0 ? 0.f : 1.f;
  }
}

__global__ void k_lp_gat_state(LightsProto p) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.x.G) return;
  lp_graph(p, g, p.x.ctrl[2 * (size_t)g], p.x.ctrl[2 * (size_t)g + 1], false, p.state, p.mask);
}

// The action step of both protocols (rl_a2c.py:135-163, rl_gatdqn.py:297-320): timer, apply_phase, toggle, reward.  The phase a
// group had before is kept beside the new one for k_lp_gat_next.
__global__ void k_lp_act(LightsProto p, const int8_t* __restrict__ actions, double global_term) {
  const LightsExt& x = p.x;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= x.G) return;
  int phase = x.ctrl[2 * (size_t)g], timer = x.ctrl[2 * (size_t)g + 1] + 1;
  p.prev_phase[g] = phase;
  if (timer == 1) {
    int cur = x.gs_cur[g], pend = x.gs_pend[g];
    apply_phase(cur, pend, phase);
    x.gs_pend[g] = pend;
  }
  const int8_t a = actions[g];
  if (a == 1 && timer >= p.min_green) { phase = 1 - phase; timer = 0; }
  *reinterpret_cast<int2*>(x.ctrl + 2 * (size_t)g) = make_int2(phase, timer);
  p.applied[g] = a;
  const long long ns = x.sums[4 * (size_t)g], ew = x.sums[4 * (size_t)g + 1];
  if (p.protocol == 1) p.reward[g] = -((double)(ns + ew) + 0.25 * (double)((ns - ew) * (ns - ew)));
  else p.reward[g] = -((double)(ns + ew) + global_term);
}

// next_state of the GAT step: after k_lp_act, so both phase columns exist and the pass stays parallel
__global__ void k_lp_gat_next(LightsProto p) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.x.G) return;
  lp_graph(p, g, p.x.ctrl[2 * (size_t)g], p.x.ctrl[2 * (size_t)g + 1], true, p.next, nullptr);
}

// np.argmax of a q row (the first maximum: a tie is 0); 2 marks a row with a NaN or an infinity
__global__ void k_lp_greedy(const float* __restrict__ q, int G, uint8_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const float q0 = q[2 * (size_t)g], q1 = q[2 * (size_t)g + 1];
  out[g] = (isfinite(q0) && isfinite(q1)) ? (q1 > q0 ? 1 : 0) : 2;
}

}  // namespace
