// lights_proto_api.h - the ts_lights_proto_* entries (include/trafficsim_lights_proto.h): the host side of the A2C and GAT-DQN
// protocols whose kernels are in lights_proto.h.  Part of the single translation unit engine.hip (included at its end).
//
// The epsilon-greedy draw chain is sequential and data dependent (two words per group, more when randrange rejects), so it runs
// where the engine keeps the global stream: on the host.  k_lp_greedy reduces q to one byte per group, G bytes come down, the
// chosen actions go up.
#pragma once
#include "../../include/trafficsim_lights_proto.h"

static_assert(sizeof(TsLightsProtoConfig) == 24 && sizeof(TsLightsProtoInfo) == 48 && sizeof(TsLightsProtoDevice) == 56,
              "lights_proto structs as the Python binding declares them");

namespace {

int lp_enter(E* e, bool need_protocol) {
  TRY(le_enter(e));
  if (need_protocol && !e->lp.protocol) return fail(e, TS_E_STATE, "lights_proto: ts_lights_proto_config has not run");
  e->lp.p.x = e->le.x;
  return TS_OK;
}

int lp_floats(const E* e) { return e->lp.protocol == TS_LP_GAT ? TS_LP_GAT_NODES * TS_LP_GAT_FEATURES : TS_LP_A2C_DIM; }

// 0.01 * avg_trip_duration + 1.0 * avg_time_per_block of the generator's cached_stats (rl_gatdqn.py:311-318; the "total"
// quotients of dynamic_traffic_generator.py:580-605)
double lp_global_term(const E* e) {
  const TsCachedStats& c = e->gen.cs;
  if (!c.valid) return 0.0;
  auto safe = [](double a, double b) { return b != 0.0 ? a / b : 0.0; };
  double dur[2], tpu[2];
  for (int k = 0; k < 2; k++) {
    dur[k] = safe(c.total_duration[k] + c.dur_live[k], (double)(c.count_completed[k] + c.n_live[k]));
    tpu[k] = safe(c.total_duration[k] + c.dur_live[k], (double)(c.total_distance[k] + c.dist_live[k]));
  }
  const double avg_dur = 0.5 * (dur[0] + dur[1]), avg_tpb = 0.5 * (tpu[0] + tpu[1]);
  return 0.01 * avg_dur + 1.0 * avg_tpb;
}

// the action step on device actions `dev`, then the outputs
int lp_step(E* e, const int8_t* dev, double* reward, float* next_state) {
  const LightsProto& p = e->lp.p;
  const int G = p.x.G, gb = e->le.gblock;
  TRY(le_sums(e));
  hipLaunchKernelGGL(k_lp_act, dim3(le_grid(e, gb)), dim3(gb), 0, e->stream, p, dev, e->lp.protocol == TS_LP_GAT ? lp_global_term(e) : 0.0);
  if (e->lp.protocol == TS_LP_GAT) hipLaunchKernelGGL(k_lp_gat_next, dim3(le_grid(e, gb)), dim3(gb), 0, e->stream, p);
  HIPOK(hipGetLastError());
  e->lp.calls++;
  if (reward && G) HIPOK(hipMemcpyAsync(reward, p.reward, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (next_state && G) HIPOK(hipMemcpyAsync(next_state, p.next, (size_t)G * 45 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

}  // namespace

extern "C" {

int ts_lights_proto_config(ts_handle e, const TsLightsProtoConfig* cfg) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, false));
  if (!cfg) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  if (cfg->protocol != TS_LP_A2C && cfg->protocol != TS_LP_GAT) return fail(e, TS_E_INVALID, "lights_proto: protocol must be TS_LP_A2C or TS_LP_GAT");
  if (cfg->min_green < 0 || !(cfg->eps_min >= 0.0 && cfg->eps_min <= 1.0) || !(cfg->eps_decay >= 0.0) || !std::isfinite(cfg->eps_decay))
    return fail(e, TS_E_INVALID, "lights_proto: min_green >= 0, eps_min in [0, 1] and a finite eps_decay >= 0");
  if (e->lp.protocol) return fail(e, TS_E_STATE, "lights_proto: a protocol is already configured");
  if (e->le.calls > 0) return fail(e, TS_E_STATE, "lights_proto: configure before the first control call");
  LightsProto& p = e->lp.p;
  const size_t G = (size_t)p.x.G;
  const bool gat = cfg->protocol == TS_LP_GAT;
  const size_t fl = gat ? 45 : 13;
  HIPOK(dalloc(e, &p.state, G * fl)); HIPOK(dalloc(e, &p.reward, G)); HIPOK(dalloc(e, &p.prev_phase, G)); HIPOK(dalloc(e, &p.applied, G));
  uint64_t bytes = G * (fl * 4 + 8 + 4 + 1);
  if (gat) {
    HIPOK(dalloc(e, &p.mask, G * 5)); HIPOK(dalloc(e, &p.next, G * 45)); HIPOK(dalloc(e, &p.greedy, G));
    HIPOK(dalloc(e, &e->lp.d_eps, G)); HIPOK(dalloc(e, &e->lp.q_stage, G * 2));
    bytes += G * (20 + 180 + 1 + 8 + 8);
  }
  e->lp.eps.assign(G, gat ? 1.0 : 0.0);   // (intersection_light_group.py:102)
  if (G) {
    HIPOK(hipMemsetAsync(p.state, 0, G * fl * 4, e->stream)); HIPOK(hipMemsetAsync(p.reward, 0, G * 8, e->stream));
    HIPOK(hipMemsetAsync(p.prev_phase, 0, G * 4, e->stream)); HIPOK(hipMemsetAsync(p.applied, 0, G, e->stream));
    if (gat) {
      HIPOK(hipMemsetAsync(p.mask, 0, G * 20, e->stream)); HIPOK(hipMemsetAsync(p.next, 0, G * 180, e->stream));
      HIPOK(hipMemcpyAsync(e->lp.d_eps, e->lp.eps.data(), G * 8, hipMemcpyHostToDevice, e->stream));
    }
    HIPOK(hipStreamSynchronize(e->stream));
  }
  e->lp.h_greedy.assign(G, 0); e->lp.h_act.assign(G, 0);
  e->lp.bytes = bytes;
  e->lp.protocol = p.protocol = cfg->protocol;
  e->lp.min_green = p.min_green = cfg->min_green;
  e->lp.eps_min = cfg->eps_min; e->lp.eps_decay = cfg->eps_decay;
  e->lp.calls = 0;
  return TS_OK;
}

int ts_lights_proto_observe(ts_handle e, float* state, float* mask) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, true));
  const LightsProto& p = e->lp.p;
  const bool gat = e->lp.protocol == TS_LP_GAT;
  if (mask && !gat) return fail(e, TS_E_INVALID, "lights_proto: the A2C protocol has no mask");
  const int G = p.x.G, gb = e->le.gblock;
  TRY(le_sums(e));
  if (gat) hipLaunchKernelGGL(k_lp_gat_state, dim3(le_grid(e, gb)), dim3(gb), 0, e->stream, p);
  else hipLaunchKernelGGL(k_lp_a2c_state, dim3(le_grid(e, gb)), dim3(gb), 0, e->stream, p);
  HIPOK(hipGetLastError());
  if (state && G) HIPOK(hipMemcpyAsync(state, p.state, (size_t)G * lp_floats(e) * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (mask && G) HIPOK(hipMemcpyAsync(mask, p.mask, (size_t)G * 5 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  return TS_OK;
}

int ts_lights_proto_act(ts_handle e, const int8_t* actions, int32_t on_device, double* reward, float* next_state) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, true));
  if (!actions) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  if (next_state && e->lp.protocol != TS_LP_GAT) return fail(e, TS_E_INVALID, "lights_proto: the A2C protocol has no next state");
  const int8_t* dev = nullptr;
  TRY(le_bytes(e, actions, on_device, 0, "an action", &dev));
  return lp_step(e, dev, reward, next_state);
}

int ts_lights_proto_act_q(ts_handle e, const float* q, int32_t on_device, int8_t* actions_out, double* reward, float* next_state) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, true));
  if (e->lp.protocol != TS_LP_GAT) return fail(e, TS_E_STATE, "lights_proto: the epsilon-greedy step belongs to the GAT protocol");
  if (!q) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  const LightsProto& p = e->lp.p;
  const int G = p.x.G, gb = e->le.gblock;
  auto& lp = e->lp;
  const float* dq = q;
  if (!on_device) {
    if (G) HIPOK(hipMemcpyAsync(lp.q_stage, q, (size_t)G * 2 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    dq = lp.q_stage;
  }
  hipLaunchKernelGGL(k_lp_greedy, dim3(le_grid(e, gb)), dim3(gb), 0, e->stream, dq, G, p.greedy);
  HIPOK(hipGetLastError());
  if (G) HIPOK(hipMemcpyAsync(lp.h_greedy.data(), p.greedy, (size_t)G, hipMemcpyDeviceToHost, e->stream));
  HIPOK(hipStreamSynchronize(e->stream));
  for (int g = 0; g < G; g++) if (lp.h_greedy[g] > 1) return fail(e, TS_E_INVALID, "lights_proto: a q-value is not finite");
  if (!e->rng_global.seeded()) return fail(e, TS_E_STATE, "lights_proto: seed the global RNG stream first");
  // rl_gatdqn.py:289-295, groups in table order
  for (int g = 0; g < G; g++) {
    const double u = e->rng_global.random();
    lp.h_act[g] = u < lp.eps[g] ? (int8_t)e->rng_global.randbelow(2) : (int8_t)lp.h_greedy[g];
    lp.eps[g] = std::max(lp.eps_min, lp.eps[g] - lp.eps_decay);
  }
  if (G) {
    HIPOK(hipMemcpyAsync(e->le.stage, lp.h_act.data(), (size_t)G, hipMemcpyHostToDevice, e->stream));
    HIPOK(hipMemcpyAsync(lp.d_eps, lp.eps.data(), (size_t)G * 8, hipMemcpyHostToDevice, e->stream));
  }
  TRY(lp_step(e, e->le.stage, reward, next_state));
  if (actions_out && G) memcpy(actions_out, lp.h_act.data(), (size_t)G);
  return TS_OK;
}

int ts_lights_proto_download(ts_handle e, double* epsilon) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, true));
  if (!epsilon) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  if (!e->lp.eps.empty()) memcpy(epsilon, e->lp.eps.data(), e->lp.eps.size() * sizeof(double));
  return TS_OK;
}

int ts_lights_proto_device(ts_handle e, TsLightsProtoDevice* out) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, true));
  if (!out) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  HIPOK(hipStreamSynchronize(e->stream));
  const LightsProto& p = e->lp.p;
  out->state = p.state; out->mask = p.mask; out->next_state = p.next; out->reward = p.reward; out->actions = p.applied;
  out->epsilon = e->lp.d_eps;
  out->n_groups = p.x.G; out->protocol = e->lp.protocol;
  return TS_OK;
}

int ts_lights_proto_info(ts_handle e, TsLightsProtoInfo* out) {
  if (!e) return TS_E_INVALID;
  TRY(lp_enter(e, false));
  if (!out) return fail(e, TS_E_INVALID, "lights_proto: null pointer");
  out->protocol = e->lp.protocol; out->min_green = e->lp.min_green;
  out->n_groups = e->le.x.G; out->state_floats = e->lp.protocol ? lp_floats(e) : 0;
  out->eps_min = e->lp.eps_min; out->eps_decay = e->lp.eps_decay;
  out->calls = e->lp.calls; out->device_bytes = e->lp.bytes;
  return TS_OK;
}

}  // extern "C"
