/*
 * trafficsim_lights_proto.h - external light control, the A2C and GAT-DQN batched protocols: the environment side of the
 * reference's run_a2c_control and run_batched_gat_dqn_control on the device - state, action rule, reward, next state and
 * the epsilon-greedy step.
 *
 * An extension of trafficsim_lights_ext.h, implemented by libtrafficsim_hip.so only, on a handle whose algorithm is
 * TS_LIGHTS_EXTERNAL.  a2c.py stands for utilities/light_group_managment/rl_a2c.py, gat.py for rl_gatdqn.py, group.py for
 * agents/city_structure_entities/intersection_light_group.py.  Under both names ("RL_A2C_BATCHED", "GAT_DQN_BATCHED") a
 * group's own step() decides nothing (group.py:413-420) and the controller is called at the top of CityModel.step()
 * (city_model.py:1839-1848): between two ts_step calls here.
 *
 * The protocol is a property of the extension, chosen once with ts_lights_proto_config before the first control call.
 * Afterwards ts_lights_ext_config / _observe / _act answer TS_E_STATE; ts_lights_ext_request, _download, _set_static and
 * _info keep working (the controller columns _rl_phase / rl_timer are shared).
 *
 * What the engine does NOT do: learn.  update_a2c and _train_dqn (which draws random.sample from the global stream) are the
 * caller's, like train_rl_batch is under the simple protocol.
 *
 * Common rules (a2c.py:135-146, gat.py:297-303), per group in table order: rl_timer += 1; if it is 1,
 * apply_phase(_rl_phase) - which may overwrite a pending phase; if action == 1 and rl_timer >= min_green, _rl_phase flips
 * and rl_timer = 0.  min_green is 5 under both (A2C reads TRAFFIC_LIGHT_MIN_GREEN, which config.py does not define, and
 * gets its getattr default; GAT reads GAT_TRAFFIC_RL_MIN_GREEN = 5).  t_norm = rl_timer / 30.  Neighbours, intersection_size
 * (0 for every group) and penalty_score as in trafficsim_lights_ext.h.  Vectors are built in doubles and rounded to float32
 * once.
 *
 * A2C state [G][13] (a2c.py:41-70):
 *   0-3   local_ns, local_ew, p_ns, p_ew on occupancy_map
 *   4-5   means of the neighbours' _pressure_ns / _pressure_ew: nothing in the reference sets these attributes - 0
 *   6-7   one-hot of _rl_phase
 *   8     t_norm
 *   9-10  intersection_size, penalty_score
 *   11    mean of the neighbours' intersection_size_factor: never set either - 0
 *   12    sum of the neighbours' penalty_score / max(1, neighbours)
 * A2C reward after the action (a2c.py:149-163): -(double)((ns + ew) + 0.25 * (ns - ew)^2).  The reference samples the
 * action from TensorFlow's own generator: the caller supplies actions, no stream of the engine moves, and the protocol has
 * no next state.
 *
 * GAT-DQN state [G][5][9] with mask [G][5] (gat.py:105-173).  Node 0 is the group: ns, ew, p_ns, p_ew, phase one-hot,
 * t_norm, intersection_size, penalty_score.  Nodes 1-4 are the neighbours in the fixed order N, S, E, W, found by the
 * direction code of the table entry (TsLightTables: N 0, E 1, S 2, W 3), not by slot, each with the same nine figures
 * computed for the neighbour - except that its t_norm reads `_rl_timer`, which nothing sets: 0.  An absent direction is
 * nine zeros with mask 0.  mask = [1, m_N, m_S, m_E, m_W].
 *
 * GAT-DQN step (gat.py:283-331), per group i in table order:
 *   1. u = random.random() on the GLOBAL stream (TS_RNG_GLOBAL);
 *   2. u < epsilon_i: action = random.randrange(2), i.e. getrandbits(2) redrawn while >= 2; else argmax(q_i), a tie is 0;
 *   3. epsilon_i = max(eps_min, epsilon_i - eps_decay) in doubles; every group starts at 1.0 (group.py:102);
 *   4. the common action rule;
 *   5. reward = -((double)(ns + ew) + (0.01 * avg_dur + 1.0 * avg_tpb)), avg_dur = 0.5 * (avg_duration_internal +
 *      avg_duration_through), avg_tpb = 0.5 * (avg_time_per_unit_internal + avg_time_per_unit_through) of the traffic
 *      generator's cached_stats as they stand at the call (TsCachedStats, the "total" quotients; 0 before the first update
 *      and without a generator);
 *   6. next_state = get_gat_state(ig) INSIDE the loop: a neighbour j < i shows its post-action phase, a neighbour j > i its
 *      pre-action phase, the centre its own post-action phase and timer.
 * The draws move everything the run computes afterwards.  ts_lights_proto_act (caller-chosen actions) draws nothing and
 * leaves epsilon alone.
 *
 * Calls: only between ts_step calls, from the handle's caller thread.
 *   TS_E_UNSUPPORTED  the handle's algorithm is not TS_LIGHTS_EXTERNAL (every entry).
 *   TS_E_STATE        ts_set_lights has not run; ts_lights_proto_config after the first control call of either protocol or
 *                     a second time; any other entry before ts_lights_proto_config; ts_lights_proto_act_q under A2C.
 *   TS_E_INVALID      a null pointer, an unknown protocol, min_green < 0, eps outside [0, 1] or a negative / non-finite
 *                     decay, an action outside {0, 1}, a non-finite q, a non-NULL next_state under A2C.
 * A refused call changes nothing (and draws nothing).
 *
 * Checkpoints: protocol, configuration, per-group epsilon and the call count travel in a second trailing section behind the
 * one of trafficsim_lights_ext.h, written only once a protocol is configured: every other blob is byte for byte what it
 * was.  A load onto a handle with another protocol or configuration (or none) is TS_E_INVALID and leaves the target
 * untouched.
 *
 * Sharded mode: like trafficsim_lights_ext.h, every rank makes the same calls; the ranks' global streams stay in step
 * because they draw the same words.
 */
#ifndef TRAFFICSIM_LIGHTS_PROTO_H
#define TRAFFICSIM_LIGHTS_PROTO_H

#include "trafficsim_lights_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LP_A2C 1
#define TS_LP_GAT 2
#define TS_LP_A2C_DIM 13
#define TS_LP_GAT_NODES 5
#define TS_LP_GAT_FEATURES 9
#define TS_LP_DEFAULT_MIN_GREEN 5   /* GAT_TRAFFIC_RL_MIN_GREEN; getattr(Defaults, "TRAFFIC_LIGHT_MIN_GREEN", 5) */
#define TS_LP_DEFAULT_EPS_MIN 0.1   /* EPS_MIN (config.py:399) */
#define TS_LP_DEFAULT_EPS_DECAY 1e-5 /* EPS_DECAY_RATE (config.py:400) */

typedef struct TsLightsProtoConfig {
  int32_t protocol;  /* TS_LP_A2C or TS_LP_GAT */
  int32_t min_green;
  double eps_min, eps_decay; /* GAT only; ignored (and stored as given) under A2C */
} TsLightsProtoConfig;

typedef struct TsLightsProtoInfo {
  int32_t protocol, min_green; /* protocol 0: none configured */
  int32_t n_groups, state_floats; /* floats per group of a state: 13 or 45 */
  double eps_min, eps_decay;
  int64_t calls;         /* ts_lights_proto_act / _act_q calls so far */
  uint64_t device_bytes; /* device memory the protocol's arrays hold */
} TsLightsProtoInfo;

/* Device pointers for zero-copy consumers.  Owned by the engine, valid until ts_destroy; rewritten by the calls named. */
typedef struct TsLightsProtoDevice {
  float* state;      /* [G][13] or [G][5][9]: ts_lights_proto_observe */
  float* mask;       /* [G][5] (GAT; NULL under A2C): ts_lights_proto_observe */
  float* next_state; /* [G][5][9] (GAT; NULL under A2C): ts_lights_proto_act / _act_q */
  double* reward;    /* [G]: ts_lights_proto_act / _act_q */
  int8_t* actions;   /* [G] the actions the last act / act_q applied */
  double* epsilon;   /* [G] (GAT; NULL under A2C) */
  int32_t n_groups, protocol;
} TsLightsProtoDevice;

/* Only once, before the first control call of either protocol. */
int ts_lights_proto_config(ts_handle h, const TsLightsProtoConfig* cfg);

/* state: [G][13] (A2C) or [G][5][9] (GAT) floats or NULL; mask: [G][5] floats or NULL (must be NULL under A2C).  No side
 * effects: nothing is stored, it may be called any number of times. */
int ts_lights_proto_observe(ts_handle h, float* state, float* mask);

/* The action rule with caller-chosen actions under either protocol.  reward: [G] doubles or NULL; next_state: [G][5][9]
 * floats or NULL, must be NULL under A2C.  on_device != 0: `actions` is a device pointer. */
int ts_lights_proto_act(ts_handle h, const int8_t* actions, int32_t on_device, double* reward, float* next_state);

/* GAT only: the epsilon-greedy step on q [G][2] (on_device != 0: a device pointer).  actions_out: [G] bytes or NULL. */
int ts_lights_proto_act_q(ts_handle h, const float* q, int32_t on_device, int8_t* actions_out, double* reward, float* next_state);

/* epsilon: [G] doubles (GAT; zeros under A2C) */
int ts_lights_proto_download(ts_handle h, double* epsilon);

/* Waits for the engine's stream. */
int ts_lights_proto_device(ts_handle h, TsLightsProtoDevice* out);

/* Works before ts_lights_proto_config too (protocol 0). */
int ts_lights_proto_info(ts_handle h, TsLightsProtoInfo* out);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_LIGHTS_PROTO_H */
