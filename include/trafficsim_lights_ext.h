/*
 * trafficsim_lights_ext.h - external light control: the environment side of the reference's batched learning controller,
 * on the device.  The per-group state vector, the action protocol, and direct phase requests.
 *
 * An extension of trafficsim.h, implemented by libtrafficsim_hip.so only; the CPU oracle has no external control.
 * Paths are relative to the reference's Simulation/ directory like in trafficsim.h; rl_simple.py stands for
 * utilities/light_group_managment/rl_simple.py, group.py for agents/city_structure_entities/intersection_light_group.py.
 *
 * Algorithm.  Under TS_LIGHTS_EXTERNAL (the reference's "NEIGHBOR_RL_BATCHED") a group's own step() runs no algorithm and
 * goes straight to _execute_phase_change (group.py:396-423); groups still start with pending_phase = 0 (group.py:115-116).
 * Whoever controls the lights calls in between two ts_step calls, on the maps as they stand there, like
 * CityModel.step() does before anything else (city_model.py:1833-1836).  The call runs whether or not a phase change is
 * pending, so its apply_phase can overwrite a pending phase (group.py:391-393), which no in-step algorithm can.
 *
 * What the engine does NOT do: learn.  There is no policy, no train_rl_batch and no reward here.  The reference's reward,
 * -(pressure_ns + pressure_ew) plus optional neighbour means of the same pairs (rl_simple.py:240-248), is identically 0
 * because pressure_ew = -pressure_ns exactly (rl_simple.py:54-55); build one from the state vector or the observation
 * planes (trafficsim_observe.h).
 *
 * Phase A - ts_lights_ext_observe (rl_simple.py:209-216, 95-143): for every group in table order, as float32 [G][dim]:
 *
 *   index  field                                                                      dimensions
 *   0-3    local_ns, local_ew, p_ns = ns - ew, p_ew = -p_ns on occupancy_map          all
 *          (sums over ns_in_coords / ew_in_coords, rl_simple.py:30-60; an empty list sums to 0)
 *   4-5    one-hot of _rl_phase                                                       all
 *   6      rl_timer / 30.0                                                            all
 *   7-8    intersection_size, penalty_score                                           11, 13, 17, 19
 *   9-10   their means over the neighbours                                            11, 13, 17, 19
 *   11-12  mean pressure_ns, pressure_ew of the neighbours                            13, 17, 19
 *   13-16  the four local figures on stuck_map                                        17, 19
 *   17-18  the neighbours' means again (the same stored values as 11-12)              19
 *
 *   - every mean divides by max(1, number of neighbours).
 *   - neighbours are get_neighbor_groups().values() (group.py:293-296): TsLightTables::g_neighbors_ctor until the group's
 *     first executed phase change, g_neighbors after it, slots k = 0..3 in order; an entry without a group (-1) is no
 *     neighbour (none occurs in the reference's worlds).
 *   - the reference builds the vector from Python floats and tf.convert_to_tensor(..., float32) rounds once
 *     (rl_simple.py:219): computed in double here, rounded once.
 *   - the stored pressures.  avg_neighbor_pressures (rl_simple.py:63-78) recomputes nothing for a neighbour that already
 *     has a pressure_ns attribute.  So group i reads from a neighbour j < i what j wrote in this call - its occupancy
 *     pressure up to 13 dimensions, its STUCK-map pressure above, because get_rl_state ends on
 *     compute_pressure(ig, stuck_map) there (rl_simple.py:133-137) - and from a neighbour j > i what the previous call
 *     left.  In the very first call the attribute is absent and is computed from the occupancy map on the spot.  The
 *     pair is dynamic state that persists across ticks (and travels in checkpoints).
 *   - static features (group.py:156-165).  Both are computed by the group's constructor.  intersection_size is
 *     len(intersection_cells) / 16 at that moment, and the model hands the group its cells only afterwards
 *     (city_model.py:1639): it is 0 for every group of the reference, and 0 here.  penalty_score is the mean of the
 *     R1 / R2 / R3 penalties (TsParams::road_type_penalty_r*) over every light's incoming + outgoing blocks, which are
 *     the four coordinate lists of TsLightTables together (duplicates count).  By default the engine takes the blocks'
 *     road types from the world's road_type plane when ts_set_lights runs.  That plane shows an R2 cell of the ring road
 *     as 1 (city_model.py:2170-2172) where the reference's mean reads CellAgent.road_type = "R2": a caller that knows the
 *     cells' own types passes exact values with ts_lights_ext_set_static.  The Python side does so from a per-group count
 *     of R1 / R2 / R3 blocks, which is the reference's double whenever the penalties' partial sums are exact (multiples of a
 *     power of two, like config.py's 0.5 / 5 / 50); with other penalties it may differ from the reference's block-by-block
 *     sum in the last bit.
 *
 * Phase B - ts_lights_ext_act (rl_simple.py:226-252), per group: rl_timer += 1; if rl_timer == 1, apply_phase(_rl_phase);
 * if action == 1 and rl_timer >= min_green (SRL_MIN_GREEN = 5, config.py:377), _rl_phase = 1 - _rl_phase and rl_timer = 0;
 * then next_state = get_rl_state(ig), by which time every neighbour holds this call's value.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_UNSUPPORTED  the handle's algorithm is not TS_LIGHTS_EXTERNAL (every entry).
 *   - TS_E_STATE        ts_set_lights has not run; ts_lights_ext_config / _set_static after the first control call;
 *                       ts_lights_ext_config / _observe / _act once another protocol is configured (trafficsim_lights_proto.h,
 *                       which brings the reference's A2C and GAT-DQN rewards onto the device).
 *   - TS_E_INVALID      a null pointer, a dimension outside {7, 11, 13, 17, 19}, min_green < 0, an action outside {0, 1},
 *                       a requested phase outside {-1, 0, 1}.  Nothing is applied then.
 *
 * Checkpoints (trafficsim_checkpoint.h).  _rl_phase, rl_timer, the stored pressure pair, the "first call done" flag, the
 * observe-before-act state, dimension and min-green are simulation state: a blob written under TS_LIGHTS_EXTERNAL carries
 * them in a trailing section (blobs of every other algorithm are unchanged).  A load onto a handle configured with another
 * dimension or min-green is refused with TS_E_INVALID and leaves the target untouched.
 *
 * Sharded mode (ts_set_replan_sharding): the controller state is replicated; every rank must make the same calls with the
 * same actions.  Nothing is exchanged.
 */
#ifndef TRAFFICSIM_LIGHTS_EXT_H
#define TRAFFICSIM_LIGHTS_EXT_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LIGHTS_EXT_DEFAULT_DIM 13      /* SRL_INPUT_DIMENSIONS (config.py:365) */
#define TS_LIGHTS_EXT_DEFAULT_MIN_GREEN 5 /* SRL_MIN_GREEN (config.py:377) */
#define TS_LIGHTS_EXT_MAX_DIM 19

typedef struct TsLightsExtInfo {
  int32_t state_dim, min_green;
  int32_t n_groups;
  int32_t observed;      /* 1: phase A has run since the last ts_step / ts_lights_ext_act (the state vector is cached) */
  int64_t calls;         /* control calls so far: phase A runs (each ts_lights_ext_act without a cached observe counts once too) */
  uint64_t device_bytes; /* device memory held by the extension */
} TsLightsExtInfo;

/* Device pointers for zero-copy consumers (torch tensors over engine memory).  Owned by the engine, valid until ts_destroy;
 * the contents change with every control call (and `controller` / `stored` with ts_checkpoint_load). */
typedef struct TsLightsExtDevice {
  float* state;        /* [G][state_dim], what the last phase A computed */
  float* next_state;   /* [G][state_dim], what the last ts_lights_ext_act computed */
  int32_t* controller; /* [G][2]: _rl_phase, rl_timer */
  int32_t* stored;     /* [G][2]: pressure_ns, pressure_ew as the last control call left them */
  int32_t n_groups, state_dim;
} TsLightsExtDevice;

/* SRL_INPUT_DIMENSIONS and SRL_MIN_GREEN.  Only before the first control call. */
int ts_lights_ext_config(ts_handle h, int32_t state_dim, int32_t min_green);

/* intersection_size / penalty_score of every group ([G] doubles each; NULL = leave as it is).  Only before the first
 * control call (of any protocol).  Not part of a checkpoint: like the light tables, a load target is set up the same way first. */
int ts_lights_ext_set_static(ts_handle h, const double* intersection_size, const double* penalty_score);

/* Phase A.  out: [G][state_dim] floats or NULL.  A second call before the next ts_lights_ext_act or ts_step returns the
 * cached vector: phase A moves the stored pressures and must not run twice on the same maps. */
int ts_lights_ext_observe(ts_handle h, float* out);

/* Phase B with one action (0 or 1) per group; runs phase A first if it has not run since the last step.  on_device != 0:
 * `actions` is a device pointer (read on the engine's stream).  next_state: [G][state_dim] floats or NULL. */
int ts_lights_ext_act(ts_handle h, const int8_t* actions, int32_t on_device, float* next_state);

/* apply_phase(phase) on every group whose entry is 0 or 1 (-1 = none), for controllers that follow no such protocol.
 * Touches no protocol state (_rl_phase, rl_timer, stored pressures, the cached observe). */
int ts_lights_ext_request(ts_handle h, const int8_t* phases, int32_t on_device);

/* rows: [G][2] = _rl_phase, rl_timer */
int ts_lights_ext_download(ts_handle h, int32_t* rows);

/* Waits for the engine's stream. */
int ts_lights_ext_device(ts_handle h, TsLightsExtDevice* out);

int ts_lights_ext_info(ts_handle h, TsLightsExtInfo* out);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_LIGHTS_EXT_H */
