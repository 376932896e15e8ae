"""ctypes binding of the C-ABI declared in include/trafficsim.h.

`CApi(lib, prefix)` wraps one shared library exporting `<prefix>create`, `<prefix>step`, ...
The product uses `prefix="ts_"` with trafficsimulation_amd/csrc/libtrafficsim_hip.so (see
`_lib.py`); tests additionally instantiate it over the CPU oracle (`tso_`, oracle/libtso.so) so
that both sides of a parity check are driven through identical host code.
"""
from __future__ import annotations

import ctypes as C
import zlib
from typing import Dict, Optional, Sequence

import numpy as np

# ---- enums (mirror include/trafficsim.h) ----------------------------------------------------
TS_OK, TS_E_INVALID, TS_E_STATE, TS_E_DEVICE, TS_E_UNSUPPORTED, TS_E_CAPACITY = 0, -1, -2, -3, -4, -5
LIGHT_ALGORITHMS = {
    "DISABLED": 0, "FIXED_TIME": 1, "QUEUE_ACTUATED": 2, "PRESSURE_CONTROL": 3,
    "NEIGHBOR_PRESSURE_CONTROL": 4, "NEIGHBOR_GREEN_WAVE": 5,
    # external control (include/trafficsim_lights_ext.h): the groups decide nothing in their own step(); the reference's name
    # for it is its batched learning controller, whose environment side this is
    "EXTERNAL": 6, "NEIGHBOR_RL_BATCHED": 6,
}
LIGHTS_EXT_DIMS = (7, 11, 13, 17, 19)
M_FIELDS = ["spawn_idx", "population", "target_x", "target_y", "vehicle_type", "service_phase"]
TRIP_SERVICE_FOOD, TRIP_SERVICE_WASTE = 3, 4
AGENT_LIGHT_GROUP, AGENT_NOOP, AGENT_RAIN_MANAGER, AGENT_CLOCK, AGENT_CITY_BLOCK = 0, 1, 2, 3, 6
MAP_OCCUPANCY, MAP_STOP, MAP_STUCK, MAP_RAIN = 0, 1, 2, 3
RNG_GLOBAL, RNG_SCHEDULER = 0, 1
POP = {"undefined": 0, "internal": 1, "through": 2}
V_FIELDS = ["spawn_idx", "x", "y", "base_speed", "current_speed", "max_steps", "direction", "stuck_ticks",
            "cooldown", "flags", "stranded_left", "steps_traveled", "path_len", "path_crc", "overtake_dur",
            "detour_dur"]
G_FIELDS = ["current_phase", "pending_phase", "queue_timer", "gap_timer", "last_arrival", "fixed_time_timer",
            "ft_phase", "ns_pressure", "ew_pressure"]
F_EARLY_EXIT, F_STUCK, F_PARKED, F_COLLISION, F_MALFUNCTION, F_OVERTAKING, F_DETOUR, F_BLOCKED, F_HAS_PREV = (
    1 << i for i in range(9))


class TsParams(C.Structure):
    _fields_ = [
        ("vehicle_min_speed", C.c_int32), ("vehicle_max_speed", C.c_int32),
        ("vehicle_awareness_range", C.c_int32), ("rain_enabled", C.c_int32),
        ("rain_speed_reduction", C.c_int32), ("pathfinding_cooldown", C.c_int32),
        ("pathfinding_cache", C.c_int32), ("stuck_recompute_threshold", C.c_int32),
        ("stuck_recompute_threshold_intersection", C.c_int32), ("contraflow_overtake_active", C.c_int32),
        ("max_contraflow_overtake_steps", C.c_int32), ("contraflow_overtake_duration", C.c_int32),
        ("stuck_contraflow_enabled", C.c_int32), ("stuck_contraflow_threshold", C.c_int32),
        ("stuck_contraflow_threshold_intersection", C.c_int32), ("max_contraflow_stuck_detour_steps", C.c_int32),
        ("contraflow_stuck_detour_duration", C.c_int32), ("malfunction_active", C.c_int32),
        ("malfunction_duration", C.c_int32), ("sideswipe_active", C.c_int32), ("sideswipe_duration", C.c_int32),
        ("malfunction_chance", C.c_double), ("sideswipe_chance", C.c_double),
        ("contraflow_penalty", C.c_int32), ("obstacle_penalty_vehicle", C.c_int32),
        ("obstacle_penalty_stop", C.c_int32), ("road_type_penalties_enabled", C.c_int32),
        ("turn_penalty_enabled", C.c_int32), ("turn_penalty", C.c_int32),
        ("dynamic_penalties_enabled", C.c_int32), ("_pad0", C.c_int32),
        ("road_type_penalty_r1", C.c_double), ("road_type_penalty_r2", C.c_double),
        ("road_type_penalty_r3", C.c_double), ("dynamic_penalty_scale", C.c_double),
        ("light_algorithm", C.c_int32), ("transition_duration_enabled", C.c_int32),
        ("transition_clearance_enabled", C.c_int32), ("all_red_duration", C.c_int32),
        ("green_duration", C.c_int32), ("qa_min_green", C.c_int32), ("qa_max_green", C.c_int32),
        ("qa_gap", C.c_int32), ("enable_traffic", C.c_int32), ("time_per_step_seconds", C.c_int32),
        ("eager_density", C.c_int32), ("rain_radius_min", C.c_int32), ("rain_radius_max", C.c_int32),
        ("rain_occurrences_max", C.c_int32), ("rain_cooldown", C.c_int32), ("rain_spawn_offset", C.c_int32),
        ("rain_spawn_chance", C.c_double),
        ("stuck_despawn_enabled", C.c_int32), ("stuck_despawn_threshold", C.c_int32),
        ("stuck_despawn_threshold_intersection", C.c_int32), ("respect_awareness", C.c_int32),
        ("pathfinding_batching", C.c_int32),
    ]


class TsWorld(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("allowed_dirs_map", C.c_void_p),
                ("is_road_map", C.c_void_p), ("road_type_map", C.c_void_p), ("intersection_map", C.c_void_p)]


_LT_PTRS = ["g_light_off", "light_xy", "light_ctrl_off", "light_ctrl_xy", "g_ns_off", "g_ns", "g_ew_off", "g_ew",
            "g_icell_off", "g_icell_xy", "g_ns_in_off", "g_ns_in_xy", "g_ns_out_off", "g_ns_out_xy",
            "g_ew_in_off", "g_ew_in_xy", "g_ew_out_off", "g_ew_out_xy", "g_neighbors", "g_neighbors_ctor"]


class TsLightTables(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("n_lights", C.c_int32)] + [(n, C.c_void_p) for n in _LT_PTRS]


class TsRainInfo(C.Structure):
    _fields_ = [("has_manager", C.c_int32), ("n_rains", C.c_int32), ("cooldown", C.c_int32), ("counter", C.c_int32)]


# include/trafficsim_observe.h: plane indices and the fields of ts_observe_groups
OBS_PLANES = ["present", "waiting", "speed", "enter_n", "enter_e", "enter_s", "enter_w"]
OBS_ENTER = OBS_PLANES[3:]
OG_FIELDS = ["ns_waiting", "ns_present", "ew_waiting", "ew_present", "enter_n", "enter_e", "enter_s", "enter_w"]


# include/trafficsim_render.h: the TS_RL_* layer bits (bit k = RENDER_LAYERS[k]), limits, TsRenderView, TsRenderInfo
RENDER_LAYERS = ["signals", "rain", "vehicles", "heat", "routes"]
RL_SIGNALS, RL_RAIN, RL_VEHICLES, RL_HEAT, RL_ROUTES = (1 << k for k in range(5))
RL_ALL = 31
RENDER_MAX_TYPES, RENDER_MAX_ROUTES, RENDER_MAX_SCALE, RENDER_MAX_SIDE, RENDER_DEFAULT_RADIUS = 64, 4096, 64, 8192, 169


class TsRenderView(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("cells_w", C.c_int32), ("cells_h", C.c_int32), ("zoom", C.c_int32),
                ("shrink", C.c_int32), ("layers", C.c_uint32), ("flip_y", C.c_int32), ("heat_plane", C.c_int32),
                ("heat_max", C.c_uint32), ("vehicle_radius_256", C.c_int32), ("background", C.c_uint8 * 4)]


class TsRenderInfo(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("has_vehicle_palette", C.c_int32), ("has_heat_lut", C.c_int32), ("n_routes", C.c_int32),
                ("last_w", C.c_int32), ("last_h", C.c_int32), ("frames", C.c_int64), ("device_bytes", C.c_uint64)]


def render_layer_mask(layers) -> int:
    """A TS_RL_* mask from None (signals, rain and vehicles), a ready mask, one name or names of RENDER_LAYERS."""
    if layers is None:
        return RL_SIGNALS | RL_RAIN | RL_VEHICLES
    if isinstance(layers, (int, np.integer)):
        return int(layers)
    mask = 0
    for name in ([layers] if isinstance(layers, str) else layers):
        if name not in RENDER_LAYERS:
            raise ValueError(f"unknown render layer {name!r} (one of {', '.join(RENDER_LAYERS)})")
        mask |= 1 << RENDER_LAYERS.index(name)
    return mask


class TsObserveInfo(C.Structure):
    _fields_ = [("plane_mask", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("ticks", C.c_int64),
                ("device_bytes", C.c_uint64)]


# include/trafficsim_demand.h: the fields of ts_demand_groups, TsDemandQuery, TsDemandInfo
DEMAND_MAX_BINS = 8
DG_FIELDS = ["ns_in", "ew_in", "enter_n", "enter_e", "enter_s", "enter_w"]


class TsDemandQuery(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("bin_cells", C.c_int32), ("open_tail", C.c_int32), ("n_select", C.c_int32),
                ("select_on_device", C.c_int32), ("reserved", C.c_int32), ("select", C.c_void_p)]


class TsDemandInfo(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("bin_cells", C.c_int32), ("open_tail", C.c_int32), ("selected", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("tick", C.c_int64), ("vehicles", C.c_int64),
                ("steps", C.c_uint64), ("bin_steps", C.c_uint64 * 8), ("device_bytes", C.c_uint64)]


# include/trafficsim_triplog.h: TsTripRecord as a numpy record, the TS_TRIP_END_* codes, TsTripLogInfo
TRIP_DTYPE = np.dtype([(n, np.int32) for n in (
    "spawn_idx", "population", "vehicle_type", "end_reason", "origin_x", "origin_y", "dest_x", "dest_y", "end_x", "end_y",
    "spawn_step", "end_step", "distance", "stuck_ticks")] + [("depart_elapsed", np.float64), ("end_elapsed", np.float64)])
assert TRIP_DTYPE.itemsize == 72
TRIP_END = {"arrived": 0, "despawned": 1, "removed": 2}
TRIPLOG_MAX_ZONES = 1024


class TsTripLogInfo(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("count", C.c_int64), ("dropped", C.c_int64), ("groups", C.c_int64),
                ("device_bytes", C.c_uint64)]


class TsLightsExtInfo(C.Structure):
    _fields_ = [("state_dim", C.c_int32), ("min_green", C.c_int32), ("n_groups", C.c_int32), ("observed", C.c_int32),
                ("calls", C.c_int64), ("device_bytes", C.c_uint64)]


class TsLightsExtDevice(C.Structure):
    _fields_ = [("state", C.c_void_p), ("next_state", C.c_void_p), ("controller", C.c_void_p), ("stored", C.c_void_p),
                ("n_groups", C.c_int32), ("state_dim", C.c_int32)]


class TsLightsProtoConfig(C.Structure):
    _fields_ = [("protocol", C.c_int32), ("min_green", C.c_int32), ("eps_min", C.c_double), ("eps_decay", C.c_double)]


class TsLightsProtoInfo(C.Structure):
    _fields_ = [("protocol", C.c_int32), ("min_green", C.c_int32), ("n_groups", C.c_int32), ("state_floats", C.c_int32),
                ("eps_min", C.c_double), ("eps_decay", C.c_double), ("calls", C.c_int64), ("device_bytes", C.c_uint64)]


class TsLightsProtoDevice(C.Structure):
    _fields_ = [("state", C.c_void_p), ("mask", C.c_void_p), ("next_state", C.c_void_p), ("reward", C.c_void_p),
                ("actions", C.c_void_p), ("epsilon", C.c_void_p), ("n_groups", C.c_int32), ("protocol", C.c_int32)]


# include/trafficsim_lights_proto.h: the protocols of the external light control beyond the simple one, by the reference's
# algorithm names.  Not light algorithms of the engine: world.build_engine translates them to EXTERNAL plus a protocol.
LIGHT_PROTOCOLS = {"RL_A2C_BATCHED": 1, "GAT_DQN_BATCHED": 2}
LP_A2C, LP_GAT = 1, 2


class TsCounters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "stuck", "collisions", "malfunctions", "overtaking", "in_stuck_detour", "parked", "live_internal",
        "live_through", "count_completed_internal", "count_completed_through", "total_distance_internal",
        "total_distance_through", "errored_internal", "errored_through")] + [
        ("total_duration_internal", C.c_double), ("total_duration_through", C.c_double), ("elapsed", C.c_double)] + [
        (n, C.c_int64) for n in ("step_count", "agent_steps", "astar_calls", "astar_expansions",
                                 "astar_relaxations", "move_rounds", "rng_fixups", "created_internal",
                                 "created_through", "created_service_food", "created_service_waste",
                                 "live_service_food", "live_service_waste")]


class TsTrafficZone(C.Structure):
    _fields_ = [("start_hour", C.c_int32), ("end_hour", C.c_int32), ("through_distribution", C.c_double),
                ("n_internal", C.c_int32), ("origin_type", C.c_int32 * 8), ("dest_type", C.c_int32 * 8),
                ("fraction", C.c_double * 8)]


class TsTrafficTables(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("blk_type", C.c_void_p), ("blk_entr_off", C.c_void_p),
                ("blk_entr_xy", C.c_void_p), ("n_highway_entrances", C.c_int32), ("highway_entrances_xy", C.c_void_p),
                ("n_highway_exits", C.c_int32), ("highway_exits_xy", C.c_void_p),
                ("internal_population_per_day", C.c_int32), ("passing_population_per_day", C.c_int32),
                ("start_offset_seconds", C.c_int32), ("n_zones", C.c_int32), ("zones", TsTrafficZone * 8),
                ("total_service_vehicles_food", C.c_int32), ("total_service_vehicles_waste", C.c_int32),
                ("service_load_time", C.c_int32), ("gradual_city_block_resources", C.c_int32),
                ("food_consumption_ticks", C.c_int32), ("waste_production_ticks", C.c_int32),
                ("needs_food_type_mask", C.c_int32), ("produces_waste_type_mask", C.c_int32),
                ("service_max_load_food", C.c_double), ("service_max_load_waste", C.c_double),
                ("food_capacity_per_cell", C.c_double), ("waste_capacity_per_cell", C.c_double),
                ("blk_inner_cells", C.c_void_p), ("blk_service_off", C.c_void_p), ("blk_service_xy", C.c_void_p),
                ("statistics_update_interval", C.c_int32)]


class TsCachedStats(C.Structure):
    """include/trafficsim.h: DynamicTrafficAgent._update_cached_stats' raw figures (index 0..3 = internal, through,
    service_food, service_waste)."""
    _fields_ = [("valid", C.c_int32), ("pad_", C.c_int32), ("update_step", C.c_int64),
                ("dur_live", C.c_double * 2), ("dist_live", C.c_int64 * 2), ("n_live", C.c_int64 * 2),
                ("stuck_ticks_sum", C.c_int64), ("stuck_ticks_max", C.c_int64),
                ("stuck", C.c_int64), ("collisions", C.c_int64), ("malfunctions", C.c_int64), ("parked", C.c_int64),
                ("overtaking", C.c_int64), ("in_stuck_detour", C.c_int64),
                ("live_internal", C.c_int64), ("live_through", C.c_int64), ("live_service_food", C.c_int64), ("live_service_waste", C.c_int64),
                ("count_completed", C.c_int64 * 2), ("total_distance", C.c_int64 * 2), ("total_duration", C.c_double * 2),
                ("daily_total", C.c_int64 * 4), ("created", C.c_int64 * 4), ("errored", C.c_int64 * 4),
                ("eta", C.c_double * 4), ("avg_daily_difference", C.c_double)]


# Defaults.TIME_ZONES (config.py:155-236) with block types as indices into AVAILABLE_CITY_BLOCKS
_BT = {"Res": 0, "Off": 1, "Mar": 2, "Lei": 3, "Oth": 4}
DEFAULT_TIME_ZONES = [
    (6, 9, 0.15, [("Res", "Off", 0.05), ("Res", "Mar", 0.05), ("Res", "Lei", 0.02), ("Res", "Oth", 0.03)]),
    (9, 12, 0.20, [("Res", "Mar", 0.10), ("Res", "Oth", 0.04), ("Off", "Oth", 0.06)]),
    (12, 15, 0.15, [("Res", "Mar", 0.07), ("Res", "Oth", 0.03), ("Off", "Oth", 0.05)]),
    (15, 18, 0.15, [("Res", "Mar", 0.03), ("Off", "Oth", 0.05), ("Mar", "Oth", 0.05), ("Lei", "Oth", 0.02)]),
    (18, 21, 0.12, [("Res", "Oth", 0.02), ("Res", "Lei", 0.02), ("Off", "Lei", 0.02), ("Mar", "Lei", 0.02),
                    ("Oth", "Lei", 0.02), ("Mar", "Oth", 0.01), ("Lei", "Oth", 0.01)]),
    (21, 24, 0.10, [("Off", "Res", 0.03), ("Mar", "Res", 0.03), ("Lei", "Res", 0.02), ("Oth", "Res", 0.02)]),
    (0, 3, 0.08, [("Off", "Res", 0.02), ("Lei", "Res", 0.04), ("Oth", "Res", 0.01), ("Res", "Lei", 0.01)]),
    (3, 6, 0.05, [("Res", "Mar", 0.02), ("Res", "Lei", 0.02), ("Res", "Oth", 0.01)]),
]


# Defaults attribute name -> TsParams field (config.py)
DEFAULTS_TO_PARAMS = {
    "VEHICLE_MIN_SPEED": "vehicle_min_speed", "VEHICLE_MAX_SPEED": "vehicle_max_speed",
    "VEHICLE_AWARENESS_RANGE": "vehicle_awareness_range", "RAIN_ENABLED": "rain_enabled",
    "RAIN_SPEED_REDUCTION": "rain_speed_reduction", "PATHFINDING_COOLDOWN": "pathfinding_cooldown",
    "PATHFINDING_CACHE": "pathfinding_cache", "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": "stuck_recompute_threshold",
    "VEHICLE_STUCK_RECOMPUTE_THRESHOLD_INTERSECTION": "stuck_recompute_threshold_intersection",
    "VEHICLE_CONTRAFLOW_OVERTAKE_ACTIVE": "contraflow_overtake_active",
    "VEHICLE_MAX_CONTRAFLOW_OVERTAKE_STEPS": "max_contraflow_overtake_steps",
    "VEHICLE_CONTRAFLOW_OVERTAKE_DURATION": "contraflow_overtake_duration",
    "VEHICLE_STUCK_CONTRAFLOW_ENABLED": "stuck_contraflow_enabled",
    "VEHICLE_STUCK_CONTRAFLOW_THRESHOLD": "stuck_contraflow_threshold",
    "VEHICLE_STUCK_CONTRAFLOW_THRESHOLD_INTERSECTION": "stuck_contraflow_threshold_intersection",
    "VEHICLE_MAX_CONTRAFLOW_STUCK_DETOUR_STEPS": "max_contraflow_stuck_detour_steps",
    "VEHICLE_CONTRAFLOW_STUCK_DETOUR_DURATION": "contraflow_stuck_detour_duration",
    "VEHICLE_MALFUNCTION_ACTIVE": "malfunction_active", "VEHICLE_MALFUNCTION_CHANCE": "malfunction_chance",
    "VEHICLE_MALFUNCTION_DURATION": "malfunction_duration",
    "VEHICLE_SIDESWIPE_COLLISION_ACTIVE": "sideswipe_active",
    "VEHICLE_SIDESWIPE_COLLISION_CHANCE": "sideswipe_chance",
    "VEHICLE_SIDESWIPE_COLLISION_DURATION": "sideswipe_duration",
    "VEHICLE_CONTRAFLOW_PENALTY": "contraflow_penalty",
    "VEHICLE_OBSTACLE_PENALTY_VEHICLE": "obstacle_penalty_vehicle",
    "VEHICLE_OBSTACLE_PENALTY_STOP": "obstacle_penalty_stop",
    "VEHICLE_ROAD_TYPES_PENALTIES_ENABLED": "road_type_penalties_enabled",
    "VEHICLE_ROAD_TYPES_PENALTY_R1": "road_type_penalty_r1", "VEHICLE_ROAD_TYPES_PENALTY_R2": "road_type_penalty_r2",
    "VEHICLE_ROAD_TYPES_PENALTY_R3": "road_type_penalty_r3",
    "VEHICLE_TURN_PENALTY_ENABLED": "turn_penalty_enabled", "VEHICLE_TURN_PENALTY": "turn_penalty",
    "VEHICLE_DYNAMIC_PENALTIES_ENABLED": "dynamic_penalties_enabled",
    "VEHICLE_DYNAMIC_PENALTY_SCALE": "dynamic_penalty_scale",
    "TRAFFIC_LIGHT_AGENT_ALGORITHM": "light_algorithm",
    "TRAFFIC_LIGHT_TRANSITION_DURATION_ENABLED": "transition_duration_enabled",
    "TRAFFIC_LIGHT_TRANSITION_CLEARANCE_ENABLED": "transition_clearance_enabled",
    "TRAFFIC_LIGHT_ALL_RED_DURATION": "all_red_duration", "TRAFFIC_LIGHT_GREEN_DURATION": "green_duration",
    "TRAFFIC_LIGHT_QUEUE_ACTUATED_MIN_GREEN": "qa_min_green",
    "TRAFFIC_LIGHT_QUEUE_ACTUATED_MAX_GREEN": "qa_max_green", "TRAFFIC_LIGHT_QUEUE_ACTUATED_GAP": "qa_gap",
    "ENABLE_TRAFFIC": "enable_traffic", "TIME_PER_STEP_IN_SECONDS": "time_per_step_seconds",
    "RAIN_RADIUS_MIN": "rain_radius_min", "RAIN_RADIUS_MAX": "rain_radius_max",
    "RAIN_OCCURRENCES_MAX": "rain_occurrences_max", "RAIN_COOLDOWN": "rain_cooldown",
    "RAIN_SPAWN_OFFSET": "rain_spawn_offset", "RAIN_SPAWN_CHANCE": "rain_spawn_chance",
    "VEHICLE_STUCK_DESPAWN_ENABLED": "stuck_despawn_enabled", "VEHICLE_STUCK_DESPAWN_THRESHOLD": "stuck_despawn_threshold",
    "VEHICLE_STUCK_DESPAWN_THRESHOLD_INTERSECTION": "stuck_despawn_threshold_intersection",
    "VEHICLE_RESPECT_AWARENESS": "respect_awareness",
    "PATHFINDING_BATCHING": "pathfinding_batching",
}
# switches whose non-default value selects a code path this build does not carry: (unsupported value, why).
# params_from_defaults refuses them loudly instead of running the default behaviour.
UNSUPPORTED_DEFAULTS = {
}


# ts_exchange_fn (include/trafficsim.h): all-gather of variable-size host byte buffers
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_int64))


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"trafficsim error {code}: {msg}")
        self.code = code


# ---- the entries (every header under include/, plus the debugging hooks the headers leave out) ----------------------
# group -> (what an engine without the group "has no", {entry name without the prefix: argtypes}).  "core" is
# include/trafficsim.h: both libraries export all of it and CApi binds it at construction.  An extension group is
# include/trafficsim_<group>.h; the CPU oracle has none of those, nor the hooks, so CApi._ext binds them on first use.
_H, _P, _I32, _I64, _U32, _U64 = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64      # (_H: a ts_handle)
_PP, _PI32, _PI64, _PU64 = C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
ENTRIES = {
    "core": (None, {
        "default_params": [C.POINTER(TsParams)],
        "last_error": [_H],
        "create": [C.POINTER(TsWorld), C.POINTER(TsParams), _PP],
        "destroy": [_H],
        "num_vehicles": [_H],
        "num_groups": [_H],
        "num_scheduled": [_H],
        "num_blocks": [_H],
        "num_spawned": [_H],
        "rain_spawn": [_H],
        "set_lights": [_H, C.POINTER(TsLightTables)],
        "schedule_add": [_H, _I32, _I32],
        "set_traffic_generator": [_H, C.POINTER(TsTrafficTables)],
        "cached_stats": [_H, C.POINTER(TsCachedStats)],
        "seed": [_H, _I32, _P, _U32],
        "seed_int": [_H, _I32, _U64],
        "rng_state": [_H, _I32, _P, C.POINTER(C.c_uint32)],
        "add_vehicles": [_H, _I32] + [_P] * 5,
        "add_vehicles_dirs": [_H, _I32] + [_P] * 5,
        "remove_vehicle": [_H, _I32, _I32],
        "upload_map": [_H, _I32, _P],
        "step": [_H, _I32],
        "download_map": [_H, _I32, _P],
        "download_density": [_H, _P],
        "download_vehicles": [_H, _P, _I32],
        "download_path": [_H, _I32, _P, _I32],
        "download_groups": [_H, _P],
        "download_blocks": [_H, _P],
        "rain_info": [_H, C.POINTER(TsRainInfo)],
        "add_service_vehicle": [_H, _I32, _I32, _I32],
        "group_links": [_H, _I32, _I32],
        "download_vehicle_meta": [_H, _P, _I32],
        "download_service_vehicles": [_H, _P, _P, _P, _I32],
        "counters": [_H, C.POINTER(TsCounters)],
        "astar": [_H] + [_I32] * 7 + [_P, _I32],
        "debug_set_occupancy": [_H, _P],
        "set_device": [_I32],
        "set_replan_sharding": [_H, _I32, _I32, _P, _P],
        "set_replan_sharding_device": [_H, _I32, _I32, _P, _P],
        "profile_enable": [_H, _I32],
        "profile_name": [_I32],
        "profile_get": [_H, _I32, C.POINTER(C.c_double), _PI64, _PI64],
    }),
    "checkpoint": ("checkpoints", {
        "checkpoint_size": [_H, _PU64],
        "checkpoint_save": [_H, _P, _U64, _PU64],
        "checkpoint_load": [_H, _P, _U64],
    }),
    "astar_batch": ("batched pathfinder", {
        "astar_batch": [_H, _I32, _P, _PI64],
        "astar_batch_fetch": [_H, _P, _P],
        "astar_batch_device": [_H, _PP, _PP, _PI32, _PI64],
    }),
    "observe": ("traffic observation", {
        "observe_start": [_H, _U32],
        "observe_stop": [_H],
        "observe_reset": [_H],
        "observe_info": [_H, C.POINTER(TsObserveInfo)],
        "observe_download": [_H, _I32, _P],
        "observe_pooled": [_H, _I32, _I32, _P],
        "observe_regions": [_H, _I32, _I32, _P, _P],
        "observe_groups": [_H, _P],
        "observe_device": [_H, _I32, _PP],
    }),
    "demand": ("route demand", {
        "demand_compute": [_H, C.POINTER(TsDemandQuery), C.POINTER(TsDemandInfo)],
        "demand_info": [_H, C.POINTER(TsDemandInfo)],
        "demand_download": [_H, _I32, _I32, _P],
        "demand_pooled": [_H, _I32, _I32, _I32, _P],
        "demand_groups": [_H, _P],
        "demand_device": [_H, _I32, _I32, _PP],
        "demand_release": [_H],
    }),
    "triplog": ("trip log", {
        "triplog_start": [_H, _I64],
        "triplog_stop": [_H],
        "triplog_clear": [_H],
        "triplog_info": [_H, C.POINTER(TsTripLogInfo)],
        "triplog_read": [_H, _I64, _I64, _P],
        "triplog_device": [_H, _PP, _PI64],
        "triplog_set_zones": [_H, _P, _I32],
        "triplog_od": [_H, _U32, _P, _P, _P, _PU64],
    }),
    "lights_ext": ("external light control", {
        "lights_ext_config": [_H, _I32, _I32],
        "lights_ext_set_static": [_H, _P, _P],
        "lights_ext_observe": [_H, _P],
        "lights_ext_act": [_H, _P, _I32, _P],
        "lights_ext_request": [_H, _P, _I32],
        "lights_ext_download": [_H, _P],
        "lights_ext_device": [_H, C.POINTER(TsLightsExtDevice)],
        "lights_ext_info": [_H, C.POINTER(TsLightsExtInfo)],
    }),
    "lights_proto": ("light protocols", {
        "lights_proto_config": [_H, C.POINTER(TsLightsProtoConfig)],
        "lights_proto_observe": [_H, _P, _P],
        "lights_proto_act": [_H, _P, _I32, _P, _P],
        "lights_proto_act_q": [_H, _P, _I32, _P, _P, _P],
        "lights_proto_download": [_H, _P],
        "lights_proto_device": [_H, C.POINTER(TsLightsProtoDevice)],
        "lights_proto_info": [_H, C.POINTER(TsLightsProtoInfo)],
    }),
    "render": ("renderer", {
        "render_set_cells": [_H, _P, _I32, _P],
        "render_set_vehicle_palette": [_H, _P],
        "render_set_heat_lut": [_H, _P],
        "render_set_routes": [_H, _I32, _P, _P],
        "render_size": [C.POINTER(TsRenderView), _PI32, _PI32],
        "render": [_H, C.POINTER(TsRenderView), _P],
        "render_device": [_H, C.POINTER(TsRenderView), _PP],
        "render_info": [_H, C.POINTER(TsRenderInfo)],
    }),
    # the hooks are two groups because their refusals name two different things
    "debug_batch": ("batched pathfinder", {"debug_batch_info": [_H, _P, _I32]}),
    "debug_quad": ("quad searcher", {"debug_quad_stats": [_H, _P, _I32], "debug_quad_walks": [_H, _P, _I32],
                                     "debug_arena_info": [_H, _P, _I32]}),      # (the arena the quads' tables share with k_replan's)
}
# the entries that do not return an int status
RESTYPES = {"default_params": None, "last_error": C.c_char_p, "profile_name": C.c_char_p, "triplog_read": C.c_int64}
_GROUP_OF = {name: group for group, (_, entries) in ENTRIES.items() for name in entries}


def _wrap_device(ptr, nbytes, device):
    """A uint8 torch tensor over `nbytes` of device memory at `ptr` (no copy; the engine owns the memory)."""
    import torch

    class _Raw:
        __cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Raw(), device=device)


def _info_dict(info) -> dict:
    """An info struct field by field: the doubles as float, every other field as int."""
    return {n: (float if t is C.c_double else int)(getattr(info, n)) for n, t in info._fields_}


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def approach_penalty_score(counts, penalties) -> np.ndarray:
    """IntersectionLightGroup.penalty_score (intersection_light_group.py:156-165) from a (G, 4) table of
    [blocks, R1 blocks, R2 blocks, R3 blocks] per group and the three road-type penalties: their mean over the blocks.
    The reference adds the penalties block by block; the counts give the same double whenever every partial sum is exact -
    penalties that are multiples of a power of two, like config.py's 0.5 / 5 / 50 - and may differ from it in the last bit
    otherwise (the table does not carry the order of the blocks)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 4)
    p1, p2, p3 = (float(p) for p in penalties)
    return np.where(c[:, 0] > 0, (c[:, 1] * p1 + c[:, 2] * p2 + c[:, 3] * p3) / np.maximum(c[:, 0], 1), 0.0)


def path_crc(xy) -> int:
    """crc32 of a path as int32 (x, y) pairs, 0 if empty - the TS_V_PATH_CRC convention."""
    a = _i32(xy).reshape(-1, 2)
    if a.size == 0:
        return 0
    return zlib.crc32(a.tobytes()) & 0xFFFFFFFF


class CApi:
    """One engine instance behind the C-ABI (`prefix` = "ts_" for the HIP engine)."""

    def __init__(self, lib: C.CDLL, prefix: str):
        self.lib, self.prefix = lib, prefix
        self.h = C.c_void_p()
        self._keep = []
        for name, argtypes in ENTRIES["core"][1].items():
            fn = self._f(name)
            fn.restype, fn.argtypes = RESTYPES.get(name, C.c_int), argtypes

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def _ext(self, name: str):
        """An entry of an extension group or a debugging hook of ENTRIES, bound on first use: the CPU oracle shares this
        class and has none of them."""
        phrase, entries = ENTRIES[_GROUP_OF[name]]
        fn = getattr(self.lib, self.prefix + name, None) if self.prefix == "ts_" else None
        if fn is None:
            raise EngineError(TS_E_UNSUPPORTED, f"{self.prefix}{name}: this engine has no {phrase}")
        if fn.argtypes is None:      # (the library hands out one function object per name: bound once, not per call)
            fn.restype, fn.argtypes = RESTYPES.get(name, C.c_int), entries[name]
        return fn

    def _has(self, name: str) -> bool:
        """Whether this engine has the extension group of entry `name`."""
        return name in _GROUP_OF and self.prefix == "ts_" and hasattr(self.lib, self.prefix + name)

    def _device_view(self, who: str, fallback: str, ptr, dtype: str, shape, device=None):
        """A torch tensor of `dtype` (a torch dtype's name) and `shape` over the engine's own device memory at `ptr` (no
        copy), on `device` (default: the device the engine was created on); a fresh empty tensor when the shape holds
        nothing.  `who` is the calling method and `fallback` its host-side alternative, for the error messages."""
        try:
            import torch
        except ImportError as ex:
            raise RuntimeError(f"{who} needs torch ({fallback})") from ex
        device = torch.device(device) if device is not None else torch.device("cuda", self.debug_batch_info()["device"])
        dt, shape = getattr(torch, dtype), tuple(int(n) for n in shape)
        count = int(np.prod(shape, dtype=np.int64))
        if count == 0:
            return torch.zeros(shape, dtype=dt, device=device)
        try:
            raw = _wrap_device(ptr, count * torch.empty(0, dtype=dt).element_size(), device)
        except RuntimeError as ex:
            raise RuntimeError(f"{who}: torch cannot reach the engine's device - import torch before the engine library "
                               f"is loaded, or {fallback}") from ex
        return raw.view(dt).view(shape)

    def _own_tensor(self, t, what: str, dtype: str, shape) -> bool:
        """Check a torch tensor the engine is to read in place: contiguous, of `dtype` (a torch dtype's name) and `shape`,
        and if it is on a GPU, on the engine's - its stream is then waited for (the engine reads on its own stream).
        Returns whether it is on the device."""
        import torch
        if t.dtype != getattr(torch, dtype) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{what}: a torch tensor must be contiguous {dtype} of shape {tuple(shape)}")
        if t.is_cuda:
            dev = self.debug_batch_info()["device"]
            if t.device.index != dev:
                raise ValueError(f"{what}: the tensor is on {t.device}, the engine on cuda:{dev}")
            torch.cuda.current_stream(t.device).synchronize()
        return t.is_cuda

    def _pooled_out(self, factor):
        """(zeroed (ceil(H / factor), ceil(W / factor)) uint64 output, the factor as the int32 the entry takes) of the two
        pooled downloads; a factor below 1 goes through for the engine to refuse."""
        f = int(factor)
        out = np.zeros((-(-self.H // f), -(-self.W // f)) if f >= 1 else (1, 1), dtype=np.uint64)
        return out, max(min(f, 0x7FFFFFFF), -1)

    def _chk(self, rc: int) -> int:
        if rc < 0:
            msg = self._f("last_error")(self.h) if self.h else b""
            raise EngineError(rc, (msg or b"").decode())
        return rc

    # ---- construction ----------------------------------------------------------------------
    def default_params(self) -> TsParams:
        p = TsParams()
        self._f("default_params")(C.byref(p))
        return p

    def params_from_defaults(self, overrides: Optional[dict] = None) -> TsParams:
        """TsParams from config.py defaults plus `Defaults`-style overrides (UPPER_CASE keys)."""
        p = self.default_params()
        for k, v in (overrides or {}).items():
            if k in UNSUPPORTED_DEFAULTS and bool(v) == UNSUPPORTED_DEFAULTS[k][0]:
                raise EngineError(TS_E_UNSUPPORTED, f"{k}={v!r}: {UNSUPPORTED_DEFAULTS[k][1]}")
            if k in DEFAULTS_TO_PARAMS:
                field = DEFAULTS_TO_PARAMS[k]
                if field == "light_algorithm":
                    if v not in LIGHT_ALGORITHMS:
                        raise EngineError(TS_E_UNSUPPORTED, f"light algorithm {v!r} is out of scope (RL variants)")
                    v = LIGHT_ALGORITHMS[v]
                setattr(p, field, type(getattr(p, field))(v))
        return p

    def create(self, allowed_dirs, is_road, road_type, intersection, params: TsParams):
        a = np.ascontiguousarray(allowed_dirs, dtype=np.uint8)
        r = np.ascontiguousarray(is_road, dtype=np.int8)
        t = np.ascontiguousarray(road_type, dtype=np.int8)
        i = np.ascontiguousarray(intersection, dtype=np.int8)
        H, W = a.shape
        assert r.shape == t.shape == i.shape == (H, W)
        self.W, self.H = W, H
        w = TsWorld(W, H, a.ctypes.data, r.ctypes.data, t.ctypes.data, i.ctypes.data)
        rc = self._f("create")(C.byref(w), C.byref(params), C.byref(self.h))
        if rc < 0:
            raise EngineError(rc, "create failed")
        self._light_algorithm = int(params.light_algorithm)
        self._road_type_penalties = (float(params.road_type_penalty_r1), float(params.road_type_penalty_r2), float(params.road_type_penalty_r3))
        return self

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lights(self, tables: dict):
        """`tables`: the G1 light tables (keys as in tests/golden world tables / citygen)."""
        t = TsLightTables()
        arrs = {
            "g_light_off": tables["g_light_off"], "light_xy": tables["light_xy"],
            "light_ctrl_off": tables["light_ctrl_off"], "light_ctrl_xy": tables["light_ctrl_xy"],
            "g_ns_off": tables["g_ns_lights_off"], "g_ns": tables["g_ns_lights"],
            "g_ew_off": tables["g_ew_lights_off"], "g_ew": tables["g_ew_lights"],
            "g_icell_off": tables["g_icell_off"], "g_icell_xy": tables["g_icell_xy"],
            "g_ns_in_off": tables["g_ns_in_off"], "g_ns_in_xy": tables["g_ns_in_xy"],
            "g_ns_out_off": tables["g_ns_out_off"], "g_ns_out_xy": tables["g_ns_out_xy"],
            "g_ew_in_off": tables["g_ew_in_off"], "g_ew_in_xy": tables["g_ew_in_xy"],
            "g_ew_out_off": tables["g_ew_out_off"], "g_ew_out_xy": tables["g_ew_out_xy"],
            "g_neighbors": tables["g_neighbors"],
            "g_neighbors_ctor": tables.get("g_neighbors_ctor", tables["g_neighbors"]),
        }
        keep = {k: _i32(v) for k, v in arrs.items()}
        t.n_groups = len(keep["g_light_off"]) - 1
        t.n_lights = len(keep["light_ctrl_off"]) - 1
        for k, v in keep.items():
            setattr(t, k, v.ctypes.data)
        self._chk(self._f("set_lights")(self.h, C.byref(t)))
        self.n_groups = t.n_groups
        # external control: penalty_score from the cells' own road types where the tables carry them (the road_type plane the
        # engine falls back to shows an R2 cell of the ring road as R1)
        if "g_approach_road_types" in tables and self.prefix == "ts_" and getattr(self, "_light_algorithm", None) == LIGHT_ALGORITHMS["EXTERNAL"]:
            self.lights_set_static(penalty_score=approach_penalty_score(tables["g_approach_road_types"], self._road_type_penalties))

    def cached_stats(self) -> Dict[str, object]:
        """DynamicTrafficAgent.cached_stats as the statistics panel reads it (ui_modules/traffic_statistics.py): the
        reference's keys and quotients (dynamic_traffic_generator.py:562-648) formed from ts_cached_stats' raw figures;
        {} until the generator's first update, like the reference's dict."""
        c = TsCachedStats()
        self._chk(self._f("cached_stats")(self.h, C.byref(c)))
        if not c.valid:
            return {}

        def safe(a, b):
            return a / b if b else 0.0
        out: Dict[str, object] = {}
        names = ("internal", "through")
        for what, num_c, num_l, den_c, den_l in (
                ("avg_duration", c.total_duration, c.dur_live, c.count_completed, c.n_live),
                ("avg_time_per_unit", c.total_duration, c.dur_live, c.total_distance, c.dist_live)):
            for k, nm in enumerate(names):
                out[f"{what}_{nm}_completed"] = safe(num_c[k], den_c[k])
            for k, nm in enumerate(names):
                out[f"{what}_{nm}_live"] = safe(num_l[k], den_l[k])
            for k, nm in enumerate(names):
                out[f"{what}_{nm}_total"] = safe(num_c[k] + num_l[k], den_c[k] + den_l[k])
        for what in ("avg_duration", "avg_time_per_unit"):
            for nm in names:
                out[f"{what}_{nm}"] = out[f"{what}_{nm}_total"]
        out["avg_daily_difference"] = c.avg_daily_difference
        out["count_completed_internal"] = int(c.count_completed[0])
        for f in ("live_internal", "live_through", "live_service_food", "live_service_waste", "collisions", "malfunctions", "parked",
                  "overtaking", "stuck"):
            out[f] = int(getattr(c, f))
        out["live_average_stuck_duration"] = (c.stuck_ticks_sum / c.stuck) if c.stuck > 0 else 0.0
        out["live_max_stuck_duration"] = int(c.stuck_ticks_max)
        out["in_stuck_detour"] = int(c.in_stuck_detour)
        for k, kind in enumerate(("internal", "through", "service_food", "service_waste")):
            total, created = int(c.daily_total[k]), int(c.created[k])
            out[f"daily_total_{kind}"] = total
            out[f"created_{kind}"] = created
            out[f"remaining_{kind}"] = total - created
            out[f"percentage_created_{kind}"] = (created / total * 100) if total else 0.0
            out[f"errored_{kind}"] = int(c.errored[k]) if k < 2 else 0.0      # (getattr(self, "errored_service_*", 0.0): no such attribute)
            out[f"eta_{kind}"] = None if c.eta[k] != c.eta[k] else float(c.eta[k])
        return out

    def set_traffic_generator(self, tables: dict, internal_per_day=10000, passing_per_day=2400,
                              start_offset_seconds=6 * 3600, zones=None, service: Optional[dict] = None,
                              statistics_update_interval: int = 20):
        """DynamicTrafficAgent.__init__: `tables` carries blk_type / blk_entr_off / blk_entr_xy /
        highway_entrances_xy / highway_exits_xy (golden world-table keys).  Generates day 0 (global stream)."""
        t = TsTrafficTables()
        keep = dict(bt=_i32(tables["blk_type"]), bo=_i32(tables["blk_entr_off"]), bx=_i32(tables["blk_entr_xy"]),
                    hi=_i32(tables["highway_entrances_xy"]), ho=_i32(tables["highway_exits_xy"]))
        t.n_blocks = len(keep["bt"])
        t.blk_type, t.blk_entr_off, t.blk_entr_xy = keep["bt"].ctypes.data, keep["bo"].ctypes.data, keep["bx"].ctypes.data
        t.n_highway_entrances = len(keep["hi"].reshape(-1, 2))
        t.highway_entrances_xy = keep["hi"].ctypes.data
        t.n_highway_exits = len(keep["ho"].reshape(-1, 2))
        t.highway_exits_xy = keep["ho"].ctypes.data
        t.internal_population_per_day, t.passing_population_per_day = int(internal_per_day), int(passing_per_day)
        t.start_offset_seconds = int(start_offset_seconds)
        t.statistics_update_interval = int(statistics_update_interval)
        zs = zones if zones is not None else DEFAULT_TIME_ZONES
        t.n_zones = len(zs)
        for i, (h0, h1, thr, pairs) in enumerate(zs):
            z = t.zones[i]
            z.start_hour, z.end_hour, z.through_distribution, z.n_internal = h0, h1, thr, len(pairs)
            for k, (o, dd, fr) in enumerate(pairs):
                z.origin_type[k], z.dest_type[k], z.fraction[k] = _BT[o], _BT[dd], fr
        if "blk_inner_cells" in tables:
            service = service or {}
            keep["bi"] = _i32(tables["blk_inner_cells"])
            keep["so"], keep["sx"] = _i32(tables["blk_service_off"]), _i32(tables["blk_service_xy"])
            t.blk_inner_cells, t.blk_service_off, t.blk_service_xy = (
                keep["bi"].ctypes.data, keep["so"].ctypes.data, keep["sx"].ctypes.data)
            t.total_service_vehicles_food = int(service.get("service_food", 0))
            t.total_service_vehicles_waste = int(service.get("service_waste", 0))
            t.service_load_time = int(service.get("load_time", 20))
            t.gradual_city_block_resources = int(service.get("gradual", True))
            t.food_consumption_ticks = int(service.get("food_consumption_ticks", 50))
            t.waste_production_ticks = int(service.get("waste_production_ticks", 100))
            t.needs_food_type_mask = int(service.get("needs_food_type_mask", 0b01100))
            t.produces_waste_type_mask = int(service.get("produces_waste_type_mask", 0b11111))
            t.service_max_load_food = float(service.get("max_load_food", 50.0))
            t.service_max_load_waste = float(service.get("max_load_waste", 250.0))
            t.food_capacity_per_cell = float(service.get("food_capacity_per_cell", 2.0))
            t.waste_capacity_per_cell = float(service.get("waste_capacity_per_cell", 1.5))
        self._chk(self._f("set_traffic_generator")(self.h, C.byref(t)))

    def schedule_add(self, kind: int, count: int = 1):
        self._chk(self._f("schedule_add")(self.h, kind, count))

    def seed_state(self, stream: int, state):
        """`state` = random.getstate() (or just its [1] tuple of 625 ints)."""
        tup = state[1] if (isinstance(state, tuple) and len(state) == 3) else state
        arr = np.asarray(tup, dtype=np.uint64)
        assert arr.size == 625
        mt = np.ascontiguousarray(arr[:624].astype(np.uint32))
        self._chk(self._f("seed")(self.h, stream, mt.ctypes.data, int(arr[624])))

    def seed_int(self, stream: int, seed: int):
        self._chk(self._f("seed_int")(self.h, stream, seed))

    def rng_state(self, stream: int):
        mt = np.zeros(624, dtype=np.uint32)
        idx = C.c_uint32()
        self._chk(self._f("rng_state")(self.h, stream, mt.ctypes.data, C.byref(idx)))
        return mt, idx.value

    def rng_fingerprint(self, stream: int):
        mt, idx = self.rng_state(stream)
        return zlib.crc32(mt.tobytes()) & 0xFFFFFFFF, idx

    def add_vehicles(self, start_xy, goal_xy, population_type=None, path_off=None, path_xy=None):
        s, g = _i32(start_xy).reshape(-1, 2), _i32(goal_xy).reshape(-1, 2)
        n = len(s)
        pt = _i32(population_type if population_type is not None else np.zeros(n))
        po = px = None
        if path_off is not None:
            po, px = _i32(path_off), _i32(path_xy).reshape(-1, 2)
            assert len(po) == n + 1
        self._chk(self._f("add_vehicles")(
            self.h, n, s.ctypes.data, g.ctypes.data, pt.ctypes.data,
            po.ctypes.data if po is not None else None, px.ctypes.data if px is not None else None))

    def add_vehicles_dirs(self, start_xy, goal_xy, population_type, path_off, path_dirs):
        """Routes as direction codes (N0 E1 S2 W3), one byte per step; path_off is int64."""
        s, g = _i32(start_xy).reshape(-1, 2), _i32(goal_xy).reshape(-1, 2)
        n = len(s)
        pt = _i32(population_type if population_type is not None else np.zeros(n))
        po = np.ascontiguousarray(path_off, dtype=np.int64)
        pd = np.ascontiguousarray(path_dirs, dtype=np.uint8)
        assert len(po) == n + 1 and len(pd) == po[-1]
        self._chk(self._f("add_vehicles_dirs")(self.h, n, s.ctypes.data, g.ctypes.data, pt.ctypes.data,
                                                po.ctypes.data, pd.ctypes.data))

    def remove_vehicle(self, spawn_idx: int, population_type: int = 0):
        """CityModel.remove_vehicle between ticks; `spawn_idx` = column 0 of vehicles().  `population_type` (POP[...]) is the
        reference's argument of that name: the live counter it names drops by one, 'undefined' (the default) touches none."""
        self._chk(self._f("remove_vehicle")(self.h, int(spawn_idx), int(population_type)))

    def upload_map(self, which: int, arr):
        a = np.ascontiguousarray(arr, dtype=np.int8)
        assert a.shape == (self.H, self.W)
        self._chk(self._f("upload_map")(self.h, which, a.ctypes.data))

    def set_device(self, device: int):
        rc = self._f("set_device")(device)
        if rc < 0:
            raise EngineError(rc, f"cannot select HIP device {device}")

    def profile_enable(self, on: bool = True):
        self._chk(self._f("profile_enable")(self.h, int(on)))

    def profile(self) -> dict:
        """{kernel name: (total_ms, launches, items)} measured with HIP events on the engine's stream."""
        out = {}
        for k in range(self._f("profile_count")()):
            ms, n, it = C.c_double(), C.c_int64(), C.c_int64()
            self._chk(self._f("profile_get")(self.h, k, C.byref(ms), C.byref(n), C.byref(it)))
            out[self._f("profile_name")(k).decode()] = (ms.value, n.value, it.value)
        return out

    def set_replan_sharding(self, rank: int, world: int, callback, device_buffers: bool = False):
        """ts_set_replan_sharding (host buffers) / ts_set_replan_sharding_device (device buffers): `callback` is an
        EXCHANGE_FN instance (kept alive here) or None for world == 1."""
        self._exchange_cb = callback
        ptr = C.cast(callback, C.c_void_p) if callback is not None else None
        name = "set_replan_sharding_device" if device_buffers else "set_replan_sharding"
        self._chk(self._f(name)(self.h, int(rank), int(world), ptr, None))

    def debug_set_occupancy(self, arr):
        """Test hook: overwrite occupancy_map without placing vehicles (A*/density KATs)."""
        a = np.ascontiguousarray(arr, dtype=np.int8)
        assert a.shape == (self.H, self.W)
        self._chk(self._f("debug_set_occupancy")(self.h, a.ctypes.data))

    # ---- stepping and read-back ---------------------------------------------------------------
    def step(self, n: int = 1):
        self._chk(self._f("step")(self.h, n))

    def num_vehicles(self) -> int:
        return self._chk(self._f("num_vehicles")(self.h))

    def num_scheduled(self) -> int:
        return self._chk(self._f("num_scheduled")(self.h))

    def map(self, which: int) -> np.ndarray:
        out = np.zeros((self.H, self.W), dtype=np.int8)
        self._chk(self._f("download_map")(self.h, which, out.ctypes.data))
        return out

    def density(self) -> np.ndarray:
        out = np.zeros((self.H, self.W), dtype=np.float32)
        self._chk(self._f("download_density")(self.h, out.ctypes.data))
        return out

    def vehicles(self) -> np.ndarray:
        n = self.num_vehicles()
        out = np.zeros((max(n, 1), len(V_FIELDS)), dtype=np.int32)
        got = self._chk(self._f("download_vehicles")(self.h, out.ctypes.data, max(n, 1)))
        return out[:got]

    def path(self, active_pos: int) -> np.ndarray:
        n = self._chk(self._f("download_path")(self.h, active_pos, None, 0))
        out = np.zeros((max(n, 1), 2), dtype=np.int32)
        self._chk(self._f("download_path")(self.h, active_pos, out.ctypes.data, max(n, 1)))
        return out[:n]

    def groups(self) -> np.ndarray:
        n = self._chk(self._f("num_groups")(self.h))
        out = np.zeros((max(n, 1), len(G_FIELDS)), dtype=np.int32)
        self._chk(self._f("download_groups")(self.h, out.ctypes.data))
        return out[:n]

    def num_spawned(self) -> int:
        return self._chk(self._f("num_spawned")(self.h))

    def vehicle_meta(self) -> np.ndarray:
        """[n][M_FIELDS] rows in the order of vehicles(): population, target, vehicle type, service phase."""
        n = self.num_vehicles()
        out = np.zeros((max(n, 1), len(M_FIELDS)), dtype=np.int32)
        got = self._chk(self._f("download_vehicle_meta")(self.h, out.ctypes.data, max(n, 1)))
        return out[:got]

    def service_vehicles(self):
        """(spawn_idx [n], loads [n][2] = current / max, block [n]) of the live service vehicles, by spawn index."""
        cap = max(self.num_vehicles(), 1)
        idx = np.zeros(cap, dtype=np.int32)
        loads = np.zeros((cap, 2), dtype=np.float64)
        blk = np.zeros(cap, dtype=np.int32)
        n = self._chk(self._f("download_service_vehicles")(self.h, idx.ctypes.data, loads.ctypes.data, blk.ctypes.data, cap))
        return idx[:n], loads[:n], blk[:n]

    def group_links(self, group: int, repopulate: bool = False) -> bool:
        """get_opposite_traffic_lights()'s side effect / state (see ts_group_links)."""
        return bool(self._chk(self._f("group_links")(self.h, int(group), int(bool(repopulate)))))

    def add_service_vehicle(self, x: int, y: int, service_type: int):
        """ServiceVehicleAgent(vid, model, entrance, sv_type) from the UI (vehicle_control.py:182-206)."""
        self._chk(self._f("add_service_vehicle")(self.h, int(x), int(y), int(service_type)))

    def rain_info(self) -> TsRainInfo:
        r = TsRainInfo()
        self._chk(self._f("rain_info")(self.h, C.byref(r)))
        return r

    def rain_spawn(self):
        """RainManager.add_random_rain() between ticks (the /spawn_rain handler)."""
        self._chk(self._f("rain_spawn")(self.h))

    def num_blocks(self) -> int:
        return self._chk(self._f("num_blocks")(self.h))

    def blocks(self) -> np.ndarray:
        """(food_units, waste_units) per CityBlock, city_blocks order."""
        n = self._chk(self._f("num_blocks")(self.h))
        out = np.zeros((max(n, 1), 2), dtype=np.float64)
        self._chk(self._f("download_blocks")(self.h, out.ctypes.data))
        return out[:n]

    def counters(self) -> TsCounters:
        c = TsCounters()
        self._chk(self._f("counters")(self.h, C.byref(c)))
        return c

    QUAD_STATS = ("jobs", "handbacks", "window", "heap", "budget", "path_buffer", "policy_bail", "policy_overflow",
                  "searches", "epoch_wraps", "passes", "sift_third_level", "sift_blocking_steps")

    def debug_quad_stats(self) -> dict:
        """Debugging hook (ts_debug_quad_stats, not part of include/trafficsim.h): the quad searcher's counters over this
        engine's quad passes - entries it took, hand-backs to k_replan in all and by reason, searches started, table-epoch
        wraps, passes, and the sift-down's steps beyond LDS (on the third level fetched ahead / blocking, below it)."""
        fn = self._ext("debug_quad_stats")
        out = np.zeros(len(self.QUAD_STATS), dtype=np.int64)
        n = self._chk(fn(self.h, out.ctypes.data, len(out)))
        assert n == len(out), f"ts_debug_quad_stats reports {n} counters, this wrapper knows {len(out)}"
        return dict(zip(self.QUAD_STATS, (int(v) for v in out)))

    ARENA_INFO = ("to_quads", "to_waves", "clears", "big_dist_flag", "big_dist_seen", "arena_shared", "arena_quad")
    QUAD_WALKS = ("walks", "cells", "round_trips", "odd", "len1", "len2")

    def _debug_words(self, entry, names) -> dict:
        fn = self._ext(entry)
        out = np.zeros(len(names), dtype=np.int64)
        n = self._chk(fn(self.h, out.ctypes.data, len(out)))
        assert n == len(out), f"ts_{entry} reports {n} words, this wrapper knows {len(out)}"
        return dict(zip(names, (int(v) for v in out)))

    def debug_arena_info(self) -> dict:
        """Debugging hook (ts_debug_arena_info, not part of include/trafficsim.h): the table arena k_replan and the quads share -
        hand-overs each way, clears run, the big-dist flag on the device and the hand-overs that found it set, whether the
        quads' tables alias the arena and whether they hold it now."""
        return self._debug_words("debug_arena_info", self.ARENA_INFO)

    def debug_quad_walks(self) -> dict:
        """Debugging hook (ts_debug_quad_walks, not part of include/trafficsim.h): the quads' walks back along found paths - walks,
        cells written, HBM round trips, walks of odd length (ended on the first cell of a pair), of one cell, of two."""
        return self._debug_words("debug_quad_walks", self.QUAD_WALKS)

    # ---- checkpoints (include/trafficsim_checkpoint.h) ----------------------------------------------
    def checkpoint_size(self) -> int:
        """Exact size in bytes of a checkpoint of the current state."""
        n = C.c_uint64()
        self._chk(self._ext("checkpoint_size")(self.h, C.byref(n)))
        return n.value

    def checkpoint_save(self) -> bytes:
        """Every piece of dynamic state as one canonical blob (between steps only)."""
        fn = self._ext("checkpoint_save")
        n = self.checkpoint_size()
        buf = np.empty(max(n, 1), dtype=np.uint8)
        got = C.c_uint64()
        self._chk(fn(self.h, buf.ctypes.data, n, C.byref(got)))
        return buf[:got.value].tobytes()

    def checkpoint_load(self, blob) -> None:
        """Replace all dynamic state with a blob from checkpoint_save of an engine built from the same world."""
        fn = self._ext("checkpoint_load")
        a = np.frombuffer(bytes(blob) if not isinstance(blob, (bytes, bytearray, np.ndarray)) else blob, dtype=np.uint8)
        a = np.ascontiguousarray(a)
        self._chk(fn(self.h, a.ctypes.data if a.size else None, a.size))

    def astar(self, sx, sy, gx, gy, soft_obstacles=False, ignore_flow=False, maximum_steps=0x7FFFFFFF):
        cap = self.W * self.H
        out = np.zeros((cap, 2), dtype=np.int32)
        n = self._chk(self._f("astar")(self.h, sx, sy, gx, gy, int(soft_obstacles), int(ignore_flow),
                                       int(maximum_steps), out.ctypes.data, cap))
        return out[:n].copy()

    # ---- query batches (include/trafficsim_astar_batch.h) -------------------------------------------
    @property
    def has_astar_batch(self) -> bool:
        """(the CPU oracle answers queries one by one)"""
        return self._has("astar_batch")

    @staticmethod
    def astar_queries(queries) -> np.ndarray:
        """(n, 7) int32 rows sx, sy, gx, gy, soft_obstacles, ignore_flow, maximum_steps from an (n, 7) or (n, 4) integer
        array; four columns mean a strict search that respects the flow and has no step limit."""
        q = np.asarray(queries)
        if q.size == 0:
            return np.zeros((0, 7), dtype=np.int32)
        if q.ndim != 2 or q.shape[1] not in (4, 7) or not np.issubdtype(q.dtype, np.integer):
            raise ValueError(f"queries must be an (n, 7) or (n, 4) integer array, got {q.dtype} {q.shape}")
        out = np.zeros((q.shape[0], 7), dtype=np.int32)
        out[:, 6] = 0x7FFFFFFF
        out[:, :q.shape[1]] = np.clip(q, -0x80000000, 0x7FFFFFFF)      # (what int32 cannot hold stays out of bounds / unlimited)
        return np.ascontiguousarray(out)

    def astar_batch_run(self, queries) -> int:
        """ts_astar_batch: run the queries, leave the CSR result on the device; returns the total number of path cells."""
        fn = self._ext("astar_batch")
        q = self.astar_queries(queries)
        total = C.c_int64()
        self._chk(fn(self.h, q.shape[0], q.ctypes.data if q.size else None, C.byref(total)))
        return total.value

    def astar_batch_fetch(self):
        """The last batch's result on the host: (off int64[n + 1], xy int32[total, 2])."""
        dev = self._ext("astar_batch_device")
        n, total = C.c_int32(), C.c_int64()
        self._chk(dev(self.h, None, None, C.byref(n), C.byref(total)))
        off = np.zeros(n.value + 1, dtype=np.int64)
        xy = np.zeros((total.value, 2), dtype=np.int32)
        self._chk(self._ext("astar_batch_fetch")(self.h, off.ctypes.data, xy.ctypes.data if total.value else None))
        return off, xy

    def astar_batch(self, queries):
        """Many A* queries on the current maps in one launch -> (off int64[n + 1], xy int32[total, 2]): CSR in query order,
        off[i]:off[i + 1] the (x, y) cells of query i's path without its start cell, empty for 'no path'.  Every query is
        answered exactly as `astar` answers it."""
        self.astar_batch_run(queries)
        return self.astar_batch_fetch()

    # ---- traffic observation (include/trafficsim_observe.h) ------------------------------------------
    @property
    def has_observe(self) -> bool:
        return self._has("observe_start")

    @staticmethod
    def _obs_plane(name) -> int:
        if isinstance(name, str):
            if name not in OBS_PLANES:
                raise ValueError(f"unknown observation plane {name!r} (one of {', '.join(OBS_PLANES)})")
            return OBS_PLANES.index(name)
        return int(name)

    def observe_start(self, planes=None):
        """Allocate and zero the named planes (default: all of OBS_PLANES; names, indices or a ready bit mask) and observe from
        the next tick on.  Starting again re-allocates and zeroes."""
        fn = self._ext("observe_start")
        if planes is None:
            mask = (1 << len(OBS_PLANES)) - 1
        elif isinstance(planes, (int, np.integer)):
            mask = int(planes)
        else:
            mask = 0
            for p in ([planes] if isinstance(planes, str) else planes):
                mask |= 1 << self._obs_plane(p)
        if not 0 <= mask <= 0xFFFFFFFF:
            raise ValueError(f"plane mask {mask} does not fit 32 bits")
        self._chk(fn(self.h, mask))

    def observe_stop(self):
        self._chk(self._ext("observe_stop")(self.h))

    def observe_reset(self):
        """Zero the planes and the tick count."""
        self._chk(self._ext("observe_reset")(self.h))

    def observe_info(self) -> dict:
        """{"planes": names held, "mask", "ticks", "width", "height", "device_bytes"}; no planes when observation is off."""
        info = TsObserveInfo()
        self._chk(self._ext("observe_info")(self.h, C.byref(info)))
        return {"planes": [n for k, n in enumerate(OBS_PLANES) if info.plane_mask >> k & 1], "mask": int(info.plane_mask),
                "ticks": int(info.ticks), "width": int(info.width), "height": int(info.height),
                "device_bytes": int(info.device_bytes)}

    def observe_plane(self, name) -> np.ndarray:
        """One whole plane as an (H, W) uint32 array."""
        out = np.zeros((self.H, self.W), dtype=np.uint32)
        self._chk(self._ext("observe_download")(self.h, self._obs_plane(name), out.ctypes.data))
        return out

    def observe_pooled(self, name, factor: int) -> np.ndarray:
        """The plane summed over factor x factor blocks on the device: (ceil(H / factor), ceil(W / factor)) uint64."""
        fn = self._ext("observe_pooled")
        out, f = self._pooled_out(factor)
        self._chk(fn(self.h, self._obs_plane(name), f, out.ctypes.data))
        return out

    def observe_regions(self, name, rects) -> np.ndarray:
        """Sums of the plane over rectangles (x0, y0, x1, y1), half-open, clipped to the map: uint64 [n]."""
        fn = self._ext("observe_regions")
        r = np.ascontiguousarray(np.clip(np.asarray(rects, dtype=np.int64).reshape(-1, 4), -0x80000000, 0x7FFFFFFF), dtype=np.int32)
        out = np.zeros(len(r), dtype=np.uint64)
        self._chk(fn(self.h, self._obs_plane(name), len(r), r.ctypes.data if len(r) else None, out.ctypes.data if len(r) else None))
        return out

    def observe_groups(self) -> np.ndarray:
        """[G][OG_FIELDS] int64: WAITING and PRESENT over every light group's ns_in / ew_in cells, the four ENTER planes
        over its intersection cells."""
        fn = self._ext("observe_groups")
        n = self._chk(self._f("num_groups")(self.h))
        out = np.zeros((max(n, 1), len(OG_FIELDS)), dtype=np.int64)
        self._chk(fn(self.h, out.ctypes.data))
        return out[:n]

    def observe_device(self, name, device=None):
        """A plane as an (H, W) int32 torch tensor over the engine's own device memory (no copy; the bits are the plane's
        uint32 counts; valid until observe_stop, the next observe_start or close).  torch must have been imported before the
        engine library was loaded, as for astar_batch_device."""
        ptr = C.c_void_p()
        self._chk(self._ext("observe_device")(self.h, self._obs_plane(name), C.byref(ptr)))
        return self._device_view("observe_device", "use observe_plane for a host array", ptr.value, "int32", (self.H, self.W), device)

    # ---- route demand (include/trafficsim_demand.h) ---------------------------------------------------
    @property
    def has_demand(self) -> bool:
        return self._has("demand_compute")

    @staticmethod
    def _dm_info(info: TsDemandInfo) -> dict:
        return {"n_bins": int(info.n_bins), "bin_cells": int(info.bin_cells), "open_tail": bool(info.open_tail),
                "selected": bool(info.selected), "width": int(info.width), "height": int(info.height), "tick": int(info.tick),
                "vehicles": int(info.vehicles), "steps": int(info.steps),
                "bin_steps": [int(info.bin_steps[b]) for b in range(int(info.n_bins))], "device_bytes": int(info.device_bytes)}

    @staticmethod
    def _dm_dir(dir) -> int:
        if dir is None:
            return -1
        if isinstance(dir, str):
            if dir.upper() not in ("N", "E", "S", "W"):
                raise ValueError(f"unknown direction {dir!r} (one of N, E, S, W)")
            return "NESW".index(dir.upper())
        return int(dir)

    def demand_compute(self, n_bins: int = 1, bin_cells: int = 1, open_tail: bool = True, select=None) -> dict:
        """Count the remaining main path of every live vehicle (or of those whose byte in `select`, indexed by spawn index, is
        not 0) into [bin][direction] planes on the device: step k of a path goes to bin k // bin_cells, steps beyond the last
        bin to the last one (`open_tail`) or nowhere.  `select`: a numpy array, or a uint8 torch tensor on the engine's device
        (read there, no copy).  Returns demand_info()."""
        fn = self._ext("demand_compute")
        q = TsDemandQuery(n_bins=int(n_bins), bin_cells=int(bin_cells), open_tail=int(bool(open_tail)))
        keep = None
        if select is not None:
            if hasattr(select, "data_ptr"):
                import torch
                if select.dtype != torch.uint8 or not select.is_cuda or not select.is_contiguous() or select.dim() != 1:
                    raise ValueError("demand_compute: a tensor select is 1-d contiguous uint8 on the engine's device")
                torch.cuda.current_stream(select.device).synchronize()
                keep = select
                q.select, q.n_select, q.select_on_device = select.data_ptr() or None, int(select.numel()), 1
            else:
                sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
                keep = sel if sel.size else np.zeros(1, dtype=np.uint8)   # (an empty mask still reaches the length check)
                q.select, q.n_select = keep.ctypes.data, int(sel.size)
        info = TsDemandInfo()
        self._chk(fn(self.h, C.byref(q), C.byref(info)))
        del keep
        return self._dm_info(info)

    def demand_info(self) -> dict:
        """{"n_bins", "bin_cells", "open_tail", "selected", "width", "height", "tick", "vehicles", "steps", "bin_steps",
        "device_bytes"} of the result held; n_bins 0 when there is none."""
        info = TsDemandInfo()
        self._chk(self._ext("demand_info")(self.h, C.byref(info)))
        return self._dm_info(info)

    def demand_plane(self, bin: int = 0, dir=None) -> np.ndarray:
        """One plane as an (H, W) uint32 array; dir 0..3 or "N" / "E" / "S" / "W", None: the sum of the four (added on the
        device)."""
        out = np.zeros((self.H, self.W), dtype=np.uint32)
        self._chk(self._ext("demand_download")(self.h, int(bin), self._dm_dir(dir), out.ctypes.data))
        return out

    def demand_pooled(self, factor: int, bin: int = 0, dir=None) -> np.ndarray:
        """The plane summed over factor x factor blocks on the device: (ceil(H / factor), ceil(W / factor)) uint64."""
        fn = self._ext("demand_pooled")
        out, f = self._pooled_out(factor)
        self._chk(fn(self.h, int(bin), self._dm_dir(dir), f, out.ctypes.data))
        return out

    def demand_groups(self) -> np.ndarray:
        """[G][n_bins][DG_FIELDS] int64: the direction-summed plane over every light group's ns_in / ew_in approach cells,
        the four direction planes over its intersection cells."""
        fn = self._ext("demand_groups")
        n, bins = self._chk(self._f("num_groups")(self.h)), self.demand_info()["n_bins"]
        out = np.zeros((max(n, 1), max(bins, 1), len(DG_FIELDS)), dtype=np.int64)
        self._chk(fn(self.h, out.ctypes.data))
        return out[:n, :bins]

    def demand_device(self, bin: int = 0, dir=0, device=None):
        """A direction plane as an (H, W) int32 torch tensor over the engine's own device memory (no copy; the bits are the
        plane's uint32 counts; valid until the next demand_compute, demand_release or close).  torch must have been imported
        before the engine library was loaded, as for observe_device."""
        ptr = C.c_void_p()
        self._chk(self._ext("demand_device")(self.h, int(bin), self._dm_dir(dir), C.byref(ptr)))
        return self._device_view("demand_device", "use demand_plane for a host array", ptr.value, "int32", (self.H, self.W), device)

    def demand_release(self):
        """Free the planes; there is no result afterwards."""
        self._chk(self._ext("demand_release")(self.h))

    # ---- cost fields (include/trafficsim_costfield.h): entries, structs and methods live in costfield.py ----------
    @property
    def costfield(self):
        """The cost-field entries of this engine, as a costfield.CostField (a view: it keeps no state of its own, so none is
        cached and the engine is not kept alive by a reference cycle)."""
        from .costfield import CostField
        return CostField(self)

    # ---- select-link analysis (include/trafficsim_selectlink.h): entries, structs and methods live in selectlink.py ----
    @property
    def selectlink(self):
        """The select-link entries of this engine, as a selectlink.SelectLink (a view like costfield)."""
        from .selectlink import SelectLink
        return SelectLink(self)

    # ---- jam detection (include/trafficsim_jams.h): entries, structs and methods live in jams.py ----
    @property
    def jams(self):
        """The jam-detection entries of this engine, as a jams.Jams (a view like costfield)."""
        from .jams import Jams
        return Jams(self)

    # ---- trip log (include/trafficsim_triplog.h) ----------------------------------------------------
    @property
    def has_triplog(self) -> bool:
        return self._has("triplog_start")

    def triplog_start(self, capacity: int):
        """Allocate a log of `capacity` records and log every vehicle that leaves from now on.  Starting again frees the old
        log: the new one is empty."""
        self._chk(self._ext("triplog_start")(self.h, max(min(int(capacity), 2 ** 63 - 1), -1)))
        self._tl_zones = 0

    def triplog_stop(self):
        self._chk(self._ext("triplog_stop")(self.h))
        self._tl_zones = 0

    def triplog_clear(self):
        """Empty the log; capacity and zone plane stay."""
        self._chk(self._ext("triplog_clear")(self.h))

    def triplog_info(self) -> dict:
        """{"capacity", "count", "dropped", "groups", "device_bytes"}; all zero when the log is off."""
        info = TsTripLogInfo()
        self._chk(self._ext("triplog_info")(self.h, C.byref(info)))
        return _info_dict(info)

    def trips(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records [first, first + n) of the log (default: all from `first` on) as a TRIP_DTYPE array, in log order."""
        fn = self._ext("triplog_read")
        if n is None:
            n = max(self.triplog_info()["count"] - int(first), 0)
        out = np.zeros(max(int(n), 1), dtype=TRIP_DTYPE)
        got = self._chk(fn(self.h, int(first), int(n), out.ctypes.data))
        return out[:got]

    def triplog_device(self, device=None):
        """The kept records as a (count, 18) int32 torch tensor over the engine's own device memory (no copy; a record is 18
        words: the 14 int32 fields, then the two doubles as word pairs; valid until triplog_stop, the next triplog_start or
        close).  torch must have been imported before the engine library was loaded, as for observe_device."""
        ptr, count = C.c_void_p(), C.c_int64()
        self._chk(self._ext("triplog_device")(self.h, C.byref(ptr), C.byref(count)))
        return self._device_view("triplog_device", "use trips for a host array", ptr.value, "int32",
                                 (count.value, TRIP_DTYPE.itemsize // 4), device)

    def triplog_set_zones(self, zone_of_cell, n_zones: int):
        """One (H, W) int32 plane: the zone 0 .. n_zones - 1 of every cell, -1 = none.  n_zones = 0 drops the plane."""
        fn = self._ext("triplog_set_zones")
        z = None
        if zone_of_cell is not None:
            z = np.ascontiguousarray(zone_of_cell, dtype=np.int32)
            if z.shape != (self.H, self.W):
                raise ValueError(f"the zone plane must be ({self.H}, {self.W}), got {z.shape}")
        self._chk(fn(self.h, z.ctypes.data if z is not None else None, max(min(int(n_zones), 0x7FFFFFFF), -1)))
        self._tl_zones = int(n_zones)

    @staticmethod
    def _tl_mask(reasons) -> int:
        if reasons is None:
            return sum(1 << k for k in TRIP_END.values())
        if isinstance(reasons, (int, np.integer)):
            return int(reasons)
        mask = 0
        for r in ([reasons] if isinstance(reasons, str) else reasons):
            if r not in TRIP_END:
                raise ValueError(f"unknown end reason {r!r} (one of {', '.join(TRIP_END)})")
            mask |= 1 << TRIP_END[r]
        return mask

    def triplog_od(self, reasons=None, count=True, duration=True, distance=True) -> dict:
        """Origin / destination sums over the records whose end reason is in `reasons` (names, a bit mask, default all),
        reduced on the device: {"count" uint64, "duration" float64, "distance" uint64} as (n_zones, n_zones) arrays indexed
        [zone(origin), zone(dest)] (a matrix switched off is left out), and "unzoned"."""
        fn = self._ext("triplog_od")
        nz = getattr(self, "_tl_zones", 0)
        out = {}
        if count:
            out["count"] = np.zeros((nz, nz), dtype=np.uint64)
        if duration:
            out["duration"] = np.zeros((nz, nz), dtype=np.float64)
        if distance:
            out["distance"] = np.zeros((nz, nz), dtype=np.uint64)
        unz = C.c_uint64()
        ptr = {k: (v.ctypes.data if v.size else None) for k, v in out.items()}
        mask = self._tl_mask(reasons)
        if not 0 <= mask <= 0xFFFFFFFF:
            raise ValueError(f"reason mask {mask} does not fit 32 bits")
        self._chk(fn(self.h, mask, ptr.get("count"), ptr.get("duration"), ptr.get("distance"), C.byref(unz)))
        out["unzoned"] = int(unz.value)
        return out

    # ---- external light control (include/trafficsim_lights_ext.h) ------------------------------------
    @property
    def has_lights_ext(self) -> bool:
        return self._has("lights_ext_observe")

    def lights_config(self, state_dim: int = 13, min_green: int = 5):
        """SRL_INPUT_DIMENSIONS (7, 11, 13, 17 or 19) and SRL_MIN_GREEN; only before the first control call."""
        self._chk(self._ext("lights_ext_config")(self.h, int(state_dim), int(min_green)))

    def lights_set_static(self, intersection_size=None, penalty_score=None):
        """The two static features of every group as float64 [G] (None = leave); only before the first control call."""
        fn = self._ext("lights_ext_set_static")
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (intersection_size, penalty_score)]
        for v in a:
            if v is not None and v.shape != (self.n_groups,):
                raise ValueError(f"a static feature must have shape ({self.n_groups},), got {v.shape}")
        self._chk(fn(self.h, *(v.ctypes.data if v is not None and v.size else None for v in a)))

    def lights_info(self) -> dict:
        """{"state_dim", "min_green", "n_groups", "observed", "calls", "device_bytes"}"""
        info = TsLightsExtInfo()
        self._chk(self._ext("lights_ext_info")(self.h, C.byref(info)))
        return _info_dict(info)

    def lights_observe(self, to_host: bool = True):
        """Phase A: the state vector of every group, (G, state_dim) float32.  A second call before the next lights_act or
        step returns the same (cached) vector.  to_host=False only runs it (the vector is in lights_device()["state"])."""
        fn = self._ext("lights_ext_observe")
        if not to_host:
            self._chk(fn(self.h, None))
            return None
        dim = self.lights_info()["state_dim"]
        out = np.zeros((max(self.n_groups, 1), dim), dtype=np.float32)
        self._chk(fn(self.h, out.ctypes.data))
        return out[:self.n_groups]

    def _le_bytes(self, v, what):
        """An int8 vector of one entry per group as (pointer, on_device, keep-alive): numpy / sequences on the host, a torch
        tensor on the engine's device as it is."""
        if type(v).__module__.split(".")[0] == "torch":
            if self._own_tensor(v, what, "int8", (self.n_groups,)):
                return v.data_ptr(), 1, v
            v = v.numpy()
        a = np.ascontiguousarray(np.clip(np.asarray(v, dtype=np.int64), -128, 127), dtype=np.int8)
        if a.shape != (self.n_groups,):
            raise ValueError(f"{what}: one entry per group ({self.n_groups}), got shape {a.shape}")
        return a.ctypes.data, 0, a

    def lights_act(self, actions, want_next: bool = True):
        """Phase B with one action (0 keep, 1 switch) per group - numpy, a sequence, or an int8 torch tensor on the engine's
        device (read there, no copy).  Runs phase A first if lights_observe has not run since the last step.  Returns the
        next-state vectors (G, state_dim) float32, or None with want_next=False."""
        fn = self._ext("lights_ext_act")
        ptr, on_dev, keep = self._le_bytes(actions, "actions")
        out = None
        if want_next:
            out = np.zeros((max(self.n_groups, 1), self.lights_info()["state_dim"]), dtype=np.float32)
        self._chk(fn(self.h, ptr, on_dev, out.ctypes.data if out is not None else None))
        del keep
        return out[:self.n_groups] if out is not None else None

    def lights_request(self, phases):
        """apply_phase(phase) on every group whose entry is 0 or 1; -1 = no request.  For controllers that do not follow the
        observe / act protocol; touches none of its state."""
        fn = self._ext("lights_ext_request")
        ptr, on_dev, keep = self._le_bytes(phases, "phases")
        self._chk(fn(self.h, ptr, on_dev))
        del keep

    def lights_controller(self) -> np.ndarray:
        """(G, 2) int32: _rl_phase, rl_timer of every group."""
        fn = self._ext("lights_ext_download")
        out = np.zeros((max(self.n_groups, 1), 2), dtype=np.int32)
        self._chk(fn(self.h, out.ctypes.data))
        return out[:self.n_groups]

    def lights_device(self, device=None) -> dict:
        """{"state", "next_state": (G, state_dim) float32, "controller", "stored": (G, 2) int32} as torch tensors over the
        engine's own device memory (no copy; valid until close; the engine rewrites them in every control call).  torch must
        have been imported before the engine library was loaded, as for observe_device."""
        d = TsLightsExtDevice()
        self._chk(self._ext("lights_ext_device")(self.h, C.byref(d)))
        G, dim = int(d.n_groups), int(d.state_dim)
        spec = {"state": (d.state, "float32", (G, dim)), "next_state": (d.next_state, "float32", (G, dim)),
                "controller": (d.controller, "int32", (G, 2)), "stored": (d.stored, "int32", (G, 2))}
        return {k: self._device_view("lights_device", "use lights_observe / lights_controller for host arrays", ptr, dt, shape, device)
                for k, (ptr, dt, shape) in spec.items()}

    # ---- A2C / GAT-DQN light protocols (include/trafficsim_lights_proto.h) ------------------------------
    def lights_proto_config(self, protocol, min_green: int = 5, eps_min: float = 0.1, eps_decay: float = 1e-5):
        """Choose the A2C (1, "RL_A2C_BATCHED") or GAT-DQN (2, "GAT_DQN_BATCHED") protocol; once, before the first control call."""
        cfg = TsLightsProtoConfig(int(LIGHT_PROTOCOLS.get(protocol, protocol)), int(min_green), float(eps_min), float(eps_decay))
        self._chk(self._ext("lights_proto_config")(self.h, C.byref(cfg)))

    def lights_proto_info(self) -> dict:
        """{"protocol" (0: none), "min_green", "n_groups", "state_floats", "eps_min", "eps_decay", "calls", "device_bytes"}"""
        info = TsLightsProtoInfo()
        self._chk(self._ext("lights_proto_info")(self.h, C.byref(info)))
        return _info_dict(info)

    def lights_proto_observe(self, to_host: bool = True):
        """A2C: the state (G, 13) float32.  GAT: (features (G, 5, 9), mask (G, 5)) float32.  No side effects.
        to_host=False only runs it (nothing comes down; the results are in lights_proto_device()) and returns None."""
        fn = self._ext("lights_proto_observe")
        if not to_host:
            self._chk(fn(self.h, None, None))
            return None
        gat = self.lights_proto_info()["protocol"] == LP_GAT
        G = max(self.n_groups, 1)
        state = np.zeros((G, 5, 9) if gat else (G, 13), dtype=np.float32)
        mask = np.zeros((G, 5), dtype=np.float32) if gat else None
        self._chk(fn(self.h, state.ctypes.data, mask.ctypes.data if gat else None))
        return (state[:self.n_groups], mask[:self.n_groups]) if gat else state[:self.n_groups]

    def lights_proto_act(self, actions, want_next=None, to_host: bool = True):
        """The action rule with caller-chosen actions (numpy, a sequence or an int8 torch tensor on the engine's device): draws
        nothing, leaves epsilon alone.  Returns the rewards (G,) float64 under A2C, (rewards, next features) under GAT
        (want_next=False: the rewards only).  to_host=False: nothing comes down (the results are in lights_proto_device())
        and None is returned."""
        fn = self._ext("lights_proto_act")
        ptr, on_dev, keep = self._le_bytes(actions, "actions")
        if not to_host:
            self._chk(fn(self.h, ptr, on_dev, None, None))
            return None
        if want_next is None:
            want_next = self.lights_proto_info()["protocol"] == LP_GAT
        G = max(self.n_groups, 1)
        reward = np.zeros(G, dtype=np.float64)
        nxt = np.zeros((G, 5, 9), dtype=np.float32) if want_next else None
        self._chk(fn(self.h, ptr, on_dev, reward.ctypes.data, nxt.ctypes.data if nxt is not None else None))
        del keep
        return (reward[:self.n_groups], nxt[:self.n_groups]) if nxt is not None else reward[:self.n_groups]

    def lights_proto_act_q(self, q, want_next: bool = True, to_host: bool = True):
        """GAT: the epsilon-greedy step on q (G, 2) float32 - numpy or a torch tensor on the engine's device - drawing from
        the engine's global stream.  Returns (actions int8, rewards float64, next features); want_next=False leaves the next
        features on the device ((actions, rewards)); to_host=False brings nothing down (actions, rewards and next state are in
        lights_proto_device()) and returns None."""
        fn = self._ext("lights_proto_act_q")
        keep, on_dev = q, 0
        if type(q).__module__.split(".")[0] == "torch" and q.is_cuda:
            self._own_tensor(q, "q", "float32", (self.n_groups, 2))
            ptr, on_dev = q.data_ptr(), 1
        else:
            keep = np.ascontiguousarray(q.numpy() if hasattr(q, "numpy") else q, dtype=np.float32)
            if keep.shape != (self.n_groups, 2):
                raise ValueError(f"q: two values per group ({self.n_groups}, 2), got shape {keep.shape}")
            ptr = keep.ctypes.data if keep.size else np.zeros(2, np.float32).ctypes.data
        if not to_host:
            self._chk(fn(self.h, ptr, on_dev, None, None, None))
            return None
        G = max(self.n_groups, 1)
        acts, reward = np.zeros(G, dtype=np.int8), np.zeros(G, dtype=np.float64)
        nxt = np.zeros((G, 5, 9), dtype=np.float32) if want_next else None
        self._chk(fn(self.h, ptr, on_dev, acts.ctypes.data, reward.ctypes.data, nxt.ctypes.data if nxt is not None else None))
        del keep
        out = (acts[:self.n_groups], reward[:self.n_groups])
        return out + (nxt[:self.n_groups],) if nxt is not None else out

    def lights_proto_controller(self) -> np.ndarray:
        """(G,) float64: epsilon of every group (zeros under A2C); _rl_phase / rl_timer are lights_controller()."""
        out = np.zeros(max(self.n_groups, 1), dtype=np.float64)
        self._chk(self._ext("lights_proto_download")(self.h, out.ctypes.data))
        return out[:self.n_groups]

    def lights_proto_device(self, device=None) -> dict:
        """{"state", "mask", "next_state", "reward", "actions", "epsilon"} as torch tensors over the engine's own device memory
        (entries the protocol does not have are left out); torch must have been imported before the engine library was loaded."""
        d = TsLightsProtoDevice()
        self._chk(self._ext("lights_proto_device")(self.h, C.byref(d)))
        G = int(d.n_groups)
        gat = int(d.protocol) == LP_GAT
        spec = {"state": (d.state, "float32", (G, 5, 9) if gat else (G, 13)), "reward": (d.reward, "float64", (G,)),
                "actions": (d.actions, "int8", (G,))}
        if gat:
            spec.update(mask=(d.mask, "float32", (G, 5)), next_state=(d.next_state, "float32", (G, 5, 9)),
                        epsilon=(d.epsilon, "float64", (G,)))
        return {k: self._device_view("lights_proto_device", "use lights_proto_observe / lights_proto_controller for host arrays",
                                     ptr, dt, shape, device)
                for k, (ptr, dt, shape) in spec.items()}

    # ---- device renderer (include/trafficsim_render.h) ------------------------------------------------
    @property
    def has_render(self) -> bool:
        return self._has("render")

    @staticmethod
    def _heat_plane(name) -> int:
        """A TS_OBS_* index from a plane name or index; "flow" is TS_OBS_NPLANES, the sum of the four ENTER planes."""
        return len(OBS_PLANES) if name == "flow" else CApi._obs_plane(name)

    @staticmethod
    def _u8(a, shape, what) -> np.ndarray:
        a = np.asarray(a)
        if a.shape != tuple(shape) or a.dtype.kind not in "iub" or (a.size and (a.min() < 0 or a.max() > 255)):
            raise ValueError(f"{what} must be integers 0..255 of shape {tuple(shape)}, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a, dtype=np.uint8)

    def render_set_cells(self, type_plane, cell_palette):
        """The static type code per cell ((H, W), every code < n_types) and the cell palette
        ((n_types, 2 pend, 2 stop, 2 rain, 4) RGBA; render.cell_palette builds the reference's)."""
        fn = self._ext("render_set_cells")
        pal = np.asarray(cell_palette)
        n_types = pal.shape[0] if pal.ndim == 5 else -1
        pal = self._u8(pal, (max(n_types, 0), 2, 2, 2, 4), "cell_palette")
        tp = self._u8(type_plane, (self.H, self.W), "type_plane")
        self._chk(fn(self.h, tp.ctypes.data, n_types, pal.ctypes.data))

    def render_set_vehicle_palette(self, pal):
        """(3 kind, 4 status, 2 flash, 4) RGBA; render.vehicle_palette builds the reference's."""
        fn = self._ext("render_set_vehicle_palette")
        self._chk(fn(self.h, self._u8(pal, (3, 4, 2, 4), "vehicle palette").ctypes.data))

    def render_set_heat_lut(self, lut):
        """(256, 4) RGBA, A = blend weight."""
        fn = self._ext("render_set_heat_lut")
        self._chk(fn(self.h, self._u8(lut, (256, 4), "heat LUT").ctypes.data))

    def render_set_routes(self, spawn_idx, rgba=(255, 0, 255, 160)):
        """The vehicles (spawn indices, at most RENDER_MAX_ROUTES; an empty list clears) whose remaining paths the routes
        layer draws, and the colour they are blended in with (A = blend weight)."""
        fn = self._ext("render_set_routes")
        ids = _i32(np.asarray(spawn_idx, dtype=np.int64).reshape(-1))
        col = self._u8(rgba, (4,), "route colour")
        self._chk(fn(self.h, len(ids), ids.ctypes.data if len(ids) else None, col.ctypes.data))

    def render_size(self, view: TsRenderView):
        """(width, height) in pixels of the frame a view gives."""
        fn = self._ext("render_size")
        w, h = C.c_int32(), C.c_int32()
        self._chk(fn(C.byref(view), C.byref(w), C.byref(h)))
        return w.value, h.value

    def render(self, view: TsRenderView) -> np.ndarray:
        """One frame as an (h, w, 4) uint8 array (RGBA, alpha 255)."""
        fn = self._ext("render")
        w, h = self.render_size(view)
        out = np.zeros((h, w, 4), dtype=np.uint8)
        self._chk(fn(self.h, C.byref(view), out.ctypes.data))
        return out

    def render_device(self, view: TsRenderView, device=None):
        """One frame as an (h, w, 4) uint8 torch tensor over the engine's own frame buffer (no copy; valid until the next
        render or close).  torch must have been imported before the engine library was loaded, as for observe_device."""
        fn = self._ext("render_device")
        w, h = self.render_size(view)
        ptr = C.c_void_p()
        self._chk(fn(self.h, C.byref(view), C.byref(ptr)))
        return self._device_view("render_device", "use render for a host array", ptr.value, "uint8", (h, w, 4), device)

    def render_info(self) -> dict:
        """{"n_types", "has_vehicle_palette", "has_heat_lut", "n_routes", "last_w", "last_h", "frames", "device_bytes"}"""
        info = TsRenderInfo()
        self._chk(self._ext("render_info")(self.h, C.byref(info)))
        return {"n_types": int(info.n_types), "has_vehicle_palette": bool(info.has_vehicle_palette),
                "has_heat_lut": bool(info.has_heat_lut), "n_routes": int(info.n_routes), "last_w": int(info.last_w),
                "last_h": int(info.last_h), "frames": int(info.frames), "device_bytes": int(info.device_bytes)}

    BATCH_INFO = ("slots", "side_slots", "arena_shared", "arena_quad", "last_waves", "last_usable", "last_arena_quad",
                  "last_passes", "device")

    def debug_batch_info(self) -> dict:
        """Debugging hook (ts_debug_batch_info, not part of the headers): the searcher slots as they are now (count, the side
        waves' share, whether the quads' tables alias the arena / hold it) and what the last query batch ran on (waves of its
        widest launch, slots it was allowed, whether the quads held the arena then, launches it took), and the engine's device."""
        fn = self._ext("debug_batch_info")
        out = np.zeros(len(self.BATCH_INFO), dtype=np.int32)
        n = self._chk(fn(self.h, out.ctypes.data, len(out)))
        assert n == len(out), f"ts_debug_batch_info reports {n} words, this wrapper knows {len(out)}"
        return dict(zip(self.BATCH_INFO, (int(v) for v in out)))

    def astar_batch_device(self, device=None):
        """The last batch's (off, xy) as torch tensors over the engine's own device memory (no copy; valid as long as the
        result can be fetched).  `device`: default the device the engine was created on.  torch must have been imported before
        the engine library was loaded (as the torch-side callers in dist.py do): the two then share one HIP runtime; loaded the
        other way round torch finds no device, and this method says so."""
        p_off, p_xy, n, total = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int64()
        self._chk(self._ext("astar_batch_device")(self.h, C.byref(p_off), C.byref(p_xy), C.byref(n), C.byref(total)))
        who, fallback = "astar_batch_device", "use astar_batch / astar_batch_fetch for host arrays"
        return (self._device_view(who, fallback, p_off.value, "int64", (n.value + 1,), device),
                self._device_view(who, fallback, p_xy.value, "int32", (total.value, 2), device))
