#!/usr/bin/env python3
"""Golden-vector generator (build container only; NEVER runs on the GPU box).

Executes the reference's own, unmodified source files from /root/reference with the
stand-in packages of tests/golden/standins (mesa / numba / tensorflow are not installed
here; see standins/README.md and SURVEY.md §8(c)) and records small fixtures under
tests/golden/*.npz:

  G1  world tables  (static maps, light-group tables, schedule layout, entrances/exits)
  G2  A* known-answer tests (astar_numba.py:243-281, all (soft, ignore_flow) modes)
  G3  density map (city_model.py:1764-1778, real scipy.ndimage.uniform_filter), at r = 10 and at other radii
  G2c A* known-answer tests under moved cost constants (COST_SETS; one process per set)
  G4  MT19937 streams from CPython's own `random` (random(), randint(1,5), shuffle)
  G5  per-tick traces of CityModel.step() (maps, per-vehicle tuples, RNG fingerprints)
  G6  per-tick light-group controller state

Harness rules: cpu_count()=1 before import (sequential decide phase,
deterministic); both RNG streams seeded (random.seed(s) and CityModel(seed=s));
SAVE_*_RESULTS off; model._update_density_map() before the first VehicleAgent;
density_map cast to float64 after each update so the un-jitted A* computes the soft
penalty in float64 like numba does (astar_numba.py:199-200).

Usage:  python tests/golden/make_golden.py all        (each scenario in a subprocess)
        python tests/golden/make_golden.py <scenario>
"""
import hashlib
import json
import os
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# --------------------------------------------------------------------------------------
# scenario table
# --------------------------------------------------------------------------------------
GATED = dict(PATHFINDING_COOLDOWN=10 ** 9, VEHICLE_STUCK_RECOMPUTE_THRESHOLD=10 ** 9,
             VEHICLE_STUCK_RECOMPUTE_THRESHOLD_INTERSECTION=10 ** 9,
             VEHICLE_CONTRAFLOW_OVERTAKE_ACTIVE=False, VEHICLE_STUCK_CONTRAFLOW_ENABLED=False)
CLOSED = dict(RAIN_ENABLED=False, INTERNAL_POPULATION_TRAFFIC_PER_DAY=0,
              PASSING_POPULATION_TRAFFIC_PER_DAY=0, TOTAL_SERVICE_VEHICLES_FOOD=0,
              TOTAL_SERVICE_VEHICLES_WASTE=0)

# --------------------------------------------------------------------------------------
# A* cost-constant sets (job astar_cost_kats; two of them also drive a trace each)
# --------------------------------------------------------------------------------------
# config.py's own values of every constant astar_numba.py binds at import (lines 11-24), plus the density window's radius
COST_DEFAULTS = dict(VEHICLE_CONTRAFLOW_PENALTY=5000, VEHICLE_OBSTACLE_PENALTY_VEHICLE=1000, VEHICLE_OBSTACLE_PENALTY_STOP=500,
                     VEHICLE_ROAD_TYPES_PENALTIES_ENABLED=True, VEHICLE_ROAD_TYPES_PENALTY_R1=0.5,
                     VEHICLE_ROAD_TYPES_PENALTY_R2=5, VEHICLE_ROAD_TYPES_PENALTY_R3=50.0, VEHICLE_TURN_PENALTY_ENABLED=True,
                     VEHICLE_TURN_PENALTY=10, VEHICLE_DYNAMIC_PENALTIES_ENABLED=True, VEHICLE_DYNAMIC_PENALTY_SCALE=4.0,
                     VEHICLE_AWARENESS_RANGE=10)
# astar_numba's module constant for each of them
COST_MODULE_NAMES = dict(VEHICLE_CONTRAFLOW_PENALTY="CONTRA_PENALTY", VEHICLE_OBSTACLE_PENALTY_VEHICLE="VEHICLE_PENALTY",
                         VEHICLE_OBSTACLE_PENALTY_STOP="STOP_PENALTY", VEHICLE_ROAD_TYPES_PENALTIES_ENABLED="ROAD_TYPES_PENALTY_ENABLED",
                         VEHICLE_ROAD_TYPES_PENALTY_R1="ROAD_TYPES_PENALTY_R1", VEHICLE_ROAD_TYPES_PENALTY_R2="ROAD_TYPES_PENALTY_R2",
                         VEHICLE_ROAD_TYPES_PENALTY_R3="ROAD_TYPES_PENALTY_R3", VEHICLE_TURN_PENALTY_ENABLED="VEHICLE_TURN_PENALTY_ENABLED",
                         VEHICLE_TURN_PENALTY="VEHICLE_TURN_PENALTY", VEHICLE_DYNAMIC_PENALTIES_ENABLED="VEHICLE_DYNAMIC_PENALTIES_ENABLED",
                         VEHICLE_DYNAMIC_PENALTY_SCALE="VEHICLE_DYNAMIC_PENALTY_SCALE")
# name -> defaults: the overrides; half: the form the engine's searches must take (all penalties multiples of 0.5, scale <= 64,
# veh * (1 + scale) * 2 < 2^21); occupancy: "base" = run_astar_kats' draw (1/8 of the road cells), "dense" = 1/4 of them;
# may_coincide: exempt from the "10 % of the paths differ from the defaults' paths" condition, with the reason
COST_SETS = {
    "ints": dict(half=True, occupancy="base", defaults=dict(
        VEHICLE_TURN_PENALTY=3, VEHICLE_CONTRAFLOW_PENALTY=700, VEHICLE_OBSTACLE_PENALTY_VEHICLE=100, VEHICLE_OBSTACLE_PENALTY_STOP=50,
        VEHICLE_ROAD_TYPES_PENALTY_R1=2, VEHICLE_ROAD_TYPES_PENALTY_R2=0, VEHICLE_ROAD_TYPES_PENALTY_R3=9)),
    "flags_off": dict(half=True, occupancy="base", may_coincide="no exemption needed in practice, but a map whose cheapest routes are "
                      "also its shortest and straightest ones answers the same with and without the three penalties",
                      defaults=dict(VEHICLE_TURN_PENALTY_ENABLED=False, VEHICLE_ROAD_TYPES_PENALTIES_ENABLED=False,
                                    VEHICLE_DYNAMIC_PENALTIES_ENABLED=False)),
    "turn0": dict(half=True, occupancy="base", may_coincide="a turn costs 0 instead of 10: only routes that traded a turn for a "
                  "detour of < 10 change", defaults=dict(VEHICLE_TURN_PENALTY_ENABLED=True, VEHICLE_TURN_PENALTY=0)),
    "quarter": dict(half=False, occupancy="base", defaults=dict(
        VEHICLE_ROAD_TYPES_PENALTY_R1=2.25, VEHICLE_ROAD_TYPES_PENALTY_R2=0.75, VEHICLE_ROAD_TYPES_PENALTY_R3=9.25)),
    # veh 320, not 333: 333 * 0.3 * d = 99.9 d is a whole number only for d a multiple of 10/999, which no float32 in (0, 1] is,
    # so with 333 the truncation cases this set is here for cannot exist; 320 * 0.3 = 96 makes every density k/32 one
    "nondyadic": dict(half=False, occupancy="dense", whole_cells=20, defaults=dict(
        VEHICLE_ROAD_TYPES_PENALTY_R1=0.3, VEHICLE_ROAD_TYPES_PENALTY_R2=1.7, VEHICLE_ROAD_TYPES_PENALTY_R3=12.1,
        VEHICLE_DYNAMIC_PENALTY_SCALE=0.3, VEHICLE_OBSTACLE_PENALTY_VEHICLE=320, VEHICLE_AWARENESS_RANGE=6)),
    "scale_half": dict(half=True, occupancy="dense", whole_cells=20, defaults=dict(
        VEHICLE_DYNAMIC_PENALTY_SCALE=0.3, VEHICLE_OBSTACLE_PENALTY_VEHICLE=1000, VEHICLE_AWARENESS_RANGE=3)),
    "switch_lo": dict(half=True, occupancy="base", may_coincide="both sides of the switch run the same cost model, and the two "
                      "scales price an occupied cell alike up to 0.8 %", defaults=dict(VEHICLE_DYNAMIC_PENALTY_SCALE=64.0, VEHICLE_OBSTACLE_PENALTY_VEHICLE=100)),
    "switch_hi": dict(half=False, occupancy="base", may_coincide="as switch_lo",
                      defaults=dict(VEHICLE_DYNAMIC_PENALTY_SCALE=64.5, VEHICLE_OBSTACLE_PENALTY_VEHICLE=100)),
    "field_edge": dict(half=True, occupancy="base", defaults=dict(VEHICLE_DYNAMIC_PENALTY_SCALE=64.0, VEHICLE_OBSTACLE_PENALTY_VEHICLE=16000)),
}
ASTAR_INF = 0x3F3F3F3F


def cost_constants(name):
    """Every constant of COST_DEFAULTS under the set `name` ("defaults" = config.py untouched)."""
    return {**COST_DEFAULTS, **(COST_SETS[name]["defaults"] if name != "defaults" else {})}


SCENARIOS = {
    # config-2 style: car-following + move only (lights disabled, replans gated off)
    "carfollow_64_s1": dict(size=64, seed=1, vehicles=60, ticks=80,
                            defaults={**CLOSED, **GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "DISABLED"}),
    "carfollow_96_s2": dict(size=96, seed=2, vehicles=400, ticks=60,
                            defaults={**CLOSED, **GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "DISABLED"}),
    "carfollow_128_s3": dict(size=128, seed=3, vehicles=900, ticks=50,
                             defaults={**CLOSED, **GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "DISABLED"}),
    # lights on (queue actuated), replans still gated off: isolates the light kernels
    "lights_qa_96_s2": dict(size=96, seed=2, vehicles=300, ticks=120,
                            defaults={**CLOSED, **GATED}),
    "lights_fixed_64_s4": dict(size=64, seed=4, vehicles=60, ticks=100,
                               defaults={**CLOSED, **GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "FIXED_TIME"}),
    # NOTE: "PRESSURE_CONTROL" cannot be captured: run_pressure_control reshapes the occupancy map to
    # (-1, 2) before indexing it as [y, x] (intersection_light_group.py:449-454) -> IndexError when the
    # helper runs un-jitted (and an out-of-row read under numba).  Reference defect; parity unpinned.
    "lights_npress_96_s6": dict(size=96, seed=6, vehicles=200, ticks=60,
                                defaults={**CLOSED, **GATED,
                                          "TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_PRESSURE_CONTROL"}),
    "lights_gwave_96_s7": dict(size=96, seed=7, vehicles=200, ticks=60,
                               defaults={**CLOSED, **GATED,
                                         "TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_GREEN_WAVE"}),
    # config-3 style: defaults (queue-actuated lights, full replanning policy), closed population
    "full_64_s1": dict(size=64, seed=1, vehicles=50, ticks=120, defaults={**CLOSED}),
    "full_96_s8": dict(size=96, seed=8, vehicles=250, ticks=80, defaults={**CLOSED}),
    # strandings made frequent: malfunction / sideswipe / contraflow overtake / stuck detour paths
    "faults_64_s9": dict(size=64, seed=9, vehicles=70, ticks=150,
                         defaults={**CLOSED, "VEHICLE_MALFUNCTION_CHANCE": 0.004,
                                   "VEHICLE_MALFUNCTION_DURATION": 25,
                                   "VEHICLE_SIDESWIPE_COLLISION_CHANCE": 0.2,
                                   "VEHICLE_SIDESWIPE_COLLISION_DURATION": 30}),
    # _despawn_check (vehicle_base.py:695-706) switched on with low thresholds: stuck vehicles leave mid-run (errored_* counters)
    "despawn_96_s25": dict(size=96, seed=25, vehicles=260, ticks=140,
                           defaults={**CLOSED, "VEHICLE_STUCK_DESPAWN_ENABLED": True, "VEHICLE_STUCK_DESPAWN_THRESHOLD": 14,
                                     "VEHICLE_STUCK_DESPAWN_THRESHOLD_INTERSECTION": 4}),
    # VEHICLE_RESPECT_AWARENESS: every search of the replanning policy masks obstacles outside the field of view
    "fov_96_s26": dict(size=96, seed=26, vehicles=220, ticks=100, defaults={**CLOSED, "VEHICLE_RESPECT_AWARENESS": True}),
    # trips that end where they start (vehicle_base.py:657-661): the vehicle despawns INSIDE the decide phase and the list
    # iterator of run_parallel_decide (city_model.py:1817-1827) skips the vehicle that follows it; `start_goal` = indices of
    # such vehicles (first / last of the list, neighbours, runs of three)
    "startgoal_96_s27": dict(size=96, seed=27, vehicles=120, ticks=60, defaults={**CLOSED},
                             start_goal=[0, 7, 8, 20, 21, 22, 40, 55, 56, 90, 118, 119]),
    # config-5 style: sub-block roads + L-shaped carves
    "carve_96_s10": dict(size=96, seed=10, vehicles=200, ticks=60,
                         defaults={**CLOSED}, model_kwargs=dict(carve_subblock_roads=True)),
    # "next" row 2: the traffic generator spawning internal + through trips mid-tick (rain and service vehicles off)
    "dta_64_s12": dict(size=64, seed=12, vehicles=20, ticks=260,
                       defaults={"RAIN_ENABLED": False, "TOTAL_SERVICE_VEHICLES_FOOD": 0, "TOTAL_SERVICE_VEHICLES_WASTE": 0}),
    "dta_96_s13": dict(size=96, seed=13, vehicles=40, ticks=160,
                       defaults={"RAIN_ENABLED": False, "TOTAL_SERVICE_VEHICLES_FOOD": 0, "TOTAL_SERVICE_VEHICLES_WASTE": 0,
                                 "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 60000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 20000}),
    # "next" row 4: rain clouds (RainManager / RainAgent) on a closed population
    "rain_96_s14": dict(size=96, seed=14, vehicles=150, ticks=220,
                        defaults={"INTERNAL_POPULATION_TRAFFIC_PER_DAY": 0, "PASSING_POPULATION_TRAFFIC_PER_DAY": 0,
                                  "TOTAL_SERVICE_VEHICLES_FOOD": 0, "TOTAL_SERVICE_VEHICLES_WASTE": 0, **GATED,
                                  "RAIN_RADIUS_MIN": 10, "RAIN_RADIUS_MAX": 30, "RAIN_SPAWN_CHANCE": 0.2}),
    # "next" row 3: service vehicles + CityBlock food / waste (rain off); long enough for several service trips
    "service_64_s15": dict(size=64, seed=15, vehicles=10, ticks=900, defaults={"RAIN_ENABLED": False}),
    # the same with a large fleet: several vehicles servicing at once (parked blockers, contested service cells,
    # decide-phase arrivals), strandings frequent
    "service_heavy_96_s16": dict(size=96, seed=16, vehicles=20, ticks=500,
                                 defaults={"RAIN_ENABLED": False, "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 3000,
                                           "PASSING_POPULATION_TRAFFIC_PER_DAY": 1500,
                                           "TOTAL_SERVICE_VEHICLES_FOOD": 600, "TOTAL_SERVICE_VEHICLES_WASTE": 600,
                                           "VEHICLE_MALFUNCTION_CHANCE": 0.002, "VEHICLE_MALFUNCTION_DURATION": 25}),
    # config-5 style with every subsystem on: sub-block roads + L-shaped carves, traffic generator, service fleet,
    # rain, queue-actuated lights, full replanning policy
    "config5_96_s17": dict(size=96, seed=17, vehicles=60, ticks=300,
                           defaults={"RAIN_RADIUS_MIN": 10, "RAIN_RADIUS_MAX": 25, "RAIN_SPAWN_CHANCE": 0.15,
                                     "TOTAL_SERVICE_VEHICLES_FOOD": 200, "TOTAL_SERVICE_VEHICLES_WASTE": 200,
                                     "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 6000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 2400},
                           model_kwargs=dict(carve_subblock_roads=True)),
    # non-square grids with every subsystem on (wide and tall): row-major indexing, rain drift, exits on all four edges
    "rect_96x64_s18": dict(size=96, height=64, seed=18, vehicles=60, ticks=220,
                           defaults={"RAIN_RADIUS_MIN": 8, "RAIN_RADIUS_MAX": 20, "RAIN_SPAWN_CHANCE": 0.15,
                                     "TOTAL_SERVICE_VEHICLES_FOOD": 150, "TOTAL_SERVICE_VEHICLES_WASTE": 150,
                                     "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 8000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 3000}),
    "rect_64x112_s19": dict(size=64, height=112, seed=19, vehicles=60, ticks=220,
                            defaults={"RAIN_RADIUS_MIN": 8, "RAIN_RADIUS_MAX": 20, "RAIN_SPAWN_CHANCE": 0.15,
                                      "TOTAL_SERVICE_VEHICLES_FOOD": 150, "TOTAL_SERVICE_VEHICLES_WASTE": 150,
                                      "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 8000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 3000},
                            model_kwargs=dict(carve_subblock_roads=True)),
    # a ragged grid: neither side a multiple of the device's 8-cell tile (100 = 12 tiles + 4 cells, 75 = 9 tiles + 3 cells),
    # closed population under the default replanning policy (the shape of full_96_s8)
    "ragged_100x75_s33": dict(size=100, height=75, seed=33, vehicles=220, ticks=70, defaults={**CLOSED}),
    # constructor variants of the world under a live run (every subsystem on): full-width intersections, a highway ring,
    # no ring road, forward light ranges feeding the neighbour-pressure controller's "out" lanes
    "unopt_96_s21": dict(size=96, seed=21, vehicles=60, ticks=200, defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_GREEN_WAVE"},
                         model_kwargs=dict(optimized_intersections=False)),
    "ring_r1_112_s22": dict(size=112, seed=22, vehicles=60, ticks=200, defaults={}, model_kwargs=dict(ring_road_type="R1")),
    "noring_96_s23": dict(size=96, seed=23, vehicles=60, ticks=200, defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "FIXED_TIME"},
                          model_kwargs=dict(ring_road_type=None)),
    "fwdrange_96_s24": dict(size=96, seed=24, vehicles=60, ticks=200,
                            defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_PRESSURE_CONTROL"},
                            model_kwargs=dict(forward_traffic_light_range=True,
                                              forward_traffic_light_range_intersections="Include in Range")),
    # the reference exactly as it ships: CityModel() at its default 200 x 200 with config.py untouched
    "default_200_s20": dict(size=200, seed=20, vehicles=120, ticks=160, defaults={}),
    # config 1 of BASELINE.json: everything on (rain, traffic generator, service vehicles, city blocks)
    "config1_64_s11": dict(size=64, seed=11, vehicles=50, ticks=500, defaults={}),
    # PATHFINDING_BATCHING=False (vehicle_base.py:666-685): step_decide inside step(), in the scheduler's shuffled order
    "nobatch_full_96_s28": dict(size=96, seed=28, vehicles=250, ticks=80, defaults={**CLOSED, "PATHFINDING_BATCHING": False}),
    "nobatch_config1_64_s29": dict(size=64, seed=29, vehicles=50, ticks=300, defaults={"PATHFINDING_BATCHING": False}),
    # ... with a busy service fleet (vehicles that start a service inside their own step_decide, i.e. inside their step())
    "nobatch_service_96_s30": dict(size=96, seed=30, vehicles=20, ticks=400,
                                   defaults={"RAIN_ENABLED": False, "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 3000,
                                             "PASSING_POPULATION_TRAFFIC_PER_DAY": 2000, "TOTAL_SERVICE_VEHICLES_FOOD": 3000,
                                             "TOTAL_SERVICE_VEHICLES_WASTE": 3000, "SERVICE_VEHICLE_LOAD_TIME": 1,
                                             "SERVICE_VEHICLE_MAX_LOAD_FOOD": 50, "PATHFINDING_BATCHING": False}),
    # the shape of full_96_s8 with the A* cost constants moved (COST_SETS below): every search of a live run - spawn, replans,
    # soft retries, contraflow detours - under non-default penalties.  PATHFINDING_COOLDOWN 2 and a stuck threshold of 10 make
    # vehicles replan (and fall back to soft searches) several times as often as the defaults do, so that ~80 ticks record
    # a few hundred searches beyond the spawn-time ones.
    # ... all-integer penalties (half-unit searches, the only form the quad searcher runs) and a density window of r = 6
    "costs_int_96_s31": dict(size=96, seed=31, vehicles=250, ticks=80,
                             defaults={**CLOSED, **COST_SETS["ints"]["defaults"], "VEHICLE_AWARENESS_RANGE": 6,
                                       "PATHFINDING_COOLDOWN": 2, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": 10}),
    # ... non-dyadic road-type penalties and scale: searches in doubles, costs stored truncated
    "costs_frac_96_s32": dict(size=96, seed=32, vehicles=250, ticks=80,
                              defaults={**CLOSED, **COST_SETS["nondyadic"]["defaults"],
                                        "PATHFINDING_COOLDOWN": 2, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": 10}),
}


def _setup_paths():
    import multiprocessing
    multiprocessing.cpu_count = lambda: 1
    sys.path.insert(0, os.path.join(HERE, "standins"))
    sys.path.insert(1, REF)


def _crc_path(path):
    import numpy as np
    if not path:
        return 0
    a = np.asarray(path, dtype=np.int32).reshape(-1, 2)
    return zlib.crc32(a.tobytes()) & 0xFFFFFFFF


def _rng_fp(state):
    """(crc32 of the 624 key words, index) of a random.getstate() tuple."""
    import numpy as np
    words = np.asarray(state[1][:624], dtype=np.uint32)
    return zlib.crc32(words.tobytes()) & 0xFFFFFFFF, int(state[1][624])


DIRI = {"N": 0, "E": 1, "S": 2, "W": 3, None: -1}


def world_tables(m):
    """G1: everything the hot path consumes from world-gen."""
    import numpy as np
    from Simulation.config import Defaults as _D
    Defaults_AVAILABLE = _D.AVAILABLE_CITY_BLOCKS
    from Simulation.agents.city_structure_entities.intersection_light_group import IntersectionLightGroup
    from Simulation.agents.city_structure_entities.city_block import CityBlock
    out = dict(
        width=np.int32(m.width), height=np.int32(m.height),
        allowed_dirs_map=m.allowed_dirs_map.copy(), is_road_map=m.is_road_map.copy(),
        road_type_map=m.road_type_map.copy(), intersection_map=m.intersection_map.copy(),
        stop_map0=m.stop_map.copy(),
    )
    # what the portrayal layer reads per cell: CellAgent.cell_type (as an index into this list) and .block_id (0 = None)
    names = ["Wall", "Sidewalk", "Nothing", "R1", "R2", "R3", "Intersection", "BlockEntrance", "HighwayEntrance",
             "HighwayExit", "ControlledRoad", "TrafficLight", "Residential", "Office", "Market", "Leisure", "Other", "Empty"]
    ctm = np.zeros((m.height, m.width), dtype=np.int8)
    bim = np.zeros((m.height, m.width), dtype=np.int32)
    for y in range(m.height):
        for x in range(m.width):
            c = m.get_cell_contents(x, y)[0]
            ctm[y, x] = names.index(c.cell_type)
            bim[y, x] = c.block_id or 0
    out["cell_type_map"], out["block_id_map"] = ctm, bim
    groups = m.intersection_light_groups
    gidx = {id(g): i for i, g in enumerate(groups)}
    # ragged tables: (offsets[G+1], flat values)
    def ragged(rows, width):
        off = [0]
        flat = []
        for r in rows:
            flat.extend(r)
            off.append(len(flat) // width if width > 1 else len(flat))
        arr = np.asarray(flat, dtype=np.int32)
        if width > 1:
            arr = arr.reshape(-1, width)
        return np.asarray(off, dtype=np.int32), arr

    light_rows, ctrl_rows_per_light = [], []
    lights_flat = []          # every light of every group, in group.traffic_lights order
    light_off = [0]
    for g in groups:
        for tl in g.traffic_lights:
            lights_flat.append(tl)
        light_off.append(len(lights_flat))
    lidx = {id(tl): i for i, tl in enumerate(lights_flat)}
    out["g_light_off"] = np.asarray(light_off, dtype=np.int32)
    out["light_xy"] = np.asarray([tl.position for tl in lights_flat], dtype=np.int32).reshape(-1, 2)
    out["light_ctrl_off"], out["light_ctrl_xy"] = ragged(
        [[c for cb in tl.controlled_blocks for c in cb.position] for tl in lights_flat], 2)
    # populate_links() runs inside the group constructor, BEFORE the model assigns
    # cell.intersection_group (city_model.py:1639-1650), so at construction opposite_pairs is empty
    # and neighbor_groups only sees earlier groups.  The first _execute_phase_change that reaches
    # get_opposite_traffic_lights() (intersection_light_group.py:303-307, 369) re-runs
    # populate_links() and the tables become complete.  Record both states without disturbing the
    # model: "ctor" = as constructed, full = after re-population.
    nb_ctor = np.full((len(groups), 4, 2), -1, dtype=np.int32)
    for i, g in enumerate(groups):
        for k, (d, ng) in enumerate((g.neighbor_groups or {}).items()):
            nb_ctor[i, k] = (DIRI[d], gidx.get(id(ng), -1))
        assert g.opposite_pairs == {"N-S": [], "W-E": []}, g.opposite_pairs
    out["g_neighbors_ctor"] = nb_ctor
    # intermediate_groups: a set of agents (iteration order carries no meaning) -> ascending group indices
    out["g_intermediate_ctor_off"], out["g_intermediate_ctor"] = ragged(
        [sorted(gidx[id(x)] for x in (g.intermediate_groups or ())) for g in groups], 1)
    saved = [(g.neighbor_groups, g.intermediate_groups, g.opposite_pairs) for g in groups]
    for g in groups:
        g.populate_links()
    out["g_ns_lights_off"], out["g_ns_lights"] = ragged(
        [[lidx[id(tl)] for tl in g.opposite_pairs["N-S"]] for g in groups], 1)
    out["g_ew_lights_off"], out["g_ew_lights"] = ragged(
        [[lidx[id(tl)] for tl in g.opposite_pairs["W-E"]] for g in groups], 1)
    nb = np.full((len(groups), 4, 2), -1, dtype=np.int32)
    for i, g in enumerate(groups):
        for k, (d, ng) in enumerate((g.neighbor_groups or {}).items()):
            nb[i, k] = (DIRI[d], gidx.get(id(ng), -1))
    out["g_neighbors"] = nb
    out["g_intermediate_off"], out["g_intermediate"] = ragged(
        [sorted(gidx[id(x)] for x in (g.intermediate_groups or ())) for g in groups], 1)
    for g, (a, b, c) in zip(groups, saved):
        g.neighbor_groups, g.intermediate_groups, g.opposite_pairs = a, b, c
    out["g_icell_off"], out["g_icell_xy"] = ragged(
        [[c for cell in g.intersection_cells for c in cell.position] for g in groups], 2)
    for nm in ("ns_in", "ns_out", "ew_in", "ew_out"):
        out[f"g_{nm}_off"], out[f"g_{nm}_xy"] = ragged(
            [[int(c) for xy in np.asarray(getattr(g, nm + "_coords")).reshape(-1, 2) for c in xy]
             for g in groups], 2)
    # schedule layout in insertion order: 0 = light group, 1 = city block, 2 = rain manager,
    # 3 = traffic generator, 4 = other
    kinds = []
    for a in m.schedule.agents:
        if isinstance(a, IntersectionLightGroup):
            kinds.append(0)
        elif isinstance(a, CityBlock):
            kinds.append(1)
        elif type(a).__name__ == "RainManager":
            kinds.append(2)
        elif type(a).__name__ == "DynamicTrafficAgent":
            kinds.append(3)
        else:
            kinds.append(4)
    out["schedule_kinds0"] = np.asarray(kinds, dtype=np.int8)
    # city blocks in city_blocks dict order (what get_city_blocks_by_type iterates): type index into
    # Defaults.AVAILABLE_CITY_BLOCKS and the entrance cells of each block (CityBlock.get_entrances())
    blocks = list(getattr(m, "city_blocks", {}).values())
    types = list(Defaults_AVAILABLE)
    out["blk_id"] = np.asarray(list(getattr(m, "city_blocks", {}).keys()), dtype=np.int32)
    out["blk_type"] = np.asarray([types.index(b.block_type) for b in blocks], dtype=np.int32)
    out["blk_entr_off"], out["blk_entr_xy"] = ragged([[c for e in b.get_entrances() for c in e.position] for b in blocks], 2)
    out["blk_inner_cells"] = np.asarray([len(b.get_inner_blocks()) for b in blocks], dtype=np.int32)
    # CityBlock.get_service_road_cell (city_block.py:152-202) ranks a Python *set* of road cells with a stable sort,
    # so ties fall in CPython's set-iteration order.  Everything up to the ranking is static: replay the very same
    # sequence of set operations here, in the real interpreter, and record the ranked list per block.
    def ranked_service_cells(b):
        sidewalk_coords = [sw.get_position() for sw in b._sidewalks]
        candidates = set()
        for sx, sy in sidewalk_coords:
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                rx, ry = sx + dx, sy + dy
                if not m.in_bounds(rx, ry):
                    continue
                agents = m.get_cell_contents(rx, ry)
                if agents and agents[0].cell_type in _D.ROADS:
                    candidates.add((rx, ry))
        if not candidates:
            return []
        entrance_coords = [e.get_position() for e in b._entrances]
        for ex, ey in entrance_coords:
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                candidates.discard((ex + dx, ey + dy))
        if not candidates or not entrance_coords:
            return []
        return sorted(candidates, key=lambda rc: min(abs(rc[0] - ex) + abs(rc[1] - ey) for ex, ey in entrance_coords))
    out["blk_service_off"], out["blk_service_xy"] = ragged([[c for rc in ranked_service_cells(b) for c in rc] for b in blocks], 2)
    # labels of the UI's drop-downs (CellAgent.get_display_name), in the order of the tables they belong to
    out["display_names"] = np.asarray(json.dumps(dict(
        lights=[str(tl.get_display_name()) for tl in lights_flat],
        block_entrances=[str(c.get_display_name()) for c in m.block_entrances],
        highway_entrances=[str(c.get_display_name()) for c in m.highway_entrances],
        highway_exits=[str(c.get_display_name()) for c in m.highway_exits])))
    out["block_entrances_xy"] = np.asarray([c.position for c in m.block_entrances], dtype=np.int32).reshape(-1, 2)
    out["highway_entrances_xy"] = np.asarray([c.position for c in m.highway_entrances], dtype=np.int32).reshape(-1, 2)
    out["highway_exits_xy"] = np.asarray([c.position for c in m.highway_exits], dtype=np.int32).reshape(-1, 2)
    return out


VEH_FIELDS = ["spawn_idx", "x", "y", "base_speed", "current_speed", "max_steps", "direction",
              "stuck_ticks", "cooldown", "flags", "stranded_left", "steps_traveled",
              "path_len", "path_crc", "overtake_dur", "detour_dur"]
F_EARLY, F_STUCK, F_PARKED, F_COLL, F_MALF, F_OVER, F_DETOUR, F_BLOCKED, F_HASPREV = (1 << i for i in range(9))

GRP_FIELDS = ["current_phase", "pending_phase", "queue_timer", "gap_timer", "last_arrival",
              "fixed_time_timer", "ft_phase", "ns_pressure", "ew_pressure"]
CNT_FIELDS = ["stuck", "collisions", "malfunctions", "overtaking", "in_stuck_detour", "parked",
              "live_internal", "live_through", "count_completed_internal", "count_completed_through",
              "total_distance_internal", "total_distance_through", "errored_internal", "errored_through",
              "created_internal", "created_through", "live_service_food", "live_service_waste",
              "created_service_food", "created_service_waste"]


def veh_row(v):
    flags = 0
    flags |= F_EARLY if v._early_exit else 0
    flags |= F_STUCK if v.is_stuck else 0
    flags |= F_PARKED if v.is_parked else 0
    flags |= F_COLL if v.is_in_collision else 0
    flags |= F_MALF if v.is_in_malfunction else 0
    flags |= F_OVER if v.is_overtaking else 0
    flags |= F_DETOUR if v.is_in_stuck_detour else 0
    flags |= F_BLOCKED if v.blocked_by_vehicle else 0
    flags |= F_HASPREV if (v.previous_pos is not None and tuple(v.previous_pos) == tuple(v.pos)) else 0
    crc = _crc_path(v.path)
    return [v._g_idx, int(v.pos[0]), int(v.pos[1]), int(v.base_speed), int(v.current_speed), int(v.max_steps),
            DIRI[v.direction], int(v.stuck_ticks), int(v.path_retry_cooldown), flags,
            int(getattr(v, "_stranded_ticks_remaining", 0)), int(v.steps_traveled),
            len(v.path), crc - (1 << 32) if crc >= (1 << 31) else crc,
            int(v.overtaking_duration), int(v.stuck_detour_duration)]


def none_i(v):
    return -1 if v is None else int(v)


def run_scenario(name, stats_only=False):
    import numpy as np
    spec = SCENARIOS[name]
    _setup_paths()
    import random
    from Simulation.config import Defaults
    Defaults.SAVE_TOTAL_RESULTS = False
    Defaults.SAVE_INDIVIDUAL_RESULTS = False
    for k, v in spec["defaults"].items():
        assert hasattr(Defaults, k), k
        setattr(Defaults, k, v)
    seed = spec["seed"]
    random.seed(seed)
    from Simulation.city_model import CityModel
    from Simulation.agents.vehicles.vehicle_base import VehicleAgent
    import Simulation.agents.vehicles.vehicle_base as vb

    size = spec["size"]
    # DynamicTrafficAgent.__init__ ends with _generate_day(0), which draws from the global stream inside
    # CityModel.__init__: remember the state just before it so a replay can generate the same day
    import Simulation.agents.dynamic_traffic_generator as dtg
    pre_day0 = {}
    orig_gen = dtg.DynamicTrafficAgent._generate_day

    def gen_day(self, day_idx):
        if day_idx == 0 and "st" not in pre_day0:
            pre_day0["st"] = random.getstate()
        return orig_gen(self, day_idx)
    dtg.DynamicTrafficAgent._generate_day = gen_day
    m = CityModel(width=size, height=spec.get("height", size), seed=seed, **spec.get("model_kwargs", {}))
    if "st" in pre_day0:
        pre = pre_day0["st"][1]
    else:
        pre = random.getstate()[1]
    out = world_tables(m)
    out["scenario"] = np.asarray(json.dumps(dict(name=name, **{k: v for k, v in spec.items()})))
    out["defaults_json"] = np.asarray(json.dumps(spec["defaults"]))

    # numba float64 semantics for the soft penalty: density_map must be float64 when A* reads it
    orig_update = CityModel._update_density_map

    def upd(self):
        orig_update(self)
        self.density_map32 = self.density_map.astype(np.float32)
        self.density_map = self.density_map.astype(np.float64)
    CityModel._update_density_map = upd

    # count A* calls
    calls = {"n": 0}
    orig_astar = vb.astar

    def counting_astar(*a, **k):
        calls["n"] += 1
        return orig_astar(*a, **k)
    vb.astar = counting_astar

    m._update_density_map()

    # ---- vehicles: distinct non-intersection road starts, exit-block goals ----
    prng = random.Random(seed + 1)
    road_cells = [(x, y) for y in range(m.height) for x in range(m.width)
                  if m.is_road_map[y, x] == 1 and m.intersection_map[y, x] == 0]
    nveh = min(spec["vehicles"], len(road_cells))
    starts = prng.sample(road_cells, nveh)
    exits = m.get_exit_blocks()
    st_after_world = random.getstate()
    out["global_rng_after_worldgen"] = np.asarray(st_after_world[1], dtype=np.uint32)
    out["global_rng_before_day0"] = np.asarray(pre, dtype=np.uint32)
    dta0 = getattr(m, "dynamic_traffic_generator", None)
    out["dta_params"] = np.asarray(json.dumps(dict(
        P_int=int(Defaults.INTERNAL_POPULATION_TRAFFIC_PER_DAY), P_thr=int(Defaults.PASSING_POPULATION_TRAFFIC_PER_DAY),
        dt=int(Defaults.TIME_PER_STEP_IN_SECONDS),
        start_offset=int(Defaults.SIMULATION_STARTING_TIME_OF_DAY_HOURS * 3600 + Defaults.SIMULATION_STARTING_TIME_OF_DAY_MINUTES * 60),
        pending_day0=(len(dta0.pending) if dta0 is not None else 0),
        service_food=int(Defaults.TOTAL_SERVICE_VEHICLES_FOOD), service_waste=int(Defaults.TOTAL_SERVICE_VEHICLES_WASTE),
        max_load_food=float(Defaults.SERVICE_VEHICLE_MAX_LOAD_FOOD), max_load_waste=float(Defaults.SERVICE_VEHICLE_MAX_LOAD_WASTE),
        load_time=int(Defaults.SERVICE_VEHICLE_LOAD_TIME), gradual=bool(Defaults.GRADUAL_CITY_BLOCK_RESOURCES),
        food_capacity_per_cell=float(Defaults.FOOD_CAPACITY_PER_CELL), waste_capacity_per_cell=float(Defaults.WASTE_CAPACITY_PER_CELL),
        food_consumption_ticks=int(Defaults.FOOD_CONSUMPTION_TICKS), waste_production_ticks=int(Defaults.WASTE_PRODUCTION_TICKS))))
    out["sched_rng_initial"] = np.asarray(m.random.getstate()[1], dtype=np.uint32)
    v_start, v_goal, v_path_off, v_path_flat = [], [], [0], []
    vehicles = []
    for i, (sx, sy) in enumerate(starts):
        goal = prng.choice(exits)
        while goal.get_position() == (sx, sy):   # (a trip that ends where it starts is the business of `start_goal` below)
            goal = prng.choice(exits)
        start_cell = m.get_cell_contents(sx, sy)[0]
        if i in spec.get("start_goal", ()):
            goal = start_cell
        v = VehicleAgent(f"gv_{i}", m, start_cell, goal, population_type="through")
        v._g_idx = i
        vehicles.append(v)
        v_start.append((sx, sy))
        v_goal.append(goal.get_position())
        for p in v.path:
            v_path_flat.append((int(p[0]), int(p[1])))
        v_path_off.append(len(v_path_flat))
    out["v_start_xy"] = np.asarray(v_start, dtype=np.int32).reshape(-1, 2)
    out["v_goal_xy"] = np.asarray(v_goal, dtype=np.int32).reshape(-1, 2)
    out["v_path0_off"] = np.asarray(v_path_off, dtype=np.int32)
    out["v_path0_xy"] = np.asarray(v_path_flat, dtype=np.int32).reshape(-1, 2)
    out["astar_calls_spawn"] = np.int32(calls["n"])
    out["global_rng_after_spawn"] = np.asarray(random.getstate()[1], dtype=np.uint32)
    out["occupancy0"] = m.occupancy_map.copy()

    # vehicles spawned later by the traffic generator get indices >= nveh in creation order
    counter = {"n": nveh}
    orig_init = VehicleAgent.__init__

    def init(self, *a, **k):
        if not hasattr(self, "_g_idx"):
            self._g_idx = counter["n"]
            counter["n"] += 1
        orig_init(self, *a, **k)
    VehicleAgent.__init__ = init

    T = spec["ticks"]
    occ_t, stop_t, stuck_t, rain_t, rain_rows, blk_rows = [], [], [], [], [], []
    veh_rows, veh_off = [], [0]
    grp_rows = []
    cnt_rows = []
    rng_rows = []
    astar_per_tick = []
    nsched = []
    dta = getattr(m, "dynamic_traffic_generator", None)
    dens_ticks = {}
    raised = None
    stats_rows = []
    for t in range(T):
        c0 = calls["n"]
        try:
            m.step()
        except Exception as ex:  # the reference itself raised inside model.step(): record where, replay expects an error there
            raised = (t, f"{type(ex).__name__}: {ex}")
            T = t
            break
        astar_per_tick.append(calls["n"] - c0)
        if stats_only:      # DynamicTrafficAgent.cached_stats as the statistics panel reads it, whenever it changed
            snap = {k: (None if v is None else float(v) if isinstance(v, float) else int(v)) for k, v in dta.cached_stats.items()}
            if not stats_rows or snap != stats_rows[-1][1]:
                stats_rows.append([t, snap])
            continue
        occ_t.append(np.packbits(m.occupancy_map.astype(np.uint8).ravel()))
        stop_t.append(np.packbits(m.stop_map.astype(np.uint8).ravel()))
        stuck_t.append(np.packbits(m.stuck_map.astype(np.uint8).ravel()))
        rain_t.append(np.packbits((m.rain_map > 0).astype(np.uint8).ravel()))
        rm = getattr(m, "rain_manager", None)
        blk_rows.append([[float(b.get_food_units()), float(b.get_waste_units())] for b in getattr(m, "city_blocks", {}).values()])
        rain_rows.append([len(m.rains), rm.counter if rm else 0, rm.cooldown if rm else 0,
                          sum(r.radius for r in m.rains), int(sum(int(r.x) + int(r.y) for r in m.rains))])
        for v in m.active_vehicle_agents:
            veh_rows.append(veh_row(v))
        veh_off.append(len(veh_rows))
        grp_rows.append([[none_i(g.current_phase), none_i(g.pending_phase), g.queue_timer, g.gap_timer,
                          g.last_arrival, g.fixed_time_timer, g._ft_phase, int(g.ns_pressure), int(g.ew_pressure)]
                         for g in m.intersection_light_groups])
        cnt_rows.append([int(getattr(dta, f, 0)) if dta is not None else 0 for f in CNT_FIELDS])
        g_fp = _rng_fp(random.getstate())
        s_fp = _rng_fp(m.random.getstate())
        rng_rows.append([g_fp[0], g_fp[1], s_fp[0], s_fp[1]])
        nsched.append(len(m.schedule._agents))
        if t in (0, spec["ticks"] // 2):
            dens_ticks[t] = m.density_map32.copy()
    if stats_only:
        path = os.path.join(HERE, f"cached_stats_{name}.json")
        json.dump(dict(scenario=name, ticks=T, interval=int(Defaults.STATISTICS_UPDATE_INTERVAL), rows=stats_rows), open(path, "w"), indent=0)
        print(f"[{name}] cached_stats snapshots={len(stats_rows)} keys={len(stats_rows[-1][1]) if stats_rows else 0} -> {path}")
        return
    out["occ_t"] = np.stack(occ_t)
    out["stop_t"] = np.stack(stop_t)
    out["stuck_t"] = np.stack(stuck_t)
    out["rain_t"] = np.stack(rain_t)
    out["rain_rows"] = np.asarray(rain_rows, dtype=np.int64)
    out["blk_rows"] = np.asarray(blk_rows, dtype=np.float64)
    out["rain_params"] = np.asarray(json.dumps(dict(
        enabled=bool(Defaults.RAIN_ENABLED), radius_min=int(Defaults.RAIN_RADIUS_MIN), radius_max=int(Defaults.RAIN_RADIUS_MAX),
        occurrences_max=int(Defaults.RAIN_OCCURRENCES_MAX), cooldown=int(Defaults.RAIN_COOLDOWN),
        spawn_chance=float(Defaults.RAIN_SPAWN_CHANCE), spawn_offset=int(Defaults.RAIN_SPAWN_OFFSET))))
    out["veh_rows"] = np.asarray(veh_rows, dtype=np.int64).reshape(-1, len(VEH_FIELDS)).astype(np.int32)
    out["veh_off"] = np.asarray(veh_off, dtype=np.int32)
    out["grp_rows"] = np.asarray(grp_rows, dtype=np.int32).reshape(T, len(m.intersection_light_groups), len(GRP_FIELDS))
    out["cnt_rows"] = np.asarray(cnt_rows, dtype=np.int64)
    out["rng_rows"] = np.asarray(rng_rows, dtype=np.int64)
    out["astar_per_tick"] = np.asarray(astar_per_tick, dtype=np.int32)
    out["nsched_t"] = np.asarray(nsched, dtype=np.int32)
    for t, d in dens_ticks.items():
        out[f"density_t{t}"] = d
    if raised is not None:
        out["raised_at_tick"] = np.int32(raised[0])
        out["raised_message"] = np.asarray(raised[1][:200])
    out["veh_fields"] = np.asarray(json.dumps(VEH_FIELDS))
    out["grp_fields"] = np.asarray(json.dumps(GRP_FIELDS))
    out["cnt_fields"] = np.asarray(json.dumps(CNT_FIELDS))
    np.savez_compressed(os.path.join(HERE, f"trace_{name}.npz"), **out)
    print(f"[{name}] groups={len(m.intersection_light_groups)} vehicles={nveh} ticks={T} "
          f"astar/tick={np.mean(astar_per_tick):.2f} live_end={len(m.active_vehicle_agents)} "
          f"size={os.path.getsize(os.path.join(HERE, f'trace_{name}.npz'))}")


# --------------------------------------------------------------------------------------
# G2: A* KATs, G3: density, G4: MT streams
# --------------------------------------------------------------------------------------
def run_astar_kats():
    import numpy as np
    _setup_paths()
    import random
    from Simulation.config import Defaults
    Defaults.SAVE_TOTAL_RESULTS = False
    Defaults.SAVE_INDIVIDUAL_RESULTS = False
    for k, v in CLOSED.items():
        setattr(Defaults, k, v)
    random.seed(21)
    from Simulation.city_model import CityModel
    from Simulation.utilities.pathfinding.astar_numba import astar_numba
    out = {}
    for tag, size, seed, kw in (("a", 64, 21, {}), ("b", 80, 22, dict(carve_subblock_roads=True))):
        random.seed(seed)
        m = CityModel(width=size, height=size, seed=seed, **kw)
        prng = random.Random(seed * 7)
        road = [(x, y) for y in range(size) for x in range(size) if m.is_road_map[y, x] == 1]
        # random dynamic state: occupancy on ~12% of road cells, red on ~half of the lights
        for (x, y) in prng.sample(road, len(road) // 8):
            m.occupancy_map[y, x] = 1
        for tl in m.traffic_lights:
            if prng.random() < 0.5:
                tl.set_light_stop()
        m._update_density_map()
        dens64 = m.density_map.astype(np.float64)
        queries, paths, poff = [], [], [0]
        nq = 260
        for q in range(nq):
            (sx, sy), (gx, gy) = prng.choice(road), prng.choice(road)
            mode = q % 4
            soft, ign = bool(mode & 1), bool(mode & 2)
            maxs = 0x7FFFFFFF
            if ign:
                maxs = prng.choice([6, 20, 0x7FFFFFFF])
                if maxs != 0x7FFFFFFF:      # bounded searches: pick a nearby goal
                    cands = [(x, y) for (x, y) in road if 0 < abs(x - sx) + abs(y - sy) <= 8]
                    if cands:
                        gx, gy = prng.choice(cands)
            p = astar_numba(size, size, sx, sy, gx, gy, m.occupancy_map, m.stop_map, m.is_road_map,
                            m.road_type_map, m.allowed_dirs_map, respect_awareness=False, awareness_range=10,
                            density_map=dens64, soft_obstacles=soft, ignore_flow=ign, maximum_steps=maxs)
            queries.append([sx, sy, gx, gy, int(soft), int(ign), maxs])
            for c in p:
                paths.append((int(c[0]), int(c[1])))
            poff.append(len(paths))
        wt = world_tables(m)
        for k in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map"):
            out[f"{tag}_{k}"] = wt[k]
        out[f"{tag}_occupancy_map"] = m.occupancy_map.copy()
        out[f"{tag}_stop_map"] = m.stop_map.copy()
        out[f"{tag}_density32"] = m.density_map.astype(np.float32)
        out[f"{tag}_queries"] = np.asarray(queries, dtype=np.int64)
        out[f"{tag}_path_off"] = np.asarray(poff, dtype=np.int32)
        out[f"{tag}_path_xy"] = np.asarray(paths, dtype=np.int32).reshape(-1, 2)
        nonempty = sum(1 for i in range(nq) if poff[i + 1] > poff[i])
        print(f"[astar_kats/{tag}] {nq} queries, {nonempty} non-empty")
    np.savez_compressed(os.path.join(HERE, "astar_kats.npz"), **out)


def run_astar_fov_kats():
    """A* with respect_awareness=True (field-of-view masking, astar_numba.py:29-50): the worlds and dynamic state of
    run_astar_kats (same seeds), awareness ranges 10 and 3, all four (soft, ignore_flow) modes."""
    import numpy as np
    _setup_paths()
    import random
    from Simulation.config import Defaults
    Defaults.SAVE_TOTAL_RESULTS = False
    Defaults.SAVE_INDIVIDUAL_RESULTS = False
    for k, v in CLOSED.items():
        setattr(Defaults, k, v)
    from Simulation.city_model import CityModel
    from Simulation.utilities.pathfinding.astar_numba import astar_numba
    out = {}
    for tag, size, seed, kw in (("a", 64, 21, {}), ("b", 80, 22, dict(carve_subblock_roads=True))):
        random.seed(seed)
        m = CityModel(width=size, height=size, seed=seed, **kw)
        prng = random.Random(seed * 7)
        road = [(x, y) for y in range(size) for x in range(size) if m.is_road_map[y, x] == 1]
        for (x, y) in prng.sample(road, len(road) // 8):
            m.occupancy_map[y, x] = 1
        for tl in m.traffic_lights:
            if prng.random() < 0.5:
                tl.set_light_stop()
        m._update_density_map()
        dens64 = m.density_map.astype(np.float64)
        queries, paths, poff = [], [], [0]
        nq = 240
        differs = 0
        for q in range(nq):
            (sx, sy), (gx, gy) = prng.choice(road), prng.choice(road)
            mode = q % 4
            soft, ign = bool(mode & 1), bool(mode & 2)
            aw = 10 if (q // 4) % 2 == 0 else 3
            maxs = 0x7FFFFFFF
            if ign:
                maxs = prng.choice([6, 20, 0x7FFFFFFF])
                if maxs != 0x7FFFFFFF:
                    cands = [(x, y) for (x, y) in road if 0 < abs(x - sx) + abs(y - sy) <= 8]
                    if cands:
                        gx, gy = prng.choice(cands)
            # the density window follows the same Defaults.VEHICLE_AWARENESS_RANGE a live run passes as awareness_range
            Defaults.VEHICLE_AWARENESS_RANGE = aw
            m._update_density_map()
            dens64 = m.density_map.astype(np.float64)
            args = (size, size, sx, sy, gx, gy, m.occupancy_map, m.stop_map, m.is_road_map, m.road_type_map, m.allowed_dirs_map)
            p = astar_numba(*args, respect_awareness=True, awareness_range=aw, density_map=dens64, soft_obstacles=soft,
                            ignore_flow=ign, maximum_steps=maxs)
            p0 = astar_numba(*args, respect_awareness=False, awareness_range=aw, density_map=dens64, soft_obstacles=soft,
                             ignore_flow=ign, maximum_steps=maxs)
            differs += [tuple(c) for c in p] != [tuple(c) for c in p0]
            queries.append([sx, sy, gx, gy, int(soft), int(ign), maxs, aw])
            for c in p:
                paths.append((int(c[0]), int(c[1])))
            poff.append(len(paths))
        wt = world_tables(m)
        for k in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map"):
            out[f"{tag}_{k}"] = wt[k]
        out[f"{tag}_occupancy_map"] = m.occupancy_map.copy()
        out[f"{tag}_stop_map"] = m.stop_map.copy()
        out[f"{tag}_queries"] = np.asarray(queries, dtype=np.int64)
        out[f"{tag}_path_off"] = np.asarray(poff, dtype=np.int32)
        out[f"{tag}_path_xy"] = np.asarray(paths, dtype=np.int32).reshape(-1, 2)
        nonempty = sum(1 for i in range(nq) if poff[i + 1] > poff[i])
        print(f"[astar_fov_kats/{tag}] {nq} queries, {nonempty} non-empty, {differs} differ from the unmasked search")
    np.savez_compressed(os.path.join(HERE, "astar_fov_kats.npz"), **out)


def _cost_world(m, size, seed, occupancy):
    """The dynamic state of run_astar_kats on a fresh world (same draws from the same stream): occupancy on 1/8 of the road
    cells, red on about half of the lights; "dense" adds cells from a stream of its own until 1/4 of the road is occupied.
    Returns (road cells, the stream, positioned where run_astar_kats draws its queries)."""
    import random
    prng = random.Random(seed * 7)
    road = [(x, y) for y in range(size) for x in range(size) if m.is_road_map[y, x] == 1]
    base = prng.sample(road, len(road) // 8)
    for (x, y) in base:
        m.occupancy_map[y, x] = 1
    for tl in m.traffic_lights:
        if prng.random() < 0.5:
            tl.set_light_stop()
    if occupancy == "dense":
        taken = set(base)
        rest = [c for c in road if c not in taken]
        for (x, y) in random.Random(seed * 11).sample(rest, len(road) // 4 - len(base)):
            m.occupancy_map[y, x] = 1
    else:
        assert occupancy == "base", occupancy
    return road, prng


def run_astar_cost_set(name, occupancy, out_path):
    """One set of constants (or "defaults") in a process of its own: astar_numba.py binds its constants when it is imported."""
    import numpy as np
    from fractions import Fraction
    _setup_paths()
    import random
    from Simulation.config import Defaults
    Defaults.SAVE_TOTAL_RESULTS = False
    Defaults.SAVE_INDIVIDUAL_RESULTS = False
    for k, v in CLOSED.items():
        setattr(Defaults, k, v)
    consts = cost_constants(name)
    for k, v in consts.items():
        assert hasattr(Defaults, k), k
        if name == "defaults":
            assert getattr(Defaults, k) == v, (k, getattr(Defaults, k), v)      # COST_DEFAULTS is config.py's
        setattr(Defaults, k, v)
    from Simulation.city_model import CityModel
    import importlib
    an = importlib.import_module("Simulation.utilities.pathfinding.astar_numba")    # (the package rebinds the name to the function)
    for k, mod_name in COST_MODULE_NAMES.items():
        got = getattr(an, mod_name)
        assert got == consts[k] and type(got) is type(consts[k]), (mod_name, got, consts[k])
    aw = consts["VEHICLE_AWARENESS_RANGE"]
    turn = consts["VEHICLE_TURN_PENALTY"] if consts["VEHICLE_TURN_PENALTY_ENABLED"] else 0
    rmax = max(consts[f"VEHICLE_ROAD_TYPES_PENALTY_R{i}"] for i in (1, 2, 3)) if consts["VEHICLE_ROAD_TYPES_PENALTIES_ENABLED"] else 0
    veh, scale = consts["VEHICLE_OBSTACLE_PENALTY_VEHICLE"], consts["VEHICLE_DYNAMIC_PENALTY_SCALE"]
    dyn = consts["VEHICLE_DYNAMIC_PENALTIES_ENABLED"]
    out = {}
    for tag, size, seed, kw in (("a", 64, 21, {}), ("b", 80, 22, dict(carve_subblock_roads=True))):
        random.seed(seed)
        m = CityModel(width=size, height=size, seed=seed, **kw)
        road, prng = _cost_world(m, size, seed, occupancy)
        m._update_density_map()
        assert Defaults.VEHICLE_AWARENESS_RANGE == aw
        d32 = m.density_map.astype(np.float32)
        dens64 = m.density_map.astype(np.float64)
        occ_cells = [(x, y) for (x, y) in road if m.occupancy_map[y, x] == 1]
        # no cost can reach INF: the costs along any chain of relaxations belong to distinct cells (a cell is only entered
        # again at a smaller cost, and every step costs >= 1), so a cost is at most the sum over the cells of the map of the
        # largest cost of entering each.  (The cruder "largest step x cells" is printed beside it; field_edge exceeds that.)
        occ_pen = [int(veh * (1.0 + scale * float(dens64[y, x]))) if dyn else veh for (x, y) in occ_cells]
        step_flat = 1 + turn + consts["VEHICLE_CONTRAFLOW_PENALTY"] + consts["VEHICLE_OBSTACLE_PENALTY_STOP"] + rmax
        bound = size * size * step_flat + sum(occ_pen)
        crude = size * size * (step_flat + max(occ_pen))
        assert bound < ASTAR_INF, (name, tag, bound)
        # occupied cells whose penalty veh * (1 + scale * density) is a whole number in exact arithmetic (scale as the decimal
        # it is written as, density as the float32 it is stored as): in doubles it lands an ulp either side, int() decides
        sc = Fraction(str(scale))
        whole = sum(1 for (x, y) in occ_cells if (veh * (1 + sc * Fraction(float(d32[y, x])))).denominator == 1) if dyn else 0
        queries, paths, poff = [], [], [0]
        nq = 100
        # (a strict search whose goal cell is occupied or red fails whatever the constants are: strict queries go to free cells)
        free = [(x, y) for (x, y) in road if m.occupancy_map[y, x] == 0 and m.stop_map[y, x] == 0]
        for q in range(nq):
            mode = q % 4
            soft, ign = bool(mode & 1), bool(mode & 2)
            (sx, sy), (gx, gy) = prng.choice(road), prng.choice(road if soft else free)
            maxs = 0x7FFFFFFF
            if ign:
                maxs = prng.choice([6, 20, 0x7FFFFFFF])
                if maxs != 0x7FFFFFFF:      # bounded searches: pick a nearby goal (one the step limit does not rule out by itself)
                    cands = [(x, y) for (x, y) in (road if soft else free) if 0 < abs(x - sx) + abs(y - sy) <= min(8, maxs)]
                    if cands:
                        gx, gy = prng.choice(cands)
            elif not soft and (q // 4) % 4 != 3:
                # strict searches that respect the flow: with 1/8 of the road occupied and half of the lights red nearly every
                # long route is blocked, so three in four of them go to a goal within 10 cells
                cands = [(x, y) for (x, y) in free if 0 < abs(x - sx) + abs(y - sy) <= 10]
                if cands:
                    gx, gy = prng.choice(cands)
            p = an.astar_numba(size, size, sx, sy, gx, gy, m.occupancy_map, m.stop_map, m.is_road_map,
                               m.road_type_map, m.allowed_dirs_map, respect_awareness=False, awareness_range=aw,
                               density_map=dens64, soft_obstacles=soft, ignore_flow=ign, maximum_steps=maxs)
            queries.append([sx, sy, gx, gy, int(soft), int(ign), maxs])
            for c in p:
                paths.append((int(c[0]), int(c[1])))
            poff.append(len(paths))
        wt = world_tables(m)
        for k in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map"):
            out[f"{tag}_{k}"] = wt[k]
        out[f"{tag}_occupancy_map"] = m.occupancy_map.copy()
        out[f"{tag}_stop_map"] = m.stop_map.copy()
        out[f"{tag}_density32"] = d32
        out[f"{tag}_queries"] = np.asarray(queries, dtype=np.int64)
        out[f"{tag}_path_off"] = np.asarray(poff, dtype=np.int32)
        out[f"{tag}_path_xy"] = np.asarray(paths, dtype=np.int32).reshape(-1, 2)
        out[f"{tag}_stats"] = np.asarray([bound, crude, whole, len(occ_cells)], dtype=np.int64)
    np.savez_compressed(out_path, **out)


def run_astar_cost_kats():
    """tests/golden/astar_cost_kats.npz: the A* KATs of run_astar_kats (same worlds, same dynamic state, 100 queries per world
    over the four (soft, ignore_flow) modes, step-limited contraflow queries included) under every set of COST_SETS."""
    import tempfile
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="cost_kats_")
    jobs = [(name, spec["occupancy"]) for name, spec in COST_SETS.items()] + [("defaults", "base"), ("defaults", "dense")]
    procs = [(name, occ, subprocess.Popen([sys.executable, os.path.abspath(__file__), "astar_cost_set", name, occ,
                                           os.path.join(tmp, f"{name}_{occ}.npz")], cwd="/tmp", stdout=subprocess.DEVNULL))
             for name, occ in jobs]
    for name, occ, p in procs:
        assert p.wait() == 0, (name, occ)
    load = lambda name, occ: np.load(os.path.join(tmp, f"{name}_{occ}.npz"))
    dflt = {occ: load("defaults", occ) for occ in ("base", "dense")}
    out = {"sets": np.asarray(json.dumps(list(COST_SETS)))}
    problems = []
    for tag in ("a", "b"):
        for k in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map", "stop_map"):
            out[f"{tag}_{k}"] = dflt["base"][f"{tag}_{k}"]
        out[f"{tag}_occupancy_map_base"] = dflt["base"][f"{tag}_occupancy_map"]
        out[f"{tag}_occupancy_map_dense"] = dflt["dense"][f"{tag}_occupancy_map"]
    for name, spec in COST_SETS.items():
        k = load(name, spec["occupancy"])
        d = dflt[spec["occupancy"]]
        out[f"{name}_params"] = np.asarray(json.dumps(spec["defaults"]))
        out[f"{name}_occupancy"] = np.asarray(spec["occupancy"])
        for tag in ("a", "b"):
            for m in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map", "stop_map"):
                assert np.array_equal(k[f"{tag}_{m}"], out[f"{tag}_{m}"]), (name, tag, m)
            assert np.array_equal(k[f"{tag}_occupancy_map"], out[f"{tag}_occupancy_map_{spec['occupancy']}"])
            q, off, xy = k[f"{tag}_queries"], k[f"{tag}_path_off"], k[f"{tag}_path_xy"]
            assert np.array_equal(q, d[f"{tag}_queries"])
            doff, dxy = d[f"{tag}_path_off"], d[f"{tag}_path_xy"]
            nonempty = sum(1 for i in range(len(q)) if off[i + 1] > off[i])
            differs = sum(1 for i in range(len(q)) if off[i + 1] > off[i]
                          and not np.array_equal(xy[off[i]:off[i + 1]], dxy[doff[i]:doff[i + 1]]))
            bound, crude, whole, n_occ = (int(v) for v in k[f"{tag}_stats"])
            print(f"[astar_cost_kats/{name}/{tag}] {len(q)} queries, {nonempty} non-empty, {differs} differ from the defaults' paths, "
                  f"{whole} whole-number penalty cells of {n_occ} occupied, cost bound {bound} (largest step x cells: {crude})")
            if 2 * nonempty < len(q):
                problems.append((name, tag, "fewer than half of the queries return a path", nonempty))
            if "may_coincide" not in spec and 10 * differs < nonempty:
                problems.append((name, tag, "fewer than 10 % of the paths differ from the defaults' paths", differs, nonempty))
            if whole < spec.get("whole_cells", 0):
                problems.append((name, tag, "too few whole-number penalty cells", whole))
            out[f"{name}_{tag}_density32"] = k[f"{tag}_density32"]
            out[f"{name}_{tag}_queries"] = q
            out[f"{name}_{tag}_path_off"] = off
            out[f"{name}_{tag}_path_xy"] = xy
    assert not problems, problems      # (change the set or the dynamic state, not these conditions)
    np.savez_compressed(os.path.join(HERE, "astar_cost_kats.npz"), **out)
    print(f"[astar_cost_kats] size={os.path.getsize(os.path.join(HERE, 'astar_cost_kats.npz'))}")


def _density_ref(road, occ, r):
    """city_model.py:1764-1778 on given maps with scipy's own uniform_filter."""
    import numpy as np
    from scipy.ndimage import uniform_filter
    o = occ.astype(np.float32)
    so = uniform_filter(o, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0.0) * ((2 * r + 1) ** 2)
    rd = road.astype(np.float32)
    sr = uniform_filter(rd, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0.0) * ((2 * r + 1) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(sr > 0, so / sr, 0.0)
    assert d.dtype == np.float32, d.dtype
    return d


DENSITY_R_RADII = (1, 3, 6, 14, 16)
DENSITY_R_SHAPES = ((64, 64), (50, 97), (21, 21), (8, 40), (5, 5), (1, 33), (33, 1))


def run_density_r():
    """tests/golden/density_r_kats.npz: the density map at radii other than the default 10, on maps down to a single row or
    column (narrower than the window in one or both axes), an all-road fully occupied map and a map without roads."""
    import numpy as np
    rng = np.random.RandomState(6)
    out, maps = {}, []
    for (h, w) in DENSITY_R_SHAPES:
        road = (rng.rand(h, w) < 0.4).astype(np.int8)
        occ = ((rng.rand(h, w) < 0.4) & (road == 1)).astype(np.int8)
        maps.append((f"{h}x{w}", road, occ))
    for (h, w) in ((21, 21), (8, 40)):
        maps.append((f"full_{h}x{w}", np.ones((h, w), dtype=np.int8), np.ones((h, w), dtype=np.int8)))
        maps.append((f"noroad_{h}x{w}", np.zeros((h, w), dtype=np.int8), np.zeros((h, w), dtype=np.int8)))
    for tag, road, occ in maps:
        out[f"{tag}_road"], out[f"{tag}_occ"] = road, occ
        for r in DENSITY_R_RADII:
            out[f"{tag}_r{r}_density"] = _density_ref(road, occ, r)
    out["maps"] = np.asarray(json.dumps([t for t, _, _ in maps]))
    out["radii"] = np.asarray(DENSITY_R_RADII, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "density_r_kats.npz"), **out)
    print(f"[density_r] {len(maps)} maps x {len(DENSITY_R_RADII)} radii")


def run_density():
    """density_kats.npz (r = 10) and, through run_density_r, density_r_kats.npz (the other radii)."""
    import numpy as np
    from scipy.ndimage import uniform_filter
    run_density_r()
    rng = np.random.RandomState(5)
    out = {}
    for tag, (h, w) in (("a", (64, 64)), ("b", (50, 97)), ("c", (21, 21)), ("d", (8, 40))):
        road = (rng.rand(h, w) < 0.3).astype(np.int8)
        occ = ((rng.rand(h, w) < 0.35) & (road == 1)).astype(np.int8)
        if tag == "c":
            occ = road.copy()
        r = 10
        o = occ.astype(np.float32)
        so = uniform_filter(o, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0.0) * ((2 * r + 1) ** 2)
        rd = road.astype(np.float32)
        sr = uniform_filter(rd, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0.0) * ((2 * r + 1) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(sr > 0, so / sr, 0.0)
        assert d.dtype == np.float32, d.dtype
        out[f"{tag}_road"] = road
        out[f"{tag}_occ"] = occ
        out[f"{tag}_density"] = d
    np.savez_compressed(os.path.join(HERE, "density_kats.npz"), **out)
    print("[density] ok")


def run_mt():
    import random
    import numpy as np
    out = {}
    for s in (0, 1, 12345, 2 ** 31 + 7, 2 ** 40 + 3):
        r = random.Random(s)
        out[f"s{s}_state0"] = np.asarray(r.getstate()[1], dtype=np.uint32)
        out[f"s{s}_random"] = np.asarray([r.random() for _ in range(700)], dtype=np.float64)
        out[f"s{s}_randint15"] = np.asarray([r.randint(1, 5) for _ in range(700)], dtype=np.int32)
        out[f"s{s}_state_mid"] = np.asarray(r.getstate()[1], dtype=np.uint32)
        for n in (1, 2, 13, 1000, 4099):
            x = list(range(n))
            r.shuffle(x)
            out[f"s{s}_shuffle{n}"] = np.asarray(x, dtype=np.int32)
        out[f"s{s}_randint09999"] = np.asarray([r.randint(0, 9999) for _ in range(100)], dtype=np.int32)
        out[f"s{s}_state_end"] = np.asarray(r.getstate()[1], dtype=np.uint32)
    out["seeds"] = np.asarray([0, 1, 12345, 2 ** 31 + 7, 2 ** 40 + 3], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "mt_kats.npz"), **out)
    print("[mt] ok")


# world-only fixtures for trafficsimulation_amd/worldgen.py: (tag, width, height, seed, CityModel kwargs, Defaults overrides)
WORLD_CASES = [
    ("default200", 200, 200, 101, {}, {}),
    ("rect", 120, 90, 102, {}, {}),
    ("tall", 70, 130, 120, {}, {}),
    ("ring_r3", 96, 96, 103, dict(ring_road_type="R3"), {}),
    ("ring_r1", 96, 96, 104, dict(ring_road_type="R1"), {}),
    ("ring_none", 96, 96, 105, dict(ring_road_type=None), {}),
    ("unoptimised", 96, 96, 106, dict(optimized_intersections=False), {}),
    ("fwd_range", 128, 128, 107, dict(forward_traffic_light_range=True, forward_traffic_light_range_intersections="Include in Range"), {}),
    ("fwd_extra", 128, 128, 108, dict(forward_traffic_light_range=True, forward_traffic_light_range_intersections="Include as Extra"), {}),
    ("fwd_skip", 128, 128, 109, dict(forward_traffic_light_range=True), {}),
    ("carve_plain", 128, 128, 110, dict(carve_subblock_roads=True, subblock_roads_have_intersections=False, subblock_chance=1.0), {}),
    ("carve_dense", 128, 128, 111, dict(carve_subblock_roads=True, subblock_chance=1.0, min_subblock_spacing=3), {}),
    ("carve_r2", 128, 128, 121, dict(carve_subblock_roads=True, subblock_chance=0.8, subblock_road_type="R2"), {}),
    ("entrance_lvl1", 96, 96, 112, {}, dict(BLOCK_ENTRANCE_ROAD_LEVEL=1)),
    ("entrance_lvl2", 96, 96, 113, {}, dict(BLOCK_ENTRANCE_ROAD_LEVEL=2)),
    ("thin_wall", 80, 80, 114, dict(wall_thickness=5, sidewalk_ring_width=1, highway_offset_from_edges=3), {}),
    ("tight_blocks", 160, 160, 115, dict(min_block_spacing=4, max_block_spacing=8, r1_chance_mean=0.3, r2_chance_mean=0.4), {}),
    ("no_min_r1", 96, 96, 116, dict(min_r1_bands=0), {}),
    ("three_r1", 128, 128, 117, dict(min_r1_bands=3), {}),
    ("short_lights", 72, 72, 118, dict(traffic_light_range=2), {}),
    ("dummies", 64, 64, 119, dict(use_dummy_agents=True), {}),
    ("mostly_r3", 128, 128, 122, dict(r1_chance_mean=0.05, r2_chance_mean=0.2), {}),
] + [(f"seed{sd}", sz, sz, sd, {}, {}) for sd, sz in ((201, 64), (202, 64), (203, 80), (204, 96), (205, 96), (206, 112), (207, 128), (208, 144))]


def run_worlds():
    """tests/golden/worlds.npz: world tables + global stream state after CityModel.__init__ for WORLD_CASES."""
    import numpy as np
    _setup_paths()
    import random
    from Simulation.config import Defaults
    Defaults.SAVE_TOTAL_RESULTS = False
    Defaults.SAVE_INDIVIDUAL_RESULTS = False
    Defaults.RAIN_ENABLED = False
    Defaults.ENABLE_TRAFFIC = False
    from Simulation.city_model import CityModel
    out, index = {}, []
    for tag, w, h, seed, kw, dfl in WORLD_CASES:
        saved = {k: getattr(Defaults, k) for k in dfl}
        for k, v in dfl.items():
            setattr(Defaults, k, v)
        random.seed(seed)
        entry = dict(tag=tag, width=w, height=h, seed=seed, kwargs=kw, defaults=dfl)
        try:
            m = CityModel(width=w, height=h, seed=seed, **kw)
            t = world_tables(m)
            t["global_rng_state"] = np.asarray(random.getstate()[1], dtype=np.uint32)
            for k, v in t.items():
                out[f"{tag}/{k}"] = v
        except Exception as e:  # the reference itself rejects this configuration
            entry["raises"] = type(e).__name__
            print(f"[worlds] {tag}: reference raised {type(e).__name__}: {e}")
        for k, v in saved.items():
            setattr(Defaults, k, v)
        index.append(entry)
        print(f"[worlds] {tag} done")
    out["index"] = np.asarray(json.dumps(index))
    np.savez_compressed(os.path.join(HERE, "worlds.npz"), **out)
    print("[worlds] ok")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        jobs = ["mt", "density", "astar_kats", "astar_fov_kats", "astar_cost_kats", "worlds"] + list(SCENARIOS)
        for j in jobs:
            subprocess.run([sys.executable, os.path.abspath(__file__), j], check=True, cwd="/tmp")
        return
    if what == "mt":
        run_mt()
    elif what == "density":
        run_density()
    elif what == "astar_kats":
        run_astar_kats()
    elif what == "astar_fov_kats":
        run_astar_fov_kats()
    elif what == "astar_cost_kats":
        run_astar_cost_kats()
    elif what == "astar_cost_set":      # (a child of astar_cost_kats: one set of constants per process)
        run_astar_cost_set(sys.argv[2], sys.argv[3], sys.argv[4])
    elif what == "density_r":      # density_r_kats.npz alone (density_kats.npz is left as it is)
        run_density_r()
    elif what == "worlds":
        run_worlds()
    elif what == "stats":      # `make_golden.py stats <scenario>`: cached_stats_<scenario>.json only, the trace is left alone
        run_scenario(sys.argv[2], stats_only=True)
    else:
        run_scenario(what)


if __name__ == "__main__":
    main()
