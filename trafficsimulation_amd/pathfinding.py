"""The reference's pathfinder operator seam on the device engine.

`Simulation/agents/vehicles/vehicle_base.py:11-16` binds a module-level `astar` chosen by
`Defaults.PATHFINDING_METHOD`; every back-end has the signature of `astar_numba` (astar_numba.py:243-256) and returns
the path as (x, y) tuples without the start cell.  `astar_hip` is that callable for this build (SURVEY.md §8(b),
seam 2): the search itself is `ts_astar` (the wave-cooperative kernel of csrc/astar.h, quirks of `astar_core`
included), the maps the caller passes are handed to an engine instance that is created once per set of static maps
and reused.

    from trafficsimulation_amd.pathfinding import astar_hip as astar     # in vehicle_base.py, next to the other choices

Differences a caller can observe:
  * `density_map` is not read: the engine derives the density from `occupancy_map` with the reference's own recipe
    (`_update_density_map`, bit-exact).  That equals the array the reference passes whenever its density is current,
    i.e. everywhere inside the decide phase; a search started mid-move with a stale `density_map` (soft mode only)
    would see the fresh one here.
  * `respect_awareness=True` (field-of-view masking, off by default: config.py:278) is carried: the engine for that flag
    is created with `TsParams.respect_awareness`, `awareness_range` being its `vehicle_awareness_range`.
  * the library must be present: there is no CPU fall-back.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _capi as capi

_cache: dict = {}     # (W, H, id(is_road), id(road_type), id(allowed)) -> (engine, the three arrays, awareness_range)


def _engine_for(width, height, is_road_map, road_type_map, allowed_dirs_map, awareness_range, factory: Optional[Callable],
                respect_awareness: bool = False):
    key = (int(width), int(height), id(is_road_map), id(road_type_map), id(allowed_dirs_map), int(awareness_range), bool(respect_awareness))
    hit = _cache.get(key)
    # the arrays are kept alive by the cache entry, so an equal id() means the very same objects
    if hit is not None and hit[1] is is_road_map and hit[2] is road_type_map and hit[3] is allowed_dirs_map:
        return hit[0]
    if factory is None:
        from ._lib import new_engine
        factory = new_engine          # raises when the HIP library is missing
    api = factory()
    p = api.default_params()
    p.vehicle_awareness_range = int(awareness_range)      # window of the density map (config.py:279) and of the field of view
    p.respect_awareness = 1 if respect_awareness else 0
    a = np.asarray(allowed_dirs_map)
    if a.shape != (height, width):
        raise ValueError(f"maps must be (height, width) = ({height}, {width}) arrays, got {a.shape}")
    api.create(a, is_road_map, road_type_map, np.zeros((height, width), np.int8), p)   # A* reads no intersection map
    _cache[key] = (api, is_road_map, road_type_map, allowed_dirs_map)
    return api


def astar_hip(width: int, height: int, start_x: int, start_y: int, goal_x: int, goal_y: int,
              occupancy_map: np.ndarray, stop_map: np.ndarray, is_road_map: np.ndarray, road_type_map: np.ndarray,
              allowed_dirs_map: np.ndarray, respect_awareness: bool = False, awareness_range: int = 10,
              density_map: Optional[np.ndarray] = None, soft_obstacles: bool = False, ignore_flow: bool = False,
              maximum_steps: int = 0x7FFFFFFF, _engine_factory: Optional[Callable] = None) -> List[Tuple[int, int]]:
    """astar_numba(width, height, sx, sy, gx, gy, occupancy_map, stop_map, is_road_map, road_type_map,
    allowed_dirs_map, respect_awareness, awareness_range, density_map, soft_obstacles, ignore_flow, maximum_steps).

    One limit the reference's operator does not have: a `maximum_steps` that can actually bind must not exceed 4094 (the
    device table keeps the step count of a search node in 12 bits).  A limit of width * height or more never binds (no chain
    of relaxations revisits a cell) and is accepted, as is the default 0x7FFFFFFF; a value in between raises EngineError
    (TS_E_UNSUPPORTED) - it is never silently clipped.  The reference's own callers pass 6, 20 or nothing."""
    api = _engine_for(width, height, is_road_map, road_type_map, allowed_dirs_map, awareness_range, _engine_factory, respect_awareness)
    api.debug_set_occupancy(occupancy_map)          # the dynamic planes as the caller sees them right now
    api.upload_map(capi.MAP_STOP, stop_map)
    xy = api.astar(int(start_x), int(start_y), int(goal_x), int(goal_y), bool(soft_obstacles), bool(ignore_flow),
                   int(min(maximum_steps, 0x7FFFFFFF)))
    return [(int(x), int(y)) for x, y in xy]


def astar_hip_batch(width: int, height: int, starts, goals, occupancy_map: np.ndarray, stop_map: np.ndarray,
                    is_road_map: np.ndarray, road_type_map: np.ndarray, allowed_dirs_map: np.ndarray,
                    respect_awareness: bool, awareness_range: int, density_map: Optional[np.ndarray],
                    maximum_steps: int = 3_000, ignore_flow: bool = False, soft_obstacles: bool = True,
                    _engine_factory: Optional[Callable] = None) -> List[List[Tuple[int, int]]]:
    """The reference's "many vehicles at once" operator, `astar_tensorflow_batch(width, height, starts, goals,
    occupancy_map, stop_map, is_road_map, road_type_map, allowed_dirs_map, respect_awareness, awareness_range, density_map,
    maximum_steps=3_000, ignore_flow=False, soft_obstacles=True)` (astar_tensorflow_batch.py:383-399): names, order and
    defaults are its own.  `starts` / `goals` are equally long sequences of (x, y); path i (cells as (x, y) tuples, start
    excluded, [] for "no path") answers pair i.

    The search semantics are those of `astar_numba` - the only A* this build carries - so every path equals what
    `astar_hip` returns for the same pair, flags and maps; the searches run side by side on the device
    (`ts_astar_batch`: one launch, one wavefront per search in flight) instead of one after the other.  The caveats of
    `astar_hip` apply: `density_map` is not read (the engine derives it from `occupancy_map`), `respect_awareness` selects
    an engine created with that flag, a binding `maximum_steps` must not exceed 4094 (a limit of width * height or more
    never binds and is accepted; in between raises EngineError TS_E_UNSUPPORTED), and the library must be present."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 2) if len(starts) else np.zeros((0, 2), np.int64)
    goals = np.asarray(goals, dtype=np.int64).reshape(-1, 2) if len(goals) else np.zeros((0, 2), np.int64)
    if len(starts) != len(goals):
        raise ValueError(f"starts and goals must pair up: {len(starts)} starts, {len(goals)} goals")
    api = _engine_for(width, height, is_road_map, road_type_map, allowed_dirs_map, awareness_range, _engine_factory, respect_awareness)
    api.debug_set_occupancy(occupancy_map)          # the dynamic planes as the caller sees them right now
    api.upload_map(capi.MAP_STOP, stop_map)
    limit = int(min(maximum_steps, 0x7FFFFFFF))
    if not api.has_astar_batch:
        # an engine without the batch entry - the CPU oracle, i.e. test infrastructure: the same queries one by one
        return [[(int(x), int(y)) for x, y in api.astar(int(s[0]), int(s[1]), int(g[0]), int(g[1]), bool(soft_obstacles),
                                                        bool(ignore_flow), limit)] for s, g in zip(starts, goals)]
    q = np.zeros((len(starts), 7), dtype=np.int64)
    q[:, 0:2], q[:, 2:4] = starts, goals
    q[:, 4], q[:, 5], q[:, 6] = int(bool(soft_obstacles)), int(bool(ignore_flow)), limit
    off, xy = api.astar_batch(q)
    cells = list(map(tuple, xy.tolist()))
    return [cells[off[i]:off[i + 1]] for i in range(len(starts))]


def release():
    """Destroy the cached engine instances (device memory of every set of static maps seen so far)."""
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()
