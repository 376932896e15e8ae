"""A plain numpy model of the external light control (include/trafficsim_lights_ext.h): phases A and B of the reference's
run_batched_rl_control (utilities/light_group_managment/rl_simple.py:205-252), written from those lines.

Inputs: the light tables of a trace / world dict (g_ns_in_off ... g_neighbors_ctor, road_type_map), the occupancy and stuck
maps as (H, W) arrays, the controller state (`Ctrl`) and the actions.  Outputs: the state vectors, the next-state vectors
and the new controller state.  Everything is computed in Python floats (doubles) and rounded to float32 once, like
tf.convert_to_tensor(states, dtype=tf.float32) does (rl_simple.py:219).
"""
import numpy as np

DIMS = (7, 11, 13, 17, 19)
TIMER_NORM = 30.0     # getattr(cls, 'TRAFFIC_LIGHT_MAX_GREEN', 30): the class has no such attribute (rl_simple.py:110-113)


class Ctrl:
    """What persists between control calls, per group."""

    def __init__(self, n_groups, lights_on=True):
        self.rl_phase = np.zeros(n_groups, dtype=np.int32)      # _rl_phase
        self.rl_timer = np.zeros(n_groups, dtype=np.int32)      # rl_timer
        self.stored_ns = np.zeros(n_groups, dtype=np.int64)     # ig.pressure_ns as the last compute_pressure left it
        self.stored_ew = np.zeros(n_groups, dtype=np.int64)
        self.first_done = False                                 # every group has a pressure_ns attribute
        self.current = np.full(n_groups, -1, dtype=np.int32)    # current_phase, -1 = None
        self.pending = np.full(n_groups, 0 if lights_on else -1, dtype=np.int32)   # intersection_light_group.py:115-116
        self.repop = np.zeros(n_groups, dtype=bool)             # the group's first phase change has re-run populate_links()

    def copy(self):
        c = Ctrl(len(self.rl_phase))
        for k, v in self.__dict__.items():
            setattr(c, k, v.copy() if isinstance(v, np.ndarray) else v)
        return c

    def rows(self):
        return np.stack([self.rl_phase, self.rl_timer], axis=1).astype(np.int32)


def _cells(tabs, name, g):
    off = tabs[f"g_{name}_off"]
    return np.asarray(tabs[f"g_{name}_xy"]).reshape(-1, 2)[off[g]:off[g + 1]]


def static_features(tabs, penalties=(0.5, 5, 50.0)):
    """intersection_size and penalty_score (intersection_light_group.py:156-165).  The constructor computes both, and it runs
    before the model hands the group its intersection_cells (city_model.py:1639): len(intersection_cells) is 0 there, so the
    size is 0 for every group.  The road blocks of the penalty mean are the four coordinate lists together; their road types
    come from the table g_approach_road_types ([blocks, R1, R2, R3] per group) where the world has one, else from the
    road_type_map plane (which shows an R2 cell of the ring road as R1, city_model.py:2170-2172)."""
    G = len(tabs["g_ns_in_off"]) - 1
    if "g_approach_road_types" in tabs:
        c = np.asarray(tabs["g_approach_road_types"], dtype=np.float64)
        p1, p2, p3 = (float(p) for p in penalties)
        return np.zeros(G), np.where(c[:, 0] > 0, (c[:, 1] * p1 + c[:, 2] * p2 + c[:, 3] * p3) / np.maximum(c[:, 0], 1), 0.0)
    rt = np.asarray(tabs["road_type_map"])
    w = (0.0,) + tuple(float(p) for p in penalties)
    size = np.zeros(G)
    pen = np.zeros(G)
    for g in range(G):
        total, n = 0.0, 0
        for name in ("ns_in", "ns_out", "ew_in", "ew_out"):
            for x, y in _cells(tabs, name, g):
                total += w[int(rt[y, x])]
                n += 1
        pen[g] = total / n if n else 0.0
    return size, pen


def local_sums(tabs, flow):
    """compute_pressure's two sums for every group (rl_simple.py:50-51); an empty list sums to 0."""
    G = len(tabs["g_ns_in_off"]) - 1
    out = np.zeros((G, 2), dtype=np.int64)
    for g in range(G):
        for j, name in enumerate(("ns_in", "ew_in")):
            c = _cells(tabs, name, g)
            out[g, j] = int(flow[c[:, 1], c[:, 0]].astype(np.int64).sum()) if len(c) else 0
    return out


def _neighbours(tabs, ctrl, g):
    nb = (tabs["g_neighbors"] if ctrl.repop[g] else tabs["g_neighbors_ctor"])[g]
    return [int(n) for d, n in nb if d >= 0 and n >= 0]


def _vector(dim, g, occ_s, stk_s, ctrl, nbrs, value_of, size, pen):
    """get_rl_state (rl_simple.py:95-143); value_of(j) = (pressure_ns, pressure_ew) neighbour j holds when it is read."""
    cnt = max(1, len(nbrs))
    l_ns, l_ew = int(occ_s[g, 0]), int(occ_s[g, 1])
    v = [float(l_ns), float(l_ew), float(l_ns - l_ew), float(l_ew - l_ns)]
    v += [1.0, 0.0] if ctrl.rl_phase[g] == 0 else [0.0, 1.0]
    v.append(int(ctrl.rl_timer[g]) / TIMER_NORM)
    if dim > 7:
        v += [float(size[g]), float(pen[g]), sum(size[n] for n in nbrs) / cnt, sum(pen[n] for n in nbrs) / cnt]
    if dim > 11:
        vals = [value_of(n) for n in nbrs]
        v += [float(sum(a for a, _ in vals)) / cnt, float(sum(b for _, b in vals)) / cnt]
    if dim > 13:
        s_ns, s_ew = int(stk_s[g, 0]), int(stk_s[g, 1])
        v += [float(s_ns), float(s_ew), float(s_ns - s_ew), float(s_ew - s_ns)]
    if dim > 17:
        vals = [value_of(n) for n in nbrs]
        v += [float(sum(a for a, _ in vals)) / cnt, float(sum(b for _, b in vals)) / cnt]
    assert len(v) == dim
    return v


def _this_call(dim, occ_s, stk_s, j):
    """What group j's own get_rl_state leaves in pressure_ns / pressure_ew: its last compute_pressure is on the stuck map above
    13 dimensions (rl_simple.py:133-137), on the occupancy map otherwise."""
    s = stk_s if dim > 13 else occ_s
    return int(s[j, 0] - s[j, 1]), int(s[j, 1] - s[j, 0])


def phase_a(tabs, occ, stuck, ctrl, dim, static=None):
    """rl_simple.py:209-216, groups in table order.  Group i reads from a neighbour j < i what j wrote in this call, from j > i
    what the previous call left (avg_neighbor_pressures, 63-78: nothing is recomputed once the attribute exists); in the very
    first call the attribute is missing and is computed from the occupancy map on the spot."""
    assert dim in DIMS
    size, pen = static if static is not None else static_features(tabs)
    occ_s, stk_s = local_sums(tabs, occ), local_sums(tabs, stuck)
    G = len(occ_s)
    if not ctrl.first_done:
        ctrl.stored_ns = occ_s[:, 0] - occ_s[:, 1]
        ctrl.stored_ew = occ_s[:, 1] - occ_s[:, 0]
    out = np.zeros((G, dim), dtype=np.float64)
    for g in range(G):
        def value_of(j, g=g):
            return _this_call(dim, occ_s, stk_s, j) if j < g else (int(ctrl.stored_ns[j]), int(ctrl.stored_ew[j]))
        out[g] = _vector(dim, g, occ_s, stk_s, ctrl, _neighbours(tabs, ctrl, g), value_of, size, pen)
    for g in range(G):
        ctrl.stored_ns[g], ctrl.stored_ew[g] = _this_call(dim, occ_s, stk_s, g)
    ctrl.first_done = True
    return out.astype(np.float32)


def apply_phase(ctrl, g, phase):
    """intersection_light_group.py:386-393"""
    if phase == ctrl.current[g] or phase == ctrl.pending[g]:
        return
    ctrl.pending[g] = phase


def phase_b(tabs, occ, stuck, ctrl, actions, dim, min_green=5, static=None):
    """rl_simple.py:226-252.  By now every neighbour holds this call's value."""
    size, pen = static if static is not None else static_features(tabs)
    occ_s, stk_s = local_sums(tabs, occ), local_sums(tabs, stuck)
    G = len(occ_s)
    out = np.zeros((G, dim), dtype=np.float64)
    for g in range(G):
        ctrl.rl_timer[g] += 1
        if ctrl.rl_timer[g] == 1:
            apply_phase(ctrl, g, int(ctrl.rl_phase[g]))
        if int(actions[g]) == 1 and ctrl.rl_timer[g] >= min_green:
            ctrl.rl_phase[g] = 1 - ctrl.rl_phase[g]
            ctrl.rl_timer[g] = 0
        out[g] = _vector(dim, g, occ_s, stk_s, ctrl, _neighbours(tabs, ctrl, g),
                         lambda j: _this_call(dim, occ_s, stk_s, j), size, pen)
    return out.astype(np.float32)


def request(ctrl, phases):
    """ts_lights_ext_request: -1 = none, 0 / 1 = apply_phase on that group; no protocol state is touched."""
    for g, p in enumerate(phases):
        if int(p) >= 0:
            apply_phase(ctrl, g, int(p))


# ---- for the GPU tests of both light-control families ----------------------------------------------------------------------
FIXTURES = ["lights_ext_64_s45", "lights_ext_96_s42", "lights_ext_stuck_96_s43"]
# replanning gated off
GATED = {"PATHFINDING_COOLDOWN": 10 ** 9, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": 10 ** 9,
         "VEHICLE_STUCK_RECOMPUTE_THRESHOLD_INTERSECTION": 10 ** 9, "VEHICLE_CONTRAFLOW_OVERTAKE_ACTIVE": False,
         "VEHICLE_STUCK_CONTRAFLOW_ENABLED": False}


class Stepper:
    """An engine whose step(1) first does `before(tick)`; everything else is the engine's.  `groups` may be overridden."""

    def __init__(self, api, before, groups=None):
        self._api, self._before, self._groups, self.tick = api, before, groups, 0

    def __getattr__(self, name):
        return getattr(self._api, name)

    def step(self, n=1):
        for _ in range(n):
            self._before(self.tick)
            self._api.step(1)
            self.tick += 1

    def groups(self):
        return self._groups(self.tick - 1, self._api.groups()) if self._groups else self._api.groups()
