"""The cost-field expectation (tests/costfield_expect.py) against the reference's own recorded searches
(tests/golden/astar_cost_kats.npz), and against itself: TO as FROM on reversed edges, the owner rule, seed costs."""
import json
import os

import numpy as np
import pytest

from tests import costfield_expect as ce
from trafficsimulation_amd import costfield as cf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNBOUNDED = 0x7FFFFFFF
_kats = {}


def kats():
    if "k" not in _kats:
        z = np.load(os.path.join(GOLDEN, "astar_cost_kats.npz"))
        _kats["k"] = {n: z[n] for n in z.files}
    return _kats["k"]


def kat_rule(name, tag):
    k = kats()
    consts = {} if name == "default" else json.loads(str(k[f"{name}_params"]))
    occ = "base" if name == "default" else str(k[f"{name}_occupancy"])
    dens = k[f"{'ints' if name == 'default' else name}_{tag}_density32"]      # (same occupancy, same radius: same map)
    return ce.Rule(consts, k[f"{tag}_allowed_dirs_map"], k[f"{tag}_is_road_map"], k[f"{tag}_road_type_map"],
                   k[f"{tag}_occupancy_map_{occ}"], k[f"{tag}_stop_map"], dens)


def kat_queries(name, tag):
    """(sx, sy, gx, gy, soft, ignore_flow, the reference's path with the start in front or None) of every unbounded query."""
    k = kats()
    q, off, xy = k[f"{name}_{tag}_queries"], k[f"{name}_{tag}_path_off"], k[f"{name}_{tag}_path_xy"]
    out = []
    for i, (sx, sy, gx, gy, soft, ign, maxs) in enumerate(q.tolist()):
        if maxs != UNBOUNDED:
            continue
        path = [tuple(c) for c in xy[off[i]:off[i + 1]].tolist()]
        if path and path[0] != (sx, sy):
            path = [(sx, sy)] + path
        out.append((sx, sy, gx, gy, bool(soft), bool(ign), path or None))
    return out


def from_fields(rule, queries):
    """The FROM field of every (start, soft, ignore_flow) among the queries, computed once each."""
    fields = {}
    for sx, sy, _, _, soft, ign, _ in queries:
        key = (sx, sy, soft, ign)
        if key not in fields:
            fields[key] = ce.field(rule, [(sx, sy)], mode="from", soft=soft, ignore_flow=ign)[0]
    return fields


# what this fixture holds per set (turn0 and flags_off alike): unbounded queries, with a path, without
KAT_COUNTS = {"a": (65, 32, 33), "b": (62, 29, 33)}


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("name", ["turn0", "flags_off"])
def test_field_equals_the_reference_path_cost_where_turns_are_free(name, tag):
    """Without a turn penalty the heading does not matter, the reference's A* is optimal, and the field at the goal is the
    cost of the path it recorded; where it found none, the goal is unreachable."""
    rule, queries = kat_rule(name, tag), kat_queries(name, tag)
    fields = from_fields(rule, queries)
    equal = nopath = 0
    for sx, sy, gx, gy, soft, ign, path in queries:
        got = int(fields[(sx, sy, soft, ign)][gy, gx])
        if path is not None:
            assert path[-1] == (gx, gy)
            assert got == rule.path_cost(path, soft=soft, ignore_flow=ign), (sx, sy, gx, gy, soft, ign)
            equal += 1
        elif (sx, sy) != (gx, gy):
            assert got == ce.UNREACHABLE, (sx, sy, gx, gy, soft, ign)
            nopath += 1
    assert (len(queries), equal, nopath) == KAT_COUNTS[tag]


@pytest.mark.parametrize("tag,strictly_less", [("a", 21), ("b", 21)])
def test_field_is_at_most_the_reference_path_cost_where_turns_cost(tag, strictly_less):
    """Under set `ints` (turn penalty 3) the reference's A* keeps one heading per cell and is not optimal over headings: the
    field, exact over (cell, heading), is never more than its path's cost and often less."""
    rule, queries = kat_rule("ints", tag), kat_queries("ints", tag)
    fields = from_fields(rule, queries)
    less = n = 0
    for sx, sy, gx, gy, soft, ign, path in queries:
        if path is None:
            continue
        got, ref = int(fields[(sx, sy, soft, ign)][gy, gx]), rule.path_cost(path, soft=soft, ignore_flow=ign)
        assert ref is not None and got <= ref, (sx, sy, gx, gy, soft, ign)
        less += got < ref
        n += 1
    assert n == KAT_COUNTS[tag][1] and less == strictly_less


def test_to_is_from_on_reversed_edges():
    """value_TO(c) for seeds S = min over s of value_FROM seeded at c, read at s, plus seed_cost[s]: both are the minimum over
    the same paths c -> s."""
    rule = kat_rule("ints", "a")
    rng = np.random.default_rng(3)
    road = np.argwhere(np.asarray(rule.is_road) == 1)[:, ::-1]
    seeds = road[rng.choice(len(road), 3, replace=False)]
    cost = [4, 0, 9]
    to, owner = ce.field(rule, seeds, cost, mode="to", soft=True, ignore_flow=True)
    for x, y in road[rng.choice(len(road), 12, replace=False)].tolist():
        frm = ce.field(rule, [(x, y)], mode="from", soft=True, ignore_flow=True)[0]
        want = min((int(frm[sy, sx]) + c, i) for i, ((sx, sy), c) in enumerate(zip(seeds.tolist(), cost)))
        got = (int(to[y, x]), int(owner[y, x]))
        assert got == (want if want[0] < ce.INF else (ce.UNREACHABLE, -1)), (x, y)


def open_rule(W=9, H=7, **consts):
    """Every direction allowed everywhere, all road, nothing on it."""
    z = np.zeros((H, W), dtype=np.int8)
    return ce.Rule(dict(VEHICLE_ROAD_TYPES_PENALTIES_ENABLED=False, **consts), np.full((H, W), 15, dtype=np.uint8), z + 1, z, z, z,
                   z.astype(np.float32))


def test_owner_is_the_smallest_seed_index_among_the_nearest():
    rule = open_rule(VEHICLE_TURN_PENALTY_ENABLED=False)
    value, owner = ce.field(rule, [(6, 3), (2, 3), (2, 3)], mode="from")
    x, y = np.meshgrid(np.arange(9), np.arange(7))
    d0, d1 = abs(x - 6) + abs(y - 3), abs(x - 2) + abs(y - 3)
    assert np.array_equal(value, np.minimum(d0, d1))
    assert np.array_equal(owner, np.where(d0 <= d1, 0, 1))        # ties go to seed 0; seed 2 shares seed 1's cell and never owns
    assert not (owner == 2).any()


def test_a_seed_cost_that_loses_to_another_seeds_reach():
    rule = open_rule(VEHICLE_TURN_PENALTY_ENABLED=False)
    value, owner = ce.field(rule, [(1, 1), (3, 1)], [0, 5], mode="to")
    assert value[1, 3] == 2 and owner[1, 3] == 0                   # seed 1's own cell is cheaper through seed 0
    assert not (owner == 1).any()
    value, owner = ce.field(rule, [(1, 1), (3, 1)], [0, 1], mode="to")
    assert value[1, 3] == 1 and owner[1, 3] == 1 and value[1, 4] == 2 and owner[1, 4] == 1
    assert value[1, 2] == 1 and owner[1, 2] == 0                   # (2, 1): 1 either way, the smaller index owns


def test_max_cost_clips_and_turns_are_charged_after_the_first_step():
    rule = open_rule(VEHICLE_TURN_PENALTY=3)
    value, _ = ce.field(rule, [(4, 3)], mode="from")
    assert value[3, 8] == 4 and value[5, 4] == 2 and value[4, 5] == 2 + 3      # straight runs are free of turns, an L pays one
    clipped, owner = ce.field(rule, [(4, 3)], mode="from", max_cost=4)
    assert np.array_equal(clipped, np.where(value <= 4, value, ce.UNREACHABLE)) and np.array_equal(owner == -1, value > 4)


def test_python_constants_match_the_expectation():
    assert (cf.CF_INF, cf.CF_UNREACHABLE) == (ce.INF, ce.UNREACHABLE)
