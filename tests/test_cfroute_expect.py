"""The route expectation (tests/cfroute_expect.py) pinned to the definitions that exist already, without an engine: its labels
form the planes of tests/costfield_expect.py, its routes cost under `Rule` what the field says and end where the owner
plane says, a start heading pays its turn, and on the reference's recorded searches (tests/golden/astar_cost_kats.npz) a
route costs what the reference's path costs where turns are free and at most that where they are not."""
import numpy as np
import pytest

from tests import cfroute_expect as re_
from tests import costfield_expect as ce
from tests.test_costfield_expect import kat_queries, kat_rule

PARAM_SETS = ["default", "turn0", "flags_off", "ints"]
_cache = {}


def seeds_of(rule):
    """Six road cells, two of them twice: seed 6 undercuts seed 1 on its cell, seed 7 ties with seed 4."""
    road = np.argwhere(np.asarray(rule.is_road) == 1)[:, ::-1]
    pick = road[np.random.default_rng(11).choice(len(road), 6, replace=False)]
    return np.concatenate([pick, pick[[1, 4]]]), [0, 7, 3, 0, 12, 1, 2, 12]


def case(name, tag, mode):
    """(rule, seeds, costs, query, labels, hop plane) of one world, parameter set and mode, computed once."""
    key = (name, tag, mode)
    if key not in _cache:
        rule = kat_rule(name, tag)
        seeds, cost = seeds_of(rule)
        q = dict(mode=mode, soft=True, ignore_flow=(mode == "from"))
        L = re_.labels(rule, seeds, cost, **q)
        _cache[key] = (rule, seeds, cost, q, L, re_.hop_plane(rule, L, seeds, cost, **q))
    return _cache[key]


def price(rule, cells, p, **modes):
    """Rule.path_cost for a path whose first step is taken with heading p."""
    total = 0
    for (x, y), (nx, ny) in zip(cells[:-1], cells[1:]):
        d = list(zip(ce.DX, ce.DY)).index((nx - x, ny - y))
        c = rule.step(x, y, d, p, **modes)
        assert c is not None, "a route takes a step that does not exist"
        total, p = total + c, d
    return total


CASES = [(n, t, m) for n in PARAM_SETS for t in ("a", "b") for m in ("from", "to")]


@pytest.mark.parametrize("name,tag,mode", CASES)
def test_labels_form_the_planes_of_the_cost_field_expectation(name, tag, mode):
    rule, seeds, cost, q, L, _ = case(name, tag, mode)
    want_v, want_o = ce.field(rule, seeds, cost, **q)
    got_v, got_o = re_.planes(rule, L, mode)
    assert np.array_equal(got_v, want_v) and np.array_equal(got_o, want_o)
    assert (want_v != ce.UNREACHABLE).sum() > 100


@pytest.mark.parametrize("name,tag,mode", CASES)
def test_routes_cost_what_the_field_says_and_end_at_the_owner(name, tag, mode):
    rule, seeds, cost, q, L, hops = case(name, tag, mode)
    modes = {k: v for k, v in q.items() if k != "mode"}
    value, owner = re_.planes(rule, L, mode)
    nh = re_.headings(rule)
    assert nh == (1 if name in ("turn0", "flags_off") else 4)      # (a penalty of 0, the penalty switched off)
    routed = 0
    for y, x in np.argwhere(np.asarray(rule.is_road) == 1).tolist():
        dirs, c, o = re_.route(hops, L, mode, nh, (x, y))
        assert (c, o) == (int(value[y, x]), int(owner[y, x])), (x, y)
        if o < 0:
            assert dirs == []
            continue
        cells = re_.cells_of((x, y), dirs, mode)
        assert rule.path_cost(cells, **modes) == c - cost[o], (x, y)
        assert cells[0 if mode == "from" else -1] == tuple(seeds[o].tolist()) and cells[-1 if mode == "from" else 0] == (x, y)
        routed += 1
    assert routed > 100


@pytest.mark.parametrize("name,tag", [(n, t) for n in PARAM_SETS for t in ("a", "b")])
def test_a_start_heading_pays_its_turn(name, tag):
    rule, seeds, cost, q, L, hops = case(name, tag, "to")
    modes = {k: v for k, v in q.items() if k != "mode"}
    nh = re_.headings(rule)
    dearer = turned = 0
    for y, x in np.argwhere(np.asarray(rule.is_road) == 1)[::3].tolist():
        free = re_.route(hops, L, "to", nh, (x, y))
        for p in range(4):
            dirs, c, o = re_.route(hops, L, "to", nh, (x, y), p)
            assert (o < 0) == (free[2] < 0), (x, y, p)
            if o < 0:
                continue
            cells = re_.cells_of((x, y), dirs, "to")
            assert price(rule, cells, p, **modes) == c - cost[o] and cells[-1] == tuple(seeds[o].tolist()), (x, y, p)
            assert free[1] <= c <= free[1] + (rule.turn if nh == 4 else 0), (x, y, p)
            dearer += c > free[1]
            turned += bool(dirs) and dirs[0] != p and price(rule, cells, p, **modes) > rule.path_cost(cells, **modes)
    # with turns that cost, some heading makes the way dearer and some first step pays the penalty; without, none
    assert (dearer > 0 and turned > 0) if nh == 4 else (dearer == 0 and turned == 0)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("name", ["turn0", "flags_off", "ints"])
def test_routes_against_the_recorded_reference_searches(name, tag):
    """A FROM field seeded at a query's start: the route to the goal costs exactly the reference's path where turns are free
    (turn0, flags_off) and at most that under `ints`; no route where the reference found none.  The first five starts that
    have a path, with every query they appear in."""
    rule = kat_rule(name, tag)
    nh = re_.headings(rule)
    queries = kat_queries(name, tag)
    keys = []
    for sx, sy, _, _, soft, ign, path in queries:
        if path is not None and (sx, sy, soft, ign) not in keys:
            keys.append((sx, sy, soft, ign))
    checked = 0
    for sx, sy, soft, ign in keys[:5]:
        modes = dict(soft=soft, ignore_flow=ign)
        L = re_.labels(rule, [(sx, sy)], mode="from", **modes)
        hops = re_.hop_plane(rule, L, [(sx, sy)], mode="from", **modes)
        for qx, qy, gx, gy, qs, qi, path in queries:
            if (qx, qy, qs, qi) != (sx, sy, soft, ign):
                continue
            dirs, c, o = re_.route(hops, L, "from", nh, (gx, gy))
            if path is None:
                assert o == -1 or (gx, gy) == (sx, sy)
                continue
            ref = rule.path_cost(path, **modes)
            cells = re_.cells_of((gx, gy), dirs, "from")
            assert o == 0 and cells[0] == (sx, sy) and rule.path_cost(cells, **modes) == c
            assert c <= ref if name == "ints" else c == ref, (sx, sy, gx, gy, c, ref)
            checked += 1
    assert checked >= 5
