"""tests/selectlink_expect.py against tests/demand_expect.py on the golden traces, without an engine: the identities that tie the
select-link rule to the demand planes, and the coverage conditions that keep the fixtures from being vacuous (vehicles that cross
none, one and several gates, a gate crossed twice by one vehicle, a direction the mask shuts out, an empty gate, a closed tail
that drops crossings)."""
import functools

import numpy as np
import pytest

from tests import demand_expect as de
from tests import selectlink_expect as se
from tests.trace_util import trace_path
from trafficsimulation_amd.world import load_trace

TRACES = ["carfollow_64_s1", "carfollow_128_s3", "lights_qa_96_s2"]
LATER = 9                               # the one later tick
# vehicles that cross none / exactly one / several gates of set A before the first tick
FIRST_TICK_A = {"carfollow_64_s1": (34, 3, 23), "carfollow_128_s3": (336, 74, 490), "lights_qa_96_s2": (123, 38, 139)}


@functools.lru_cache(maxsize=None)
def case(name, t):
    """(trace, H, W, vehicles, spawn, n_spawned, whole-path planes, set A, set B) at tick t."""
    tr = load_trace(trace_path(name))
    H, W = int(tr["height"]), int(tr["width"])
    veh, spawn = de.fixture_vehicles(tr, t)
    whole = de.planes(H, W, veh)[0]
    A, B = se.gate_sets(whole, tr["is_road_map"])
    return tr, H, W, veh, spawn, len(tr["v_start_xy"]), whole, A, B


def popcount(m):
    return np.array([bin(int(v)).count("1") for v in m])


@pytest.mark.parametrize("query", de.QUERIES)
@pytest.mark.parametrize("t", [-1, LATER])
@pytest.mark.parametrize("name", TRACES)
def test_identities(name, t, query):
    tr, H, W, veh, spawn, n, whole, A, B = case(name, t)
    n_bins, bin_cells, open_tail = query
    planes = de.planes(H, W, veh, n_bins, bin_cells, bool(open_tail))
    for gates in (A, B):
        r = se.walk(H, W, veh, spawn, n, gates, n_bins, bin_cells, bool(open_tail))
        assert np.array_equal(r["cross"], se.from_planes(planes, gates)), "cross is not the planes summed over the gates' accepting cells"
        assert np.array_equal(r["pair"], r["pair"].T)
        assert np.array_equal(np.diag(r["pair"]), [int((r["mask"] >> g & 1).sum()) for g in range(len(gates))])
        assert int(r["pair"].sum()) == int((popcount(r["mask"]) ** 2).sum())
        assert int(r["crossings"].sum()) == int(r["cross"].sum()) == r["t_crossings"]
        assert np.all(r["crossings"] >= popcount(r["mask"])) and r["t_vehicles"] == len(veh)
        assert np.array_equal(r["first_step"] >= 0, r["mask"] != 0) and np.array_equal(r["first_gate"] >= 0, r["mask"] != 0)
        hit = r["mask"] != 0
        assert np.all(r["mask"][hit] >> r["first_gate"][hit].astype(np.uint32) & 1 == 1)
        assert np.array_equal(se.selected(r), r["walked"].astype(np.uint8))
        g0 = 1 << int(r["first_gate"][hit][0]) if hit.any() else 1
        some, rest = se.selected(r, any=g0), se.selected(r, none=g0)
        assert np.array_equal(some + rest, r["walked"].astype(np.uint8)) and np.array_equal(some, se.selected(r, all=g0))


@pytest.mark.parametrize("t", [-1, LATER])
@pytest.mark.parametrize("name", TRACES)
def test_the_fixtures_are_not_vacuous(name, t):
    tr, H, W, veh, spawn, n, whole, A, B = case(name, t)
    a = se.walk(H, W, veh, spawn, n, A)
    bits = popcount(a["mask"][a["walked"]])
    none, one, several = int((bits == 0).sum()), int((bits == 1).sum()), int((bits >= 2).sum())
    assert none > 0 and one > 0 and several > 0, (none, one, several)
    if t == -1:
        assert (none, one, several) == FIRST_TICK_A[name]
    x, y = A[0][0]
    assert 2 <= int((whole[:, y, x] > 0).sum()) <= 3, "the most loaded cell is entered from two or three directions"
    b = se.walk(H, W, veh, spawn, n, B)
    assert np.any(b["crossings"] > popcount(b["mask"])), "no vehicle crosses one gate of set B more than once"
    shut = [whole[d, cy, cx] for gate in B[:8] for cx, cy, ch in gate for d in range(4) if "NESW"[d] != ch]
    assert max(shut) > 0, "no direction that set B's masks shut out carries planned load"
    assert not b["cross"][8].any() and not b["pair"][8].any() and not (b["mask"] >> 8 & 1).any(), "the gate on an unused road cell"
    assert b["cross"][:8].any()
    closed, tail = se.walk(H, W, veh, spawn, n, A, 3, 5, False), se.walk(H, W, veh, spawn, n, A, 3, 5, True)
    assert 0 < closed["t_crossings"] < tail["t_crossings"], "a closed tail drops no crossing"
    assert tail["cross"].sum() == a["cross"].sum()


def test_od_and_selection_by_hand():
    """Three vehicles on a 4 x 3 map, two gates: the rule worked by hand."""
    H, W = 3, 4
    veh = [(0, 0, [(1, 0), (2, 0), (3, 0)]),              # east along the bottom row
           (3, 1, [(2, 1), (2, 0), (1, 0)]),              # west, south, west
           (0, 2, [])]                                     # no path left
    spawn, n = [0, 2, 3], 5
    gates = [[(2, 0, "E"), (1, 0, "W")], [(2, 0, "S"), (3, 0)]]
    r = se.walk(H, W, veh, spawn, n, gates, 2, 2, True)
    assert r["mask"].tolist() == [3, 0, 3, 0, 0] and r["crossings"].tolist() == [2, 0, 2, 0, 0]
    assert r["first_step"].tolist() == [1, -1, 1, -1, -1] and r["first_gate"].tolist() == [0, -1, 1, -1, -1]
    assert r["walked"].tolist() == [True, False, True, True, False]
    want = np.zeros((2, 2, 4), np.uint64)
    want[0, 0, 1] = want[1, 1, 1] = want[1, 0, 2] = want[0, 1, 3] = 1
    assert np.array_equal(r["cross"], want) and r["pair"].tolist() == [[2, 2], [2, 2]]
    assert (r["t_vehicles"], r["t_crossing"], r["t_crossings"]) == (3, 2, 4)
    short = se.walk(H, W, veh, spawn, n, gates, 1, 2, False)
    assert short["mask"].tolist() == [1, 0, 2, 0, 0] and short["crossings"].tolist() == [1, 0, 1, 0, 0]
    assert se.selected(r).tolist() == [1, 0, 1, 1, 0] and se.selected(r, none=1).tolist() == [0, 0, 0, 1, 0]
    assert se.selected(short, any=2).tolist() == [0, 0, 1, 0, 0] and se.selected(short, all=3).tolist() == [0] * 5
    zones = np.array([[0, 0, 1, 1], [0, -1, 1, 1], [-1, 0, 1, 1]], dtype=np.int32)
    pos = np.array([[0, 0], [9, 9], [3, 1], [0, 2], [9, 9]])
    goal = np.array([[3, 0], [9, 9], [1, 0], [2, 2], [9, 9]])
    counts, unzoned = se.od(se.selected(r), pos, goal, zones, 2)
    assert counts.tolist() == [[0, 1], [1, 0]] and unzoned == 1
