"""Routes along a cost field through the Mesa-style facade: CityModel.routes_along() with vehicle agents as starts against
RouteField.trace() with their rows, assigned_load() against load_plane() and the expectation, the example's --evacuate, and
save / load / deepcopy / pickle, which carry no hop plane."""
import copy
import pickle

import numpy as np
import pytest

from tests import cfroute_expect as re_
from tests.engine_util import city_model, refused, run_example
from tests.test_gpu_costfield_facade import rule_of
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd.mesa_api import CityModel

pytestmark = pytest.mark.gpu

TICKS = 20


@pytest.fixture(scope="module")
def city():
    m = city_model(64, seed=11, traffic=dict(P_int=200000, P_thr=60000))
    for _ in range(TICKS):
        m.step()
    yield m
    m.close()


def rows_of(m, vehicles):
    """(cells, headings) of the vehicle agents, from the engine's rows."""
    rows = {int(r[0]): r for r in m.engine.vehicles()}
    f = capi.V_FIELDS.index
    xy = np.asarray([[rows[v._spawn_idx][f("x")], rows[v._spawn_idx][f("y")]] for v in vehicles], dtype=np.int32)
    head = np.asarray([max(int(rows[v._spawn_idx][f("direction")]), -1) for v in vehicles], dtype=np.int8)
    return xy, head


def test_routes_along_with_vehicle_agents_equals_trace_with_their_rows(city):
    m = city
    vehicles = list(m.active_vehicle_agents)
    assert len(vehicles) > 5 and len(m.highway_exits) > 1
    xy, head = rows_of(m, vehicles)
    assert (head >= 0).any()
    got = m.routes_along(m.highway_exits, vehicles + [(30, 31)])
    r = m.engine.costfield.routes
    starts, heads = np.concatenate([xy, [[30, 31]]]).astype(np.int32), np.concatenate([head, [-1]]).astype(np.int8)
    assert np.array_equal(got["starts"], starts) and np.array_equal(got["headings"], heads) and got["held"] and got["tick"] == TICKS
    r.trace(starts, heads)
    off, dirs, cost, owner = r.routes()
    coff, cells = r.cells()
    assert np.array_equal(got["off"], off) and np.array_equal(got["dirs"], dirs) and np.array_equal(got["cost"], cost) and np.array_equal(got["owner"], owner)
    assert len(got["routes"]) == len(starts) and all(np.array_equal(p, cells[coff[i]:coff[i + 1]]) for i, p in enumerate(got["routes"]))
    # ... and both are the rule's
    seeds = [e.position for e in m.highway_exits]
    rule = rule_of(m)
    L = re_.labels(rule, seeds, mode="to", soft=True)
    want = re_.batch(re_.hop_plane(rule, L, seeds, mode="to", soft=True), L, "to", re_.headings(rule), starts, heads)
    for g, w in zip((off, dirs, cost, owner), want):
        assert np.array_equal(g, w)
    assert (owner >= 0).sum() > 5
    # FROM: no headings, the routes arrive at the vehicles
    frm = m.routes_along(m.highway_exits, vehicles, mode="from", free_flow=True)
    assert frm["mode"] == "from" and all(len(p) == 0 or tuple(p[-1]) == tuple(s) for p, s in zip(frm["routes"], xy.tolist()))


def test_assigned_load_equals_load_plane(city):
    m = city
    vehicles = list(m.active_vehicle_agents)
    xy, head = rows_of(m, vehicles)
    w = np.arange(1, len(vehicles) + 1, dtype=np.uint32)
    got = m.assigned_load(m.highway_exits, vehicles, weights=w)
    r = m.engine.costfield.routes
    assert np.array_equal(got["load"], r.load_plane()) and np.array_equal(got["by_direction"], np.stack([r.load_plane(d) for d in range(4)]))
    assert np.array_equal(got["load"], got["by_direction"].sum(axis=0, dtype=np.uint32)) and got["steps"] == int(got["load"].sum(dtype=np.uint64)) > 0
    r.trace(xy, head)
    off, dirs, _, owner = r.routes()
    assert np.array_equal(got["by_direction"], re_.load_planes((m.height, m.width), "to", xy, off, dirs, w))
    assert got["routes"] == int((owner >= 0).sum()) and got["unreached"] == int((owner < 0).sum())


def test_save_load_deepcopy_and_pickle_carry_no_hop_plane(city, tmp_path):
    m = city
    want = m.routes_along(m.highway_exits, [(30, 31)])
    assert m.engine.costfield.routes.info()["held"]
    path = str(tmp_path / "city.npz")
    m.save(path)
    for how, other in (("load", CityModel.load(path)), ("deepcopy", copy.deepcopy(m)), ("pickle", pickle.loads(pickle.dumps(m)))):
        r = other.engine.costfield.routes
        info = r.info()
        assert not info["held"] and info["trace_n"] == 0 and info["load_routes"] == 0, f"{how}: a new engine starts without routes"
        refused(capi.TS_E_STATE, lambda: r.trace([(30, 31)]), lambda: r.routes(0, 0), lambda: r.load_plane())
        got = other.routes_along(other.highway_exits, [(30, 31)])
        assert np.array_equal(got["dirs"], want["dirs"]) and np.array_equal(got["cost"], want["cost"]), how
        other.close()
    assert m.engine.costfield.routes.info()["held"]


def test_run_city_writes_the_evacuation_load(tmp_path):
    out = tmp_path / "evac.npy"
    r = run_example("run_city.py", "--size", 96, "--ticks", 30, "--evacuate", out)
    assert "evacuation:" in r.stdout and "exits in" in r.stdout, r.stdout[-2000:]
    load = np.load(out)
    assert load.shape == (96, 96) and load.dtype == np.uint32 and load.sum() > 0
