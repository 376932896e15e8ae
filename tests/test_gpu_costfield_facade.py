"""Cost fields through the Mesa-style facade: CityModel.cost_field(), catchments() and isochrones() on a seed-built city
against the definition and against CApi, a catchment plane as the trip log's zones, and save / load / deepcopy."""
import copy

import numpy as np
import pytest

from tests import costfield_expect as ce
from tests.engine_util import city_model, refused, run_example
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import costfield as cf
from trafficsimulation_amd.mesa_api import CityModel

pytestmark = pytest.mark.gpu

TICKS = 20


@pytest.fixture(scope="module")
def city():
    m = city_model(64, seed=11, traffic=dict(P_int=200000, P_thr=60000), trip_log=4096)
    for _ in range(TICKS):
        m.step()
    yield m
    m.close()


def rule_of(m):
    eng = m.engine
    return ce.Rule.from_params(eng.params_from_defaults(m._defaults), m.allowed_dirs_map, m.is_road_map, m.road_type_map,
                               eng.map(capi.MAP_OCCUPANCY), eng.map(capi.MAP_STOP), eng.density())


def test_cost_field_takes_pairs_cells_and_vehicles(city):
    m = city
    assert len(m.active_vehicle_agents) > 5 and len(m.highway_exits) > 0
    v = m.active_vehicle_agents[0]
    seeds = [m.highway_exits[0], v, (30, 31)]
    xy = [m.highway_exits[0].position, v.pos, (30, 31)]
    got = m.cost_field(seeds, mode="to")
    assert got["seeds"].tolist() == [list(p) for p in xy] and got["tick"] == TICKS and got["mode"] == "to" and got["soft_obstacles"]
    want_v, want_o = ce.field(rule_of(m), xy, mode="to", soft=True)
    assert np.array_equal(got["cost"], want_v) and np.array_equal(got["owner"], want_o)
    assert got["reached"] == int((want_v != ce.UNREACHABLE).sum()) > 100
    frm = m.cost_field(seeds, mode="from", seed_cost=[0, 4, 2], soft=False, ignore_flow=True, max_cost=5000)
    want_v, want_o = ce.field(rule_of(m), xy, [0, 4, 2], mode="from", soft=False, ignore_flow=True, max_cost=5000)
    assert np.array_equal(frm["cost"], want_v) and np.array_equal(frm["owner"], want_o) and frm["max_cost"] == 5000
    with pytest.raises(ValueError):
        m.cost_field(seeds, mode="sideways")


def test_catchments_are_zones_for_the_trip_log(city):
    m = city
    c = m.catchments("highway_exits")
    n = len(m.highway_exits)
    assert c["n"] == n <= capi.TRIPLOG_MAX_ZONES and c["seeds"].tolist() == [list(e.position) for e in m.highway_exits]
    zone = c["zone"]
    assert zone.dtype == np.int32 and zone.shape == (m.height, m.width) and zone.min() >= -1 and zone.max() < n
    assert np.array_equal(zone == -1, c["cost"] == cf.CF_UNREACHABLE)
    want_v, want_o = ce.field(rule_of(m), c["seeds"], mode="to", soft=True)
    assert np.array_equal(zone, want_o) and np.array_equal(c["cost"], want_v)
    for k, (x, y) in enumerate(c["seeds"].tolist()):
        assert c["cost"][y, x] == 0 and zone[y, x] == min(j for j, s in enumerate(c["seeds"].tolist()) if s == [x, y]) <= k
    # the plane as it is: the zones of the OD matrix
    m.engine.triplog_set_zones(zone, n)
    od = m.engine.triplog_od()
    assert od["count"].shape == (n, n)
    by_cells = m.catchments([(10, 10), (50, 50)], free_flow=True)
    assert by_cells["n"] == 2 and set(np.unique(by_cells["zone"]).tolist()) <= {-1, 0, 1}
    entr = m.catchments("block_entrances")
    assert entr["n"] == len(m.block_entrances) and entr["zone"].max() < entr["n"]
    with pytest.raises(ValueError):
        m.catchments("depots")


def test_isochrones_count_road_cells_on_the_device(city):
    m = city
    thr = [0, 5, 20, 80, 500, 5000, 10 ** 6]
    iso = m.isochrones([m.highway_exits[0]], thr)
    plane = m.engine.costfield.plane("cost")
    on_road = plane[m.is_road_map == 1]
    assert iso["road_cells"].tolist() == [int((on_road <= t).sum()) for t in thr]
    assert iso["road_cells"][0] >= 1 and iso["road_cells"][-1] > iso["road_cells"][1] and iso["thresholds"].tolist() == thr
    free = m.isochrones([m.highway_exits[0]], thr, free_flow=True)
    assert (free["road_cells"] >= iso["road_cells"]).all()            # (obstacles only ever add cost)


def test_save_load_and_deepcopy_drop_the_result(city, tmp_path):
    m = city
    want = m.cost_field([(30, 31)], mode="to")
    path = str(tmp_path / "city.npz")
    m.save(path)
    for how, other in (("load", CityModel.load(path)), ("deepcopy", copy.deepcopy(m))):
        assert other.engine.costfield.info()["n_seeds"] == 0, f"{how}: a new engine starts without a result"
        refused(capi.TS_E_STATE, lambda: other.engine.costfield.plane("cost"))
        got = other.cost_field([(30, 31)], mode="to")
        assert np.array_equal(got["cost"], want["cost"]) and np.array_equal(got["owner"], want["owner"]), how
        other.close()
    assert m.engine.costfield.info()["n_seeds"] == 1


def test_run_city_writes_the_cost_plane(tmp_path):
    out = tmp_path / "cost.npy"
    r = run_example("run_city.py", "--size", 64, "--seed", 11, "--ticks", 20, "--isochrone", "30,31", out)
    assert "cost to (30, 31):" in r.stdout, r.stdout[-2000:]
    cost = np.load(out)
    assert cost.shape == (64, 64) and cost.dtype == np.uint32 and cost[31, 30] == 0 and (cost != cf.CF_UNREACHABLE).sum() > 100
