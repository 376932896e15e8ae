"""Jam detection through the Mesa-style facade: CityModel.jams() with its sort and `top`, queue_report() keyed like
intersection_report(), jam_vehicles() / jam_load() against the label plane and planned_load(), save / load / deepcopy / pickle,
and examples/run_city.py --jams."""
import copy
import pickle
import re

import numpy as np
import pytest

from tests import jams_expect as je
from tests.engine_util import city_model, refused, run_example
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd.jams import JAM_DTYPE, JG_FIELDS
from trafficsimulation_amd.mesa_api import CityModel

pytestmark = pytest.mark.gpu

TICKS = 40
V = je.V


@pytest.fixture(scope="module")
def city():
    m = city_model(96, seed=5, traffic=dict(P_int=200000, P_thr=60000, service_food=40, service_waste=40))
    for _ in range(TICKS):
        m.step()
    yield m
    m.close()


def expectation(m, link, min_ticks=1):
    rows = m.engine.vehicles()
    return je.expect(je.count_plane(rows, m.height, m.width, min_ticks), link, m.allowed_dirs_map, m.intersection_map, rows,
                     m.engine.num_spawned(), min_ticks, tr=m.tables)


def test_jams_sorts_and_cuts(city):
    m = city
    for link, min_ticks in (("flow", 1), ("grid", 2)):
        want = expectation(m, je.FLOW if link == "flow" else je.GRID, min_ticks)
        got = m.jams(min_ticks, link)
        n = want["info"]["n_jams"]
        assert n > 3 and got["n"] == n == len(got["jams"]) and got["tick"] == TICKS and got["held"]
        assert got["standing_vehicles"] == want["info"]["standing_vehicles"] > 0 and got["largest_cells"] == want["info"]["largest_cells"]
        assert got["label"].shape == (m.height, m.width) and np.array_equal(got["label"], want["label"])
        assert got["jams"].dtype == JAM_DTYPE and sorted(got["number"].tolist()) == list(range(n))
        assert np.array_equal(got["jams"], want["records"][got["number"]])
        keys = [(-int(r["cells"]), int(r["root_y"]) * m.width + int(r["root_x"])) for r in got["jams"]]
        assert keys == sorted(keys), "not sorted by (cells descending, root ascending)"
        top = m.jams(min_ticks, link, top=3)
        assert len(top["jams"]) == 3 and top["n"] == n and np.array_equal(top["jams"], got["jams"][:3])
        assert len(m.jams(min_ticks, link, top=0)["jams"]) == 0 and len(m.jams(min_ticks, link, top=10 ** 6)["jams"]) == n


def test_queue_report_is_keyed_like_the_intersection_report(city):
    m = city
    want = expectation(m, je.FLOW)["groups"]
    rep = m.queue_report()
    m.observe()
    keys = set(m.intersection_report()[0]) & {"group", "index"}
    m.observe(planes=())
    assert keys == {"group", "index"} and len(rep) == len(want) == len(m.intersection_light_groups) > 0
    f = JG_FIELDS.index
    for g, r in enumerate(rep):
        assert r["index"] == g and r["group"] == m.intersection_light_groups[g].id and r["tick"] == TICKS
        for ax in ("ns", "ew"):
            assert (r[f"queue_{ax}"], r[f"queue_vehicles_{ax}"], r[f"queue_extent_{ax}"], r[f"longest_wait_{ax}"], r[f"jams_{ax}"]) == tuple(
                int(want[g, f(ax + "_" + k)]) for k in ("cells", "vehicles", "extent", "stuck_max", "jams"))
        assert r["box_cells"] == int(want[g, f("box_cells")])
    assert sum(r["queue_ns"] + r["queue_ew"] for r in rep) > 0


def test_jam_vehicles_and_their_load(city):
    m = city
    got = m.jams()
    j = int(got["number"][0])                                    # the largest jam
    rows = m.engine.vehicles()
    st = je.standing_rows(rows)
    want = sorted(int(r[V["spawn_idx"]]) for r in st if got["label"][r[V["y"]], r[V["x"]]] == j)
    agents = m.jam_vehicles(j)
    assert len(want) >= int(got["jams"][0]["cells"]) > 1 and [a._spawn_idx for a in agents] == want
    assert all(got["label"][a.pos[1], a.pos[0]] == j for a in agents)
    load = m.jam_load(j, bins=2, bin_cells=12)
    ref = m.planned_load(vehicles=agents, bins=2, bin_cells=12)
    assert load["vehicles"] == len(agents) and load["steps"] == ref["steps"]
    assert np.array_equal(load["by_direction"], ref["by_direction"]) and np.array_equal(load["load"], ref["load"])
    assert m.jam_vehicles(got["n"]) == []
    with pytest.raises(ValueError):
        m.jam_vehicles(-1)


def test_save_load_copy_and_pickle_start_without_a_result(city, tmp_path):
    m = city
    want = m.jams()
    path = str(tmp_path / "city.npz")
    m.save(path)
    for how, other in (("load", CityModel.load(path)), ("deepcopy", copy.deepcopy(m)), ("pickle", pickle.loads(pickle.dumps(m)))):
        i = other.engine.jams.info()
        assert (i["held"], i["device_bytes"]) == (False, 0), f"{how}: a new engine starts without a result"
        refused(capi.TS_E_STATE, lambda: other.jam_vehicles(0), other.engine.jams.records, lambda: other.engine.jams.plane("label"))
        got = other.jams()
        assert np.array_equal(got["jams"], want["jams"]) and np.array_equal(got["label"], want["label"]), how
        other.close()
    assert m.engine.jams.info()["held"]


def test_run_city_writes_the_records(tmp_path):
    m = city_model(96, seed=1)
    for _ in range(TICKS):
        m.step()
    want = m.jams()
    m.close()
    assert want["n"] > 0
    out = tmp_path / "jams.npy"
    r = run_example("run_city.py", "--size", 96, "--ticks", TICKS, "--jams", out)
    said = re.search(r"jams: (\d+) with (\d+) standing vehicles on (\d+) cells", r.stdout)
    assert said, r.stdout[-2000:]
    rec = np.load(out)
    assert rec.dtype == JAM_DTYPE and np.array_equal(rec, want["jams"])
    assert (int(said.group(1)), int(said.group(2)), int(said.group(3))) == (want["n"], want["standing_vehicles"], want["standing_cells"])
