"""External light control through the Mesa-style facade: light_states / control_lights / request_phases, the controller
columns on the group views, save / load / deepcopy / pickle in the middle of a controlled run, and examples/train_lights.py."""
import copy
import pickle

import numpy as np
import pytest

from tests import lights_ext_expect as lx
from tests.engine_util import city_model, run_example
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd.mesa_api import CityModel

pytestmark = pytest.mark.gpu

DIM = 17


def make_model():
    return city_model(96, seed=42, traffic=dict(P_int=30000, P_thr=8000),
                      defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_RL_BATCHED", "SRL_INPUT_DIMENSIONS": DIM, "RAIN_ENABLED": False})


def actions_for(t, G):
    return (np.random.default_rng(300 + t).random(G) < 0.4).astype(np.int8)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def state_of(m):
    e = m.engine
    return {"blob": e.checkpoint_save(), "ctrl": e.lights_controller(), "groups": e.groups(), "veh": e.vehicles(),
            "occ": e.map(capi.MAP_OCCUPANCY), "stop": e.map(capi.MAP_STOP)}


def assert_same(a, b, ctx):
    for k in a:
        assert (a[k] == b[k]) if isinstance(a[k], bytes) else np.array_equal(a[k], b[k]), f"{ctx}: {k}"


@pytest.fixture(scope="module")
def model():
    m = make_model()
    G = len(m.intersection_light_groups)
    ctrl = lx.Ctrl(G)
    static = lx.static_features(m.tables)
    assert "g_approach_road_types" in m.tables       # world-gen supplies the cells' own road types for penalty_score
    for t in range(30):
        rows = m.engine.groups()
        ctrl.current, ctrl.pending = rows[:, 0].copy(), rows[:, 1].copy()
        ctrl.repop = np.asarray([bool(m.engine.group_links(g, False)) for g in range(G)])
        occ, stuck = m.occupancy_map, m.stuck_map
        s = m.light_states()
        assert s.shape == (G, DIM) and same_bits(s, lx.phase_a(m.tables, occ, stuck, ctrl, DIM, static)), f"tick {t}"
        assert same_bits(m.light_states(), s)
        a = actions_for(t, G)
        n = m.control_lights(a)
        assert same_bits(n, lx.phase_b(m.tables, occ, stuck, ctrl, a, DIM, 5, static)), f"tick {t}"
        g = m.intersection_light_groups[t % G]
        assert (g._rl_phase, g.rl_timer) == tuple(int(v) for v in ctrl.rows()[t % G])
        assert g.pending_phase == (None if ctrl.pending[t % G] < 0 else int(ctrl.pending[t % G]))
        m.step()
    yield m
    m.close()


def continue_both(a, b, t0, ticks, ctx):
    G = len(a.intersection_light_groups)
    for t in range(t0, t0 + ticks):
        act = actions_for(t, G)
        assert same_bits(a.light_states(), b.light_states()), f"{ctx}: states at tick {t}"
        assert same_bits(a.control_lights(act), b.control_lights(act)), f"{ctx}: next states at tick {t}"
        a.step()
        b.step()
    assert_same(state_of(a), state_of(b), ctx)


def test_request_phases(model):
    twin = copy.deepcopy(model)
    G = len(twin.intersection_light_groups)
    rows = twin.engine.groups()
    want = np.where(rows[:, 1] < 0, 1 - np.maximum(rows[:, 0], 0), -1).astype(np.int8)     # the other phase wherever none is pending
    before = twin.engine.lights_controller()
    twin.request_phases(want)
    after = twin.engine.groups()
    asked = want >= 0
    assert asked.any() and np.array_equal(after[asked, 1], want[asked]) and np.array_equal(after[~asked], rows[~asked])
    assert np.array_equal(twin.engine.lights_controller(), before)
    assert [g.pending_phase for g in twin.intersection_light_groups] == [None if p < 0 else int(p) for p in after[:, 1]]
    twin.step()
    twin.close()


def test_deepcopy_mid_run(model):
    before = state_of(model)
    model.light_states()                       # copied between observe and act
    twin = copy.deepcopy(model)
    assert twin.engine.h.value != model.engine.h.value and twin.engine.lights_info() == model.engine.lights_info()
    continue_both(model, twin, 30, 8, "deepcopy")
    assert before["blob"] != state_of(model)["blob"]
    twin.close()


def test_pickle_and_save_load(model, tmp_path):
    other = pickle.loads(pickle.dumps(model))
    path = str(tmp_path / "city.npz")
    model.save(path)
    loaded = CityModel.load(path)
    assert loaded.engine.lights_info()["state_dim"] == DIM
    assert_same(state_of(model), state_of(other), "pickle")
    assert_same(state_of(model), state_of(loaded), "load")
    continue_both(other, loaded, 40, 6, "pickle vs load")
    other.close()
    loaded.close()


def test_training_example_runs():
    r = run_example("train_lights.py", "--size", 64, "--ticks", 20, "--every", 10)
    assert "TRAIN_OK" in r.stdout, r.stdout[-2000:]
