"""The A2C / GAT-DQN protocols through the Mesa-style facade: both algorithm names are accepted, light_states / control_lights /
control_lights_q follow the numpy model, epsilon shows on the group views, and save / load, deepcopy and pickle carry the
protocol in the middle of a run.  The non-batched names stay refused."""
import copy
import pickle

import numpy as np
import pytest

from tests import lights_ext_expect as lx
from tests import lights_proto_expect as lp
from tests.engine_util import city_model, refused
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd.mesa_api import CityModel

pytestmark = pytest.mark.gpu

DECAY = 0.1
STAT_KEYS = ("avg_duration_internal", "avg_duration_through", "avg_time_per_unit_internal", "avg_time_per_unit_through")


def make_model(algo):
    return city_model(64, seed=45, traffic=dict(P_int=30000, P_thr=8000),
                      defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": algo, "RAIN_ENABLED": False, "EPS_DECAY_RATE": DECAY})


def q_for(t, G):
    return np.random.default_rng(500 + t).normal(size=(G, 2)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def model_ctrl(m, ctrl):
    G = len(m.intersection_light_groups)
    rows = m.engine.groups()
    ctrl.current, ctrl.pending = rows[:, 0].copy(), rows[:, 1].copy()
    ctrl.repop = np.asarray([bool(m.engine.group_links(g, False)) for g in range(G)])


def test_a2c_name_follows_the_model():
    m = make_model("RL_A2C_BATCHED")
    G = len(m.intersection_light_groups)
    ctrl, static = lx.Ctrl(G), lx.static_features(m.tables)
    for t in range(12):
        model_ctrl(m, ctrl)
        occ = m.occupancy_map
        s = m.light_states()
        assert s.shape == (G, 13) and bits(s) == bits(lp.a2c_state(m.tables, occ, ctrl, static)), f"tick {t}"
        a = (np.random.default_rng(t).random(G) < 0.5).astype(np.int8)
        r = m.control_lights(a)
        assert bits(r) == bits(lp.act(m.tables, occ, ctrl, a, lp.A2C, 5, static)), f"tick {t}"
        g = m.intersection_light_groups[t % G]
        assert (g._rl_phase, g.rl_timer) == tuple(int(v) for v in ctrl.rows()[t % G])
        m.step()
    # the device-only route: nothing comes down, the controller moves all the same
    model_ctrl(m, ctrl)
    a = np.ones(G, np.int8)
    assert m.light_states(to_host=False) is None and m.control_lights(a, to_host=False) is None
    lp.act(m.tables, m.occupancy_map, ctrl, a, lp.A2C, 5, static)
    assert np.array_equal(m.engine.lights_controller(), ctrl.rows())
    m.close()


def test_gat_name_round_trips_save_load_copy_and_pickle(tmp_path):
    m = make_model("GAT_DQN_BATCHED")
    G = len(m.intersection_light_groups)
    ctrl, static = lx.Ctrl(G), lx.static_features(m.tables)
    eps = np.ones(G)
    assert all(g.epsilon == 1.0 for g in m.intersection_light_groups)
    for t in range(8):
        model_ctrl(m, ctrl)
        f, k = m.light_states()
        wf, wk = lp.gat_state(m.tables, m.occupancy_map, ctrl, static)
        assert bits(f) == bits(wf) and bits(k) == bits(wk), f"tick {t}"
        occ = m.occupancy_map
        a, r, n = m.control_lights_q(q_for(t, G))
        cs = m.engine.cached_stats()
        wr, wn = lp.act(m.tables, occ, ctrl, a, lp.GAT, 5, static, [float(cs.get(key, 0.0)) for key in STAT_KEYS])
        assert bits(r) == bits(wr) and bits(n) == bits(wn), f"tick {t}: reward / next state"
        eps = lp.epsilon_after(eps, 0.1, DECAY)
        assert [g.epsilon for g in m.intersection_light_groups] == eps.tolist() and set(a.tolist()) <= {0, 1}
        m.step()
    path = tmp_path / "gat.npz"
    m.save(path)
    others = {"load": CityModel.load(path), "deepcopy": copy.deepcopy(m), "pickle": pickle.loads(pickle.dumps(m))}
    for t in range(8, 16):
        want = m.control_lights_q(q_for(t, G))
        m.step()
        for how, o in others.items():
            got = o.control_lights_q(q_for(t, G))
            assert all(bits(x) == bits(y) for x, y in zip(want, got)), f"{how} tick {t}"
            o.step()
    blob = m.engine.checkpoint_save()
    for how, o in others.items():
        assert o.engine.checkpoint_save() == blob, how
        assert o.intersection_light_groups[0].epsilon == m.intersection_light_groups[0].epsilon == 0.1
        o.close()
    assert m.light_states(to_host=False) is None and m.control_lights_q(q_for(16, G), to_host=False) is None
    assert len(m.control_lights_q(q_for(17, G), want_next=False)) == 2
    # caller-chosen actions: (rewards, next features), nothing drawn
    fp = list(m.engine.rng_fingerprint(capi.RNG_GLOBAL))
    r, n = m.control_lights(np.ones(G, np.int8))
    assert r.shape == (G,) and n.shape == (G, 5, 9) and list(m.engine.rng_fingerprint(capi.RNG_GLOBAL)) == fp
    m.close()


@pytest.mark.parametrize("name", ["GAT_DQN", "NEIGHBOR_RL"])
def test_the_non_batched_names_stay_refused(name):
    refused(capi.TS_E_UNSUPPORTED, lambda: CityModel(64, 64, seed=45, defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": name, "RAIN_ENABLED": False}))
