"""The A2C and GAT-DQN light protocols (include/trafficsim_lights_proto.h) on the device.

1. the four fixtures of tests/golden/make_golden_lights_proto.py replayed with the control call in front of every tick: state,
   mask, action, reward, next state, epsilon and controller rows against what the reference recorded, bit for bit, and the
   tick in between against the ordinary trace - whose global-stream fingerprint proves the epsilon-greedy draws;
2. a differential hunt against the numpy model (tests/lights_proto_expect.py) on other worlds with neighbour entries removed.
   The engine has no entry that writes occupancy or controller state, so both come from running: vehicles placed on the
   world's own start cells and stepped, random actions under a random min-green.  Empty approach lists are the worlds' own
   (asserted per case, so that a change of worlds cannot lose them);
3. API behaviour: act draws nothing, observe is idempotent, the protocols are exclusive, checkpoints, refusals, device tensors.

Rewards are compared bit for bit: the cached-stats comparison of tests/trace_util.py is exact, so the global term is too."""
import os

import numpy as np
import pytest

from tests import lights_ext_expect as lx
from tests import lights_proto_expect as lp
from tests import procs
from tests.engine_util import proto_engine, refused, setup_proto
from tests.lights_ext_expect import GATED, Stepper
from tests.trace_util import check_initial, replay_and_compare, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import build_engine, load_trace

pytestmark = pytest.mark.gpu

FIXTURES = ["lights_a2c_64_s45", "lights_a2c_96_s47", "lights_gat_64_s45", "lights_gat_96_s49"]
STAT_KEYS = ("avg_duration_internal", "avg_duration_through", "avg_time_per_unit_internal", "avg_time_per_unit_through")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_engine(name, **over):
    return proto_engine(name, new_engine, **over)      # (this module's new_engine: the sharded-rank worker replaces it)


# ---- 1. the reference's own controller runs ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_replays_the_reference_controller(name):
    api, tr = fixture_engine(name)
    check_initial(api, tr)
    gat = int(tr["lp_protocol"]) == lp.GAT
    info = api.lights_proto_info()
    assert (info["protocol"], info["min_green"], info["calls"]) == (int(tr["lp_protocol"]), int(tr["lp_min_green"]), 0)
    if gat:
        assert (info["eps_min"], info["eps_decay"]) == (float(tr["lp_eps_min"]), float(tr["lp_eps_decay"]))
        assert np.array_equal(api.lights_proto_controller(), np.ones(api.n_groups))

    def control(t):
        cs = api.cached_stats()
        assert [float(cs.get(k, 0.0)) for k in STAT_KEYS] == tr["lp_stats"][t].tolist(), f"tick {t}: cached_stats at the call"
        if gat:
            f, m = api.lights_proto_observe()
            assert same_bits(f, tr["lp_state"][t]) and same_bits(m, tr["lp_mask"][t]), f"tick {t}: state / mask"
            a, r, n = api.lights_proto_act_q(tr["lp_q"][t])
            assert np.array_equal(a, tr["lp_action"][t]), f"tick {t}: actions {a} != {tr['lp_action'][t]}"
            assert same_bits(n, tr["lp_next_state"][t]), f"tick {t}: next state of groups {np.nonzero((n != tr['lp_next_state'][t]).any(axis=(1, 2)))[0]}"
            assert same_bits(api.lights_proto_controller(), tr["lp_eps"][t]), f"tick {t}: epsilon"
        else:
            s = api.lights_proto_observe()
            assert same_bits(s, tr["lp_state"][t]), f"tick {t}: state of groups {np.nonzero((s != tr['lp_state'][t]).any(axis=1))[0]}"
            r = api.lights_proto_act(tr["lp_action"][t])
        assert same_bits(r, tr["lp_reward"][t]), f"tick {t}: reward {r} != {tr['lp_reward'][t]}"
        want = tr["lp_ctrl"][t]
        assert np.array_equal(api.lights_controller(), want[:, :2]), f"tick {t}: _rl_phase / rl_timer"
        assert np.array_equal(api.groups()[:, :2], want[:, 2:]), f"tick {t}: current / pending phase after the call"
    T = len(tr["lp_state"])
    assert replay_and_compare(Stepper(api, control), tr) == T
    assert api.lights_proto_info()["calls"] == T
    api.close()


# ---- 2. differential hunt against the numpy model --------------------------------------------------------------------------
HUNT_WORLDS = ["rect_64x112_s19", "ragged_100x75_s33", "carve_96_s10", "lights_ext_64_s45"]
N_CASES = int(os.environ.get("TS_RANDOM_CASES", "8"))


@pytest.mark.parametrize("case", range(N_CASES))
def test_hunt_against_the_numpy_model(case, monkeypatch):
    rng = np.random.default_rng(9000 + case)
    tr = load_trace(trace_path(HUNT_WORLDS[case % len(HUNT_WORLDS)]))
    proto = (lp.A2C, lp.GAT)[(case // 2) % 2] if case % 2 == 0 else (lp.GAT, lp.A2C)[(case // 2) % 2]
    mgreen = int(rng.choice([1, 3, 5]))
    penalties = (0.5, 5, 50.0) if case % 3 else (0.3, 5.25, 12.1)
    tables = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tr.items() if k != "g_approach_road_types"}
    kinds = np.asarray(tables["schedule_kinds0"])
    tables["schedule_kinds0"] = kinds[kinds != 2]
    G = len(tables["g_ns_in_off"]) - 1
    # neighbour entries taken out: a whole group without neighbours, single slots emptied, slots whose group is -1
    for key in ("g_neighbors", "g_neighbors_ctor"):
        nb = tables[key]
        nb[int(rng.integers(G))] = -1
        for _ in range(max(2, G // 3)):
            g, k = int(rng.integers(G)), int(rng.integers(4))
            nb[g, k] = -1 if rng.integers(2) else (nb[g, k, 0], -1)
        g, k = np.argwhere((nb[:, :, 0] >= 0) & (nb[:, :, 1] >= 0))[0]
        nb[g, k, 1] = -1
    d = {**GATED, "RAIN_ENABLED": False, "TRAFFIC_LIGHT_AGENT_ALGORITHM": ("RL_A2C_BATCHED", "GAT_DQN_BATCHED")[proto - 1],
         "GAT_TRAFFIC_RL_MIN_GREEN": mgreen, "VEHICLE_ROAD_TYPES_PENALTY_R1": penalties[0], "VEHICLE_ROAD_TYPES_PENALTY_R2": penalties[1],
         "VEHICLE_ROAD_TYPES_PENALTY_R3": penalties[2], "TRAFFIC_LIGHT_TRANSITION_CLEARANCE_ENABLED": bool(rng.integers(4) > 0)}
    if proto == lp.A2C:
        mgreen = 5      # (the reference's A2C has no setting for it)
    monkeypatch.setenv("TS_DEBUG_LIGHTS_TEAM", str((8, 4, 16, 32)[case % 4]))
    monkeypatch.setenv("TS_DEBUG_LIGHTS_BLOCK", str((8, 256, 16)[case % 3]))     # (8: several blocks of the per-group kernels)
    api = new_engine()
    build_engine(api, tables, defaults=d, global_seed=case + 1, sched_seed=case + 5)
    n = len(tr["v_start_xy"])
    api.add_vehicles(tr["v_start_xy"][:n], tr["v_goal_xy"][:n], np.full(n, capi.POP["through"], np.int32))
    assert api.lights_proto_info()["protocol"] == proto and api.lights_proto_info()["min_green"] == mgreen
    ctrl = lx.Ctrl(G)
    static = lx.static_features(tables, penalties)
    ctx = f"case {case} (protocol {proto}, G {G})"
    assert (np.diff(tables["g_ns_in_off"]) == 0).any() or (np.diff(tables["g_ew_in_off"]) == 0).any(), f"{ctx}: no empty approach list"
    for key in ("g_neighbors", "g_neighbors_ctor"):      # a group without neighbours, a slot with a direction and no group
        nb = tables[key]
        assert ((nb[:, :, 1] < 0).all(axis=1)).any() and ((nb[:, :, 0] >= 0) & (nb[:, :, 1] < 0)).any(), f"{ctx}: {key}"
    for t in range(12):
        rows = api.groups()
        ctrl.current, ctrl.pending = rows[:, 0].copy(), rows[:, 1].copy()
        ctrl.repop = np.asarray([bool(api.group_links(g, False)) for g in range(G)])
        occ = api.map(capi.MAP_OCCUPANCY)
        actions = (rng.random(G) < (0.8 if t < 6 else 0.3)).astype(np.int8)
        if proto == lp.A2C:
            want = lp.a2c_state(tables, occ, ctrl, static)
            got = api.lights_proto_observe()
            assert same_bits(got, want), f"{ctx} tick {t}: state of groups {np.nonzero((got != want).any(axis=1))[0]}"
            want_r = lp.act(tables, occ, ctrl, actions, proto, mgreen, static)
            got_r = api.lights_proto_act(actions)
        else:
            wf, wm = lp.gat_state(tables, occ, ctrl, static)
            gf, gm = api.lights_proto_observe()
            assert same_bits(gf, wf) and same_bits(gm, wm), f"{ctx} tick {t}: state of groups {np.nonzero((gf != wf).any(axis=(1, 2)))[0]}"
            want_r, want_n = lp.act(tables, occ, ctrl, actions, proto, mgreen, static)
            got_r, got_n = api.lights_proto_act(actions)
            assert same_bits(got_n, want_n), f"{ctx} tick {t}: next state of groups {np.nonzero((got_n != want_n).any(axis=(1, 2)))[0]}"
        assert same_bits(got_r, want_r), f"{ctx} tick {t}: reward"
        assert np.array_equal(api.lights_controller(), ctrl.rows()), f"{ctx} tick {t}: controller rows"
        rows = api.groups()
        assert np.array_equal(rows[:, 0], ctrl.current) and np.array_equal(rows[:, 1], ctrl.pending), f"{ctx} tick {t}: phases"
        api.step(1)
    api.close()


# ---- 3. API behaviour ------------------------------------------------------------------------------------------------------
def test_act_under_gat_draws_nothing_and_observe_is_idempotent():
    api, tr = fixture_engine("lights_gat_64_s45")
    for t in range(8):
        f1, m1 = api.lights_proto_observe()
        f2, m2 = api.lights_proto_observe()
        assert same_bits(f1, f2) and same_bits(m1, m2) and same_bits(f1, tr["lp_state"][t])
        api.lights_proto_act_q(tr["lp_q"][t])
        api.step(1)
    eps, fp, saved = api.lights_proto_controller(), list(api.rng_fingerprint(capi.RNG_GLOBAL)), api.checkpoint_save()
    api.lights_proto_observe()
    assert api.checkpoint_save() == saved, "observe changed simulation state"
    r, n = api.lights_proto_act(tr["lp_action"][8])
    assert list(api.rng_fingerprint(capi.RNG_GLOBAL)) == fp and np.array_equal(api.lights_proto_controller(), eps)
    assert same_bits(n, tr["lp_next_state"][8]) and same_bits(r, tr["lp_reward"][8])      # the same action, chosen by the caller
    assert np.array_equal(api.lights_controller(), tr["lp_ctrl"][8][:, :2])
    api.close()


def test_the_protocols_are_exclusive():
    api, tr = fixture_engine("lights_a2c_64_s45")
    z = np.zeros(api.n_groups, np.int8)
    refused(capi.TS_E_STATE, lambda: api.lights_config(13, 5), api.lights_observe, lambda: api.lights_act(z),
            lambda: api.lights_proto_config("GAT_DQN_BATCHED"), lambda: api.lights_proto_act_q(np.zeros((api.n_groups, 2), np.float32)))
    api.lights_request(z)      # the shared entries keep working
    assert api.lights_info()["n_groups"] == api.n_groups and api.lights_controller().shape == (api.n_groups, 2)
    api.close()
    # the other way round: the simple protocol has made a control call
    b = new_engine()
    setup_proto(b, tr, {**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL"})
    assert b.lights_proto_info()["protocol"] == 0
    refused(capi.TS_E_STATE, b.lights_proto_observe, lambda: b.lights_proto_act(z))      # no protocol configured
    b.lights_observe()
    refused(capi.TS_E_STATE, lambda: b.lights_proto_config("RL_A2C_BATCHED"))
    b.close()


def test_checkpoint_carries_epsilon_and_the_controller():
    a, tr = fixture_engine("lights_gat_64_s45")
    for t in range(10):
        a.lights_proto_act_q(tr["lp_q"][t])
        a.step(1)
    blob = a.checkpoint_save()
    assert len(blob) == a.checkpoint_size()
    b, _ = fixture_engine("lights_gat_64_s45")
    b.checkpoint_load(blob)
    assert b.checkpoint_save() == blob and b.lights_proto_info() == a.lights_proto_info()
    assert same_bits(b.lights_proto_controller(), tr["lp_eps"][9])
    for t in range(10, 30):      # the fork continues bit for bit, draws included
        ra, rb = a.lights_proto_act_q(tr["lp_q"][t]), b.lights_proto_act_q(tr["lp_q"][t])
        assert all(same_bits(x, y) for x, y in zip(ra, rb)) and np.array_equal(ra[0], tr["lp_action"][t]), f"tick {t}"
        a.step(1)
        b.step(1)
    assert a.checkpoint_save() == b.checkpoint_save()
    assert [int(v) for v in a.rng_fingerprint(capi.RNG_GLOBAL)] == [int(v) for v in tr["rng_rows"][29][:2]]
    a.close()
    b.close()


def test_checkpoint_refuses_another_configuration():
    a, tr = fixture_engine("lights_gat_64_s45")
    for t in range(4):
        a.lights_proto_act_q(tr["lp_q"][t])
        a.step(1)
    blob = a.checkpoint_save()
    others = [dict(EPS_DECAY_RATE=0.02), dict(GAT_TRAFFIC_RL_MIN_GREEN=4), dict(TRAFFIC_LIGHT_AGENT_ALGORITHM="RL_A2C_BATCHED"),
              dict(TRAFFIC_LIGHT_AGENT_ALGORITHM="EXTERNAL")]
    for over in others:
        b, _ = fixture_engine("lights_gat_64_s45", **over)
        before = b.checkpoint_save()
        refused(capi.TS_E_INVALID, lambda: b.checkpoint_load(blob))
        assert b.checkpoint_save() == before, "a refused load changed the target"
        refused(capi.TS_E_INVALID, lambda: a.checkpoint_load(before))     # and the plain blob does not load onto the protocol's handle
        b.close()
    assert a.checkpoint_save() == blob
    a.close()


def test_a_protocol_only_appends_its_section():
    """After the same calls, a blob written under a protocol is the EXTERNAL handle's blob - byte for byte, the header's total
    size aside - followed by the protocol's section (40 bytes of scalars, epsilon [G]): nothing before it moved."""
    tr = load_trace(trace_path("lights_gat_64_s45"))
    G = tr["lp_action"].shape[1]
    blobs = {}
    for algo in ("EXTERNAL", "GAT_DQN_BATCHED", "RL_A2C_BATCHED"):
        api = new_engine()
        setup_proto(api, tr, {**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": algo})
        for t in range(6):      # (phase requests are common to all three; they move pending phases, the ticks everything else)
            api.lights_request(np.asarray([(t + g) % 3 - 1 for g in range(G)], np.int8))
            api.step(1)
        blobs[algo] = api.checkpoint_save()
        assert len(blobs[algo]) == api.checkpoint_size()
        api.close()
    ext = blobs["EXTERNAL"]
    for algo in ("GAT_DQN_BATCHED", "RL_A2C_BATCHED"):
        b = blobs[algo]
        assert len(b) == len(ext) + 40 + 8 * G
        assert int.from_bytes(b[16:24], "little") == len(b) and int.from_bytes(ext[16:24], "little") == len(ext)      # CkHeader::total_bytes
        assert b[:16] == ext[:16] and b[24:len(ext)] == ext[24:], f"{algo}: a byte in front of the protocol's section differs"
        eps = np.frombuffer(b[len(b) - 8 * G:], dtype=np.float64)
        assert np.array_equal(eps, np.ones(G) if algo == "GAT_DQN_BATCHED" else np.zeros(G))
        assert b[len(ext):len(ext) + 4] == b"LPR1"


def test_checkpoint_refuses_a_bad_epsilon():
    a, tr = fixture_engine("lights_gat_64_s45")
    a.lights_proto_act_q(tr["lp_q"][0])
    a.step(1)
    blob = a.checkpoint_save()
    for bad in (float("nan"), 1.5, -0.25):
        b = bytearray(blob)
        b[len(b) - 8:] = np.float64(bad).tobytes()
        ex, = refused(capi.TS_E_INVALID, lambda: a.checkpoint_load(bytes(b)))
        assert "epsilon" in str(ex)
        assert a.checkpoint_save() == blob, "a refused load changed the target"
    a.close()


def test_static_features_are_fixed_once_a_protocol_has_acted():
    api, tr = fixture_engine("lights_gat_64_s45")
    G = api.n_groups
    api.lights_set_static(penalty_score=np.full(G, 2.0))      # before the first call: allowed
    assert (api.lights_proto_observe()[0][:, 0, 8] == 2.0).all()
    api.lights_proto_act(np.zeros(G, np.int8))
    refused(capi.TS_E_STATE, lambda: api.lights_set_static(penalty_score=np.full(G, 3.0)))
    assert (api.lights_proto_observe()[0][:, 0, 8] == 2.0).all()
    api.close()


def test_explicit_params_honour_or_refuse_a_protocol_name():
    tr = load_trace(trace_path("lights_a2c_64_s45"))
    api = new_engine()
    p = api.params_from_defaults({**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL"})
    build_engine(api, tr, defaults=tr["defaults_json"], params=p, global_seed=1, sched_seed=2)
    assert api.lights_proto_info()["protocol"] == lp.A2C
    api.close()
    other = new_engine()
    p = other.params_from_defaults({**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": "FIXED_TIME"})
    refused(capi.TS_E_INVALID, lambda: build_engine(other, tr, defaults=tr["defaults_json"], params=p, global_seed=1, sched_seed=2))
    other.close()


def test_bad_arguments_change_nothing():
    api, tr = fixture_engine("lights_gat_64_s45")
    G = api.n_groups
    for t in range(3):
        api.lights_proto_act_q(tr["lp_q"][t])
        api.step(1)
    before = api.checkpoint_save()
    q = tr["lp_q"][3].copy()
    q[G - 1, 1] = np.nan
    bad = [lambda: api.lights_proto_act(np.full(G, 2, np.int8)), lambda: api.lights_proto_act_q(q),
           lambda: api.lights_proto_act_q(np.full((G, 2), np.inf, np.float32))]
    for call in bad:
        refused(capi.TS_E_INVALID, call)
    with pytest.raises(ValueError):
        api.lights_proto_act_q(np.zeros((G + 1, 2), np.float32))
    assert api.checkpoint_save() == before      # (nothing applied, nothing drawn: the blob holds the global stream)
    api.close()
    a2c, tr2 = fixture_engine("lights_a2c_64_s45")
    before = a2c.checkpoint_save()
    refused(capi.TS_E_INVALID, lambda: a2c.lights_proto_act(tr2["lp_action"][0], want_next=True))      # a non-NULL next state under A2C
    assert a2c.checkpoint_save() == before
    for cfg in (dict(protocol=3), dict(protocol=2, min_green=-1), dict(protocol=2, eps_min=1.5), dict(protocol=2, eps_decay=float("nan"))):
        c = new_engine()
        setup_proto(c, tr2, {**tr2["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL"})
        refused(capi.TS_E_INVALID, lambda: c.lights_proto_config(**cfg))
        assert c.lights_proto_info()["protocol"] == 0
        c.close()
    a2c.close()


def test_every_entry_is_unsupported_under_another_algorithm():
    from tests.trace_util import setup_from_trace
    api = new_engine()
    setup_from_trace(api, load_trace(trace_path("lights_qa_96_s2")))
    z = np.zeros(api.n_groups, np.int8)
    refused(capi.TS_E_UNSUPPORTED, lambda: api.lights_proto_config("RL_A2C_BATCHED"), api.lights_proto_info, api.lights_proto_observe,
            lambda: api.lights_proto_act(z), lambda: api.lights_proto_act_q(np.zeros((api.n_groups, 2), np.float32)),
            api.lights_proto_controller, api.lights_proto_device)
    api.step(2)
    api.close()


DEVICE_SCRIPT = r'''
import numpy as np
from trafficsimulation_amd._lib import new_engine
from tests.engine_util import proto_engine as fixture_engine
bits = lambda a: np.ascontiguousarray(a).tobytes()
a, tr = fixture_engine("lights_gat_64_s45")
b, _ = fixture_engine("lights_gat_64_s45")
dev = a.lights_proto_device()
G = a.n_groups
assert tuple(dev["state"].shape) == tuple(dev["next_state"].shape) == (G, 5, 9) and tuple(dev["mask"].shape) == (G, 5)
assert dev["reward"].dtype == dev["epsilon"].dtype == torch.float64 and dev["actions"].dtype == torch.int8 and dev["state"].is_cuda
for t in range(25):
    f, m = a.lights_proto_observe()
    assert bits(dev["state"].cpu().numpy()) == bits(f) and bits(dev["mask"].cpu().numpy()) == bits(m)
    if t %% 2:      # q that never leaves the device
        acts, r, n = a.lights_proto_act_q(torch.from_numpy(tr["lp_q"][t]).to(dev["state"].device))
    else:
        acts, r, n = a.lights_proto_act_q(tr["lp_q"][t])
    rb = b.lights_proto_act_q(tr["lp_q"][t])
    assert np.array_equal(acts, tr["lp_action"][t]) and bits(r) == bits(rb[1]) == bits(tr["lp_reward"][t]) and bits(n) == bits(rb[2])
    assert bits(dev["next_state"].cpu().numpy()) == bits(n) and bits(dev["reward"].cpu().numpy()) == bits(r)
    assert np.array_equal(dev["actions"].cpu().numpy(), acts) and bits(dev["epsilon"].cpu().numpy()) == bits(tr["lp_eps"][t])
    a.step(1); b.step(1)
assert a.checkpoint_save() == b.checkpoint_save()
# nothing comes down with to_host=False: the device tensors hold what the other engine's host arrays hold
for t in range(25, 30):
    assert a.lights_proto_observe(to_host=False) is None
    f, m = b.lights_proto_observe()
    assert bits(dev["state"].cpu().numpy()) == bits(f) and bits(dev["mask"].cpu().numpy()) == bits(m)
    assert a.lights_proto_act_q(torch.from_numpy(tr["lp_q"][t]).to(dev["state"].device), to_host=False) is None
    acts, r, n = b.lights_proto_act_q(tr["lp_q"][t])
    assert np.array_equal(dev["actions"].cpu().numpy(), acts) and bits(dev["reward"].cpu().numpy()) == bits(r)
    assert bits(dev["next_state"].cpu().numpy()) == bits(n) and np.array_equal(acts, tr["lp_action"][t])
    a.step(1); b.step(1)
two = a.lights_proto_act_q(tr["lp_q"][30], want_next=False)
assert len(two) == 2 and np.array_equal(two[0], b.lights_proto_act_q(tr["lp_q"][30])[0])
assert a.checkpoint_save() == b.checkpoint_save() and bits(dev["reward"].cpu().numpy()) == bits(tr["lp_reward"][30])
a.step(1); b.step(1)
# device actions through act: no draw, and with to_host=False nothing comes down
saved = a.checkpoint_save()
assert a.lights_proto_act(torch.from_numpy(tr["lp_action"][31]).to(dev["state"].device), to_host=False) is None
assert bits(dev["reward"].cpu().numpy()) == bits(tr["lp_reward"][31]) and bits(dev["next_state"].cpu().numpy()) == bits(tr["lp_next_state"][31])
a.checkpoint_load(saved)
from trafficsimulation_amd import _capi as capi
fp = list(a.rng_fingerprint(capi.RNG_GLOBAL))
r, n = a.lights_proto_act(torch.from_numpy(tr["lp_action"][31]).to(dev["state"].device))
assert list(a.rng_fingerprint(capi.RNG_GLOBAL)) == fp and bits(r) == bits(tr["lp_reward"][31]) and bits(n) == bits(tr["lp_next_state"][31])
before = a.checkpoint_save()
try:
    a.lights_proto_act_q(torch.full((G, 2), float("nan"), device=dev["state"].device))
    raise SystemExit("a device q of NaN was accepted")
except Exception as ex:
    assert getattr(ex, "code", None) == -1, ex
assert a.checkpoint_save() == before
a.close(); b.close()
'''


def test_device_tensors_device_actions_and_device_q():
    """lights_proto_device(), act(torch tensor) and act_q(torch tensor), in a process of its own that imports torch first."""
    procs.run_python(DEVICE_SCRIPT, torch_first=True, timeout=300)
