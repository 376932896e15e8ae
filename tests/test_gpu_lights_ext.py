"""External light control (include/trafficsim_lights_ext.h) on the device.

1. both fixtures of tests/golden/make_golden_lights.py replayed: observe / act / controller rows against what the reference's
   run_batched_rl_control recorded, every tick, float32 bit for bit, and the tick in between against the ordinary trace;
2. requests derived from two existing golden traces reproduce them under TS_LIGHTS_EXTERNAL;
3. a differential hunt against the numpy model (tests/lights_ext_expect.py) on other worlds, every dimension, random actions;
4. observe is idempotent, act without observe equals observe then act;
5. checkpoints carry the controller state; 6. device tensors; 7. refusals."""
import os

import numpy as np
import pytest

from tests import lights_ext_expect as lx
from tests.lights_ext_expect import FIXTURES, GATED, Stepper
from tests import procs
from tests.engine_util import refused
from tests.trace_util import check_initial, replay_and_compare, setup_from_trace, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import build_engine, load_trace

pytestmark = pytest.mark.gpu

STUCK_SOON = {"PATHFINDING_COOLDOWN": 5, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": 2, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD_INTERSECTION": 1}


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the reference's own controller runs ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_replays_the_reference_controller(name):
    tr = load_trace(trace_path(name))
    api = new_engine()
    setup_from_trace(api, tr)
    check_initial(api, tr)
    info = api.lights_info()
    assert (info["state_dim"], info["min_green"], info["calls"]) == (int(tr["rl_dim"]), int(tr["rl_min_green"]), 0)

    def control(t):
        s = api.lights_observe()
        assert same_bits(s, tr["rl_state"][t]), f"tick {t}: state of groups {np.nonzero((s != tr['rl_state'][t]).any(axis=1))[0]}"
        n = api.lights_act(tr["rl_action"][t])
        assert same_bits(n, tr["rl_next_state"][t]), f"tick {t}: next state of groups {np.nonzero((n != tr['rl_next_state'][t]).any(axis=1))[0]}"
        want = tr["rl_ctrl"][t]
        assert np.array_equal(api.lights_controller(), want[:, :2]), f"tick {t}: _rl_phase / rl_timer"
        assert np.array_equal(api.groups()[:, :2], want[:, 2:]), f"tick {t}: current / pending phase after the call"
    T = len(tr["rl_state"])
    assert replay_and_compare(Stepper(api, control), tr) == T
    assert api.lights_info()["calls"] == T
    api.close()


# ---- 2. requests reproduce an existing golden trace ------------------------------------------------------------------------
def derived_requests(tr):
    """The phase every group asked for inside each tick of a golden run, from pending / current before and after it."""
    rows = tr["grp_rows"]
    T, G = rows.shape[:2]
    before = np.concatenate([np.tile(np.asarray([-1, 0], np.int32), (1, G, 1)), rows[:-1, :, :2]])   # (current None, pending 0)
    cur_b, pend_b, cur_a, pend_a = before[:, :, 0], before[:, :, 1], rows[:, :, 0], rows[:, :, 1]
    req = np.full((T, G), -1, dtype=np.int8)
    free = pend_b < 0
    req[free & (pend_a >= 0)] = pend_a[free & (pend_a >= 0)]
    changed = free & (pend_a < 0) & (cur_a != cur_b)
    req[changed] = cur_a[changed]
    return req


@pytest.mark.parametrize("name", ["lights_qa_96_s2", "lights_fixed_64_s4"])
def test_requests_reproduce_a_golden_trace(name):
    tr = load_trace(trace_path(name))
    req = derived_requests(tr)
    assert (req >= 0).sum() > tr["grp_rows"].shape[1]       # (more than the first phase of every group)
    ext = dict(tr, defaults_json={**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL"})
    api = new_engine()
    setup_from_trace(api, ext)
    check_initial(api, tr)

    def groups(t, got):
        # current / pending are the engine's; the timers of the in-step algorithm do not exist under EXTERNAL
        assert not got[:, 2:].any()
        return np.concatenate([got[:, :2], tr["grp_rows"][t][:, 2:]], axis=1)
    T = len(req)
    assert replay_and_compare(Stepper(api, lambda t: api.lights_request(req[t]), groups), tr) == T
    assert api.lights_info()["calls"] == 0 and not api.lights_controller().any()       # no protocol state was touched
    api.close()


# ---- 3. differential hunt against the numpy model --------------------------------------------------------------------------
HUNT_WORLDS = ["rect_64x112_s19", "ragged_100x75_s33", "carve_96_s10", "unopt_96_s21", "lights_ext_96_s42"]
BUSY_WORLDS = ["ragged_100x75_s33", "carve_96_s10", "lights_ext_96_s42"]
N_CASES = int(os.environ.get("TS_RANDOM_CASES", "10"))


def hunt_engine(case, monkeypatch):
    rng = np.random.default_rng(7000 + case)
    # odd cases run ungated on the worlds with a few hundred vehicles, so that queues build up and vehicles become stuck
    world = BUSY_WORLDS[(case // 2) % len(BUSY_WORLDS)] if case % 2 else HUNT_WORLDS[case % len(HUNT_WORLDS)]
    tr = load_trace(trace_path(world))
    # even cases walk through every dimension; the ungated ones take the two that read the stuck map
    dim = (17, 19)[(case // 2) % 2] if case % 2 else lx.DIMS[(case // 2) % len(lx.DIMS)]
    team = (8, 4, 16, 32)[(case // 2) % 4]
    penalties = (0.5, 5, 50.0) if case % 3 else (0.3, 5.25, 12.1)
    d = {**GATED, "RAIN_ENABLED": False, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL", "SRL_INPUT_DIMENSIONS": dim,
         "SRL_MIN_GREEN": int(rng.choice([1, 3, 5])), "VEHICLE_ROAD_TYPES_PENALTY_R1": penalties[0],
         "VEHICLE_ROAD_TYPES_PENALTY_R2": penalties[1], "VEHICLE_ROAD_TYPES_PENALTY_R3": penalties[2],
         "TRAFFIC_LIGHT_TRANSITION_CLEARANCE_ENABLED": bool(rng.integers(4) > 0)}
    if case % 2:      # nothing gated and a low stuck threshold: queued vehicles become stuck, the stuck map is not empty
        d.update(STUCK_SOON)
    tables = {k: v for k, v in tr.items() if k != "g_approach_road_types"}     # (the engine's own default for penalty_score)
    kinds = np.asarray(tables["schedule_kinds0"])
    tables["schedule_kinds0"] = kinds[kinds != 2]
    monkeypatch.setenv("TS_DEBUG_LIGHTS_TEAM", str(team))
    monkeypatch.setenv("TS_DEBUG_LIGHTS_BLOCK", str((256, 8, 16)[case % 3]))     # (8: three blocks of the per-group kernels at G = 18 .. 23)
    api = new_engine()
    build_engine(api, tables, defaults=d, global_seed=case + 1, sched_seed=case + 5)
    n = int(rng.integers(len(tr["v_start_xy"]) // 2, len(tr["v_start_xy"]) + 1))
    if case % 2:
        n = len(tr["v_start_xy"])
    api.add_vehicles(tr["v_start_xy"][:n], tr["v_goal_xy"][:n], np.full(n, capi.POP["through"], np.int32))
    return api, tables, d, dim, team, penalties, rng


@pytest.mark.parametrize("case", range(N_CASES))
def test_hunt_against_the_numpy_model(case, monkeypatch):
    api, tables, d, dim, team, penalties, rng = hunt_engine(case, monkeypatch)
    G = api.n_groups
    longest = max(int(np.diff(tables[f"g_{nm}_off"]).max()) for nm in ("ns_in", "ew_in"))
    # a ragged tail (G is no multiple of the 64 / team groups a wavefront serves; 18 groups at team 32 are the exception) and
    # a list that takes a team more than one stride
    assert G % (64 // team) != 0 or (G, team) in ((18, 32), (18, 16))
    assert longest > team
    ctrl = lx.Ctrl(G)
    static = lx.static_features(tables, penalties)
    ctx = f"case {case} (dim {dim}, team {team}, G {G}, longest list {longest})"
    stuck_seen = 0
    for t in range(30 if case % 2 else 14):
        rows = api.groups()
        ctrl.current, ctrl.pending = rows[:, 0].copy(), rows[:, 1].copy()
        ctrl.repop = np.asarray([bool(api.group_links(g, False)) for g in range(G)])
        occ, stuck = api.map(capi.MAP_OCCUPANCY), api.map(capi.MAP_STUCK)
        want = lx.phase_a(tables, occ, stuck, ctrl, dim, static)
        stuck_seen += int(lx.local_sums(tables, stuck).sum())
        got = api.lights_observe()
        assert same_bits(got, want), f"{ctx} tick {t}: state of groups {np.nonzero((got != want).any(axis=1))[0]}"
        if t % 5 == 3:      # a controller of the other kind in between: protocol state untouched
            ph = rng.integers(-1, 2, size=G).astype(np.int8)
            api.lights_request(ph)
            lx.request(ctrl, ph)
        actions = (rng.random(G) < (0.8 if t < 7 else 0.3)).astype(np.int8)
        want_n = lx.phase_b(tables, occ, stuck, ctrl, actions, dim, d["SRL_MIN_GREEN"], static)
        got_n = api.lights_act(actions)
        assert same_bits(got_n, want_n), f"{ctx} tick {t}: next state of groups {np.nonzero((got_n != want_n).any(axis=1))[0]}"
        assert np.array_equal(api.lights_controller(), ctrl.rows()), f"{ctx} tick {t}: controller rows"
        rows = api.groups()
        assert np.array_equal(rows[:, 0], ctrl.current) and np.array_equal(rows[:, 1], ctrl.pending), f"{ctx} tick {t}: phases"
        api.step(1)
    if case % 2:      # the stuck-map half of the vector was compared on values other than 0
        assert stuck_seen > 0, f"{ctx}: no vehicle was ever stuck on an approach cell"
    api.close()


# ---- 4. observe is idempotent; act runs phase A itself ---------------------------------------------------------------------
def fixture_engine(name="lights_ext_96_s42", dim=None):
    tr = load_trace(trace_path(name))
    if dim is not None:
        tr = dict(tr, defaults_json={**tr["defaults_json"], "SRL_INPUT_DIMENSIONS": dim})
    api = new_engine()
    setup_from_trace(api, tr)
    return api, tr


def test_observe_twice_and_act_without_observe():
    (a, tr), (b, _) = fixture_engine(), fixture_engine()
    for t in range(12):
        s1 = a.lights_observe()
        s2 = a.lights_observe()
        assert same_bits(s1, s2) and a.lights_info()["calls"] == t + 1 and a.lights_info()["observed"] == 1
        assert same_bits(s1, tr["rl_state"][t])
        na = a.lights_act(tr["rl_action"][t])
        nb = b.lights_act(tr["rl_action"][t])          # no observe: phase A runs inside
        assert same_bits(na, nb) and a.lights_info()["observed"] == 0 and b.lights_info()["calls"] == t + 1
        assert np.array_equal(a.lights_controller(), b.lights_controller()) and np.array_equal(a.groups(), b.groups())
        a.step(1)
        b.step(1)
    assert a.checkpoint_save() == b.checkpoint_save()
    # an observe that no act follows ends with the tick: the next one is a new control call
    a.lights_observe()
    a.step(1)
    assert a.lights_info()["observed"] == 0
    a.lights_observe()
    assert a.lights_info()["calls"] == 14
    a.close()
    b.close()


# ---- 5. checkpoints --------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_controller():
    a, tr = fixture_engine()
    act = tr["rl_action"]
    for t in range(20):
        a.lights_act(act[t])
        a.step(1)
    a.lights_observe()                      # saved between observe and act: the cached vector travels too
    blob = a.checkpoint_save()
    assert len(blob) == a.checkpoint_size()
    b, _ = fixture_engine()
    b.checkpoint_load(blob)
    assert b.checkpoint_save() == blob
    assert b.lights_info() == a.lights_info() and b.lights_info()["observed"] == 1
    for t in range(20, 40):
        sa, sb = a.lights_observe(), b.lights_observe()
        assert same_bits(sa, sb) and same_bits(sa, tr["rl_state"][t]), f"tick {t}"
        assert same_bits(a.lights_act(act[t]), b.lights_act(act[t]))
        a.step(1)
        b.step(1)
    assert a.checkpoint_save() == b.checkpoint_save()
    a.close()
    b.close()


def test_checkpoint_refuses_another_configuration():
    a, tr = fixture_engine()
    for t in range(6):
        a.lights_act(tr["rl_action"][t])
        a.step(1)
    blob = a.checkpoint_save()
    for other in (dict(dim=13), dict(min_green=4)):
        b, _ = fixture_engine(dim=other.get("dim"))
        if "min_green" in other:
            b.lights_config(19, other["min_green"])
        for t in range(3):
            b.lights_act(tr["rl_action"][t])
            b.step(1)
        before = b.checkpoint_save()
        ex, = refused(capi.TS_E_INVALID, lambda: b.checkpoint_load(blob))
        assert "min-green" in str(ex)
        assert b.checkpoint_save() == before, "a refused load changed the target"
        b.close()
    a.close()


def test_blob_sizes_follow_the_format():
    """A QUEUE_ACTUATED blob has the size the format documented in DESIGN.md gives (no section of the extension); the same
    world under EXTERNAL adds exactly the trailing section."""
    tr = load_trace(trace_path("lights_qa_96_s2"))
    N = int(tr["width"]) * int(tr["height"])
    nv = len(tr["v_start_xy"])
    words = int(((np.diff(tr["v_path0_off"]) + 15) // 16).sum())
    kinds = np.asarray(tr["schedule_kinds0"])
    G = len(tr["g_light_off"]) - 1
    n_sched = len(kinds) + nv
    assert not (kinds == 2).any()
    want = (64 + 6280            # header, CkScalars
            + 8 * 8              # eight empty length-prefixed containers (no blocks are registered: their section is empty)
            + 9 * N + 95 * nv + 8 * nv + 4 * words
            + 4 * nv + 5 * n_sched + 4 * int((kinds == 1).sum()) + 13 * 4 * G)
    sizes = {}
    for algo in ("QUEUE_ACTUATED", "EXTERNAL"):
        t2 = dict(tr, defaults_json={**tr["defaults_json"], "TRAFFIC_LIGHT_AGENT_ALGORITHM": algo, "PATHFINDING_CACHE": False})
        api = new_engine()
        setup_from_trace(api, t2, explicit_paths=True)
        assert api.num_scheduled() == n_sched
        sizes[algo] = api.checkpoint_size()
        assert len(api.checkpoint_save()) == sizes[algo]
        api.close()
    assert sizes["QUEUE_ACTUATED"] == want
    assert sizes["EXTERNAL"] == want + 24 + G * (8 + 8 + 13 * 4)


# ---- 6. device tensors -----------------------------------------------------------------------------------------------------
DEVICE_SCRIPT = r'''
import numpy as np
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace
from tests.trace_util import setup_from_trace, trace_path
tr = load_trace(trace_path("lights_ext_stuck_96_s43"))
a, b = new_engine(), new_engine()
for e in (a, b):
    setup_from_trace(e, tr)
dev = a.lights_device()
G, dim = a.n_groups, 19
assert tuple(dev["state"].shape) == tuple(dev["next_state"].shape) == (G, dim) and dev["state"].dtype == torch.float32
assert tuple(dev["controller"].shape) == tuple(dev["stored"].shape) == (G, 2) and dev["controller"].dtype == torch.int32
seen = 0
for t in range(40):
    s = a.lights_observe()
    assert dev["state"].is_cuda and np.array_equal(dev["state"].cpu().numpy().view(np.uint32), s.view(np.uint32))
    act = torch.from_numpy(tr["rl_action"][t].astype(np.int8)).to(dev["state"].device)      # actions that never leave the device
    na = a.lights_act(act)
    nb = b.lights_act(tr["rl_action"][t])
    assert np.array_equal(na.view(np.uint32), nb.view(np.uint32)) and np.array_equal(na.view(np.uint32), tr["rl_next_state"][t].view(np.uint32))
    assert np.array_equal(dev["next_state"].cpu().numpy().view(np.uint32), na.view(np.uint32))
    assert np.array_equal(dev["controller"].cpu().numpy(), a.lights_controller())
    p = dev["stored"].cpu().numpy()
    assert np.array_equal(p[:, 0], -p[:, 1]) and np.array_equal(p[:, 0].astype(np.float32), s[:, 15])      # the stuck-map pressure at 19
    seen += int((p != 0).sum())
    a.step(1); b.step(1)
assert seen > 0, "the stored stuck-map pressure was 0 throughout"
assert a.checkpoint_save() == b.checkpoint_save()
bad = torch.full((G,), 2, dtype=torch.int8, device=dev["state"].device)
before = a.checkpoint_save()
try:
    a.lights_act(bad)
    raise SystemExit("a device action of 2 was accepted")
except Exception as ex:
    assert getattr(ex, "code", None) == -1, ex
assert a.checkpoint_save() == before
a.close(); b.close()
'''


def test_device_tensors_and_device_actions():
    """lights_device() and lights_act(torch tensor), in a process of its own that imports torch before it loads the engine."""
    procs.run_python(DEVICE_SCRIPT, torch_first=True, timeout=300)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_every_entry_is_unsupported_under_another_algorithm():
    api = new_engine()
    setup_from_trace(api, load_trace(trace_path("lights_qa_96_s2")))
    z = np.zeros(api.n_groups, np.int8)
    refused(capi.TS_E_UNSUPPORTED, lambda: api.lights_config(13, 5), lambda: api.lights_set_static(np.zeros(api.n_groups), None), api.lights_info,
            api.lights_observe, lambda: api.lights_act(z), lambda: api.lights_request(z), api.lights_controller)
    api.step(2)
    api.close()


def test_bad_arguments_change_nothing():
    api, tr = fixture_engine()
    G = api.n_groups
    for t in range(3):
        api.lights_act(tr["rl_action"][t])
        api.step(1)
    before = api.checkpoint_save()
    bad_actions = [np.full(G, 2, np.int8), np.concatenate([np.zeros(G - 1, np.int8), [-1]]).astype(np.int8)]
    for v in bad_actions:
        refused(capi.TS_E_INVALID, lambda: api.lights_act(v))
    refused(capi.TS_E_INVALID, lambda: api.lights_request(np.full(G, -2, np.int8)))
    for dim, mg in ((12, 5), (19, -1)):
        refused(capi.TS_E_INVALID, lambda: api.lights_config(dim, mg))
    refused(capi.TS_E_STATE, lambda: api.lights_config(13, 5))     # a valid configuration, but control calls have been made
    with pytest.raises(ValueError):
        api.lights_act(np.zeros(G + 1, np.int8))
    assert api.checkpoint_save() == before and api.lights_info()["observed"] == 0
    api.close()
