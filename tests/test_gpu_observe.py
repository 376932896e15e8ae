"""Traffic observation (include/trafficsim_observe.h) on the GPU: the planes against what the golden traces say they must
hold (tests/observe_util.py), a run that observation does not change, the device-side reductions, a large world's
invariants, the life cycle of the planes and the sharded mode."""
import copy
import os

import numpy as np
import pytest

from tests import observe_util as ou
from tests import procs
from tests.engine_util import assert_same_state, city_model, engine_for, full_state, refused
from tests.observe_util import REPLAN_TRACES, UNCAPPED_REPLAN_TRACES
from tests.trace_util import NO_ASTAR_TRACES, replay_and_compare
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd._lib import new_engine

pytestmark = pytest.mark.gpu

SAMPLED, ENTER = slice(0, 3), slice(3, 7)


# ---- 1. exact planes on the traces that only replay their spawn-time paths -------------------------------------
@pytest.mark.parametrize("name", NO_ASTAR_TRACES)
def test_replay_only_traces_are_exact_every_tick(name):
    api, tr = engine_for(name, explicit_paths=True)
    api.observe_start()
    want = np.zeros((7, int(tr["height"]), int(tr["width"])), dtype=np.uint32)
    for t in range(ou.n_ticks(tr)):
        api.step(1)
        want[SAMPLED] += ou.sampled_delta(tr, t)
        want[ENTER] += ou.enter_replay(tr, t)
        got = ou.read_planes(api)
        for k, plane in enumerate(capi.OBS_PLANES):
            assert np.array_equal(got[k], want[k]), f"tick {t}: plane {plane} differs at {np.argwhere(got[k] != want[k])[:4].tolist()}"
    assert api.observe_info()["ticks"] == ou.n_ticks(tr)
    assert api.counters().astar_calls == 0
    api.close()


# ---- 2. traces with replanning: sampled planes exact, ENTER exact outside the uncertain cells ---------------------------
@pytest.mark.parametrize("name", REPLAN_TRACES + UNCAPPED_REPLAN_TRACES)
def test_reconstructed_traces(name):
    api, tr = engine_for(name)
    api.observe_start()
    snaps = []
    engine_step = api.step

    def step(n=1):
        engine_step(n)
        snaps.append(ou.read_planes(api))
    api.step = step
    T = replay_and_compare(api, tr)          # the run itself is the reference's, tick by tick, with observation on
    assert len(snaps) >= T > 0
    want = np.zeros((3,) + snaps[0].shape[1:], dtype=np.uint32)
    before = np.zeros_like(snaps[0])
    lo = hi = 0
    for t in range(T):
        want += ou.sampled_delta(tr, t)
        for k in range(3):
            assert np.array_equal(snaps[t][k], want[k]), f"tick {t}: plane {capi.OBS_PLANES[k]}"
        e = ou.enter_reconstruct(tr, t)
        delta = snaps[t][ENTER] - before[ENTER]
        keep = ~e["uncertain"]
        assert np.array_equal(delta[:, keep], e["exact"][:, keep]), \
            f"tick {t}: ENTER differs outside the uncertain cells at {np.argwhere(delta[:, keep] != e['exact'][:, keep])[:4].tolist()}"
        known = int(e["exact"].sum()) + e["unc_known"]
        assert known <= int(delta.sum()) <= known + e["unc_slack"], f"tick {t}: ENTER grew by {int(delta.sum())}, the rows allow {known} .. {known + e['unc_slack']}"
        lo, hi = lo + known, hi + known + e["unc_slack"]
        before = snaps[t]
    assert lo <= int(snaps[T - 1][ENTER].astype(np.uint64).sum()) <= hi
    api.close()


# ---- 3. on, off and started mid-run -----------------------------------------------------------------------------------------
def test_on_off_and_mid_run_compute_the_same():
    name, T, late = "full_96_s8", 40, 10
    off, _ = engine_for(name)
    off.step(T)
    on, _ = engine_for(name)
    on.observe_start()
    on.step(late)
    at_late = ou.read_planes(on)
    on.step(T - late)
    mid, _ = engine_for(name)
    mid.step(late)
    mid.observe_start()
    mid.step(T - late)
    want = full_state(off)
    assert_same_state(want, full_state(on), "observation on")
    assert_same_state(want, full_state(mid), "observation started at tick 10")
    assert off.counters().astar_calls > 0
    full, part = ou.read_planes(on), ou.read_planes(mid)
    assert np.array_equal(part, full - at_late)
    assert on.observe_info()["ticks"] == T and mid.observe_info()["ticks"] == T - late and off.observe_info()["mask"] == 0
    for a in (off, on, mid):
        a.close()


# ---- 4. reductions ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def observed_rect():
    api, tr = engine_for("rect_64x112_s19")
    api.observe_start()
    api.step(80)
    planes = ou.read_planes(api)
    assert planes[0].shape == (112, 64) or planes[0].shape == (64, 112)
    assert planes[ENTER].sum() > 0 and planes[1].sum() > 0
    yield api, tr, planes
    api.close()


@pytest.mark.parametrize("factor", [1, 8, 7, 1000])
def test_pooled(observed_rect, factor):
    api, _, planes = observed_rect
    for k, name in enumerate(capi.OBS_PLANES):
        got = api.observe_pooled(name, factor)
        want = ou.pooled(planes[k], factor)
        assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), f"{name} pooled by {factor}"


def test_regions(observed_rect):
    api, _, planes = observed_rect
    H, W = planes[0].shape
    rects = [(0, 0, W, H), (0, 0, 0, 0), (5, 5, 5, 9), (9, 9, 3, 3), (-10, -10, 4, 4), (W - 3, H - 3, W + 50, H + 50), (W, H, W + 5, H + 5),
             (7, 11, 8, 12), (-5, 20, 10 ** 6, 21), (3, 4, 40, 90)]
    ys, xs = np.nonzero(planes[0])
    rects.append((int(xs[0]), int(ys[0]), int(xs[0]) + 1, int(ys[0]) + 1))      # a single cell that is not zero
    for k, name in enumerate(capi.OBS_PLANES):
        assert np.array_equal(api.observe_regions(name, rects), ou.region_sums(planes[k], rects)), name
    assert api.observe_regions("present", []).shape == (0,)


def test_groups(observed_rect):
    api, tr, planes = observed_rect
    got = api.observe_groups()
    assert got.dtype == np.int64 and got.shape == (len(tr["g_icell_off"]) - 1, len(capi.OG_FIELDS)) and got.shape[0] > 0
    want = ou.group_sums(tr, planes)
    assert np.array_equal(got, want)
    assert want[:, 4:].sum() > 0 and want[:, :4].sum() > 0


DEVICE_SCRIPT = r'''
import numpy as np
from trafficsimulation_amd import _capi as capi
from tests.engine_util import engine_for
api, _ = engine_for("full_96_s8")
api.observe_start()
api.step(12)
for name in capi.OBS_PLANES:
    t = api.observe_device(name)
    host = api.observe_plane(name)
    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == host.shape
    assert np.array_equal(t.cpu().numpy().view(np.uint32), host) and (host.sum() > 0 or name == "waiting")
flow = sum(api.observe_device(n).to(torch.int64) for n in capi.OBS_ENTER)      # (consumed on the device, no copy to the host)
assert int(flow.sum()) == sum(int(api.observe_plane(n).sum()) for n in capi.OBS_ENTER) > 0
api.close()
'''


def test_device_pointer_is_the_plane():
    """observe_device(): a torch tensor over the engine's own plane.  In a process of its own that imports torch before it
    loads the engine, the way the torch-side callers (dist.py) run."""
    procs.run_python(DEVICE_SCRIPT, torch_first=True, timeout=300)


# ---- 5. a 512 x 512 world through a replanning wave: invariants ----------------------------------------------------------
def test_large_world_invariants():
    import bench
    tables, routes, _ = bench.make_workload(512, 25_000, 3)
    api = new_engine()
    bench.setup(api, tables, routes, 3, policy="full")
    assert api.num_vehicles() >= 20_000
    api.observe_start()
    V = ou.V
    rows = api.vehicles()
    before = np.zeros((7, 512, 512), dtype=np.uint32)
    for t in range(14):
        api.step(1)
        now = api.vehicles()
        planes = ou.read_planes(api)
        delta = planes - before
        steps0 = dict(zip(rows[:, V["spawn_idx"]].tolist(), rows[:, V["steps_traveled"]].tolist()))
        alive = [int(s) - steps0[int(i)] for i, s in zip(now[:, V["spawn_idx"]], now[:, V["steps_traveled"]]) if int(i) in steps0]
        vanished = len(rows) - len(alive)
        grown = int(delta[ENTER].sum())
        assert sum(alive) <= grown <= sum(alive) + ou.MAX_MOVE * vanished, f"tick {t}: ENTER grew by {grown}, steps by {sum(alive)}, {vanished} vanished"
        assert int(delta[0].sum()) == len(now) == api.num_vehicles(), f"tick {t}: PRESENT"
        assert (planes[1] <= planes[0]).all(), f"tick {t}: WAITING exceeds PRESENT"
        assert int(delta[2].sum()) == int(now[:, V["current_speed"]].sum()), f"tick {t}: SPEED"
        rows, before = now, planes
    assert api.counters().astar_calls > 0, "no replanning wave in this run"
    assert int(before[1].sum()) > 0
    api.close()


# ---- 6. life cycle ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_errors():
    api, tr = engine_for("lights_qa_96_s2", explicit_paths=True)
    H, W = int(tr["height"]), int(tr["width"])
    assert api.has_observe and api.observe_info() == {"planes": [], "mask": 0, "ticks": 0, "width": W, "height": H, "device_bytes": 0}
    refused(capi.TS_E_STATE, lambda: api.observe_plane("present"), api.observe_reset, api.observe_groups, lambda: api.observe_pooled("present", 4),
            lambda: api.observe_regions("present", [(0, 0, 1, 1)]), lambda: api.observe_device("present"))
    api.observe_stop()                       # (off already: fine)
    refused(capi.TS_E_INVALID, *(lambda bad=bad: api.observe_start(bad) for bad in (0, 1 << 7, 0xFFFFFFFF)))
    api.observe_start(["present", "enter_n"])
    info = api.observe_info()
    assert info["planes"] == ["present", "enter_n"] and info["device_bytes"] == 2 * 4 * W * H and info["ticks"] == 0
    api.step(3)
    assert api.observe_info()["ticks"] == 3 and api.observe_plane("present").sum() == sum(len(ou.rows_at(tr, t)) for t in range(3))
    refused(capi.TS_E_STATE, lambda: api.observe_plane("waiting"), api.observe_groups, lambda: api.observe_pooled("speed", 2))
    refused(capi.TS_E_INVALID, lambda: api.observe_plane(7), lambda: api.observe_plane(-1), lambda: api.observe_pooled("present", 0),
            lambda: api.observe_pooled("present", -3))
    api.observe_reset()
    assert api.observe_info()["ticks"] == 0 and api.observe_plane("present").sum() == 0 and api.observe_plane("enter_n").sum() == 0
    # a checkpoint load rewinds the run, not what was observed of it
    blob = api.checkpoint_save()
    api.step(4)
    held = [api.observe_plane("present"), api.observe_plane("enter_n")]
    api.checkpoint_load(blob)
    assert api.observe_info()["ticks"] == 4 and api.observe_info()["planes"] == ["present", "enter_n"]
    assert np.array_equal(api.observe_plane("present"), held[0]) and np.array_equal(api.observe_plane("enter_n"), held[1])
    # another mask: new planes, from zero
    api.observe_start(["waiting", "speed", "enter_n"])
    assert api.observe_info()["planes"] == ["waiting", "speed", "enter_n"] and api.observe_plane("enter_n").sum() == 0
    api.observe_stop()
    assert api.observe_info()["mask"] == 0
    api.step(2)                              # (and the run goes on)
    api.close()


def test_one_step_of_five_adds_what_five_steps_of_one_add():
    a, _ = engine_for("full_96_s8")
    b, _ = engine_for("full_96_s8")
    a.observe_start(), b.observe_start()
    a.step(5)
    for _ in range(5):
        b.step(1)
    assert np.array_equal(ou.read_planes(a), ou.read_planes(b)) and ou.read_planes(a)[ENTER].sum() > 0
    assert a.observe_info()["ticks"] == b.observe_info()["ticks"] == 5
    a.close(), b.close()


def test_facade_observes_and_copies_come_without(tmp_path):
    from trafficsimulation_amd.mesa_api import CityModel
    m = city_model(200, seed=1)
    m.observe()
    for _ in range(30):
        m.step()
    obs = m.observations()
    assert obs["ticks"] == 30 and set(capi.OBS_PLANES) <= set(obs)
    assert np.array_equal(obs["flow"], sum(obs[n].astype(np.uint64) for n in capi.OBS_ENTER)) and obs["flow"].sum() > 0
    seen = obs["present"] > 0
    assert np.isnan(obs["mean_speed"][~seen]).all() and np.array_equal(obs["mean_speed"][seen], obs["speed"][seen] / obs["present"][seen])
    rep = m.intersection_report()
    rows = m.engine.observe_groups()
    assert len(rep) == len(rows) == len(m.intersection_light_groups) > 0
    for g, r in enumerate(rep):
        assert (r["waiting_ns"], r["waiting_ew"]) == (int(rows[g, 0]), int(rows[g, 2])) and r["throughput"] == int(rows[g, 4:].sum())
    twin = copy.deepcopy(m)
    assert twin.engine.observe_info()["mask"] == 0 and m.engine.observe_info()["ticks"] == 30
    path = os.path.join(tmp_path, "m.npz")
    m.save(path)
    loaded = CityModel.load(path)
    assert loaded.engine.observe_info()["mask"] == 0
    m.observe(planes=())
    assert m.engine.observe_info()["mask"] == 0
    for x in (m, twin, loaded):
        x.close()


# ---- 7. sharded mode: every rank holds the same planes --------------------------------------------------------------------
WORKER = r'''
import numpy as np
from tests.engine_util import engine_for
from tests.trace_util import replay_and_compare
from tests import observe_util as ou
api, tr = engine_for(%(trace)r)
sr = tdist.ShardedReplans().attach(api)
api.observe_start()
n = replay_and_compare(api, tr)
assert sr.calls > 0
np.save(os.path.join(OUTDIR, "planes%%d.npy" %% rank), ou.read_planes(api))
api.close()
'''


def test_sharded_ranks_hold_equal_planes():
    name = "full_96_s8"
    _, saved, _ = procs.run_ranks(WORKER, 2, timeout=600, trace=name)
    ranks = [saved[f"planes{r}.npy"] for r in range(2)]
    api, tr = engine_for(name)
    api.observe_start()
    api.step(ou.n_ticks(tr))
    single = ou.read_planes(api)
    api.close()
    assert single[ENTER].sum() > 0
    assert np.array_equal(ranks[0], ranks[1]) and np.array_equal(ranks[0], single)
