"""The host tail of k_replan's passes (csrc/replan.h RTail, csrc/replan_host.h, csrc/astar_host.h): searches abandoned on the device,
finished on host threads and replayed by a re-run of their step_decide.  Nothing in a run's result may depend on it: every test
here holds the engine against the reference's traces or the CPU oracle, with hand-offs forced (TS_TAIL_FORCE), through the real
rule (the idle counter, with a handful of searcher slots) and beside the other paths of a pass (the spill form of the search
loop, the pool-full retry, sharded ranks), and checks that searches really went to the host (the profile row host_replan_tail).
The 512^2 oracle run is computed once and shared."""
import os

import numpy as np
import pytest

from tests import kats_util as K
from tests import procs
from tests import test_gpu_parity as P
from tests.engine_util import MAPS, compare_full, engine_for, small_engine
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import _lib

pytestmark = pytest.mark.gpu

TICKS_512 = 9


def profiled(api):
    """api with its profile switched on as soon as the engine exists (the row host_replan_tail is a profile row)."""
    create = api.create

    def create_then(*a, **k):
        r = create(*a, **k)
        api.profile_enable(True)
        return r
    api.create = create_then
    return api


def tail_items(api):
    """(passes with a tail, searches finished on the host) so far"""
    ms, launches, items = api.profile()["host_replan_tail"]
    return launches, items


@pytest.fixture()
def hip():
    api = profiled(_lib.new_engine())
    yield api
    api.close()


# ---- the host searcher through the operator seam ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_host_searcher_astar_kats(hip, golden_dir, tag, monkeypatch):
    """TS_ASTAR_HOST=1: ts_astar runs csrc/astar_host.h on a fresh copy of the A* snapshot - the reference's 260 queries per map."""
    monkeypatch.setenv("TS_ASTAR_HOST", "1")
    P.test_hip_astar_kats(hip, golden_dir, tag)
    assert hip.counters().astar_calls == 260      # (counted like the device's own)


@pytest.mark.parametrize("name,tag", [(s, t) for s, t in K.COST_CASES if K.COST_SETS[s]])
def test_host_searcher_astar_cost_kats(hip, golden_dir, name, tag, monkeypatch):
    """... and under the moved cost constants that keep the searches in half units."""
    monkeypatch.setenv("TS_ASTAR_HOST", "1")
    K.run_astar_cost_kats(hip, golden_dir, name, tag)


# ---- forced hand-offs against the reference's traces --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full_96_s8", "default_200_s20", "costs_int_96_s31", "ragged_100x75_s33"])
def test_forced_handoffs_reproduce_reference_trace(hip, name, monkeypatch):
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    P.test_hip_reproduces_reference_trace(hip, name)
    assert tail_items(hip)[1] > 0


@pytest.mark.parametrize("name", ["costs_frac_96_s32", "fov_96_s26"])
def test_feature_is_off_for_fractional_costs_and_field_of_view(hip, name, monkeypatch):
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    P.test_hip_reproduces_reference_trace(hip, name)
    assert tail_items(hip) == (0, 0)


def test_forced_handoffs_with_the_spill_form_and_the_pool_full_retry(monkeypatch):
    """The small-heap build (most searches in the HBM-spill form of the loop, table epochs that wrap) with every search of 32
    expansions handed over: hand-off, replay and spill form together, strict searches that come back empty from the host followed
    by the soft one on the device; then once more with almost no room reserved in the path pool, so that step_decides re-run after
    a hand-off find the pool full and are queued again."""
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    for per_entry in (None, "2"):
        if per_entry:
            monkeypatch.setenv("TS_DEBUG_POOL_PER_ENTRY", per_entry)
        api = profiled(small_engine())
        P.test_hip_reproduces_reference_trace(api, "full_96_s8")
        assert tail_items(api)[1] > 0
        api.close()


# ---- 512^2 through a replanning wave, against the oracle (one oracle run for all) ---------------------------------------------------
class Recorded:
    """The oracle's run, tick by tick, behind the part of the engine interface engine_util.compare reads."""
    def __init__(self, cpu, ticks):
        self.rows, self.t = [], -1
        for _ in range(ticks):
            cpu.step(1)
            self.rows.append({"maps": {w: cpu.map(w) for w in MAPS}, "veh": cpu.vehicles(), "groups": cpu.groups(),
                              "rng": {s: cpu.rng_fingerprint(s) for s in (capi.RNG_GLOBAL, capi.RNG_SCHEDULER)},
                              "sched": cpu.num_scheduled(), "counters": cpu.counters()})

    def step(self, n):
        self.t += n

    def map(self, which):
        return self.rows[self.t]["maps"][which]

    def vehicles(self):
        return self.rows[self.t]["veh"]

    def groups(self):
        return self.rows[self.t]["groups"]

    def rng_fingerprint(self, s):
        return self.rows[self.t]["rng"][s]

    def num_scheduled(self):
        return self.rows[self.t]["sched"]

    def counters(self):
        return self.rows[self.t]["counters"]

    def close(self):
        self.t = -1


@pytest.fixture(scope="module")
def world_512():
    import bench
    from oracle import pyoracle
    tables, routes, _ = bench.make_workload(512, 12_000, 7)
    cpu = pyoracle.load()
    bench.setup(cpu, tables, routes, 7, policy="full")
    rec = Recorded(cpu, TICKS_512)
    cpu.close()
    return tables, routes, rec


def run_512(world, make=None):
    """The HIP engine on the shared 512^2 world against the recorded oracle run; (its counters, its tail row, its checkpoint)."""
    import bench
    tables, routes, rec = world
    h = (make or _lib.new_engine)()
    bench.setup(h, tables, routes, 7, policy="full")
    h.profile_enable(True)
    ch = compare_full(h, rec, TICKS_512, close=False)
    row, blob = tail_items(h), h.checkpoint_save()
    h.close()
    rec.close()
    return ch, row, blob


def test_forced_handoffs_512_and_counters_of_a_switched_off_run(world_512, monkeypatch):
    """State equal to the oracle's with every search of 32 expansions finished on the host - and the searches counted exactly as a
    run with the feature off counts them: the abandoned parts nowhere, the host's searches as the device's would have been."""
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    forced, row, _ = run_512(world_512)
    assert row[1] > 0
    monkeypatch.delenv("TS_TAIL_FORCE")
    monkeypatch.setenv("TS_TAIL", "0")
    off, row_off, _ = run_512(world_512)
    assert row_off == (0, 0)
    assert (forced.astar_calls, forced.astar_expansions, forced.astar_relaxations) == (off.astar_calls, off.astar_expansions, off.astar_relaxations)
    assert off.astar_calls > 5_000


@pytest.mark.parametrize("slots,t_max", [(8, 4), (1, 1)])
def test_the_tail_rule_through_the_idle_counter(world_512, slots, t_max, monkeypatch):
    """No forcing: eight searcher waves of which the last four hand over once the others have found the queue empty; then a single
    wave, which is the last idle one and the tail at once (its hand-offs leave entries in the queue, which the next pass serves)."""
    monkeypatch.setenv("TS_ASTAR_SLOTS", str(slots))
    monkeypatch.setenv("TS_TAIL_MAX", str(t_max))
    monkeypatch.setenv("TS_TAIL_FLOOR", "64")
    ch, row, blob = run_512(world_512)
    assert row[1] > 0 and ch.astar_calls > 5_000
    if slots > t_max:
        # (no pass ends with entries left in the queue here.)  What a checkpoint stores - the queue's counters among it - must not
        # tell how many searches went to the host: byte for byte the checkpoint of the same run with the feature off
        monkeypatch.setenv("TS_TAIL", "0")
        _, row_off, blob_off = run_512(world_512)
        assert row_off == (0, 0) and blob == blob_off


# ---- sharded ranks -----------------------------------------------------------------------------------------------------------------
WORKER = r'''
import numpy as np
from tests.engine_util import engine_for, MAPS
from tests.trace_util import replay_and_compare
api, tr = engine_for(%(trace)r)
api.profile_enable(True)
sr = tdist.ShardedReplans().attach(api)
n = replay_and_compare(api, tr)
assert sr.calls > 0
c = api.counters()
res.update(items=int(api.profile()["host_replan_tail"][2]), astar_calls=int(c.astar_calls))
np.savez(os.path.join(OUTDIR, "state%%d.npz" %% rank), veh=api.vehicles(), groups=api.groups(), **{"map%%d" %% w: api.map(w) for w in MAPS})
api.close()
'''


def test_sharded_ranks_with_forced_handoffs_hold_the_single_rank_state(monkeypatch):
    name = "full_96_s8"
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    res, saved, _ = procs.run_ranks(WORKER, 2, env=dict(os.environ), timeout=600, trace=name)
    assert res[0]["items"] + res[1]["items"] > 0
    one, tr = engine_for(name)
    from tests.trace_util import replay_and_compare
    replay_and_compare(one, tr)
    want = dict(veh=one.vehicles(), groups=one.groups(), **{"map%d" % w: one.map(w) for w in MAPS})
    one.close()
    for r in (0, 1):
        got = saved["state%d.npz" % r]
        for k, v in want.items():
            assert np.array_equal(got[k], v), f"rank {r}: {k}"
