"""The device extensions (observation, trip log, external light control, the A2C / GAT-DQN protocols, renderer, route demand,
cost fields, routes along a cost field, select-link) on the engine's other paths: the quad searcher, its windowed build, the
small-heap build, the host tail of a replanning pass, a tight and a collected path pool, PATHFINDING_BATCHING=False, the
traffic generator, two sharded ranks.

1. The mode matrix.  Every mode replays a golden trace tick by tick against the trace with tests/ext_sidecar.py switched on:
   after every 10th tick and after the last, Sidecar.check asserts the in-mode rules and returns a bundle of every output;
   the bundles of a mode equal those of the default mode of the same trace byte for byte.  Every mode asserts that its path
   was taken.
2. External light control and the protocols: two sharded ranks replay a lights_ext and a GAT fixture in which searches run
   (every recorded array and the global-stream fingerprint, on both ranks); the numpy-model hunt's ungated cases on the quad
   searcher, on a pool collected every tick and with PATHFINDING_BATCHING=False."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import demand_expect as de
from tests import ext_sidecar as xs
from tests import lights_ext_expect as lx
from tests import procs
from tests import test_gpu_lights_ext as LE
from tests.engine_util import QUADWIN_WINDOW, SMALL, check_quad_stats, quadwin_engine, refused, small_engine
from tests.ext_sidecar import GENERATOR_PARKED_AT, GENERATOR_SPAWNED, GENERATOR_T, GENERATOR_TRACE, LIGHTS_EXT_FIXTURE, LIGHTS_PROTO_FIXTURE
from tests.test_gpu_replan_tail import profiled
from tests.trace_util import setup_from_trace, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace

pytestmark = pytest.mark.gpu

SWITCHES = ("TS_QUAD", "TS_QUAD_MIN", "TS_DEBUG_POOL_PER_ENTRY", "TS_DEBUG_POOL_GC", "TS_TAIL", "TS_TAIL_FORCE", "TS_TAIL_MAX",
            "TS_TAIL_FLOOR", "TS_ASTAR_HOST")
EXPLICIT = {"carfollow_128_s3"}                       # replayed on its recorded spawn-time paths: the exact fixture expectation
SHARDED_TRACES = ["full_96_s8", "startgoal_96_s27"]


def ticks_for(name, tr):
    return GENERATOR_T if name == GENERATOR_TRACE else xs.ticks_of(tr)


def run_mode(name, engine=new_engine, profile=True):
    """One replay of trace `name` with the sidecar on: (api, trace, sidecar, flattened bundles).  The caller closes api."""
    tr = load_trace(trace_path(name))
    api = engine()
    setup_from_trace(api, tr, explicit_paths=name in EXPLICIT)
    if profile:
        api.profile_enable(True)
    sc = xs.Sidecar(api, tr, fixture_paths=name in EXPLICIT)
    flat = xs.flatten(xs.run_trace(api, tr, ticks_for(name, tr), sc))
    return api, tr, sc, flat


def analyses_of(stats):
    """The figures of the cost-field, route and select-link sections of a sidecar's (or a rank's) stats: all positive."""
    row = {k: int(stats[k]) for k in ("fields_compared", "routes_compared", "selectlink_computes")}
    assert min(row.values()) > 0, row
    return row


def report(mode, name, api, sc, **more):
    gc = api.profile().get("pool_gc", (0, 0, 0))
    row = dict(mode=mode, trace=name, check_ticks=sc.stats["checks"], paths_compared=sc.stats["paths"], pool_gc=int(gc[1]),
               astar_calls=int(api.counters().astar_calls), **analyses_of(sc.stats), **more)
    print("EXT_PATHS " + json.dumps(row))
    return row


def tailed_engine():
    """The shipped build with its profile on from create: the row host_replan_tail counts every search finished on the host."""
    return profiled(new_engine())


def tail_items(api):
    return int(api.profile()["host_replan_tail"][2])


def trace_calls(tr, T):
    return int(tr["astar_calls_spawn"]) + int(np.sum(tr["astar_per_tick"][:T]))


@pytest.fixture(scope="module")
def default_mode():
    """name -> (api, trace, sidecar, bundles) of the shipped build on one GPU with no switch set; once per trace."""
    cache = {}

    def get(name):
        if name not in cache:
            assert not [k for k in SWITCHES if k in os.environ], "the default mode runs with no engine switch set"
            cache[name] = run_mode(name, profile=False)
        return cache[name]
    yield get
    for api, *_ in cache.values():
        api.close()


# ---- 1. the mode matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full_96_s8", "ragged_100x75_s33", "carfollow_128_s3", "startgoal_96_s27"])
def test_default(default_mode, name):
    api, tr, sc, flat = default_mode(name)
    T = ticks_for(name, tr)
    assert sc.stats["checks"] == len(xs.check_ticks(T)) and sc.stats["paths"] > 0 and flat
    assert api.counters().astar_calls == (0 if name in EXPLICIT else trace_calls(tr, T))
    assert any(k.endswith("frame_routes") and (v[..., :3] == np.asarray(xs.ROUTE_RGBA[:3])).all(axis=2).any() for k, v in flat.items())
    assert sc.leaver is not None, "no listed route belongs to a vehicle that leaves during the run"
    print("EXT_PATHS " + json.dumps(dict(mode="default", trace=name, check_ticks=sc.stats["checks"], paths_compared=sc.stats["paths"],
                                          **analyses_of(sc.stats))))


@pytest.mark.parametrize("name", ["full_96_s8", "ragged_100x75_s33"])
def test_quads(default_mode, monkeypatch, name):
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "1")
    api, tr, sc, flat = run_mode(name)
    jobs = api.debug_quad_stats()["jobs"]
    report("quads", name, api, sc, quad_jobs=jobs)
    assert jobs > 0
    xs.assert_same_bundles(flat, want, f"quads, {name}")
    api.close()


@pytest.mark.parametrize("name", ["full_96_s8", "ragged_100x75_s33"])
def test_quadwin(default_mode, monkeypatch, name):
    """The quadwin build: the quads' tables are a window of 72 cells on maps that are larger both ways, so searches that
    leave it are handed back to k_replan (reason `window`) beside every extension."""
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "1")
    api, tr, sc, flat = run_mode(name, engine=quadwin_engine)
    assert min(int(tr["width"]), int(tr["height"])) > QUADWIN_WINDOW
    st = check_quad_stats(api.debug_quad_stats())
    report("quadwin", name, api, sc, quad_jobs=st["jobs"], window=st["window"])
    assert st["window"] > 0
    xs.assert_same_bundles(flat, want, f"quadwin, {name}")
    api.close()


@pytest.mark.parametrize("name", ["full_96_s8", "ragged_100x75_s33"])
def test_host_tail(default_mode, monkeypatch, name):
    """TS_TAIL_FORCE=32: every search of 32 expansions is abandoned on the device, finished on a host thread from a host copy
    of the snapshot, and its step_decide is re-run - the trip log, the ENTER planes, the route layer and every reader of the
    pool on what that second attempt wrote."""
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    api, tr, sc, flat = run_mode(name, engine=tailed_engine, profile=False)
    row = report("host_tail", name, api, sc, host_replan_tail=tail_items(api))
    assert row["host_replan_tail"] > 0
    assert row["astar_calls"] == trace_calls(tr, xs.ticks_of(tr))
    xs.assert_same_bundles(flat, want, f"host_tail, {name}")
    api.close()


def test_host_tail_gc(default_mode, monkeypatch):
    """... with a collection at the top of every tick and in front of every replan: a re-run step_decide writes into a pool
    that has just been collected."""
    name = "full_96_s8"
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_TAIL_FORCE", "32")
    monkeypatch.setenv("TS_DEBUG_POOL_GC", "1")
    api, tr, sc, flat = run_mode(name, engine=tailed_engine, profile=False)
    row = report("host_tail_gc", name, api, sc, host_replan_tail=tail_items(api))
    assert row["host_replan_tail"] > 0 and row["pool_gc"] >= xs.ticks_of(tr), row
    assert row["astar_calls"] == trace_calls(tr, xs.ticks_of(tr))
    xs.assert_same_bundles(flat, want, "host_tail_gc")
    api.close()


def test_smallheap(default_mode):
    name = "full_96_s8"
    want = default_mode(name)[3]
    api, tr, sc, flat = run_mode(name, engine=small_engine)
    report("smallheap", name, api, sc)
    assert isinstance(api.lib, ctypes.CDLL) and os.path.samefile(api.lib._name, SMALL)
    assert api.counters().astar_calls == trace_calls(tr, xs.ticks_of(tr))
    xs.assert_same_bundles(flat, want, "smallheap")
    api.close()


def test_tight_pool(default_mode, monkeypatch):
    name = "full_96_s8"
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_DEBUG_POOL_PER_ENTRY", "2")
    api, tr, sc, flat = run_mode(name)
    report("tight_pool", name, api, sc)
    assert api.counters().astar_calls == trace_calls(tr, xs.ticks_of(tr))
    xs.assert_same_bundles(flat, want, "tight_pool")
    api.close()


@pytest.mark.parametrize("name", ["carfollow_128_s3", "full_96_s8"])
def test_gc(default_mode, monkeypatch, name):
    """A collection at the top of every tick and in front of every replan (TS_DEBUG_POOL_GC): every reader of
    (path_off, path_cur, path_len) on paths that k_pool_gc has moved, shortened and left with path_cur inside a word."""
    want = default_mode(name)[3]
    monkeypatch.setenv("TS_DEBUG_POOL_GC", "1")
    api, tr, sc, flat = run_mode(name)
    T = xs.ticks_of(tr)
    row = report("gc", name, api, sc)
    assert row["pool_gc"] >= T, f"{row['pool_gc']} collections in {T} ticks"
    far = xs.since_written(tr, T)
    assert max(far.values()) >= xs.GC_MIN_CELLS, "no checked path has lost a word to a collection"
    xs.assert_same_bundles(flat, want, f"gc, {name}")
    api.close()


def test_nobatch():
    """PATHFINDING_BATCHING=False is the trace's own setting, so this run is the default mode of its trace: the in-mode rules,
    on paths that the one-vehicle-at-a-time decide wrote."""
    name = "nobatch_full_96_s28"
    api, tr, sc, flat = run_mode(name)
    assert tr["defaults_json"]["PATHFINDING_BATCHING"] is False
    row = report("nobatch", name, api, sc)
    assert row["astar_calls"] > 0 and row["astar_calls"] == trace_calls(tr, xs.ticks_of(tr))
    api.close()


def test_generator(default_mode):
    """The armed traffic generator and service vehicles (spawns inside ticks, parked and servicing vehicles), then route demand
    with a host mask after the vehicle count has more than doubled."""
    name = GENERATOR_TRACE
    api, tr, sc, flat = default_mode(name)
    n0, n = len(tr["v_start_xy"]), api.num_spawned()
    assert xs.generator_ticks(tr) == (GENERATOR_T, GENERATOR_SPAWNED, GENERATOR_PARKED_AT)
    assert n >= GENERATOR_SPAWNED > 2 * n0 and sc.stats["checks"] == GENERATOR_T // 10
    assert api.counters().astar_calls > 0
    print("EXT_PATHS " + json.dumps(dict(mode="generator", trace=name, check_ticks=sc.stats["checks"], paths_compared=sc.stats["paths"],
                                          spawned=n, astar_calls=int(api.counters().astar_calls), **analyses_of(sc.stats))))
    # select-link while n_vehicles_total grows: the per-vehicle arrays were allocated again between computes ...
    grown = sc.stats["n_spawned"]
    assert len(grown) == sc.stats["checks"] and len(set(grown)) >= 3 and grown[0] <= 50 < grown[-1] == n, grown
    # ... and hold, by spawn index, vehicles the generator placed beside the zeros of vehicles that have left (the engine's
    # arrays are these, compared at the last check tick)
    last = sc.last_walk
    alive = set(int(v) for v in last["spawn"])
    assert len(last["mask"]) == n and any(v >= n0 and last["mask"][v] != 0 for v in alive), "no vehicle of the generator crosses a gate"
    gone = [v for v in range(n0) if v not in alive]
    assert gone and all((int(last["mask"][v]), int(last["crossings"][v]), int(last["first_step"][v]), int(last["first_gate"][v])) == (0, 0, -1, -1)
                        for v in gone), "a departed vehicle's spawn index does not read 0 / 0 / -1 / -1"
    H, W = int(tr["height"]), int(tr["width"])
    veh, spawn = de.engine_vehicles(api)
    mask = (np.arange(n) % 2 == 0).astype(np.uint8)
    picked = [v for v, s in zip(veh, spawn) if mask[s]]
    assert 0 < len(picked) < len(veh) and any(s >= n0 and mask[s] for s in spawn)
    q = (4, 16, 1)
    info = api.demand_compute(*q, select=mask)
    planes = xs.read_planes(api, 4)
    assert np.array_equal(planes, de.planes(H, W, picked, 4, 16, True))
    assert info["selected"] and info["vehicles"] == len(picked) and info["steps"] == de.remaining_steps(picked) > 0
    refused(capi.TS_E_INVALID, lambda: api.demand_compute(*q, select=np.ones(n0, dtype=np.uint8)))     # the length the mask had before the generator's spawns
    assert api.demand_info() == info and np.array_equal(xs.read_planes(api, 4), planes), "the refused compute touched the result"


SHARDED_WORKER = r'''
import numpy as np
import torch
from tests import ext_sidecar as xs
from tests.engine_util import engine_for
for name in %(traces)r:
    api, tr = engine_for(name, after_create=lambda a: a.profile_enable(True))      # (the profile on from create, as tailed_engine)
    sr = tdist.ShardedReplans(device=torch.device("cuda", 0), device_direct=True).attach(api)
    sc = xs.Sidecar(api, tr)
    flat = xs.flatten(xs.run_trace(api, tr, xs.ticks_of(tr), sc))      # (every rank runs the in-mode rules on imported paths)
    np.savez(os.path.join(OUTDIR, "bundles_%%s_%%d.npz" %% (name, rank)), **flat)
    res[name] = dict(exchanges=sr.calls, bytes=sr.bytes_sent, check_ticks=sc.stats["checks"], paths_compared=sc.stats["paths"],
                     pool_gc=int(api.profile()["pool_gc"][1]), astar_calls=int(api.counters().astar_calls),
                     host_replan_tail=int(api.profile()["host_replan_tail"][2]),
                     **{k: sc.stats[k] for k in ("fields_compared", "routes_compared", "selectlink_computes")})
    api.close()
'''
SHARDED_LEGS = {"plain": {}, "gc": {"TS_DEBUG_POOL_GC": "1"}, "tail": {"TS_TAIL_FORCE": "32"}}


@pytest.mark.parametrize("gc", [False, True, "tail"])
def test_sharded2(default_mode, gc):
    """Two ranks, records exchanged between device buffers: each rank plans half of every queue and imports the other half
    (k_replan_import: re-allocated words, path_cur = 0); with gc the pool is also collected at every tick and replan; with
    "tail" each rank finishes the searches of 32 expansions of its half on host threads (TS_TAIL_FORCE).  On every rank the
    sidecar walks, routes and counts over paths of which half were imported."""
    leg = {False: "plain", True: "gc"}.get(gc, gc)
    traces = SHARDED_TRACES if leg == "plain" else ["full_96_s8"]
    ranks, saved, _ = procs.run_ranks(SHARDED_WORKER, 2, env=dict(os.environ, **SHARDED_LEGS[leg]), timeout=600, traces=traces)
    for name in traces:
        want = default_mode(name)[3]
        tr = default_mode(name)[1]
        for r in range(2):
            row = ranks[r][name]
            print("EXT_PATHS " + json.dumps(dict(mode="sharded2" if leg == "plain" else "sharded2_" + leg, trace=name, rank=r, **row)))
            assert row["exchanges"] > 0 and row["bytes"] > 0, f"rank {r} planned or exchanged nothing on {name}"
            analyses_of(row)
            assert (row["pool_gc"] >= xs.ticks_of(tr)) if leg == "gc" else True
            assert (row["host_replan_tail"] > 0) if leg == "tail" else True, f"rank {r} finished no search on the host"
            xs.assert_same_bundles(saved[f"bundles_{name}_{r}.npz"], want, f"rank {r} of 2, {name}")
        assert ranks[0][name]["astar_calls"] == ranks[1][name]["astar_calls"] == trace_calls(tr, xs.ticks_of(tr))


# ---- 2. external light control and the protocols on the other paths -------------------------------------------------------
LIGHTS_WORKER = r'''
import torch
from tests import test_gpu_lights_ext as LE, test_gpu_lights_proto as LP
for mod, name in ((LE, %(ext)r), (LP, %(proto)r)):
    made = []
    plain = mod.new_engine

    def sharded_engine():
        """An engine that turns to sharded replans as soon as its vehicles are placed (where the sharded traces attach)."""
        api = plain()
        place = api.add_vehicles

        def add_vehicles(*a, **k):
            out = place(*a, **k)
            made.append((api, tdist.ShardedReplans(device=torch.device("cuda", 0), device_direct=True).attach(api)))
            return out
        api.add_vehicles = add_vehicles
        close = api.close
        api.close = lambda: (made.append(int(api.counters().astar_calls)), close())[1]
        return api
    mod.new_engine = sharded_engine
    # the single-engine replay itself, every assertion of it: each recorded array bit for bit and, inside replay_and_compare,
    # the global and scheduler stream fingerprints of every tick
    mod.test_replays_the_reference_controller(name)
    mod.new_engine = plain
    (api, sr), calls = made
    res[name] = dict(exchanges=sr.calls, bytes=sr.bytes_sent, astar_calls=calls)
'''


def test_light_control_fixtures_on_two_sharded_ranks():
    chosen = xs.light_fixtures_with_searches(lx.FIXTURES), xs.light_fixtures_with_searches(["lights_gat_64_s45", "lights_gat_96_s49"])
    assert chosen == ([LIGHTS_EXT_FIXTURE], [LIGHTS_PROTO_FIXTURE])
    ranks, _, _ = procs.run_ranks(LIGHTS_WORKER, 2, timeout=600, ext=LIGHTS_EXT_FIXTURE, proto=LIGHTS_PROTO_FIXTURE)
    for name in (LIGHTS_EXT_FIXTURE, LIGHTS_PROTO_FIXTURE):
        tr = load_trace(trace_path(name))
        for r in range(2):
            row = ranks[r][name]
            print("EXT_PATHS " + json.dumps(dict(mode="lights_sharded2", trace=name, rank=r, **row)))
            assert row["exchanges"] > 0 and row["bytes"] > 0, f"rank {r} planned or exchanged nothing on {name}"
            assert row["astar_calls"] == int(tr["astar_calls_spawn"]) + int(np.sum(tr["astar_per_tick"]))


@pytest.mark.parametrize("case", [1, 3])
@pytest.mark.parametrize("path", ["quads", "gc", "nobatch"])
def test_light_control_hunt_on_other_paths(path, case, monkeypatch):
    """test_gpu_lights_ext.test_hunt_against_the_numpy_model, its ungated cases, as it stands: lx.phase_a / lx.phase_b need
    only the engine's maps, so they hold on any path."""
    if path == "quads":
        monkeypatch.setenv("TS_QUAD", "1")
        monkeypatch.setenv("TS_QUAD_MIN", "1")
    elif path == "gc":
        monkeypatch.setenv("TS_DEBUG_POOL_GC", "1")
    else:
        build = LE.build_engine
        monkeypatch.setattr(LE, "build_engine", lambda api, tables, defaults, **k: build(api, tables, defaults={**defaults, "PATHFINDING_BATCHING": False}, **k))
    seen = {}

    def engine():
        api = new_engine()
        step, close = api.step, api.close

        def first_step(n=1):
            if "before" not in seen:           # (the searches so far are the spawn-time planner's)
                seen["before"] = int(api.counters().astar_calls)
                api.profile_enable(True)
            return step(n)

        def last(*a):
            seen["after"], seen["gc"] = int(api.counters().astar_calls), int(api.profile()["pool_gc"][1])
            seen["quad_jobs"], seen["ticks"] = api.debug_quad_stats()["jobs"], int(api.counters().step_count)
            return close(*a)
        api.step, api.close = first_step, last
        return api
    monkeypatch.setattr(LE, "new_engine", engine)
    LE.test_hunt_against_the_numpy_model(case, monkeypatch)
    print("EXT_PATHS " + json.dumps(dict(mode="hunt_" + path, case=case, **seen)))
    assert seen["after"] > seen["before"], "no search ran inside the ticks of the hunt"
    if path == "quads":      # (case 3 has fractional road-type penalties: searches in doubles, which the quads leave to k_replan)
        assert (seen["quad_jobs"] > 0) == (case % 3 != 0)
    if path == "gc":
        assert seen["gc"] >= seen["ticks"]
