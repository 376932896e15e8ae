"""Engines and their state, for every test module and rank worker that needs them: an engine set up from a trace or as a
HIP / oracle pair on a synthetic world, the test builds of csrc/Makefile, state snapshots and their comparisons, the refusal
idiom, the facade tests' model builder and example runner.  No pytest here: the rank workers import this module too."""
import ctypes
import json
import os
import sys

import numpy as np

from tests import procs
from tests.trace_util import setup_from_trace, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import _lib
from trafficsimulation_amd.world import build_engine, load_trace

MAPS = (capi.MAP_OCCUPANCY, capi.MAP_STOP, capi.MAP_STUCK)


# ---- engines ------------------------------------------------------------------------------------------------------------------
def engine_for(name, explicit_paths=False, after_create=None):
    """(engine, trace): an engine set up from golden trace `name`.  after_create(api) runs between create and the first
    vehicle's placement (the trip log has to be on by then)."""
    tr = load_trace(trace_path(name))
    api = _lib.new_engine()
    if after_create:
        create = api.create

        def create_then(*a, **k):
            r = create(*a, **k)
            after_create(api)
            return r
        api.create = create_then
    setup_from_trace(api, tr, explicit_paths=explicit_paths)
    return api, tr


def setup_proto(api, tr, defaults=None):
    """Like trace_util.setup_from_trace, with the traffic generator always armed: the reference's model has one under a closed
    population too, and its cached_stats (over the vehicles placed by hand) feed the GAT reward."""
    dta = json.loads(str(tr["dta_params"]))
    build_engine(api, tr, defaults=defaults or tr["defaults_json"], global_state=tr["global_rng_before_day0"],
                 sched_state=tr["sched_rng_initial"])
    api.set_traffic_generator(tr, internal_per_day=dta["P_int"], passing_per_day=dta["P_thr"],
                              start_offset_seconds=dta["start_offset"], service=dta)
    want = np.asarray(tr["global_rng_after_worldgen"], dtype=np.uint64)
    got = api.rng_state(capi.RNG_GLOBAL)
    assert got[1] == int(want[624]) and np.array_equal(got[0], want[:624].astype(np.uint32)), "day-0 trip generation"
    n = len(tr["v_start_xy"])
    api.add_vehicles(tr["v_start_xy"], tr["v_goal_xy"], np.full(n, capi.POP["through"], dtype=np.int32))
    return api


def proto_engine(name, make_engine=None, **over):
    """(engine, trace) of a light-protocol fixture through setup_proto, `over` laid over the fixture's defaults."""
    tr = load_trace(trace_path(name))
    api = (make_engine or _lib.new_engine)()
    setup_proto(api, tr, {**tr["defaults_json"], **over} if over else None)
    return api, tr


def build_lib(build):
    return os.path.join(os.path.dirname(_lib.LIB_PATH), f"libtrafficsim_hip_{build}.so")


def engine_of(build):
    """The constructor of "shipped" or of a test build of csrc/Makefile ("smallheap", "quadwin", "quadtail")."""
    if build == "shipped":
        return _lib.new_engine

    def make():
        if not os.path.exists(build_lib(build)):
            raise _lib.EngineUnavailable(f"{build_lib(build)} is missing - `make -C trafficsimulation_amd/csrc` builds it")
        return capi.CApi(ctypes.CDLL(build_lib(build)), "ts_")
    return make


SMALL = build_lib("smallheap")
small_engine, quadwin_engine = engine_of("smallheap"), engine_of("quadwin")
QUADWIN_WINDOW = 72         # TS_QUAD_WINDOW of the quadwin build
QUAD_REASONS = ("window", "heap", "budget", "path_buffer", "policy_bail", "policy_overflow")


def check_quad_stats(st):
    """What ts_debug_quad_stats must say about any run in which the quads took work: every hand-back has exactly one reason,
    and only a search that was started can be abandoned."""
    assert st["passes"] > 0 and st["jobs"] > 0, st
    assert sum(st[r] for r in QUAD_REASONS) == st["handbacks"], st
    assert st["handbacks"] <= st["jobs"], st
    assert st["window"] + st["heap"] + st["budget"] + st["path_buffer"] <= st["searches"], st
    return st


def pair(size, vehicles, seed, policy):
    """HIP engine and CPU oracle on the same synthetic world / routes / seeds."""
    import bench
    from oracle import pyoracle
    tables, routes, _ = bench.make_workload(size, vehicles, seed)
    hip_api, cpu_api = _lib.new_engine(), pyoracle.load()
    bench.setup(hip_api, tables, routes, seed, extra=policy)
    bench.setup(cpu_api, tables, routes, seed, extra=policy)
    return hip_api, cpu_api


def pair_full(size, vehicles, seed, extra=None, carves=False):
    """HIP engine and CPU oracle under the reference's default policy (bench.py --policy full: QUEUE_ACTUATED lights,
    replanning, contraflow, malfunctions / sideswipes) on the same synthetic world / routes / seeds."""
    import bench
    from oracle import pyoracle
    tables, routes, _ = bench.make_workload(size, vehicles, seed, carves=carves)
    hip_api, cpu_api = _lib.new_engine(), pyoracle.load()
    bench.setup(hip_api, tables, routes, seed, extra=extra, policy="full")
    bench.setup(cpu_api, tables, routes, seed, extra=extra, policy="full")
    return hip_api, cpu_api


# ---- HIP engine against the oracle ---------------------------------------------------------------------------------------------
def same_state(h, c, ctx=""):
    """The one HIP-vs-oracle comparison (any two engines): maps, vehicle rows, groups, both streams, the schedule's length."""
    for which in MAPS:
        assert np.array_equal(h.map(which), c.map(which)), f"{ctx}: map {which}"
    a, b = h.vehicles(), c.vehicles()
    assert a.shape == b.shape, f"{ctx}: live vehicles {a.shape} vs {b.shape}"
    if not np.array_equal(a, b):
        r, col = np.argwhere(a != b)[0]
        raise AssertionError(f"{ctx}: vehicle row {r} field {capi.V_FIELDS[col]}: hip {a[r, col]} cpu {b[r, col]}")
    assert np.array_equal(h.groups(), c.groups()), f"{ctx}: light groups"
    assert h.rng_fingerprint(capi.RNG_GLOBAL) == c.rng_fingerprint(capi.RNG_GLOBAL), f"{ctx}: global RNG"
    assert h.rng_fingerprint(capi.RNG_SCHEDULER) == c.rng_fingerprint(capi.RNG_SCHEDULER), f"{ctx}: scheduler RNG"
    assert h.num_scheduled() == c.num_scheduled(), f"{ctx}: scheduled agents"


COUNTERS = ("stuck", "live_through", "count_completed_through", "total_distance_through", "agent_steps", "elapsed", "step_count")
COUNTERS_FULL = COUNTERS + ("overtaking", "in_stuck_detour", "collisions", "malfunctions", "astar_calls")


def compare(h, c, ticks, every=1, counters=COUNTERS + ("total_duration_through",), astar=False, close=True):
    """Step both `ticks` times, same_state after every `every`-th tick and the last, then the counters; HIP's counters."""
    for t in range(ticks):
        h.step(1)
        c.step(1)
        if (t + 1) % every and t != ticks - 1:
            continue
        same_state(h, c, f"tick {t}")
        if astar:
            assert h.counters().astar_calls == c.counters().astar_calls, f"tick {t}: A* calls"
    ch, cc = h.counters(), c.counters()
    for f in counters:
        assert getattr(ch, f) == getattr(cc, f), f
    if close:
        h.close()
        c.close()
    return ch


def compare_full(h, c, ticks, every=1, close=True):
    """compare() for a pair_full(): the searches counted alike at every compared tick, the full policy's counters."""
    return compare(h, c, ticks, every, COUNTERS_FULL, astar=True, close=close)


# ---- one engine's state, to hold against a twin's ----------------------------------------------------------------------------------
def full_state(api):
    c = api.counters()
    return {"maps": [api.map(w) for w in MAPS + (capi.MAP_RAIN,)], "veh": api.vehicles(), "groups": api.groups(),
            "rng": [api.rng_fingerprint(capi.RNG_GLOBAL), api.rng_fingerprint(capi.RNG_SCHEDULER)],
            "counters": [getattr(c, f) for f, _ in capi.TsCounters._fields_], "blob": api.checkpoint_save()}


def assert_same_state(a, b, ctx):
    for i, (p, q) in enumerate(zip(a["maps"], b["maps"])):
        assert np.array_equal(p, q), f"{ctx}: map {i}"
    assert np.array_equal(a["veh"], b["veh"]), f"{ctx}: vehicle rows"
    assert np.array_equal(a["groups"], b["groups"]), f"{ctx}: groups"
    assert a["rng"] == b["rng"], f"{ctx}: RNG streams"
    assert a["counters"] == b["counters"], f"{ctx}: counters"
    assert a["blob"] == b["blob"], f"{ctx}: checkpoint bytes"


def deep_state(api):
    """The checkpoint tests' snapshot: what full_state's blob holds, read back through the getters (paths, stream states,
    links, service vehicles, rain) so that a difference has a name."""
    s = {"maps": [api.map(w) for w in MAPS + (capi.MAP_RAIN,)],
         "veh": api.vehicles(), "meta": api.vehicle_meta(), "groups": api.groups(), "blocks": api.blocks(),
         "links": [api.group_links(g) for g in range(len(api.groups()))],
         "rng": [api.rng_state(capi.RNG_GLOBAL), api.rng_state(capi.RNG_SCHEDULER)],
         "stats": api.cached_stats(), "svc": api.service_vehicles(), "rain": tuple(getattr(api.rain_info(), f) for f in
                                                                                  ("has_manager", "n_rains", "cooldown", "counter"))}
    s["paths"] = [api.path(i) for i in range(api.num_vehicles())]
    c = api.counters()
    s["counters"] = {f: getattr(c, f) for f, _ in capi.TsCounters._fields_}
    return s


def assert_same_deep_state(x, y, ctx):
    for k in x:
        a, b = x[k], y[k]
        if k in ("maps", "paths"):
            assert len(a) == len(b), f"{ctx}: {k}"
            for i, (p, q) in enumerate(zip(a, b)):
                assert np.array_equal(p, q), f"{ctx}: {k}[{i}]"
        elif k == "rng":
            for (m1, i1), (m2, i2) in zip(a, b):
                assert i1 == i2 and np.array_equal(m1, m2), f"{ctx}: RNG state"
        elif k == "svc":
            for p, q in zip(a, b):
                assert np.array_equal(p, q), f"{ctx}: service vehicles"
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b), f"{ctx}: {k}"
        else:
            assert str(a) == str(b), f"{ctx}: {k}: {a} != {b}"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def refused(code, *calls):
    """Every call raises capi.EngineError with exactly `code`; the exceptions, for the sites that read their text too."""
    raised = []
    for i, call in enumerate(calls):
        try:
            call()
        except capi.EngineError as e:
            assert e.code == code, f"call {i}: refused with {e.code} ({e}), not {code}"
            raised.append(e)
        else:
            raise AssertionError(f"call {i} was not refused (expected EngineError {code})")
    return raised


# ---- the facade tests ---------------------------------------------------------------------------------------------------------------
def city_model(size, seed, traffic=None, **kw):
    """A seed-built square CityModel whose traffic is examples/run_city.py's TRAFFIC with `traffic` laid over it."""
    from trafficsimulation_amd.mesa_api import CityModel
    if os.path.join(procs.ROOT, "examples") not in sys.path:
        sys.path.insert(0, os.path.join(procs.ROOT, "examples"))
    from run_city import TRAFFIC
    return CityModel(size, size, seed=seed, traffic=dict(TRAFFIC, **(traffic or {})), **kw)


def run_example(script, *args):
    """examples/<script> with args, to its end; the completed process."""
    return procs.run([sys.executable, os.path.join(procs.ROOT, "examples", script), *map(str, args)], timeout=300)
