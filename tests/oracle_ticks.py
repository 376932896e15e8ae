"""An engine held against the oracle tick by tick, with the oracle's side computed once per world and shared by every test of
the session that asks for it again (engine_util.pair_full / compare_full run it anew for every engine).  No pytest here."""
import numpy as np

import bench
from trafficsimulation_amd import _capi as capi
from tests.engine_util import MAPS

_cache = {}


def _snap(api):
    return {"maps": [api.map(w) for w in MAPS], "veh": api.vehicles(), "groups": api.groups(),
            "rng": (api.rng_fingerprint(capi.RNG_GLOBAL), api.rng_fingerprint(capi.RNG_SCHEDULER)),
            "sched": api.num_scheduled(), "astar_calls": int(api.counters().astar_calls)}


def workload(size, vehicles, seed):
    key = ("w", size, vehicles, seed)
    if key not in _cache:
        _cache[key] = bench.make_workload(size, vehicles, seed)[:2]
    return _cache[key]


def oracle_ticks(size, vehicles, seed, ticks):
    """The oracle's state after each of `ticks` ticks under the default policy (pair_full's set-up); never modified afterwards."""
    key = ("o", size, vehicles, seed, ticks)
    if key not in _cache:
        from oracle import pyoracle
        tables, routes = workload(size, vehicles, seed)
        c = bench.setup(pyoracle.load(), tables, routes, seed, policy="full")
        try:
            snaps = []
            for _ in range(ticks):
                c.step(1)
                snaps.append(_snap(c))
            _cache[key] = snaps
        finally:
            c.close()
    return _cache[key]


def run_exact(engine, size, vehicles, seed, ticks, read):
    """A fresh engine() through `ticks` ticks of that world, same_state's comparisons and the A* calls against the oracle's on
    every tick; returns read(api), taken before the engine is closed, and the oracle's A* calls at the end."""
    want = oracle_ticks(size, vehicles, seed, ticks)
    tables, routes = workload(size, vehicles, seed)
    h = bench.setup(engine(), tables, routes, seed, policy="full")
    try:
        for t in range(ticks):
            h.step(1)
            got, ref = _snap(h), want[t]
            for k, (a, b) in enumerate(zip(got["maps"], ref["maps"])):
                assert np.array_equal(a, b), f"tick {t}: map {k}"
            assert got["veh"].shape == ref["veh"].shape and np.array_equal(got["veh"], ref["veh"]), f"tick {t}: vehicle rows"
            assert np.array_equal(got["groups"], ref["groups"]), f"tick {t}: light groups"
            assert got["rng"] == ref["rng"] and got["sched"] == ref["sched"], f"tick {t}: streams / schedule"
            assert got["astar_calls"] == ref["astar_calls"], f"tick {t}: A* calls"
        return read(h), want[-1]["astar_calls"]
    finally:
        h.close()
