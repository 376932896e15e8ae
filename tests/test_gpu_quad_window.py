"""k_replan_quad (csrc/astar_quad.h) in the forms the shipped workloads run it in and the other quad tests never reach.

On maps wider or taller than TS_QUAD_WINDOW (1152) the quads' tables are a window centred on the search's start - origins
that go negative near the map's edges, relaxations bounded to the window, a search that meets a candidate outside it handed
back to k_replan - and searches that outgrow the expansion budget, the heap or the path buffer are handed back too.  The
other quad tests run at 768^2 and smaller with the shipped limits, where none of that happens.

`libtrafficsim_hip_quadwin.so` is the engine built with a 72-cell window, a 600-expansion budget, a 64-entry heap of which 4
slots are in LDS, and a 96-cell path buffer (csrc/Makefile): every hand-back reason fires on small maps, and the replays and
oracle comparisons below check that nothing a hand-back leaves behind shows in the results.  Every test reads the quads'
own counters (ts_debug_quad_stats) to prove it reached the paths it is about."""
import json

import pytest

from trafficsimulation_amd import _lib
from trafficsimulation_amd.world import load_trace
from tests.engine_util import QUADWIN_WINDOW, check_quad_stats, compare_full, pair_full, quadwin_engine
from tests.trace_util import replay_and_compare, setup_from_trace, trace_path

pytestmark = pytest.mark.gpu

WINDOW = QUADWIN_WINDOW     # TS_QUAD_WINDOW of the quadwin build
SHIPPED_WINDOW = 1152       # ... and of the shipped one


@pytest.fixture(autouse=True)
def quads_on_every_queue(monkeypatch):
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "1")


# What the quads of the quadwin build do on each trace.  A trace fixes every search the engine makes (the replay must match the
# reference tick for tick), so which of them the quads give back, and why, is fixed by the fixture and the build's limits alone -
# not by the number of quad slots or the order the waves run in.  Anything that moves the window (its origin, its bound), the
# budget, the heap or the path-buffer accounting moves these numbers, even where the results stay exact (a hand-back is replanned
# by k_replan).  A change to the limits in csrc/Makefile has to update them.
PINNED_KEYS = ("jobs", "handbacks", "window", "heap", "budget", "path_buffer", "policy_bail", "policy_overflow", "searches")
PINNED = {
    "full_64_s1": (618, 105, 0, 0, 0, 0, 105, 0, 1219),
    "faults_64_s9": (1117, 77, 0, 3, 44, 0, 30, 0, 2356),
    "config1_64_s11": (21145, 3355, 0, 0, 0, 3, 3352, 0, 42257),
    "full_96_s8": (2938, 2012, 1912, 41, 39, 0, 20, 0, 5737),
    "startgoal_96_s27": (630, 462, 444, 11, 5, 2, 0, 0, 1156),
    "carve_96_s10": (1309, 940, 849, 42, 49, 0, 0, 0, 2522),
    "ring_r1_112_s22": (2060, 1605, 1525, 39, 41, 0, 0, 0, 3733),
    "default_200_s20": (2991, 2771, 2571, 23, 177, 0, 0, 0, 5320),
    "rect_64x112_s19": (5528, 4168, 2706, 0, 1, 0, 1461, 0, 10845),
    "rect_96x64_s18": (2732, 2122, 2080, 6, 4, 0, 32, 0, 5293),
    "costs_int_96_s31": (4369, 2594, 2396, 11, 149, 0, 38, 0, 8565),
}
# (every reason of a search's hand-back occurs on some trace)
assert all(any(v[PINNED_KEYS.index(r)] > 0 for v in PINNED.values()) for r in ("window", "heap", "budget", "path_buffer"))

# (trace, windowed in x, windowed in y) on the quadwin build
TRACES = [("full_64_s1", False, False), ("faults_64_s9", False, False), ("config1_64_s11", False, False),
          ("full_96_s8", True, True), ("startgoal_96_s27", True, True), ("carve_96_s10", True, True),
          ("ring_r1_112_s22", True, True), ("default_200_s20", True, True),
          ("rect_64x112_s19", False, True), ("rect_96x64_s18", True, False),
          # non-default turn / obstacle / road-type penalties and a density window of r = 6 in the quads' half-unit costs
          ("costs_int_96_s31", True, True)]


@pytest.mark.parametrize("name,wx,wy", TRACES)
def test_quadwin_reproduces_reference_trace(name, wx, wy):
    """Every tick of a captured run against the reference's recorded state, every replanning queue on the quads with small
    limits: without a window (64^2: the map fits it), windowed on both axes, and windowed on one axis only."""
    api = quadwin_engine()
    try:
        tr = load_trace(trace_path(name))
        assert (int(tr["width"]) > WINDOW, int(tr["height"]) > WINDOW) == (wx, wy)
        setup_from_trace(api, tr, explicit_paths=False)
        n = replay_and_compare(api, tr)
        assert n == len(tr["veh_off"]) - 1
        assert api.counters().astar_calls == int(tr["astar_calls_spawn"]) + int(tr["astar_per_tick"].sum())
        st = check_quad_stats(api.debug_quad_stats())
        print("QSTATS", json.dumps(dict(name=name, **st)))
        assert {k: st[k] for k in PINNED_KEYS} == dict(zip(PINNED_KEYS, PINNED[name])), st
        if wx or wy:
            assert st["window"] > 0, st
        else:       # (a table that covers the whole map: no neighbour is ever outside it, and g never nears 2^22 here)
            assert st["window"] == 0, st
    finally:
        api.close()


def _oracle_pair_on(monkeypatch, engine, size, vehicles, seed):
    monkeypatch.setattr(_lib, "new_engine", engine)
    return pair_full(size, vehicles, seed)


def _compare_and_stats(h, c, ticks, every=1):
    try:
        compare_full(h, c, ticks, every=every, close=False)
        return check_quad_stats(h.debug_quad_stats())
    finally:
        h.close()
        c.close()


def test_quadwin_vs_oracle_512_through_a_replanning_wave(monkeypatch):
    """512^2 / 12 000 vehicles through the first replanning wave, state for state every tick: thousands of windowed searches,
    handed back for their window, heap and expansion budget (the path buffer's reason occurs on the traces: config1_64_s11,
    startgoal_96_s27)."""
    h, c = _oracle_pair_on(monkeypatch, quadwin_engine, 512, 12_000, 7)
    st = _compare_and_stats(h, c, 9)
    print(st)
    assert st["jobs"] > 5_000
    for r in ("window", "heap", "budget"):
        assert st[r] > 0, (r, st)


def test_quadwin_with_a_full_path_pool(monkeypatch):
    """TS_DEBUG_POOL_PER_ENTRY=2 on the quadwin build: hand-backs and pool-full retries meet in requeue_in_list0 (what k_replan
    did not get to of the hand-backs, then the entries that found the pool full) - state for state against the oracle."""
    monkeypatch.setenv("TS_DEBUG_POOL_PER_ENTRY", "2")
    h, c = _oracle_pair_on(monkeypatch, quadwin_engine, 512, 12_000, 9)
    st = _compare_and_stats(h, c, 8)
    print(st)
    assert st["handbacks"] > 0 and st["window"] > 0


@pytest.mark.parametrize("build", ["shipped", "quadwin"])
def test_quad_table_epochs_wrap(monkeypatch, build):
    """TS_QUAD_SLOTS=16: one quad wave serves every queue, so its sixteen tables see more than 255 searches each and their
    8-bit epochs wrap (the quad clears its table and starts over at epoch 1) inside a replanning wave - against the oracle."""
    monkeypatch.setenv("TS_QUAD_SLOTS", "16")
    engine = quadwin_engine if build == "quadwin" else _lib.new_engine
    h, c = _oracle_pair_on(monkeypatch, engine, 512, 12_000, 7)
    st = _compare_and_stats(h, c, 9)
    print(build, st)
    assert st["searches"] > 16 * 256, st
    assert st["epoch_wraps"] > 0, st


def test_shipped_window_on_a_map_larger_than_it(monkeypatch):
    """The shipped build on the smallest workload wider than its 1152-cell window: 1280^2, through the first replanning wave
    (tick 5) and two ticks beyond it, against the oracle every other tick.  Searches that reach 576 cells from their start
    are handed back."""
    h, c = _oracle_pair_on(monkeypatch, _lib.new_engine, 1280, SHIPPED_VEHICLES, 5)
    st = _compare_and_stats(h, c, 8, every=2)
    print(st)
    assert st["window"] > 0, st


SHIPPED_VEHICLES = 12_000
