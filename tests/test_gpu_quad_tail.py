"""k_replan_quad's sift-down beyond its LDS share (csrc/astar_quad.h): the three levels a turn fetches ahead and the blocking
levels below them.

The first sift-down step beyond LDS requests the hole's children, grandchildren and great-grandchildren together and walks
the three levels in registers (`quad_sift2_load_both`, `quad_sift2_apply`, `quad_sift1_apply`); a hole that sinks further goes
on two levels per round trip, both loads of a step on their way together (`quad_sift2_load<true>`).  At the shipped 156 LDS
slots the first of these steps starts on level 6 and the blocking ones need a heap beyond 1 022 entries, which small maps
hardly produce.  Two test builds bring both to the 64^2-200^2 reference traces (csrc/Makefile):

* `libtrafficsim_hip_quadtail.so`: 12 slots in LDS, a 64-entry heap.  The step fetched ahead starts on level 2 and meets one
  level (heaps of 8-15 entries), two (16-31) or all three (32-63);
* `libtrafficsim_hip_quadwin.so`: 4 slots in LDS, a 64-entry heap.  The step fetched ahead starts at the root, and the blocking
  step below it (levels 4 and 5) runs for every heap beyond 15 entries whose hole sinks that far.

Every test replays a captured run with every replanning queue on the quads and compares it with the reference tick for tick,
or runs a 512^2 world against the oracle, and reads the quads' counters (ts_debug_quad_stats) to prove that it reached the
steps it is about."""
import json

import pytest

from trafficsimulation_amd import _lib
from trafficsimulation_amd.world import load_trace
from tests.engine_util import compare_full, engine_of, pair_full
from tests.trace_util import replay_and_compare, setup_from_trace, trace_path

pytestmark = pytest.mark.gpu

REASONS = ("window", "heap", "budget", "path_buffer", "policy_bail", "policy_overflow")
# the traces tests/test_gpu_quad_window.py replays
TRACES = ["full_64_s1", "faults_64_s9", "config1_64_s11", "full_96_s8", "startgoal_96_s27", "carve_96_s10", "ring_r1_112_s22",
          "default_200_s20", "rect_64x112_s19", "rect_96x64_s18", "costs_int_96_s31"]


@pytest.fixture(autouse=True)
def quads_on_every_queue(monkeypatch):
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "1")


def check_stats(st):
    assert st["passes"] > 0 and st["jobs"] > 0, st
    assert sum(st[r] for r in REASONS) == st["handbacks"], st
    assert st["handbacks"] <= st["jobs"], st
    return st


def replay(build, name):
    api = engine_of(build)()
    try:
        tr = load_trace(trace_path(name))
        setup_from_trace(api, tr, explicit_paths=False)
        n = replay_and_compare(api, tr)
        assert n == len(tr["veh_off"]) - 1
        assert api.counters().astar_calls == int(tr["astar_calls_spawn"]) + int(tr["astar_per_tick"].sum())
        st = check_stats(api.debug_quad_stats())
        print("QSTATS", json.dumps(dict(build=build, name=name, **st)))
        return st
    finally:
        api.close()


@pytest.mark.parametrize("name", TRACES)
def test_quadtail_reproduces_reference_trace(name):
    """Every tick of a captured run against the reference's recorded state on the quadtail build: heaps of up to 63 entries
    below 12 LDS slots, so the step fetched ahead decides on its third level (heaps beyond 31 entries) in every trace."""
    st = replay("quadtail", name)
    assert st["sift_third_level"] > 0, st
    # (the blocking levels would start at slot 63, which a 64-entry heap never has as a child at a pop)
    assert st["sift_blocking_steps"] == 0, st


@pytest.mark.parametrize("name", ["full_96_s8", "default_200_s20", "rect_64x112_s19"])
def test_quadwin_reaches_the_blocking_levels(name):
    """The quadwin build on three of the traces (windowed on both axes, on one): the step fetched ahead covers levels 1-3, the
    blocking step with its two loads in one round trip levels 4-5."""
    st = replay("quadwin", name)
    assert st["sift_third_level"] > 0 and st["sift_blocking_steps"] > 0, st


@pytest.mark.parametrize("build", ["shipped", "quadtail"])
def test_quad_tail_vs_oracle_512_through_a_replanning_wave(monkeypatch, build):
    """512^2 / 12 000 vehicles through the first replanning wave, state for state every tick.  The shipped build (156 LDS
    slots: the step fetched ahead starts on level 6) reaches its third level with heaps beyond 511 entries - once on this
    workload, which the seed fixes; its blocking levels need more than 1 022 entries and are not asserted here."""
    monkeypatch.setattr(_lib, "new_engine", engine_of(build))
    h, c = pair_full(512, 12_000, 7)
    try:
        compare_full(h, c, 9, close=False)
        st = check_stats(h.debug_quad_stats())
    finally:
        h.close()
        c.close()
    print("QSTATS", json.dumps(dict(build=build, **st)))
    assert st["jobs"] > 5_000, st
    assert st["sift_third_level"] > 0, st
