"""The quads' walk back along a found path, two cells per HBM round trip (csrc/astar_quad.h, the QS_FOUND block of
k_replan_quad): with the record of the current cell every lane of the quad requests the record of one of the four cells it can
have come from, and only the one on the path is interpreted.

Every queue goes to the quads (TS_QUAD_MIN=1) on the shipped build and on the two builds with small quad limits, whose 72-cell
table window makes the speculative loads leave it: replays of a trace without a window, of one windowed on one axis (96 x 64: not a
multiple of the window, origins off the tile grid) and of one whose starts lie next to their goals, and the 512^2 / 12 000 wave
against the oracle.  ts_debug_quad_walks counts the walks; the oracle of the 512^2 world runs once for the three builds."""
import pytest

from trafficsimulation_amd.world import load_trace
from tests.engine_util import check_quad_stats, engine_of
from tests.oracle_ticks import run_exact
from tests.trace_util import replay_and_compare, setup_from_trace, trace_path

pytestmark = pytest.mark.gpu

BUILDS = ["shipped", "quadwin", "quadtail"]
TRACES = ["full_64_s1", "rect_96x64_s18", "startgoal_96_s27"]


@pytest.fixture(autouse=True)
def quads_on_every_queue(monkeypatch):
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "1")
    for name in ("TS_QUAD_SLOTS", "TS_ASTAR_SLOTS", "TS_ARENA_CLEAR", "TS_DEBUG_ARENA_BIGDIST", "TS_DEBUG_QUAD_EPOCH_MAX"):
        monkeypatch.delenv(name, raising=False)


def _check_walks(w, short):
    """What any run with a few hundred found paths must show.  `short`: the run has paths of one cell and of two (a trace fixes
    every path the engine finds: full_64_s1 and rect_96x64_s18 hold dozens of each, startgoal_96_s27 - vehicles that start on
    other vehicles' goals - none of one cell)."""
    assert w["walks"] > 0 and w["cells"] >= w["walks"], w
    # a round trip yields two cells, the last one of an odd walk one
    assert 2 * w["round_trips"] == w["cells"] + w["odd"], w
    assert w["round_trips"] < w["cells"], w
    assert 0 < w["odd"] < w["walks"], w          # odd walks end on the first cell of a pair, even ones on the second
    assert w["len1"] <= w["odd"] and w["len2"] <= w["walks"] - w["odd"], w
    if short:
        assert w["len1"] > 0 and w["len2"] > 0, w


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", TRACES)
def test_walks_on_a_replayed_trace(build, name):
    api = engine_of(build)()
    try:
        tr = load_trace(trace_path(name))
        setup_from_trace(api, tr, explicit_paths=False)
        assert replay_and_compare(api, tr) == len(tr["veh_off"]) - 1
        assert api.counters().astar_calls == int(tr["astar_calls_spawn"]) + int(tr["astar_per_tick"].sum())
        check_quad_stats(api.debug_quad_stats())
        w = api.debug_quad_walks()
        print(build, name, w)
        _check_walks(w, short=not name.startswith("startgoal"))
    finally:
        api.close()


@pytest.mark.parametrize("build", BUILDS)
def test_walks_of_a_replanning_wave_against_the_oracle(build):
    """512^2 / 12 000 vehicles through the first replanning wave, state for state every tick."""
    (quads, w), _ = run_exact(engine_of(build), 512, 12_000, 7, 8, lambda h: (h.debug_quad_stats(), h.debug_quad_walks()))
    check_quad_stats(quads)
    print(build, w)
    assert quads["jobs"] > 5_000 and w["walks"] > 1_000, (quads, w)
    _check_walks(w, short=False)
