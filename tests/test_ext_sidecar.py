"""What tests/ext_sidecar.py and tests/test_gpu_ext_paths.py decide from the golden fixtures alone - no engine: the ticks of
every mode, the 17-cell condition of the collected-pool mode, the generator mode's T, the light fixtures with searches."""
import numpy as np
import pytest

from tests import ext_sidecar as xs
from tests import observe_util as ou
from tests.ext_sidecar import GENERATOR_PARKED_AT, GENERATOR_SPAWNED, GENERATOR_T, GENERATOR_TRACE, LIGHTS_EXT_FIXTURE, LIGHTS_PROTO_FIXTURE
from tests.trace_util import trace_path
from trafficsimulation_amd.world import load_trace


def test_ticks_and_check_ticks():
    assert xs.check_ticks(80) == [9, 19, 29, 39, 49, 59, 69, 79] and xs.check_ticks(50)[-1] == 49
    assert xs.check_ticks(23) == [9, 19, 22] and xs.check_ticks(1) == [0]
    want = {"full_96_s8": 80, "ragged_100x75_s33": 70, "carfollow_128_s3": 50, "nobatch_full_96_s28": 80, "startgoal_96_s27": 60,
            "config1_64_s11": 60}
    for name, T in want.items():
        assert xs.ticks_of(load_trace(trace_path(name))) == T, name


@pytest.mark.parametrize("name", ["carfollow_128_s3", "full_96_s8"])
def test_a_collection_per_tick_leaves_path_cur_inside_a_word(name):
    """At some check tick of the gc mode a live vehicle has driven at least 17 cells since its path was last written: a
    collection has dropped the path's first word (16 steps) and left path_cur = cur & 15 behind."""
    tr = load_trace(trace_path(name))
    far = xs.since_written(tr, xs.ticks_of(tr))
    assert sorted(far) == xs.check_ticks(xs.ticks_of(tr))
    assert max(far.values()) >= xs.GC_MIN_CELLS, far
    if name == "carfollow_128_s3":           # no search ever runs: since the path was written = steps_traveled
        assert int(np.sum(tr["astar_per_tick"])) == 0
        for t, cells in far.items():
            assert cells == int(ou.rows_at(tr, t)[:, ou.V["steps_traveled"]].max())
    else:
        assert int(np.sum(tr["astar_per_tick"])) > 0


def test_generator_ticks():
    tr = load_trace(trace_path(GENERATOR_TRACE))
    assert xs.generator_ticks(tr) == (GENERATOR_T, GENERATOR_SPAWNED, GENERATOR_PARKED_AT) == (260, 102, 225)
    n0 = len(tr["v_start_xy"])
    assert xs.spawned_by(tr, GENERATOR_T - 1) > 2 * n0 >= xs.spawned_by(tr, GENERATOR_T - 11), "T is not the first such multiple of 10"
    assert GENERATOR_T <= ou.n_ticks(tr)
    # the per-vehicle device arrays start with room for 1024 vehicles and double from there (ensure_vehicle_capacity in
    # csrc/host_state.h, called with 1024 by ts_create): no golden trace spawns that many, so the generator mode grows the
    # vehicle count past every host-side length taken before the run, not the device arrays
    assert xs.spawned_by(tr, ou.n_ticks(tr) - 1) < 1024


def test_light_fixtures_with_searches():
    assert xs.light_fixtures_with_searches(["lights_ext_64_s45", "lights_ext_96_s42", "lights_ext_stuck_96_s43"]) == [LIGHTS_EXT_FIXTURE]
    assert xs.light_fixtures_with_searches(["lights_gat_64_s45", "lights_gat_96_s49"]) == [LIGHTS_PROTO_FIXTURE]
    assert "lp_q" in load_trace(trace_path(LIGHTS_PROTO_FIXTURE)), "the GAT fixture is not driven through act_q"


def test_bundles_compare_byte_for_byte():
    a = xs.flatten([{"x": np.arange(4, dtype=np.int32)}, {"x": np.zeros(2, dtype=np.uint8)}])
    assert sorted(a) == ["000/x", "001/x"]
    xs.assert_same_bundles(a, {k: v.copy() for k, v in a.items()}, "copy")
    for other in ({**a, "001/x": np.zeros(2, dtype=np.int8)}, {**a, "001/x": np.ones(2, dtype=np.uint8)}, {"000/x": a["000/x"]}):
        with pytest.raises(AssertionError):
            xs.assert_same_bundles(a, other, "changed")
