"""tests/triplog_util.py against the golden traces alone (no GPU): the expectation the GPU tests hold the trip log to is itself
consistent with what the reference recorded."""
import numpy as np
import pytest

from tests import observe_util as ou
from tests import triplog_util as tu
from tests.trace_util import CLOSED_TRACES, DEFAULT_TRACES, DESPAWN_TRACES, DTA_TRACES, RAGGED_TRACES, trace_path
from trafficsimulation_amd.world import load_trace

# every closed population: placed before tick 0, population `through`
CLOSED = CLOSED_TRACES + DESPAWN_TRACES + RAGGED_TRACES
GENERATOR = DTA_TRACES + DEFAULT_TRACES


@pytest.fixture(scope="module")
def traces():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = load_trace(trace_path(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", CLOSED + GENERATOR)
def test_vanished_vehicles_are_the_completed_and_the_errored(traces, name):
    tr = traces(name)
    total = 0
    for t in range(ou.n_ticks(tr)):
        gone = tu.vanished(tr, t)
        want = tu.reason_counts(tr, t)
        assert len(gone) == want[tu.ARRIVED] + want[tu.DESPAWNED], f"tick {t}: {len(gone)} vanished, counters say {want}"
        assert (np.diff(gone) > 0).all()
        total += len(gone)
    assert total == len(tu.sequence(tr)) > 0


def test_removal_counts_of_the_fixtures(traces):
    assert len(tu.sequence(traces("carfollow_96_s2"))) == 9
    assert len(tu.sequence(traces("despawn_96_s25"))) == 211
    assert len(tu.sequence(traces("carve_96_s10"))) == 67
    # trips that end where they start leave through the decide phase, in the very first tick
    assert (tu.sequence(traces("startgoal_96_s27"))[:, 0] == 0).sum() == 12
    # ... and _despawn_check's share of despawn_96_s25
    tr = traces("despawn_96_s25")
    assert sum(tu.reason_counts(tr, t)[tu.DESPAWNED] for t in range(ou.n_ticks(tr))) == 98


@pytest.mark.parametrize("name", CLOSED)
def test_closed_traces_know_goal_and_distance_bounds(traces, name):
    tr = traces(name)
    seq = tu.sequence(tr)
    assert seq[:, 1].max() < len(tr["v_start_xy"]) == len(tr["v_goal_xy"])
    assert len(np.unique(seq[:, 1])) == len(seq), "a vehicle leaves once"
    mm = ou.max_move(tr)
    for t in range(ou.n_ticks(tr)):
        gone = tu.vanished(tr, t)
        want = tu.reason_counts(tr, t)
        if len(gone) and want[tu.DESPAWNED] == 0:
            # all arrived: the distance the counters gained lies between the last-seen sums
            lo = sum(tu.last_seen_steps(tr, t, int(i)) for i in gone)
            assert lo <= tu.arrived_distance(tr, t) <= lo + mm * len(gone), f"tick {t}"
