"""The table arena k_replan and the quads share changes hands without a clear (csrc/replan_host.h, csrc/arena_epochs.h).

A 768^2 world with TS_QUAD_SLOTS=1024 (the quads' tables alias k_replan's behind the side waves' slots, as in
test_hip_quad_and_wave_searchers_share_the_table_arena) and TS_ASTAR_SLOTS=1400 (350 side slots; the 1 050 tables of 155 262 road
cells behind them hold 544 quad tables of 768^2 cells, more than half of what was asked for - fewer k_replan slots would not),
12 000 vehicles, thirteen ticks: the oracle makes 17 434 and 13 002 searches on the two replanning waves (ticks 5 and 11: 8 700
and 6 600 queue entries) and 2 240 / 1 125 / 819 / 585 / 672 / 2 838 on the ticks after them (two searches per entry), so with
TS_QUAD_MIN=3000 the two waves go to the quads and every tick between to k_replan, whose queues right after a wave are longer
than its 350 side slots: the arena goes to the quads twice and back twice.  Every run is
held against the oracle state for state on every tick; the oracle runs once for all of them."""
import pytest

from trafficsimulation_amd import _lib
from tests.engine_util import small_engine
from tests.oracle_ticks import run_exact

pytestmark = pytest.mark.gpu

SIZE, VEHICLES, SEED, TICKS = 768, 12_000, 3, 13


def _run_exact(engine, size, vehicles, seed, ticks):
    """(arena info, quad counters, the oracle's A* calls) of a fresh engine that matched the oracle on every tick"""
    (info, quads), calls = run_exact(engine, size, vehicles, seed, ticks, lambda h: (h.debug_arena_info(), h.debug_quad_stats()))
    return info, quads, calls


@pytest.fixture(autouse=True)
def shared_arena(monkeypatch):
    monkeypatch.setenv("TS_QUAD", "1")
    monkeypatch.setenv("TS_QUAD_MIN", "3000")
    monkeypatch.setenv("TS_QUAD_SLOTS", "1024")
    monkeypatch.setenv("TS_ASTAR_SLOTS", "1400")
    for name in ("TS_ARENA_CLEAR", "TS_DEBUG_ARENA_BIGDIST", "TS_DEBUG_QUAD_EPOCH_MAX"):
        monkeypatch.delenv(name, raising=False)


def _handed_over_twice(info, quads):
    assert info["arena_shared"] == 1, info
    assert info["to_quads"] >= 2 and info["to_waves"] >= 2, info
    assert quads["passes"] >= 2 and quads["jobs"] >= 2 * 3000, quads


def test_the_arena_changes_hands_without_a_clear():
    info, quads, calls = _run_exact(_lib.new_engine, SIZE, VEHICLES, SEED, TICKS)
    print(info, quads)
    _handed_over_twice(info, quads)
    assert info["clears"] == 0 and info["big_dist_flag"] == 0 and info["big_dist_seen"] == 0, info
    assert calls > 35_000


def test_quad_epochs_wrap_while_the_arena_is_shared(monkeypatch):
    """TS_DEBUG_QUAD_EPOCH_MAX=3: a quad's table is cleared by its wave after every third search, with k_replan's records of the
    ticks between lying in it."""
    monkeypatch.setenv("TS_DEBUG_QUAD_EPOCH_MAX", "3")
    info, quads, _ = _run_exact(_lib.new_engine, SIZE, VEHICLES, SEED, TICKS)
    print(info, quads)
    _handed_over_twice(info, quads)
    assert info["clears"] == 0, info
    assert quads["epoch_wraps"] > 0 and quads["epoch_wraps"] >= quads["searches"] // 3 - 1024, quads


def test_a_big_dist_brings_the_clear_back(monkeypatch):
    """TS_DEBUG_ARENA_BIGDIST=64: nearly every search of k_replan stores a dist of 64 or more, raises the flag, and the next
    hand-over to the quads clears their tables as every hand-over used to."""
    monkeypatch.setenv("TS_DEBUG_ARENA_BIGDIST", "64")
    info, quads, _ = _run_exact(_lib.new_engine, SIZE, VEHICLES, SEED, TICKS)
    print(info, quads)
    _handed_over_twice(info, quads)
    assert info["big_dist_seen"] >= 1 and info["clears"] >= 1, info
    assert info["big_dist_flag"] == 1, info      # (raised again by the ticks after the last wave)


def test_clearing_at_every_hand_over_still_works(monkeypatch):
    monkeypatch.setenv("TS_ARENA_CLEAR", "1")
    info, quads, _ = _run_exact(_lib.new_engine, SIZE, VEHICLES, SEED, TICKS)
    print(info, quads)
    _handed_over_twice(info, quads)
    assert info["clears"] == info["to_quads"] + info["to_waves"], info


def test_k_replan_stamps_wrap_inside_their_range(monkeypatch):
    """The small-heap build (a table's stamps wrap after 300 searches) on four searcher slots through one replanning wave of a
    384^2 world: every slot's table is cleared by its wave several times, and the stamps start over inside k_replan's range."""
    monkeypatch.setenv("TS_ASTAR_SLOTS", "4")
    monkeypatch.delenv("TS_QUAD_MIN")
    monkeypatch.delenv("TS_QUAD_SLOTS")
    info, _, calls = _run_exact(small_engine, 384, 3_000, 5, 7)
    print(info, calls)
    assert calls > 4 * 300 * 2, calls      # (more than two wraps per slot however the queue was dealt out)
    assert info["clears"] == 0, info
