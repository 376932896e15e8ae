"""The numpy model of the external light control (tests/lights_ext_expect.py) against the reference: both fixtures of
tests/golden/make_golden_lights.py, from the fixtures' own maps, every tick, float32 bit for bit."""
import numpy as np
import pytest

from tests import lights_ext_expect as lx
from tests.trace_util import trace_path

FIXTURES = ["lights_ext_64_s45", "lights_ext_96_s42", "lights_ext_stuck_96_s43"]


def unpack(bits, h, w):
    return np.unpackbits(bits)[:h * w].reshape(h, w).astype(np.int8)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reproduces_the_reference(name):
    tr = dict(np.load(trace_path(name)))
    H, W, dim, mg = int(tr["height"]), int(tr["width"]), int(tr["rl_dim"]), int(tr["rl_min_green"])
    G = tr["rl_state"].shape[1]
    ctrl = lx.Ctrl(G)
    static = lx.static_features(tr)
    for t in range(len(tr["rl_state"])):
        if t:   # what the tick in between did to the groups
            ctrl.current, ctrl.pending = tr["grp_rows"][t - 1][:, 0].copy(), tr["grp_rows"][t - 1][:, 1].copy()
            ctrl.repop |= ctrl.current >= 0
        assert np.array_equal(ctrl.pending, tr["rl_pending_before"][t])
        occ, stuck = unpack(tr["rl_occ"][t], H, W), unpack(tr["rl_stuck"][t], H, W)
        s = lx.phase_a(tr, occ, stuck, ctrl, dim, static)
        assert same_bits(s, tr["rl_state"][t]), f"tick {t}: state, groups {np.nonzero((s != tr['rl_state'][t]).any(axis=1))[0]}"
        n = lx.phase_b(tr, occ, stuck, ctrl, tr["rl_action"][t], dim, mg, static)
        assert same_bits(n, tr["rl_next_state"][t]), f"tick {t}: next state"
        want = tr["rl_ctrl"][t]
        assert np.array_equal(ctrl.rows(), want[:, :2]), f"tick {t}: _rl_phase / rl_timer"
        assert np.array_equal(ctrl.current, want[:, 2]) and np.array_equal(ctrl.pending, want[:, 3]), f"tick {t}: phases"
    assert (tr["rl_reward"] == 0).all()


def test_fixture_decides_the_static_features():
    """intersection_size is 0 for every group (computed before the cells are assigned); penalty_score is not"""
    tr = np.load(trace_path("lights_ext_96_s42"))
    assert (tr["rl_state"][:, :, 7] == 0).all() and (tr["rl_state"][:, :, 9] == 0).all()
    assert (np.diff(tr["g_icell_off"]) > 0).all()
    assert len(np.unique(tr["rl_state"][:, :, 8])) > 3


def test_stuck_fixture_pins_the_stuck_half_of_the_vector():
    """fields 13-18, and 11-12 above 13 dimensions, carry values other than 0 in the ungated fixture; the neighbours' means of
    phase A differ from phase B's where a later neighbour still held the previous call's value"""
    tr = np.load(trace_path("lights_ext_stuck_96_s43"))
    st, nx = tr["rl_state"], tr["rl_next_state"]
    assert int(tr["rl_dim"]) == 19 and np.unpackbits(tr["rl_stuck"]).sum() > 0
    assert (st[:, :, 13] != 0).any() and (st[:, :, 14] != 0).any() and (st[:, :, 15] != 0).any()
    assert (st[:, :, 11] != 0).any() and np.array_equal(st[:, :, 11:13], st[:, :, 17:19])
    assert (st[:, :, 11] != nx[:, :, 11]).any()
    # at this dimension the means are of stuck-map pressures: an occupancy pressure is far larger than any of them
    assert np.abs(st[:, :, 11]).max() <= np.abs(st[:, :, 15]).max() < np.abs(st[:, :, 2]).max()
