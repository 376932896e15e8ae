"""Seed-compatible world generator (trafficsimulation_amd/worldgen.py) against worlds the reference itself built.

Fixtures: tests/golden/worlds.npz (tests/golden/make_golden.py::run_worlds - 30 configurations of CityModel's
constructor arguments, including one the reference rejects) and the world tables inside every trace_*.npz.
Every table is compared bit for bit, and so is the MT19937 state the generator leaves behind."""
import glob
import json
import os

import numpy as np
import pytest

from trafficsimulation_amd.world import load_trace
from trafficsimulation_amd.worldgen import generate_world
from tests.trace_util import GOLDEN, check_initial, replay_and_compare, seed_only as _seed_only, setup_from_trace, trace_path, world_options as _options

_WORLDS = np.load(os.path.join(GOLDEN, "worlds.npz"), allow_pickle=False)
_INDEX = json.loads(str(_WORLDS["index"]))
_EXC = {"ZeroDivisionError": ZeroDivisionError, "IndexError": IndexError, "ValueError": ValueError, "KeyError": KeyError}


@pytest.mark.parametrize("entry", _INDEX, ids=[e["tag"] for e in _INDEX])
def test_world_matches_reference(entry):
    opts = _options(entry["kwargs"], {"RAIN_ENABLED": False, "ENABLE_TRAFFIC": False, **entry["defaults"]})
    if "raises" in entry:     # the reference's constructor fails on this configuration; same failure here
        with pytest.raises(_EXC[entry["raises"]]):
            generate_world(entry["width"], entry["height"], seed=entry["seed"], **opts)
        return
    w = generate_world(entry["width"], entry["height"], seed=entry["seed"], **opts)
    tag = entry["tag"]
    want_keys = {k.split("/", 1)[1] for k in _WORLDS.files if k.startswith(tag + "/")}
    assert want_keys - {"display_names"} == set(w)      # (the labels belong to the facade: tests/test_mesa_facade.py)
    for k in sorted(w):
        want = _WORLDS[f"{tag}/{k}"]
        got = np.asarray(w[k])
        assert got.shape == want.shape and np.array_equal(got, want), f"{tag}: table {k} differs"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "trace_*.npz"))), ids=lambda p: os.path.basename(p)[6:-4])
def test_trace_world_matches_reference(path):
    tr = load_trace(path)
    sc = tr["scenario"]
    w = generate_world(sc["size"], sc.get("height", sc["size"]), seed=sc["seed"], **_options(sc.get("model_kwargs", {}), tr["defaults_json"]))
    for k in sorted(w):
        if k == "global_rng_state":
            if "global_rng_before_day0" in tr:     # state when DynamicTrafficAgent draws day 0 = right after world-gen
                assert np.array_equal(w[k], tr["global_rng_before_day0"])
        elif k in tr:                              # older fixtures hold fewer block tables
            assert np.asarray(w[k]).shape == tr[k].shape and np.array_equal(w[k], tr[k]), f"table {k} differs"


@pytest.mark.parametrize("name,ticks", [("config1_64_s11", 200), ("service_64_s15", 120), ("default_200_s20", 160)])
def test_seed_only_run_reproduces_reference_trace(oracle, name, ticks):
    """size + seed -> world-gen -> engine (the CPU oracle here; tests/test_gpu_worldgen.py runs the HIP engine):
    the per-tick trace of the reference's own CityModel(width, height, seed=seed) run."""
    tr = _seed_only(load_trace(trace_path(name)))
    setup_from_trace(oracle, tr)
    check_initial(oracle, tr)
    assert replay_and_compare(oracle, tr, ticks=ticks) == ticks


def test_rectangular_and_edge_sizes_build():
    w = generate_world(90, 60, seed=5, rain_enabled=False, enable_traffic=False)
    assert w["allowed_dirs_map"].shape == (60, 90)
    assert int(w["is_road_map"].sum()) > 0 and len(w["highway_entrances_xy"]) > 0
    for key in ("highway_entrances_xy", "highway_exits_xy"):      # both kinds sit on the outer edge of the map
        xy = np.asarray(w[key])
        assert np.all((xy[:, 0] == 0) | (xy[:, 0] == 89) | (xy[:, 1] == 0) | (xy[:, 1] == 59))
