"""bench.py's own pieces on the CPU: its threaded route walk against citygen.make_routes, and --dump-outputs' files written
from the oracle (the GPU side of both: tests/test_gpu_bench.py)."""
import os
import sys

import numpy as np
import pytest

import bench
from tests import procs
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import citygen


@pytest.mark.parametrize("size,vehicles,seed,lo,hi,carves,threads", [
    (160, 800, 8, 30, 120, False, 1), (160, 800, 8, 30, 120, False, 3), (384, 6000, 4, 30, 120, True, 5),
    (512, 12000, 2, 150, 400, False, 4), (96, 10 ** 6, 3, 5, 40, False, 2)])      # (the last: fewer road cells than vehicles)
def test_routes_match_citygen(size, vehicles, seed, lo, hi, carves, threads):
    tables = citygen.generate(size, size, seed=seed, carve_subblock_roads=carves)
    want = citygen.make_routes(tables, vehicles, seed=seed + 1, min_len=lo, max_len=hi)
    got = bench.make_routes(tables, vehicles, seed=seed + 1, min_len=lo, max_len=hi, threads=threads)
    assert len(got[0]) > 500
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _stepped_oracle(oracle, ticks=6):
    tables, routes, _ = bench.make_workload(160, 800, 5)
    bench.setup(oracle, tables, routes, 5, policy="full")
    oracle.step(ticks)
    return oracle


def test_dump_outputs_hold_the_engine_state(oracle, tmp_path):
    api = _stepped_oracle(oracle)
    bench.dump_outputs(api, str(tmp_path))
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert sorted(got) == ["counters", "groups", "occupancy", "stop", "stuck", "vehicles"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["vehicles"], api.vehicles().astype(np.float64)) and len(got["vehicles"]) > 100
    assert np.array_equal(got["groups"], api.groups().astype(np.float64))
    for name, which in (("occupancy", capi.MAP_OCCUPANCY), ("stop", capi.MAP_STOP), ("stuck", capi.MAP_STUCK)):
        assert np.array_equal(got[name], api.map(which).ravel().astype(np.float32))
    c = api.counters()
    assert got["counters"][[f for f, _ in c._fields_].index("step_count")] == c.step_count == 6


def test_dump_outputs_sample_large_tables(oracle, tmp_path, monkeypatch):
    """Above DUMP_ROWS / DUMP_CELLS: the same seeded rows and cells every time, in order."""
    monkeypatch.setattr(bench, "DUMP_ROWS", 50)
    monkeypatch.setattr(bench, "DUMP_CELLS", 1000)
    api = _stepped_oracle(oracle)
    bench.dump_outputs(api, str(tmp_path / "a"))
    bench.dump_outputs(api, str(tmp_path / "b"))
    veh, occ = api.vehicles(), api.map(capi.MAP_OCCUPANCY).ravel()
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("vehicles", "occupancy")}
    assert all(np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy"))) for n in a)
    assert a["vehicles"].shape == (50, veh.shape[1]) and a["occupancy"].shape == (1000,)
    rows = bench._sample(len(veh), 50, 1)
    assert (np.diff(rows) > 0).all() and np.array_equal(a["vehicles"], veh[rows].astype(np.float64))
    assert np.array_equal(a["occupancy"], occ[bench._sample(len(occ), 1000, 3)].astype(np.float32))


def test_steps_must_be_positive():
    with pytest.raises(AssertionError) as ex:
        procs.run([sys.executable, os.path.join(procs.ROOT, "bench.py"), "--steps", "0"], timeout=120)
    assert ex.value.proc.returncode == 2 and "--steps" in ex.value.proc.stderr
