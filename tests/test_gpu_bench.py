"""bench.py end to end on one GPU at a small size: a plain run (headline only, exactly --steps timed steps) whose
--dump-outputs files equal the CPU oracle's state after the same warm-up + timed ticks, and a --full run."""
import json
import os
import sys

import numpy as np
import pytest

import bench
from tests import procs

pytestmark = pytest.mark.gpu

SMALL = ["--size", "512", "--vehicles", "12000"]


def _run(*extra):
    out = procs.run([sys.executable, os.path.join(procs.ROOT, "bench.py"), "--gpus", "1", *SMALL, *extra], timeout=600)
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def test_bench_plain_run_dumps_the_oracle_state(oracle, tmp_path):
    row = _run("--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "hip"))
    assert row["metric"] == "agent_steps_per_sec" and row["unit"] == "agent-steps/s" and row["higher_is_better"] is True
    assert row["dtype"] == "i32" and row["value"] > 0 and row["steps"] == 3 and len(row["config"]["ticks"]) == 3
    assert abs(row["ms_per_step"] - sum(t[0] for t in row["config"]["ticks"]) / 3) < 0.05 * row["ms_per_step"] + 1.0
    assert "cpu_baseline" not in row and "secondary" not in row
    tables, routes, _ = bench.make_workload(512, 12000, 1)
    bench.setup(oracle, tables, routes, 1, policy="full")
    oracle.step(5)
    bench.dump_outputs(oracle, str(tmp_path / "cpu"))
    for name in ("vehicles", "groups", "occupancy", "stop", "stuck"):
        a, b = np.load(tmp_path / "hip" / (name + ".npy")), np.load(tmp_path / "cpu" / (name + ".npy"))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
    fields = [f for f, _ in oracle.counters()._fields_]
    a, b = np.load(tmp_path / "hip" / "counters.npy"), np.load(tmp_path / "cpu" / "counters.npy")
    for f in ("stuck", "live_through", "count_completed_through", "total_distance_through", "agent_steps", "astar_calls",
              "elapsed", "step_count"):     # (the counters both engines keep alike, tests/test_gpu_parity.py)
        assert a[fields.index(f)] == b[fields.index(f)], f


def test_bench_full_run():
    row = _run("--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "2")
    assert row["steps"] == 2 and set(row["secondary"]) == {"config2", "lights"}
    assert row["cpu_baseline"]["kind"] == "port" and row["cpu_baseline"]["value"] > 0
