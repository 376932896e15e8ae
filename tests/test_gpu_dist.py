"""Multi-GPU mode "replicated state / sharded replans" on the GPU: two ranks (two processes on this box's one GPU,
gloo underneath - RCCL refuses two ranks on one device) each replay a reference trace with the full replanning policy;
every rank plans half of each tick's searches, the results are exchanged, and BOTH ranks must match the reference's
recorded state at every tick - i.e. the N-rank result equals the 1-GPU result bit for bit."""
import json
import os
import sys

import pytest

from tests import procs

pytestmark = pytest.mark.gpu

WORKER = r'''
import numpy as np
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace
from tests.trace_util import setup_from_trace, check_initial, replay_and_compare, trace_path
os.environ.update(%(rank_env)r.get(rank, {}))      # (this rank's own engine settings, read when its engine plans)
for name in %(traces)r:
    tr = load_trace(trace_path(name))
    api = new_engine()
    setup_from_trace(api, tr, explicit_paths=False)
    check_initial(api, tr)
    if %(device_direct)r:
        import torch
        sr = tdist.ShardedReplans(device=torch.device("cuda", 0), device_direct=True).attach(api)
    else:
        sr = tdist.ShardedReplans().attach(api)
    n = replay_and_compare(api, tr)          # raises on the first tick that differs from the reference
    c = api.counters()
    res[name] = dict(ticks=n, astar_calls=int(c.astar_calls), want_calls=int(tr["astar_calls_spawn"]) + int(tr["astar_per_tick"].sum()),
                     exchanges=sr.calls, bytes=sr.bytes_sent, fp=list(api.rng_fingerprint(capi.RNG_GLOBAL)),
                     quad_jobs=api.debug_quad_stats()["jobs"])
    api.close()
'''


@pytest.mark.parametrize("world,device_direct,tight_pool,quads", [(2, False, False, False), (2, True, False, False), (2, True, True, False), (4, True, False, False),
                                                               (5, True, False, False), (2, True, False, True), (4, True, False, True)])
def test_ranks_sharded_replans_match_the_reference(world, device_direct, tight_pool, quads):
    """2, 4 and 5 ranks (with the test runner itself that is the six processes this box lets share its GPU), with the records exchanged between device buffers
    (ts_set_replan_sharding_device; the collective itself is gloo here) and once with the host-staged form."""
    # closed populations, then the agents that step on the host inside the shuffled order (traffic generator spawning and
    # planning mid-tick, service vehicles with their arrival records, rain): every rank runs those redundantly
    traces = TRACES_2 if world == 2 else TRACES_N
    env = {}
    if quads:           # (every rank's share of every queue on k_replan_quad, its hand-backs on k_replan beside it)
        env["TS_QUAD"], env["TS_QUAD_MIN"] = "1", "1"
    if tight_pool:      # (almost no room reserved in the path pool: planners find it full, the pool is garbage-collected / grown INSIDE the
        env["TS_DEBUG_POOL_PER_ENTRY"] = "2"      # sharded tick, and the export must not rely on the pool's growth to size its buffer)
    _run_ranks_and_check(world, device_direct, traces, env, {})


TRACES_2 = ["full_64_s1", "full_96_s8", "faults_64_s9", "carve_96_s10", "dta_64_s12", "rain_96_s14", "config1_64_s11", "despawn_96_s25", "startgoal_96_s27"]
TRACES_N = ["full_96_s8", "faults_64_s9", "dta_64_s12", "config1_64_s11", "startgoal_96_s27"]


@pytest.mark.parametrize("rank0_classes", [None, "1"])
def test_ranks_that_plan_on_different_searchers_match_the_reference(rank0_classes):
    """Whether a rank sends a queue to k_replan_quad is its own decision (TS_QUAD, TS_QUAD_MIN, and the quads' memory, which
    comes from that rank's free device memory).  Rank 0 plans every queue with the quads (all classes but the most expensive
    one; with TS_QUAD_CLASSES=1 only class 0, so k_replan serves classes 3, 2 and 1 beside them), rank 1 with k_replan alone.
    Both must still deal the queue out the same way - entry j of the whole sorted queue is rank j % world's, whichever kernel
    serves it - or some vehicles are planned twice and others not at all: every rank matches the reference at every tick,
    and the searches of the two ranks add up to the reference's."""
    rank_env = {0: {"TS_QUAD": "1", "TS_QUAD_MIN": "1"}, 1: {"TS_QUAD": "0"}}
    if rank0_classes:
        rank_env[0]["TS_QUAD_CLASSES"] = rank0_classes
    rows = _run_ranks_and_check(2, True, TRACES_2, {}, rank_env)
    assert sum(rows[0][name]["quad_jobs"] for name in TRACES_2) > 0          # rank 0 did plan on the quads ...
    assert all(rows[1][name]["quad_jobs"] == 0 for name in TRACES_2)         # ... and rank 1 never


def _run_ranks_and_check(world, device_direct, traces, env_all, rank_env):
    rows, _, _ = procs.run_ranks(WORKER, world, env=dict(os.environ, **env_all), timeout=900, traces=traces, device_direct=device_direct,
                                 rank_env=rank_env)
    r0 = rows[0]
    for name in traces:
        a = r0[name]
        for rb in rows[1:]:
            b = rb[name]
            assert a["ticks"] == b["ticks"] > 0
            if name != "config1_64_s11":     # (service vehicles plan inside the generator's step too: not in the fixture's per-tick count)
                assert a["astar_calls"] == b["astar_calls"] == a["want_calls"]     # the searches of all ranks add up to the reference's
            assert a["astar_calls"] == b["astar_calls"]
            assert a["fp"] == b["fp"]
            assert a["exchanges"] == b["exchanges"] > 0
        assert sum(rb[name]["bytes"] for rb in rows) > 0
        if world == 2:
            assert all(rb[name]["bytes"] > 0 for rb in rows)       # both ranks planned something
    return rows


NCCL_WORKER = r'''
import numpy as np
import torch
import torch.distributed as dist
from trafficsimulation_amd import dist as tdist
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=torch.device("cuda", 0))
sr = tdist.ShardedReplans(device=torch.device("cuda", 0))
ok = True
for n in (0, 1, 4097, 3_000_000):
    payload = np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    stacked, sizes = sr.gather_bytes(payload)
    ok &= sizes == [n] and stacked.shape == (1, max(n, 1)) and stacked[0, :n].tobytes() == payload
# the ctypes callback the engine calls (ts_exchange_fn), end to end
import ctypes as C
buf = (C.c_uint8 * 5)(1, 2, 3, 4, 5)
recv, sizes_p, stride = C.c_void_p(), C.c_void_p(), C.c_int64()
rc = sr._callback(None, C.addressof(buf), 5, C.pointer(recv), C.pointer(sizes_p), C.pointer(stride))
got = C.string_at(recv.value, 5)
ok &= rc == 0 and got == bytes([1, 2, 3, 4, 5]) and stride.value == 5 and C.cast(sizes_p.value, C.POINTER(C.c_int64))[0] == 5
print(json.dumps({"ok": bool(ok), "backend": dist.get_backend(), "calls": sr.calls}))
dist.destroy_process_group()
'''


def test_exchange_collective_over_rccl():
    """The same exchange object on a real RCCL process group (backend "nccl", buffers staged through the GPU).  One rank
    only - this box has one GPU and RCCL refuses two ranks on a device - so this checks the device staging, the padded
    all_gather and the callback plumbing, not the wire."""
    out = procs.run_python(NCCL_WORKER, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), timeout=600, port=procs.free_port())
    row = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
    assert row["ok"] and row["backend"] == "nccl" and row["calls"] == 5


def test_bench_two_ranks_over_gloo_smoke():
    """`python bench.py --gpus 2` end to end on this box's one GPU (gloo, sharded replans, device-direct exchange): the line
    reports the process group's size and that both ranks ended in the same state."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(procs.ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--size", "512", "--vehicles", "12000",
           "--steps", "4", "--warmup", "4", "--full", "--no-cpu-baseline", "--no-secondary"]
    out = procs.run(cmd, env=env, timeout=600)
    row = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
    assert row["n_gpus"] == 2 and row["scaling"] == "strong"
    assert row["config"]["ranks_hold_identical_state"] is True
    assert row["config"]["exchange"]["calls"] > 0 and row["config"]["astar"]["calls"] > 1000
