#!/usr/bin/env python3
"""Golden traces of the reference's batched light controller (build container only; never runs on the GPU box).

Runs the reference's own, unmodified `CityModel.step()` under TRAFFIC_LIGHT_AGENT_ALGORITHM = "NEIGHBOR_RL_BATCHED"
(city_model.py:1833-1836 -> rl_simple.run_batched_rl_control) through make_golden.run_scenario, so the trace arrays
are the ordinary ones (tests/trace_util.py replays them), and adds what the controller did at every tick:

  rl_state       (T, G, dim) float32   the state tensor of phase A (rl_simple.py:209-219)
  rl_action      (T, G) int8           the action drawn for every group
  rl_reward      (T, G) float64        memory[-1][2]: identically 0 (p_ew = -p_ns)
  rl_next_state  (T, G, dim) float32   memory[-1][3] rounded like the state tensor
  rl_ctrl        (T, G, 4) int32       _rl_phase, rl_timer, current_phase, pending_phase (-1 = None) after the call
  rl_pending_before (T, G) int32       pending_phase before the call
  rl_occ / rl_stuck (T, packed bits)   the two maps the call read
  rl_dim, rl_min_green
  g_intersection_size, g_penalty_score (G,) float64, g_approach_road_types (G, 4) int32: see below

The TensorFlow stand-in returns empty iterables, which would make the controller process no group.  So, inside the
imported rl_simple module only: `tf` becomes a small numpy-backed namespace (convert_to_tensor, nn.softmax(...).numpy(),
device), train_rl_batch becomes a no-op, and the shared policy is a scripted callable whose logits are so one-sided
that the drawn action is the scripted one.  No file of the reference is touched.

Usage:  python tests/golden/make_golden_lights.py all | <scenario>
"""
import io
import os
import subprocess
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SCENARIOS = {
    # the shipped default dimension on the small map
    "lights_ext_64_s45": dict(size=64, seed=45, vehicles=150, ticks=120, dim=13,
                              defaults={**mg.CLOSED, **mg.GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_RL_BATCHED",
                                        "SRL_INPUT_DIMENSIONS": 13}),
    # every field of the vector, closed population and GATED like lights_qa_96_s2
    "lights_ext_96_s42": dict(size=96, seed=42, vehicles=300, ticks=150, dim=19,
                              defaults={**mg.CLOSED, **mg.GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_RL_BATCHED",
                                        "SRL_INPUT_DIMENSIONS": 19}),
    # the same dimension with nothing gated (the default replanning policy, like full_96_s8) and a low stuck threshold: vehicles
    # become stuck on the approach cells, so the stuck-map half of the vector (fields 13-18, and 11-12 above 13 dimensions)
    # is recorded with values other than 0
    "lights_ext_stuck_96_s43": dict(size=96, seed=43, vehicles=300, ticks=60, dim=19, stuck=True,
                                    defaults={**mg.CLOSED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "NEIGHBOR_RL_BATCHED",
                                              "SRL_INPUT_DIMENSIONS": 19, "VEHICLE_STUCK_RECOMPUTE_THRESHOLD": 6}),
}


class _Tensor:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


class _Device:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _numpy_tf(np, standin):
    """What run_batched_rl_control uses of tensorflow (rl_simple.py:219-222); every other name (the constructor's
    make_policy_net and warm-up) still goes to the permissive stand-in."""
    import types

    def softmax(x, axis=-1):
        x = np.asarray(x, dtype=np.float64)
        e = np.exp(x - x.max(axis=axis, keepdims=True))
        return _Tensor(e / e.sum(axis=axis, keepdims=True))

    class _TF(types.SimpleNamespace):
        def __getattr__(self, name):
            return getattr(standin, name)
    return _TF(float32=np.float32, int32=np.int32,
               convert_to_tensor=lambda v, dtype=None: np.asarray(v, dtype=dtype),
               nn=types.SimpleNamespace(softmax=softmax),
               device=lambda name: _Device())


def write_npz(path, arrays):
    """np.savez_compressed without the wall clock in the member headers: the same arrays give the same bytes."""
    import numpy as np
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def run(name):
    import random

    import numpy as np
    spec = SCENARIOS[name]
    dim = spec["dim"]
    mg.SCENARIOS[name] = {k: v for k, v in spec.items() if k not in ("dim", "stuck")}
    mg._setup_paths()
    from Simulation.config import Defaults
    # intersection_light_group.py:13 reads the algorithm when it is first imported
    for k, v in spec["defaults"].items():
        setattr(Defaults, k, v)
    import Simulation.utilities.light_group_managment.rl_simple as rl
    rl.tf = _numpy_tf(np, rl.tf)
    rl.train_rl_batch = lambda *a, **k: None
    min_green = int(Defaults.SRL_MIN_GREEN)

    script = random.Random(1000 + spec["seed"])
    rec = dict(state=[], action=[], reward=[], next_state=[], ctrl=[], pending_before=[], occ=[], stuck=[])
    tick = {"t": 0, "scripted": None}

    def policy(states):
        # eager toggling at first (groups whose first phase is still held back by clearance get another request), then calmer
        p = 0.9 if tick["t"] < 14 else 0.3
        a = np.asarray([1 if script.random() < p else 0 for _ in range(len(states))], dtype=np.int64)
        tick["scripted"] = a
        logits = np.full((len(states), 2), -1000.0)
        logits[np.arange(len(states)), a] = 1000.0
        return logits

    orig = rl.run_batched_rl_control

    def control(groups, _policy_model):
        city = groups[0].city_model
        tick["groups"] = groups
        city.shared_rl_policy = policy
        rec["pending_before"].append([mg.none_i(g.pending_phase) for g in groups])
        rec["occ"].append(np.packbits(city.occupancy_map.astype(np.uint8).ravel()))
        rec["stuck"].append(np.packbits(city.stuck_map.astype(np.uint8).ravel()))
        for g in groups:
            g.memory.clear()
        orig(groups, city.shared_rl_policy)
        mem = [g.memory[-1] for g in groups]
        assert all(len(g.memory) == 1 for g in groups)
        rec["state"].append(np.asarray([m[0] for m in mem], dtype=np.float32))
        rec["action"].append([m[1] for m in mem])
        rec["reward"].append([float(m[2]) for m in mem])
        rec["next_state"].append(np.asarray([m[3] for m in mem], dtype=np.float32))
        rec["ctrl"].append([[g._rl_phase, g.rl_timer, mg.none_i(g.current_phase), mg.none_i(g.pending_phase)] for g in groups])
        assert np.array_equal(rec["action"][-1], tick["scripted"]), "the drawn action is not the scripted one"
        tick["t"] += 1
    rl.run_batched_rl_control = control

    saved = {}
    real_savez = np.savez_compressed

    def keep(path, **arrays):   # (run_scenario reports the file's size: let it write, the file is rewritten below)
        saved.update(arrays=arrays)
        real_savez(path, **arrays)
    np.savez_compressed = keep
    try:
        mg.run_scenario(name)
    finally:
        np.savez_compressed = real_savez
    out = saved["arrays"]
    T = len(rec["state"])
    assert T == len(out["veh_off"]) - 1 and "raised_at_tick" not in out
    out["rl_state"] = np.stack(rec["state"])
    out["rl_action"] = np.asarray(rec["action"], dtype=np.int8)
    out["rl_reward"] = np.asarray(rec["reward"], dtype=np.float64)
    out["rl_next_state"] = np.stack(rec["next_state"])
    out["rl_ctrl"] = np.asarray(rec["ctrl"], dtype=np.int32)
    out["rl_pending_before"] = np.asarray(rec["pending_before"], dtype=np.int32)
    out["rl_occ"], out["rl_stuck"] = np.stack(rec["occ"]), np.stack(rec["stuck"])
    out["rl_dim"], out["rl_min_green"] = np.int32(dim), np.int32(min_green)
    assert out["rl_state"].shape[2] == dim
    # the two static features as the constructor left them (intersection_light_group.py:156-165), and what penalty_score is a
    # mean of: CellAgent.road_type of every light's incoming + outgoing blocks as counts [blocks, R1, R2, R3] - not the
    # road_type_map plane, which shows an R2 cell of the ring road as 1 (city_model.py:2170-2172)
    groups = tick["groups"]
    out["g_intersection_size"] = np.asarray([g.intersection_size for g in groups], dtype=np.float64)
    out["g_penalty_score"] = np.asarray([g.penalty_score for g in groups], dtype=np.float64)
    types = [[b.road_type for tl in g.traffic_lights for b in tl.assigned_incoming_road_blocks + tl.assigned_outgoing_road_blocks]
             for g in groups]
    out["g_approach_road_types"] = np.asarray([[len(t), t.count("R1"), t.count("R2"), t.count("R3")] for t in types], dtype=np.int32)
    lists = sum(np.diff(out[f"g_{nm}_off"]) for nm in ("ns_in", "ns_out", "ew_in", "ew_out"))
    assert np.array_equal(out["g_approach_road_types"][:, 0], lists), "a block outside the four coordinate lists"

    # ---- coverage, on the reference run alone ----
    act, ctrl, pb = out["rl_action"], out["rl_ctrl"], out["rl_pending_before"]
    timer_before = np.concatenate([np.zeros((1, act.shape[1]), np.int32), ctrl[:-1, :, 1]])
    cov = dict(
        both_actions=bool((act == 0).any() and (act == 1).any()),
        refused_by_min_green=int(((act == 1) & (timer_before + 1 < min_green)).sum()),
        # (from the second call on: at tick 0 every group still holds the constructor's pending 0, whatever the traffic)
        pending_survives=int(((pb >= 0) & (ctrl[:, :, 3] == pb))[1:].sum()),
        pending_overwritten=int(((pb >= 0) & (ctrl[:, :, 3] >= 0) & (ctrl[:, :, 3] != pb)).sum()),
        empty_approach=int(((np.diff(out["g_ns_in_off"]) == 0) | (np.diff(out["g_ew_in_off"]) == 0)).sum()),
        no_ctor_neighbours=int((out["g_neighbors_ctor"][:, :, 0] < 0).all(axis=1).sum()),
        table_switch=int(((out["g_neighbors_ctor"] != out["g_neighbors"]).any(axis=(1, 2)) &
                          (out["grp_rows"][:, :, 0] >= 0).any(axis=0)).sum()),
        rewards_zero=bool((out["rl_reward"] == 0).all()),
        minus_one_neighbours=int(((out["g_neighbors"][:, :, 0] >= 0) & (out["g_neighbors"][:, :, 1] < 0)).sum() +
                                 ((out["g_neighbors_ctor"][:, :, 0] >= 0) & (out["g_neighbors_ctor"][:, :, 1] < 0)).sum()),
    )
    # a pending phase that survived did so because of clearance: nothing else holds one back here
    assert not Defaults.TRAFFIC_LIGHT_TRANSITION_DURATION_ENABLED and Defaults.TRAFFIC_LIGHT_TRANSITION_CLEARANCE_ENABLED
    print(f"[{name}] coverage {cov}")
    if spec.get("stuck"):
        st, nx = out["rl_state"], out["rl_next_state"]
        cov.update(
            stuck_on_approaches=int((st[:, :, 13:15] != 0).any(axis=2).sum()),          # stuck N-S / E-W sums
            stuck_pressure=int((st[:, :, 15] != 0).sum()),
            both_stuck_axes=bool((st[:, :, 13] != 0).any() and (st[:, :, 14] != 0).any()),
            neighbour_means=int(((st[:, :, 11] != 0) & (st[:, :, 17] != 0)).sum()),
            # phase A differs from phase B in the neighbours' means: a neighbour j > i still held the previous call's value
            stored_from_previous_call=int((st[:, :, 11] != nx[:, :, 11]).sum()),
            # ... and the stored value above 13 dimensions is the stuck-map pressure, not the occupancy one
            means_differ_from_occupancy=bool((out["rl_stuck"].any()) and (st[1:, :, 11] != 0).any()))
        for k in ("stuck_on_approaches", "stuck_pressure", "both_stuck_axes", "neighbour_means", "stored_from_previous_call",
                  "means_differ_from_occupancy"):
            assert cov[k], f"{name}: coverage condition {k} not met by this seed"
        print(f"[{name}] stuck coverage { {k: cov[k] for k in cov if 'stuck' in k or 'mean' in k or 'stored' in k} }")
    for k in ("both_actions", "refused_by_min_green", "pending_survives", "pending_overwritten", "empty_approach",
              "no_ctor_neighbours", "table_switch", "rewards_zero"):
        # (an overwritten pending phase needs a group whose first phase is held back for five ticks; the two gated scenarios
        # have it, the stuck scenario is not asked for it again)
        assert cov[k] or (k == "pending_overwritten" and spec.get("stuck")), f"{name}: coverage condition {k} not met by this seed"
    path = os.path.join(HERE, f"trace_{name}.npz")
    write_npz(path, out)
    print(f"[{name}] dim={dim} groups={act.shape[1]} ticks={T} size={os.path.getsize(path)}")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        for j in SCENARIOS:     # one process per scenario: the algorithm and the dimension are read at import time
            subprocess.run([sys.executable, os.path.abspath(__file__), j], check=True, cwd="/tmp")
    else:
        run(what)


if __name__ == "__main__":
    main()
