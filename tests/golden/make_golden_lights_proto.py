#!/usr/bin/env python3
"""Golden traces of the reference's A2C and GAT-DQN batched light controllers (build container only; never on the GPU box).

Runs the reference's own, unmodified `CityModel.step()` under TRAFFIC_LIGHT_AGENT_ALGORITHM = "RL_A2C_BATCHED" /
"GAT_DQN_BATCHED" (city_model.py:1839-1848 -> rl_a2c.run_a2c_control / rl_gatdqn.run_batched_gat_dqn_control) through
make_golden.run_scenario, so the trace arrays are the ordinary ones (tests/trace_util.py replays them), and adds what the
controller did in front of every tick:

  lp_state       (T, G, 13) float32 (A2C) / (T, G, 5, 9) float32 (GAT)   the state batch the policy was given
  lp_mask        (T, G, 5) float32                                        GAT only
  lp_q           (T, G, 2) float32                                        GAT only: the scripted q-values
  lp_action      (T, G) int8           the action taken (A2C: the scripted one; GAT: what the epsilon-greedy step chose)
  lp_explore     (T, G) int8           GAT only: 1 where random() < epsilon; lp_rejects (T, G) int32: randrange retries
  lp_reward      (T, G) float64
  lp_next_state  (T, G, 5, 9) float32, lp_next_mask (T, G, 5) float32    GAT only (the transition stored in ig.memory)
  lp_eps         (T, G) float64        GAT only: ig.epsilon after the call
  lp_ctrl        (T, G, 4) int32       _rl_phase, rl_timer, current_phase, pending_phase (-1 = None) after the call
  lp_pending_before (T, G) int32
  lp_occ         (T, packed bits)      the occupancy map the call read
  lp_stats       (T, 4) float64        cached_stats avg_duration_internal / _through, avg_time_per_unit_internal / _through
                                       at the call (0 where the key is missing)
  lp_protocol (1 = A2C, 2 = GAT), lp_min_green, lp_eps_min, lp_eps_decay
  g_intersection_size, g_penalty_score, g_approach_road_types: as in make_golden_lights.py

Replacements, all made from outside (no file of the reference is touched), inside the imported modules only:
  * `tf` of rl_a2c / rl_gatdqn becomes the small numpy-backed namespace of make_golden_lights plus what these two use
    (random.categorical returns the scripted action, squeeze, nn.log_softmax, gather); the actor / critic and every
    group's q-network are scripted callables; update_a2c and _train_dqn (the learners; _train_dqn would draw random.sample
    from the global stream) are no-ops;
  * Simulation.city_model.warmup_models is a no-op (under the permissive stand-in it fails on `_Any + _Any`);
  * intersection_light_group.make_gat_dqn_net returns a small object with get_weights / set_weights (the stand-in cannot be subclassed
    as a Keras layer).
The GAT draw chain is followed on a copy of the global stream (random(), then randrange(2) = getrandbits(2) with
rejection when exploring) and must end where the reference's stream ends: that is how explore / reject are known.

Usage:  python tests/golden/make_golden_lights_proto.py all | <scenario>
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_lights as mgl  # noqa: E402

A2C, GAT = 1, 2
DTA_ON = {"RAIN_ENABLED": False, "TOTAL_SERVICE_VEHICLES_FOOD": 0, "TOTAL_SERVICE_VEHICLES_WASTE": 0,
          "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 60000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 20000}
SCENARIOS = {
    "lights_a2c_64_s45": dict(size=64, seed=45, vehicles=150, ticks=60, proto=A2C,
                              defaults={**mg.CLOSED, **mg.GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "RL_A2C_BATCHED"}),
    "lights_a2c_96_s47": dict(size=96, seed=47, vehicles=300, ticks=60, proto=A2C,
                              defaults={**mg.CLOSED, **mg.GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "RL_A2C_BATCHED"}),
    # epsilon falls from 1.0 to its floor of 0.1 inside the trace: always-explore, mixed and mostly-greedy ticks
    "lights_gat_64_s45": dict(size=64, seed=45, vehicles=150, ticks=60, proto=GAT,
                              defaults={**mg.CLOSED, **mg.GATED, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "GAT_DQN_BATCHED",
                                        "EPS_DECAY_RATE": 0.03}),
    # the traffic generator on (like dta_96_s13): cached_stats, and with it the global reward term, changes during the trace
    "lights_gat_96_s49": dict(size=96, seed=49, vehicles=120, ticks=70, proto=GAT, dta=True,
                              defaults={**DTA_ON, "TRAFFIC_LIGHT_AGENT_ALGORITHM": "GAT_DQN_BATCHED", "EPS_DECAY_RATE": 0.04}),
}
STAT_KEYS = ("avg_duration_internal", "avg_duration_through", "avg_time_per_unit_internal", "avg_time_per_unit_through")


class _QNet:
    """What the group constructor and _gat_q need of a q-network; the values are scripted per control call."""

    def __init__(self):
        self.w, self.q = [], None

    def get_weights(self):
        return self.w

    def set_weights(self, w):
        self.w = w

    def __call__(self, inputs):
        return [mgl._Tensor(self.q)]


def _proto_tf(np, standin, scripted):
    tf = mgl._numpy_tf(np, standin)

    def log_softmax(x):
        x = np.asarray(x, dtype=np.float64)
        return x - x.max(axis=-1, keepdims=True) - np.log(np.exp(x - x.max(axis=-1, keepdims=True)).sum(axis=-1, keepdims=True))
    tf.nn.log_softmax = log_softmax

    class _Arr(np.ndarray):      # (indexable like a tensor, and with its .numpy())
        def numpy(self):
            return np.asarray(self)
    tf.squeeze = lambda a, axis=None: np.squeeze(np.asarray(a), axis=axis).view(_Arr)
    tf.gather = lambda row, i: row[int(i)]
    import types
    tf.random = types.SimpleNamespace(categorical=lambda logits, n: np.asarray(scripted["a"], dtype=np.int64).reshape(-1, 1))
    return tf


def run(name):
    import random

    import numpy as np
    spec = SCENARIOS[name]
    proto = spec["proto"]
    mg.SCENARIOS[name] = {k: v for k, v in spec.items() if k not in ("proto", "dta")}
    mg._setup_paths()
    from Simulation.config import Defaults
    # intersection_light_group.py:13-25 and rl_gatdqn.py:29-31 read these when they are first imported
    for k, v in spec["defaults"].items():
        setattr(Defaults, k, v)
    script = random.Random(2000 + spec["seed"])
    rec = {k: [] for k in ("state", "mask", "q", "action", "explore", "rejects", "reward", "next_state", "next_mask", "eps", "ctrl",
                           "pending_before", "occ", "stats")}
    tick = {"t": 0}
    scripted = {"a": None}

    def scripted_actions(n):
        # eager toggling at first (groups whose first phase is still held back by clearance get another request), then calmer
        p = 0.9 if tick["t"] < 14 else 0.3
        return np.asarray([1 if script.random() < p else 0 for _ in range(n)], dtype=np.int8)

    def before(groups):
        city = groups[0].city_model
        tick["groups"] = groups
        rec["pending_before"].append([mg.none_i(g.pending_phase) for g in groups])
        rec["occ"].append(np.packbits(city.occupancy_map.astype(np.uint8).ravel()))
        dta = getattr(city, "dynamic_traffic_generator", None)
        cs = getattr(dta, "cached_stats", {}) if dta else {}
        rec["stats"].append([float(cs.get(k, 0.0)) for k in STAT_KEYS])

    def after(groups):
        rec["ctrl"].append([[g._rl_phase, g.rl_timer, mg.none_i(g.current_phase), mg.none_i(g.pending_phase)] for g in groups])
        tick["t"] += 1

    import Simulation.city_model as cm
    cm.warmup_models = lambda *a, **k: None
    if proto == A2C:
        import Simulation.utilities.light_group_managment.rl_a2c as rl
        rl.tf = _proto_tf(np, rl.tf, scripted)
        rl.update_a2c = lambda *a, **k: None
        min_green = int(getattr(Defaults, "TRAFFIC_LIGHT_MIN_GREEN", 5))
        assert not hasattr(Defaults, "TRAFFIC_LIGHT_MIN_GREEN") and not hasattr(Defaults, "TRAFFIC_LIGHT_MAX_GREEN")
        stored = []
        orig_store = rl.TrajectoryBuffer.store

        def store(self, s, a, r, v, logp):
            stored.append((s, a, r))
            orig_store(self, s, a, r, v, logp)
        rl.TrajectoryBuffer.store = store
        orig = rl.run_a2c_control

        def control(groups, _actor, _critic, optimizer):
            before(groups)
            scripted["a"] = scripted_actions(len(groups))

            def actor(s_batch):
                assert s_batch.dtype == np.float32
                rec["state"].append(np.array(s_batch))
                return np.zeros((len(s_batch), 2))
            del stored[:]
            orig(groups, actor, lambda s: np.zeros((len(s), 1)), optimizer)
            assert len(stored) == len(groups)
            assert all(np.array_equal(np.asarray(s, dtype=np.float32), row) for (s, _, _), row in zip(stored, rec["state"][-1]))
            rec["action"].append([a for _, a, _ in stored])
            rec["reward"].append([r for _, _, r in stored])
            assert all(isinstance(r, float) for _, _, r in stored) and np.array_equal(rec["action"][-1], scripted["a"])
            after(groups)
        rl.run_a2c_control = control
    else:
        import Simulation.utilities.light_group_managment.rl_gatdqn as rl
        rl.tf = _proto_tf(np, rl.tf, scripted)
        rl._train_dqn = lambda *a, **k: None
        import Simulation.agents.city_structure_entities.intersection_light_group as ilg
        ilg.make_gat_dqn_net = _QNet       # (the name the group constructor calls, lines 22 and 95-96)
        min_green = int(Defaults.GAT_TRAFFIC_RL_MIN_GREEN)
        eps_min, eps_decay = float(rl.EPS_MIN), float(rl.EPS_DECAY_RATE)
        assert eps_decay == spec["defaults"]["EPS_DECAY_RATE"]
        orig = rl.run_batched_gat_dqn_control

        def control(groups):
            before(groups)
            G = len(groups)
            want = scripted_actions(G)
            q = np.asarray([[script.gauss(0, 1), script.gauss(0, 1)] for _ in range(G)], dtype=np.float32)
            for g in range(G):      # the greedy action is the scripted one, except for a tie now and then (argmax: 0)
                lo, hi = sorted(q[g])
                q[g] = (hi, hi) if script.random() < 0.1 else ((hi, lo) if want[g] == 0 else (lo, hi))
                groups[g].rl_policy.q = q[g]
                groups[g].memory.clear()
            eps0 = [float(g.epsilon) for g in groups]
            shadow = random.Random()
            shadow.setstate(random.getstate())
            orig(groups)
            explore, rejects, acts = [], [], []
            for g in range(G):      # rl_gatdqn.py:289-292 on the copy of the stream
                ex = shadow.random() < eps0[g]
                n = 0
                if ex:
                    a = shadow.getrandbits(2)
                    while a >= 2:
                        a = shadow.getrandbits(2)
                        n += 1
                else:
                    a = int(np.argmax(q[g]))
                explore.append(int(ex)); rejects.append(n); acts.append(a)
            assert shadow.getstate() == random.getstate(), "the draw chain of the control call is not the one written down here"
            mem = [g.memory[-1] for g in groups]
            assert all(len(g.memory) == 1 for g in groups)
            assert [m[2] for m in mem] == acts
            rec["state"].append(np.stack([m[0] for m in mem])); rec["mask"].append(np.stack([m[1] for m in mem]))
            assert rec["state"][-1].dtype == np.float32
            rec["q"].append(q); rec["action"].append(acts); rec["explore"].append(explore); rec["rejects"].append(rejects)
            rec["reward"].append([float(m[3]) for m in mem])
            rec["next_state"].append(np.asarray([m[4] for m in mem], dtype=np.float32))
            rec["next_mask"].append(np.asarray([m[5] for m in mem], dtype=np.float32))
            rec["eps"].append([float(g.epsilon) for g in groups])
            assert all(e == max(eps_min, e0 - eps_decay) for e, e0 in zip(rec["eps"][-1], eps0))
            after(groups)
        rl.run_batched_gat_dqn_control = control

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
    out["lp_state"] = np.stack(rec["state"])
    out["lp_action"] = np.asarray(rec["action"], dtype=np.int8)
    out["lp_reward"] = np.asarray(rec["reward"], dtype=np.float64)
    out["lp_ctrl"] = np.asarray(rec["ctrl"], dtype=np.int32)
    out["lp_pending_before"] = np.asarray(rec["pending_before"], dtype=np.int32)
    out["lp_occ"] = np.stack(rec["occ"])
    out["lp_stats"] = np.asarray(rec["stats"], dtype=np.float64)
    out["lp_protocol"], out["lp_min_green"] = np.int32(proto), np.int32(min_green)
    if proto == GAT:
        out["lp_mask"], out["lp_q"] = np.stack(rec["mask"]), np.stack(rec["q"])
        out["lp_explore"] = np.asarray(rec["explore"], dtype=np.int8)
        out["lp_rejects"] = np.asarray(rec["rejects"], dtype=np.int32)
        out["lp_next_state"], out["lp_next_mask"] = np.stack(rec["next_state"]), np.stack(rec["next_mask"])
        out["lp_eps"] = np.asarray(rec["eps"], dtype=np.float64)
        out["lp_eps_min"], out["lp_eps_decay"] = np.float64(eps_min), np.float64(eps_decay)
        assert out["lp_state"].shape[2:] == (5, 9) and out["lp_mask"].shape[2:] == (5,)
    else:
        assert out["lp_state"].shape[2:] == (13,)
    groups = tick["groups"]
    out["g_intersection_size"] = np.asarray([g.intersection_size for g in groups], dtype=np.float64)
    out["g_penalty_score"] = np.asarray([g.penalty_score for g in groups], dtype=np.float64)
    types = [[b.road_type for tl in g.traffic_lights for b in tl.assigned_incoming_road_blocks + tl.assigned_outgoing_road_blocks]
             for g in groups]
    out["g_approach_road_types"] = np.asarray([[len(t), t.count("R1"), t.count("R2"), t.count("R3")] for t in types], dtype=np.int32)
    lists = sum(np.diff(out[f"g_{nm}_off"]) for nm in ("ns_in", "ns_out", "ew_in", "ew_out"))
    assert np.array_equal(out["g_approach_road_types"][:, 0], lists), "a block outside the four coordinate lists"
    # the attributes the two state functions read with a default that nothing in the reference sets
    for g in groups:
        assert not any(hasattr(g, a) for a in ("_pressure_ns", "_pressure_ew", "intersection_size_factor", "_rl_timer"))

    # ---- coverage, on the reference run alone ----
    act, ctrl, pb = out["lp_action"], out["lp_ctrl"], out["lp_pending_before"]
    timer_before = np.concatenate([np.zeros((1, act.shape[1]), np.int32), ctrl[:-1, :, 1]])
    cov = dict(
        both_actions=bool((act == 0).any() and (act == 1).any()),
        refused_by_min_green=int(((act == 1) & (timer_before + 1 < min_green)).sum()),
        pending_survives=int(((pb >= 0) & (ctrl[:, :, 3] == pb))[1:].sum()),
        pending_overwritten=int(((pb >= 0) & (ctrl[:, :, 3] >= 0) & (ctrl[:, :, 3] != pb)).sum()),
        fewer_than_four_neighbours=int(((out["g_neighbors_ctor"][:, :, 0] >= 0).sum(axis=1) < 4).sum()),
        table_switch=int(((out["g_neighbors_ctor"] != out["g_neighbors"]).any(axis=(1, 2)) &
                          (out["grp_rows"][:, :, 0] >= 0).any(axis=0)).sum()),
        rewards_nonzero=int((out["lp_reward"] != 0).sum()),
    )
    need = ["both_actions", "refused_by_min_green", "pending_survives", "pending_overwritten", "fewer_than_four_neighbours",
            "table_switch", "rewards_nonzero"]
    if proto == A2C:
        st = out["lp_state"]
        assert not st[:, :, [4, 5, 9, 11]].any(), "a field nothing sets is not 0"
    else:
        st, nx, ex = out["lp_state"], out["lp_next_state"], out["lp_explore"]
        assert not st[:, :, 1:, 6].any() and not nx[:, :, 1:, 6].any(), "a neighbour's t_norm is not 0"
        local = -(st[:, :, 0, 0].astype(np.float64) + st[:, :, 0, 1])
        cov.update(
            explore_ticks=int(ex.sum()), exploit_ticks=int((ex == 0).sum()), randrange_rejections=int(out["lp_rejects"].sum()),
            q_ties_exploited=int(((out["lp_q"][:, :, 0] == out["lp_q"][:, :, 1]) & (ex == 0)).sum()),
            eps_reached_floor=bool((out["lp_eps"] == eps_min).any() and (out["lp_eps"][0] > 0.9).all()),
            next_differs_in_a_neighbours_phase=int((st[:, :, 1:, 4:6] != nx[:, :, 1:, 4:6]).any(axis=(2, 3)).sum()),
            absent_directions=int((out["lp_mask"][:, :, 1:] == 0).sum()),
            global_reward_term=int((out["lp_reward"] != local).sum()),
            stats_change=int((np.diff(out["lp_stats"], axis=0) != 0).any(axis=1).sum()))
        need += ["explore_ticks", "exploit_ticks", "q_ties_exploited", "eps_reached_floor", "next_differs_in_a_neighbours_phase",
                 "absent_directions", "global_reward_term"] + (["stats_change"] if spec.get("dta") else [])
        print(f"[{name}] randrange rejections: {cov['randrange_rejections']}")
    assert not Defaults.TRAFFIC_LIGHT_TRANSITION_DURATION_ENABLED and Defaults.TRAFFIC_LIGHT_TRANSITION_CLEARANCE_ENABLED
    print(f"[{name}] coverage {cov}")
    for k in need:
        # (an overwritten pending phase needs a group whose first phase is held back for five ticks: the three gated scenarios
        # have it, the one with the traffic generator on is not asked for it again)
        assert cov[k] or (k == "pending_overwritten" and spec.get("dta")), f"{name}: coverage condition {k} not met by this seed"
    path = os.path.join(HERE, f"trace_{name}.npz")
    mgl.write_npz(path, out)
    print(f"[{name}] protocol={proto} groups={act.shape[1]} ticks={T} size={os.path.getsize(path)}")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        for j in SCENARIOS:     # one process per scenario: the algorithm and the decay rate are read at import time
            subprocess.run([sys.executable, os.path.abspath(__file__), j], check=True, cwd="/tmp")
    else:
        run(what)


if __name__ == "__main__":
    main()
