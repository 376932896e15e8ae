#!/usr/bin/env python3
"""What the A2C and GAT-DQN light protocols cost: the reduced lights policy at 4096^2 / 10^6 vehicles, timed

  (a) per tick under FIXED_TIME on a library built from the parent commit (--parent-lib, optional) and on this one: the
      existing algorithms must sit inside the parent's own run-to-run spread;
  (b) observe + act per tick under each protocol, nothing brought to the host (to_host=False; a host action vector of G
      bytes up);
  (c) observe + act_q per tick under GAT-DQN with a host q of G x 2 floats, nothing brought down but the greedy bytes the
      engine itself needs; the epsilon-greedy part - k_lp_greedy, G bytes down, the sequential draw chain on the host, G
      action bytes and G epsilons up - is reported separately as act_q minus act, both measured as whole calls, with epsilon
      at 1.0 (every group explores: a random() and a randrange(2) with its rejections) and at 0 (a random() only);
  (d) the host route that (b) replaces: download the occupancy map and build the A2C vector / the GAT graph state with
      vectorised numpy, checked against the engine's output bit for bit.

The legs alternate inside every round (the two of (a) also swap places from round to round) on engines of their own (same
workload, same seeds), each warmed up before its timed window; medians and the spread (min .. max) over the rounds are reported.  No threshold is set.  Prints one JSON line and
writes it to profiles/lights_proto_probe.json (or --out).

    python profiles/lights_proto_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from lights_ext_probe import HostRoute, timed_ticks  # noqa: E402

ORDER = (0, 2, 1, 3)      # N, S, E, W as direction codes


class ProtoHostRoute(HostRoute):
    """The two state functions from a downloaded occupancy map, vectorised (tests/lights_proto_expect.py is the plain form)."""

    def sums(self, occ):
        flat = occ.ravel().astype(np.int64)
        return [self._segsum(flat[cells], off) for off, cells in self.lists]

    def tables_of(self, repop):
        nb = np.where(repop[:, None, None], self.nb["g_neighbors"], self.nb["g_neighbors_ctor"])
        return nb, (nb[:, :, 0] >= 0) & (nb[:, :, 1] >= 0)

    def a2c(self, occ, ctrl, repop):
        ns, ew = self.sums(occ)
        nb, valid = self.tables_of(repop)
        j = np.where(valid, nb[:, :, 1], 0)
        cnt = np.maximum(valid.sum(axis=1), 1).astype(np.float64)
        out = np.zeros((self.G, 13))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = ns, ew, ns - ew, ew - ns
        out[:, 6], out[:, 7] = ctrl[:, 0] == 0, ctrl[:, 0] != 0
        out[:, 8] = ctrl[:, 1] / 30.0
        out[:, 10] = self.pen
        pen_sum = np.zeros(self.G)
        for k in range(4):      # (slot order, like the reference's sum over the dict's values)
            pen_sum = pen_sum + np.where(valid[:, k], self.pen[j[:, k]], 0.0)
        out[:, 12] = pen_sum / cnt
        return out.astype(np.float32)

    def gat(self, occ, ctrl, repop):
        ns, ew = self.sums(occ)
        nb, valid = self.tables_of(repop)
        node = np.zeros((self.G, 9))
        node[:, 0], node[:, 1], node[:, 2], node[:, 3] = ns, ew, ns - ew, ew - ns
        node[:, 4], node[:, 5] = ctrl[:, 0] == 0, ctrl[:, 0] != 0
        node[:, 8] = self.pen
        feat = np.zeros((self.G, 5, 9))
        mask = np.zeros((self.G, 5))
        feat[:, 0] = node
        feat[:, 0, 6] = ctrl[:, 1] / 30.0
        mask[:, 0] = 1.0
        for d, code in enumerate(ORDER):
            n = np.full(self.G, -1, dtype=np.int64)
            for k in range(4):      # (a later entry of the same direction wins, like a dict)
                n = np.where(valid[:, k] & (nb[:, k, 0] == code), nb[:, k, 1], n)
            has = n >= 0
            feat[:, d + 1] = np.where(has[:, None], node[np.maximum(n, 0)], 0.0)
            mask[:, d + 1] = has
        return feat.astype(np.float32), mask.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=50, help="act / act_q calls per window of the draw-chain comparison")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg a)")
    ap.add_argument("--only-fixed", action="store_true", help="leg (a) alone: the FIXED_TIME comparison with the parent's library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights_proto_probe.json"))
    args = ap.parse_args()
    import bench
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    G = len(tables["g_light_off"]) - 1
    rng = np.random.default_rng(args.seed)
    n_ticks = args.warmup + args.steps
    actions = (rng.random((n_ticks, G)) < 0.3).astype(np.int8)
    qs = rng.normal(size=(n_ticks, G, 2)).astype(np.float32)
    legs = (["a_parent_fixed"] if args.parent_lib else []) + ["a_this_fixed"] + ([] if args.only_fixed else ["b_a2c", "b_gat", "c_gat_q"])
    ms = {leg: [] for leg in legs}
    control_ms = {leg: [] for leg in legs if leg[0] != "a"}
    host_ms = {"a2c": [], "gat": []}
    download_ms = []
    call_ms = {k: [] for k in ("act", "act_q_eps_1", "act_q_eps_0")}
    fp_fixed = {}

    def engine(lib, algo, proto=None, **cfg):
        api = capi.CApi(libs[lib], "ts_")
        bench.setup(api, tables, routes, args.seed, extra={"TRAFFIC_LIGHT_AGENT_ALGORITHM": algo}, policy="lights")
        if proto:
            api.lights_proto_config(proto, **cfg)
        return api

    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        # (the two FIXED_TIME legs swap places from round to round, so that neither always runs first)
        for leg in (legs if rnd % 2 == 0 or not args.parent_lib else [legs[1], legs[0]] + legs[2:]):
            if leg[0] == "a":
                api = engine("parent" if leg == "a_parent_fixed" else "this", "FIXED_TIME")
                api.step(args.warmup)
                ms[leg].append(timed_ticks(api, args.steps)[0])
                fp = (api.rng_fingerprint(capi.RNG_SCHEDULER), int(api.num_vehicles()), int(api.map(capi.MAP_OCCUPANCY).sum()),
                      int(api.map(capi.MAP_STOP).sum()))
                assert fp_fixed.setdefault("fp", fp) == fp, f"{leg}: the FIXED_TIME run differs between the libraries"
                api.close()
                continue
            proto = capi.LP_A2C if leg == "b_a2c" else capi.LP_GAT
            api = engine("this", "EXTERNAL", proto, eps_decay=0.01)

            def control(t, _api=api, base=0, _leg=leg):
                _api.lights_proto_observe(to_host=False)
                if _leg == "c_gat_q":
                    _api.lights_proto_act_q(qs[base + t], to_host=False)
                else:
                    _api.lights_proto_act(actions[base + t], to_host=False)
            for t in range(args.warmup):
                control(t)
                api.step(1)
            total, ctl = timed_ticks(api, args.steps, before=lambda t: control(t, base=args.warmup))
            ms[leg].append(total)
            control_ms[leg].append(ctl)
            if leg in ("b_a2c", "b_gat"):      # the host route next to the engine's own output, on the same maps
                host = ProtoHostRoute(tables)
                for t in range(3):
                    ctrl = api.lights_controller()
                    repop = np.asarray(api.groups()[:, 0] >= 0)      # (a group's links are re-populated by its first phase change)
                    t0 = time.perf_counter()
                    occ = api.map(capi.MAP_OCCUPANCY)
                    t1 = time.perf_counter()
                    want = host.a2c(occ, ctrl, repop) if leg == "b_a2c" else host.gat(occ, ctrl, repop)
                    t2 = time.perf_counter()
                    got = api.lights_proto_observe()
                    pairs = [(got, want)] if leg == "b_a2c" else list(zip(got, want))
                    assert all(g.tobytes() == w.tobytes() for g, w in pairs), f"{leg}: the host route and the engine disagree"
                    download_ms.append((t1 - t0) * 1e3)
                    host_ms[leg[2:]].append((t2 - t0) * 1e3)
                    api.lights_proto_act(actions[t], to_host=False)
                    api.step(1)
            api.close()
        # the epsilon-greedy part: whole calls on the same maps, act against act_q with every group exploring and with none
        for key, cfg in () if args.only_fixed else (("act", {}), ("act_q_eps_1", dict(eps_min=1.0, eps_decay=0.0)), ("act_q_eps_0", dict(eps_min=0.0, eps_decay=1.0))):
            api = engine("this", "EXTERNAL", capi.LP_GAT, **cfg)
            api.step(2)
            for t in range(3):      # (under eps_decay = 1 the first call takes epsilon from 1.0 to 0)
                api.lights_proto_act_q(qs[t], to_host=False) if key != "act" else api.lights_proto_act(actions[t], to_host=False)
            t0 = time.perf_counter()
            for t in range(args.calls):
                if key == "act":
                    api.lights_proto_act(actions[t % n_ticks], to_host=False)
                else:
                    api.lights_proto_act_q(qs[t % n_ticks], to_host=False)
            call_ms[key].append((time.perf_counter() - t0) * 1e3 / args.calls)
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    med = {k: statistics.median(v) if v else None for k, v in call_ms.items()}
    rec = dict(probe="lights_proto", size=args.size, vehicles=args.vehicles, policy="lights (reduced)", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, calls_per_window=args.calls, groups=G,
               ms_per_tick={leg: summary(v) for leg, v in ms.items()},
               observe_plus_act_ms={leg: summary(v) for leg, v in control_ms.items()},
               d_host_route_ms={k: summary(v) for k, v in host_ms.items()}, d_of_which_map_download_ms=summary(download_ms),
               whole_call_ms={k: summary(v) for k, v in call_ms.items()},
               draw_chain_ms=dict(every_group_explores=round(med["act_q_eps_1"] - med["act"], 4) if med["act"] is not None else None,
                                  no_group_explores=round(med["act_q_eps_0"] - med["act"], 4) if med["act"] is not None else None,
                                  what="act_q minus act as whole calls: k_lp_greedy, G bytes down, the host's draws, G action bytes and "
                                       "G epsilons up, the upload of q (G x 2 floats) included"))
    if args.parent_lib:
        a, b = ms["a_parent_fixed"], statistics.median(ms["a_this_fixed"])
        rec["fixed_this_minus_parent_ms"] = round(b - statistics.median(a), 4)
        rec["parent_spread_ms"] = round(max(a) - min(a), 4)
        rec["fixed_within_parent_spread"] = bool(min(a) <= b <= max(a))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
