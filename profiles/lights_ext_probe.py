#!/usr/bin/env python3
"""What external light control costs: the reduced lights policy at 4096^2 / 10^6 vehicles, timed

  (a) per tick under FIXED_TIME on a library built from the parent commit (--parent-lib, optional) and on this one: the
      existing algorithms must sit inside the parent's own run-to-run spread;
  (b) observe + act per tick under EXTERNAL (one call each, a host action vector of G bytes up, nothing down); and observe
      alone with the sums pass at 4, 8, 16 and 32 lanes per group, as the time of a whole call (three launches and a
      synchronise), which is what a caller pays - not the kernel's own time;
  (c) the host route that (b) replaces: download the occupancy and stuck maps and evaluate the state vector with numpy
      (vectorised: np.add.reduceat over the gathered approach cells, the neighbour means by fancy indexing), checked
      against the engine's vector bit for bit.

The legs alternate inside every round on engines of their own (same workload, same seeds), each warmed up before its timed
window; medians and the spread (min .. max) over the rounds are reported.  No threshold is set.  Prints one JSON line and
writes it to profiles/lights_ext_probe.json (or --out).

    python profiles/lights_ext_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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
DIM = 13


def timed_ticks(api, steps, before=None):
    """ms per tick over `steps` ticks, and of them the ms spent in `before`; the window ends in a device synchronise."""
    api.counters()
    t0 = time.perf_counter()
    ctl = 0.0
    for t in range(steps):
        if before:
            c0 = time.perf_counter()
            before(t)
            ctl += time.perf_counter() - c0
        api.step(1)
    api.counters()
    return (time.perf_counter() - t0) * 1e3 / steps, ctl * 1e3 / steps


class HostRoute:
    """Phase A of the state vector at 13 dimensions from downloaded maps, vectorised (tests/lights_ext_expect.py is the plain
    form).  The stored pressures live here, as they would in a host-side controller."""

    def __init__(self, tables, penalties=(0.5, 5, 50.0)):
        W = int(tables["width"])
        self.G = len(tables["g_ns_in_off"]) - 1
        self.lists = []
        for nm in ("ns_in", "ew_in"):
            off = np.asarray(tables[f"g_{nm}_off"]).astype(np.int64)
            xy = np.asarray(tables[f"g_{nm}_xy"]).reshape(-1, 2).astype(np.int64)
            self.lists.append((off, xy[:, 1] * W + xy[:, 0]))
        rt = np.asarray(tables["road_type_map"]).ravel()
        w = np.asarray((0.0,) + tuple(penalties))
        tot, n = np.zeros(self.G), np.zeros(self.G)
        for nm in ("ns_in", "ns_out", "ew_in", "ew_out"):
            off = np.asarray(tables[f"g_{nm}_off"]).astype(np.int64)
            xy = np.asarray(tables[f"g_{nm}_xy"]).reshape(-1, 2).astype(np.int64)
            tot += self._segsum(w[rt[xy[:, 1] * W + xy[:, 0]]], off)
            n += np.diff(off)
        self.pen = np.where(n > 0, tot / np.maximum(n, 1), 0.0)
        self.nb = {k: np.asarray(tables[k]).reshape(self.G, 4, 2) for k in ("g_neighbors", "g_neighbors_ctor")}
        self.stored = None

    @staticmethod
    def _segsum(v, off):
        out = np.zeros(len(off) - 1, dtype=v.dtype)
        nz = np.diff(off) > 0
        if len(v):
            out[nz] = np.add.reduceat(v, off[:-1][nz])
        return out

    def state(self, occ, stuck, ctrl, repop):
        flat = occ.ravel().astype(np.int64)
        ns, ew = (self._segsum(flat[cells], off) for off, cells in self.lists)
        p = ns - ew
        if self.stored is None:
            self.stored = p.copy()
        nb = np.where(repop[:, None, None], self.nb["g_neighbors"], self.nb["g_neighbors_ctor"])
        valid = (nb[:, :, 0] >= 0) & (nb[:, :, 1] >= 0)
        j = np.where(valid, nb[:, :, 1], 0)
        cnt = np.maximum(valid.sum(axis=1), 1).astype(np.float64)
        earlier = j < np.arange(self.G)[:, None]
        pj = np.where(earlier, p[j], self.stored[j]) * valid
        out = np.zeros((self.G, DIM))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = ns, ew, p, -p
        out[:, 4], out[:, 5] = ctrl[:, 0] == 0, ctrl[:, 0] != 0
        out[:, 6] = ctrl[:, 1] / 30.0
        out[:, 8] = self.pen
        pen_sum = np.zeros(self.G)
        for k in range(4):      # (slot order, like the reference's sum over the dict's values)
            pen_sum = pen_sum + np.where(valid[:, k], self.pen[j[:, k]], 0.0)
        out[:, 10] = pen_sum / cnt
        out[:, 11], out[:, 12] = pj.sum(axis=1) / cnt, (-pj).sum(axis=1) / cnt
        self.stored = p.copy()
        return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--observes", type=int, default=500, help="observe calls per window of the lanes-per-group comparison")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights_ext_probe.json"))
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
    actions = (rng.random((args.warmup + args.steps, G)) < 0.3).astype(np.int8)
    legs = (["a_parent_fixed"] if args.parent_lib else []) + ["a_this_fixed", "b_external"]
    ms = {leg: [] for leg in legs}
    control_ms, host_ms, host_download_ms, team_ms = [], [], [], {t: [] for t in (4, 8, 16, 32)}
    fp_fixed = {}
    longest = max(int(np.diff(tables[f"g_{nm}_off"]).max()) for nm in ("ns_in", "ew_in"))
    mean_len = float(np.mean([np.diff(tables[f"g_{nm}_off"]).mean() for nm in ("ns_in", "ew_in")]))
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        for leg in legs:
            api = capi.CApi(libs["parent" if leg == "a_parent_fixed" else "this"], "ts_")
            algo = "EXTERNAL" if leg == "b_external" else "FIXED_TIME"
            bench.setup(api, tables, routes, args.seed, extra={"TRAFFIC_LIGHT_AGENT_ALGORITHM": algo}, policy="lights")
            if leg != "b_external":
                api.step(args.warmup)
                ms[leg].append(timed_ticks(api, args.steps)[0])
                fp = (api.rng_fingerprint(capi.RNG_SCHEDULER), int(api.num_vehicles()), int(api.map(capi.MAP_OCCUPANCY).sum()),
                      int(api.map(capi.MAP_STOP).sum()))
                assert fp_fixed.setdefault("fp", fp) == fp, f"{leg}: the FIXED_TIME run differs between the libraries"
                api.close()
                continue
            host = HostRoute(tables)

            def control(t, _api=api, base=0):
                _api.lights_observe(to_host=False)
                _api.lights_act(actions[base + t], want_next=False)
            for t in range(args.warmup):
                control(t)
                api.step(1)
            # the host route next to the engine's own vector, on the same maps (untimed bookkeeping: controller rows, links)
            host.stored = None
            total, ctl = timed_ticks(api, args.steps, before=lambda t: control(t, base=args.warmup))
            ms[leg].append(total)
            control_ms.append(ctl)
            for t in range(3):
                ctrl = api.lights_controller()
                repop = np.asarray(api.groups()[:, 0] >= 0)      # (a group's links are re-populated by its first phase change)
                t0 = time.perf_counter()
                occ, stuck = api.map(capi.MAP_OCCUPANCY), api.map(capi.MAP_STUCK)
                t1 = time.perf_counter()
                want = host.state(occ, stuck, ctrl, repop)
                t2 = time.perf_counter()
                got = api.lights_observe()
                if t:       # (the host route's stored pressures start at its first call: compare from the second on)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the host route and the engine disagree"
                    host_download_ms.append((t1 - t0) * 1e3)
                    host_ms.append((t2 - t0) * 1e3)
                api.lights_act(actions[t], want_next=False)
                api.step(1)
            api.close()
        # lanes per group of the sums pass: observe alone, on engines of their own
        for team in team_ms:
            os.environ["TS_DEBUG_LIGHTS_TEAM"] = str(team)
            api = capi.CApi(libs["this"], "ts_")
            bench.setup(api, tables, routes, args.seed, extra={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL"}, policy="lights")
            api.step(2)
            for t in range(3):
                api.lights_observe(to_host=False)
                api.step(1)
            # phase A again and again on the same maps (an act with all-zero actions in between ends the cached observe; it is
            # not timed): args.observes calls per window, each ending in its own synchronise
            t_obs = 0.0
            zeros = np.zeros(G, np.int8)
            for t in range(args.observes):
                t0 = time.perf_counter()
                api.lights_observe(to_host=False)
                t_obs += time.perf_counter() - t0
                api.lights_act(zeros, want_next=False)
            team_ms[team].append(t_obs * 1e3 / args.observes)
            api.close()
        os.environ.pop("TS_DEBUG_LIGHTS_TEAM", None)

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    rec = dict(probe="lights_ext", size=args.size, vehicles=args.vehicles, policy="lights (reduced)", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, observes_per_window=args.observes, groups=G, state_dim=DIM, longest_approach_list=longest, mean_approach_list=round(mean_len, 2),
               ms_per_tick={leg: summary(v) for leg, v in ms.items()},
               b_observe_plus_act_ms=summary(control_ms),
               c_host_route_ms=summary(host_ms), c_of_which_two_map_downloads_ms=summary(host_download_ms),
               observe_ms_by_lanes_per_group={str(t): summary(v) for t, v in team_ms.items()})
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
