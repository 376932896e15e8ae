#!/usr/bin/env python3
"""What select-link analysis costs: the config-2 world at 4096^2 / 10^6 vehicles, timed

  (a) ts_selectlink_set_gates + ts_selectlink_compute (1, 1, 1) for 32 gates of 64 cells each, taken from the 2048 most loaded
      cells of a whole-path demand plane (stable sort, gate g = cells 64 g .. 64 g + 63, open to all directions), and the compute
      alone with the gates held;
  (b) ts_selectlink_select, ts_selectlink_od (7 random zones) and the select-link load - ts_demand_compute (1, 1, 1) with the
      select bytes from the host - for the selection any = gate 0;
  (c) ts_demand_compute (1, 1, 1) on the same state in the same call: the comparator, the same walk with an atomic per step where
      the select-link walk has a load.  No ratio is fixed in advance: both are recorded with the way it came out;
  (d) the compute for every team size (8 / 16 / 32 / 64 lanes per vehicle, TS_DEBUG_SELECTLINK_TEAM) and 1 / 2 / 4 / 8 path steps
      per lane and iteration (TS_DEBUG_SELECTLINK_CHUNK = team x steps per lane), and at the library's defaults;
  (e) the host route it replaces: ts_download_path for a random sample of vehicles plus the rule in numpy, checked against the
      engine's per-vehicle values, scaled by live vehicles / sample - an EXTRAPOLATION;
  (f) per tick with the feature never used, on a library built from the parent commit (--parent-lib, optional) and on this one,
      alternating inside every round with the legs swapping places: "unused" must sit inside the parent's own spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Each leg
is warmed up; medians and the spread (min .. max) over the rounds are reported.  Prints one JSON line and writes it to
profiles/selectlink_probe.json (or --out).

    python profiles/selectlink_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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

TEAMS, SPL = (8, 16, 32, 64), (1, 2, 4, 8)
N_GATES, GATE_CELLS = 32, 64


def timed(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n


def timed_ticks(api, steps):
    api.counters()
    t0 = time.perf_counter()
    api.step(steps)
    api.counters()
    return (time.perf_counter() - t0) * 1e3 / steps


def shape_env(team, chunk):
    for key, v in (("TS_DEBUG_SELECTLINK_TEAM", team), ("TS_DEBUG_SELECTLINK_CHUNK", chunk)):
        if v is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = str(v)


def host_route(api, capi, sample, gate_of, n_gates):
    """download_path of the sampled rows and the rule per vehicle: (mask, crossings, first_step, first_gate) of the sample."""
    V = {n: i for i, n in enumerate(capi.V_FIELDS)}
    t0 = time.perf_counter()
    rows = api.vehicles()
    out = np.zeros((len(sample), 4), dtype=np.int64)
    for j, k in enumerate(sample):
        cells = api.path(int(k)).astype(np.int64).reshape(-1, 2)
        out[j] = (0, 0, -1, -1)
        if len(cells) == 0:
            continue
        g = gate_of[cells[:, 1], cells[:, 0]]          # (every gate is open to all directions: the step's direction does not matter)
        hit = np.nonzero(g >= 0)[0]
        if len(hit):
            out[j] = (int(np.bitwise_or.reduce(1 << g[hit].astype(np.int64))), len(hit), int(hit[0]), int(g[hit[0]]))
    return out, rows, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg f)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selectlink_probe.json"))
    args = ap.parse_args()
    import bench
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    W, H = int(tables["width"]), int(tables["height"])
    shapes = [(t, t * s) for t in TEAMS for s in SPL] + [(None, None)]
    ms = {f"team{t}_chunk{c}" if t else "default": [] for t, c in shapes}
    legs_ms = {k: [] for k in ("set_gates_and_compute", "compute", "select", "od", "select_link_load", "demand_compute_1x1")}
    host_ms, tick = [], {k: [] for k in (["f_parent"] if args.parent_lib else []) + ["f_this_selectlink_unused"]}
    facts = {}
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        legs = list(tick)
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):          # the legs swap places from round to round
            api = capi.CApi(libs["parent" if leg == "f_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            tick[leg].append(timed_ticks(api, args.steps))
            if leg == "f_parent":
                api.close()
                continue
            sl = api.selectlink
            whole = api.demand_compute(1, 1, True)
            load = api.demand_plane(0)
            order = np.argsort(-load.astype(np.int64).ravel(), kind="stable")[:N_GATES * GATE_CELLS]
            gates = [[(int(i % W), int(i // W)) for i in order[g * GATE_CELLS:(g + 1) * GATE_CELLS]] for g in range(N_GATES)]
            gate_of = np.full((H, W), -1, dtype=np.int8)
            for g, gate in enumerate(gates):
                for x, y in gate:
                    gate_of[y, x] = g

            def both():
                sl.set_gates(gates)
                sl.compute(1, 1, True)
            both()
            legs_ms["set_gates_and_compute"].append(timed(both, args.calls))
            legs_ms["compute"].append(timed(lambda: sl.compute(1, 1, True), args.calls))
            legs_ms["demand_compute_1x1"].append(timed(lambda: api.demand_compute(1, 1, True), args.calls))
            for t, c in shapes:
                shape_env(t, c)
                sl.compute(1, 1, True)
                ms[f"team{t}_chunk{c}" if t else "default"].append(timed(lambda: sl.compute(1, 1, True), args.calls))
            shape_env(None, None)
            info = sl.compute(1, 1, True)
            zones = np.random.default_rng(args.seed).integers(0, 7, (H, W)).astype(np.int32)
            sl.set_zones(zones, 7)
            sel, count = sl.select(any=1)
            legs_ms["select"].append(timed(lambda: sl.select(any=1), args.calls))
            legs_ms["od"].append(timed(lambda: sl.od(any=1), args.calls))
            legs_ms["select_link_load"].append(timed(lambda: api.demand_compute(1, 1, True, select=sel), args.calls))
            cross, _ = sl.tables()
            assert info["vehicles"] == whole["vehicles"] and int(cross.sum()) == info["crossings"] == int(load.ravel()[order].sum())
            facts = dict(live_vehicles=info["vehicles"], steps=whole["steps"], crossing_vehicles=info["crossing"], crossings=info["crossings"],
                         selected_by_gate_0=count, gate_cells=N_GATES * GATE_CELLS, tick=info["tick"])
            n_live = api.num_vehicles()
            sample = np.sort(np.random.default_rng(args.seed + rnd).choice(n_live, size=min(args.sample, n_live), replace=False))
            want, rows, t_host = host_route(api, capi, sample, gate_of, N_GATES)
            got = sl.vehicles()[rows[sample, capi.V_FIELDS.index("spawn_idx")]]
            assert np.array_equal(got["mask"].astype(np.int64), want[:, 0]) and np.array_equal(got["crossings"].astype(np.int64), want[:, 1]) \
                and np.array_equal(got["first_step"], want[:, 2]) and np.array_equal(got["first_gate"], want[:, 3]), \
                "the host route and the engine disagree on the sample"
            host_ms.append(t_host * n_live / len(sample))
            sl.release()
            api.demand_release()
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    med = {k: statistics.median(v) for k, v in ms.items()}
    walk, demand = statistics.median(legs_ms["compute"]), statistics.median(legs_ms["demand_compute_1x1"])
    rec = dict(probe="selectlink", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, calls_per_window=args.calls,
               warmup=args.warmup, rounds=args.rounds, gates=N_GATES, cells_per_gate=GATE_CELLS, state=facts,
               ms_per_call={k: summary(v) for k, v in legs_ms.items()},
               compute_over_demand_compute=round(walk / demand, 3),
               which_way="the select-link walk is the faster one" if walk < demand else "the demand walk is the faster one",
               ms_per_compute_by_shape={k: summary(v) for k, v in ms.items()}, best_shape=min((k for k in med if k != "default"), key=lambda k: med[k]),
               host_route_ms_extrapolated=summary(host_ms), host_route_sample=args.sample,
               host_route_over_compute=round(statistics.median(host_ms) / walk, 1),
               ms_per_tick={k: summary(v) for k, v in tick.items()})
    if args.parent_lib:
        p, t = tick["f_parent"], statistics.median(tick["f_this_selectlink_unused"])
        rec["unused_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["unused_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
