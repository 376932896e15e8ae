#!/usr/bin/env python3
"""What the planned load costs: the config-2 world at 4096^2 / 10^6 vehicles, timed

  (a) ts_demand_compute for (n_bins, bin_cells, open_tail) = (1, 1, 1) and (4, 64, 1), for every team size (8 / 16 / 32 / 64
      lanes per vehicle, TS_DEBUG_DEMAND_TEAM) and 1 / 2 / 4 / 8 path steps per lane and iteration (TS_DEBUG_DEMAND_CHUNK =
      team x steps per lane), and at the library's defaults.  A timed call reuses the planes of the call before it: zero the
      planes, the walk kernel, the totals back, synchronise;
  (b) the host route it replaces: ts_download_path for a random sample of vehicles plus np.add.at, scaled by live vehicles /
      sample - an EXTRAPOLATION, nobody would wait for the real thing.  The sample is checked against the engine's planes
      computed with the same vehicles as `select`;
  (c) per tick with the feature never used, on a library built from the parent commit (--parent-lib, optional) and on this
      one, alternating inside every round with the legs swapping places: "unused" must sit inside the parent's own spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Each
leg is warmed up; medians and the spread (min .. max) over the rounds are reported.  From the shapes: a step is one 4-byte
atomic, a path of n remaining steps spans at least ceil(n / 16) pool words (read twice, the second time from cache), the
planes are zeroed once (n_bins * 4 * N * 4 bytes).  The figures over the call's time are rates of the whole call; no bound
of the hardware is claimed.  Prints one JSON line and writes it to profiles/demand_probe.json (or --out).

    python profiles/demand_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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

QUERIES = {"whole_path_1x1": (1, 1, True), "bins_4x64": (4, 64, True)}
TEAMS, SPL = (8, 16, 32, 64), (1, 2, 4, 8)      # lanes per vehicle x path steps per lane and iteration (chunk = team * spl)


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
    for key, v in (("TS_DEBUG_DEMAND_TEAM", team), ("TS_DEBUG_DEMAND_CHUNK", chunk)):
        if v is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = str(v)


def host_route(api, capi, sample, W, H):
    """download_path of the sampled rows and one np.add.at per vehicle: the (4, H, W) whole-path planes of the sample."""
    V = {n: i for i, n in enumerate(capi.V_FIELDS)}
    t0 = time.perf_counter()
    rows = api.vehicles()
    out = np.zeros((4, H, W), dtype=np.uint32)
    for k in sample:
        cells = api.path(int(k)).astype(np.int64).reshape(-1, 2)
        if len(cells) == 0:
            continue
        prev = np.vstack([[[rows[k, V["x"]], rows[k, V["y"]]]], cells[:-1]])
        dx, dy = cells[:, 0] - prev[:, 0], cells[:, 1] - prev[:, 1]
        d = np.where(dy == 1, 0, np.where(dx == 1, 1, np.where(dy == -1, 2, 3)))
        np.add.at(out, (d, cells[:, 1], cells[:, 0]), 1)
    return out, rows, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5, help="computes per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demand_probe.json"))
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
    ms = {q: {f"team{t}_chunk{c}" if t else "default": [] for t, c in shapes} for q in QUERIES}
    host_ms, tick = [], {k: [] for k in (["c_parent"] if args.parent_lib else []) + ["c_this_demand_unused"]}
    facts = {}
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        legs = list(tick)
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):          # the legs swap places from round to round
            api = capi.CApi(libs["parent" if leg == "c_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            tick[leg].append(timed_ticks(api, args.steps))
            if leg == "c_parent":
                api.close()
                continue
            # the computes, on the engine that just ran "unused" (its tick window is over)
            for q, query in QUERIES.items():
                for t, c in shapes:
                    shape_env(t, c)
                    api.demand_compute(*query)
                    ms[q][f"team{t}_chunk{c}" if t else "default"].append(timed(lambda: api.demand_compute(*query), args.calls))
            shape_env(None, None)
            info = api.demand_compute(1, 1, True)
            rows = api.vehicles()
            remaining = rows[:, capi.V_FIELDS.index("path_len")].astype(np.int64)
            assert info["steps"] == int(remaining.sum()) and info["vehicles"] == len(rows)
            facts = dict(live_vehicles=len(rows), steps=info["steps"], mean_remaining=round(float(remaining.mean()), 1),
                         max_remaining=int(remaining.max()), pool_bytes_min=int(((remaining + 15) // 16).sum()) * 4,
                         atomic_bytes=info["steps"] * 4, tick=info["tick"])
            sample = np.sort(np.random.default_rng(args.seed + rnd).choice(len(rows), size=min(args.sample, len(rows)), replace=False))
            planes, rows, t_host = host_route(api, capi, sample, W, H)
            select = np.zeros(api.num_spawned(), dtype=np.uint8)
            select[rows[sample, capi.V_FIELDS.index("spawn_idx")]] = 1
            got = api.demand_compute(1, 1, True, select=select)
            assert got["vehicles"] == len(sample) and got["steps"] == int(planes.sum())
            for d in range(4):
                assert np.array_equal(api.demand_plane(0, d), planes[d]), "the host route and the engine disagree on the sample"
            host_ms.append(t_host * len(rows) / len(sample))
            api.demand_release()
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    med = {q: {k: statistics.median(v) for k, v in legs.items()} for q, legs in ms.items()}
    best = {q: min((k for k in m if k != "default"), key=lambda k: m[k]) for q, m in med.items()}
    N = W * H
    rec = dict(probe="demand", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, calls_per_window=args.calls,
               warmup=args.warmup, rounds=args.rounds, state=facts,
               ms_per_compute={q: {k: summary(v) for k, v in legs.items()} for q, legs in ms.items()}, best_shape=best,
               default_steps_per_second={q: round(facts["steps"] / med[q]["default"] * 1e3) for q in QUERIES},
               default_bytes_from_shapes_over_call_time_GBps={
                   q: round((facts["pool_bytes_min"] + facts["atomic_bytes"] + QUERIES[q][0] * 4 * N * 4) / med[q]["default"] / 1e6, 1) for q in QUERIES},
               host_route_ms_extrapolated=summary(host_ms), host_route_sample=args.sample,
               host_route_over_default=round(statistics.median(host_ms) / med["whole_path_1x1"]["default"], 1),
               ms_per_tick={k: summary(v) for k, v in tick.items()})
    if args.parent_lib:
        p, t = tick["c_parent"], statistics.median(tick["c_this_demand_unused"])
        rec["unused_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["unused_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
