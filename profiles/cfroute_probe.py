#!/usr/bin/env python3
"""What routes along a cost field cost: the config-2 world at 4096^2 / 10^6 vehicles and the edge-seed TO field of
costfield_probe.py (soft), timed

  (a) ts_cfroute_compute against ts_costfield_compute on the same query, alternating inside every round with the two
      swapping places: the difference is the price of the hop kernel and of the planes that stay for walking;
  (b) ts_cfroute_trace and ts_cfroute_load with all live vehicles as starts, each held with its heading, and what they
      produced (steps, the longest route, starts without one, bytes);
  (c) the route they replace: ts_astar_batch from a sample of those starts to their owner seeds, scaled by live vehicles /
      sample - an EXTRAPOLATION.  The sample starts at --sample and is cut down when a pilot of 50 queries says it would take
      more than --astar-seconds.  Every sampled A* path is priced under the step rule (costfield_probe.path_costs) and
      checked against the cost of the same start's route traced without a heading (a search has none): never cheaper;
  (d) per tick with the feature never used, on a library built from the parent commit (--parent-lib, optional) and on this
      one, alternating inside every round with the legs swapping places: "unused" must sit inside the parent's own spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Medians
and the spread (min .. max) over the rounds are reported; the first compute of every engine is a warm-up.  No time was fixed
in advance.  Prints one JSON line and writes it to profiles/cfroute_probe.json (or --out).

    python profiles/cfroute_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--astar-seconds", type=float, default=20.0, help="what the sampled A* batch of one round may take")
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfroute_probe.json"))
    args = ap.parse_args()
    import bench
    from costfield_probe import path_costs, timed_ticks
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    W, H = int(tables["width"]), int(tables["height"])
    road_map = np.asarray(tables["is_road_map"])
    road = np.argwhere(road_map == 1)[:, ::-1].astype(np.int32)
    if "highway_exits_xy" in tables and len(tables["highway_exits_xy"]):
        exits, exits_are = np.asarray(tables["highway_exits_xy"], dtype=np.int32).reshape(-1, 2), "highway exits"
    else:
        edge = (road[:, 0] == 0) | (road[:, 1] == 0) | (road[:, 0] == W - 1) | (road[:, 1] == H - 1)
        exits, exits_are = road[edge], "road cells on the map's edge (the synthetic world has no highway exits)"
    if len(exits) == 0:
        exits, exits_are = road[:: max(len(road) // 64, 1)][:64], "64 road cells spread over the map (no road reaches the edge)"
    q = dict(mode="to", soft=True)
    ms = {k: [] for k in ("costfield_compute", "cfroute_compute", "trace", "load", "read_routes")}
    astar = dict(ms_extrapolated=[], ms_sample=[], sample=[], found=[], equal=[], route_less=[])
    tick = {k: [] for k in (["d_parent"] if args.parent_lib else []) + ["d_this_cfroute_unused"]}
    facts = {}
    f = capi.V_FIELDS.index
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        legs = list(tick)
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):          # the legs swap places from round to round
            api = capi.CApi(libs["parent" if leg == "d_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            tick[leg].append(timed_ticks(api, args.steps))
            if leg == "d_parent":
                api.close()
                continue
            # (a) the two computes, on the engine that just ran "unused" (its tick window is over)
            cf, r = api.costfield, api.costfield.routes
            r.compute(exits, **q)                                      # warm-up
            for name in (("costfield_compute", "cfroute_compute") if rnd % 2 == 0 else ("cfroute_compute", "costfield_compute")):
                t, info = timed(lambda: (cf if name == "costfield_compute" else r).compute(exits, **q))
                ms[name].append(t)
            if not r.info()["held"]:
                info = r.compute(exits, **q)
            # (b) all live vehicles, with their headings
            rows = api.vehicles()
            starts = np.ascontiguousarray(rows[:, [f("x"), f("y")]], dtype=np.int32)
            heads = np.maximum(rows[:, f("direction")], -1).astype(np.int8)
            t, batch = timed(lambda: r.trace(starts, heads))
            ms["trace"].append(t)
            t, (off, dirs, cost, owner) = timed(r.routes)
            ms["read_routes"].append(t)
            t, load = timed(lambda: r.load(starts, heads))
            ms["load"].append(t)
            assert load["steps"] == batch["steps"] and load["unreached"] == batch["unreached"]
            ri = r.info()
            # (c) the sampled A* batch: start -> owner seed, soft, with the flow; the same starts traced without a heading
            rng = np.random.default_rng(args.seed + rnd)
            has_route = np.flatnonzero(owner >= 0)
            pick = has_route[rng.choice(len(has_route), size=min(args.sample, len(has_route)), replace=False)]
            qs = lambda idx: [(int(starts[i, 0]), int(starts[i, 1]), int(exits[owner[i], 0]), int(exits[owner[i], 1]), 1, 0, 0x7FFFFFFF) for i in idx]
            t_pilot, _ = timed(lambda: api.astar_batch(qs(pick[:50])))
            n = int(max(50, min(len(pick), args.astar_seconds * 1e3 / max(t_pilot / 50, 1e-3))))
            pick = pick[:n]
            t_batch, (a_off, a_xy) = timed(lambda: api.astar_batch(qs(pick)))
            r.trace(starts[pick])
            _, _, free_cost, free_owner = r.routes()
            p = api.params_from_defaults(bench.POLICY)
            maps = (np.asarray(tables["allowed_dirs_map"]), road_map, np.asarray(tables["road_type_map"]),
                    api.map(capi.MAP_OCCUPANCY), api.map(capi.MAP_STOP), api.density())
            a_cost = path_costs(p, maps, a_off, a_xy, starts[pick].astype(np.int64))
            has = a_cost >= 0
            at_seed = (starts[pick] == exits[owner[pick]]).all(axis=1)
            assert (free_owner >= 0).all(), "a start with a route under its heading has none without"
            # the search goes to the owner under the vehicle's heading; without one the nearest seed may be another: no dearer
            assert (free_cost[has].astype(np.int64) <= a_cost[has]).all(), "an A* path is cheaper than the route"
            astar["ms_sample"].append(t_batch)
            astar["ms_extrapolated"].append(t_batch * len(starts) / n)
            astar["sample"].append(n)
            astar["found"].append(int(has.sum()))
            astar["equal"].append(int((free_cost[has] == a_cost[has]).sum()))
            astar["route_less"].append(int((free_cost[has] < a_cost[has]).sum()))
            facts = dict(road_cells=int(len(road)), exits=int(len(exits)), exits_are=exits_are, live_vehicles=int(len(starts)),
                         tick=info["tick"], headings=info["headings"], starts_on_their_seed=int(at_seed.sum()),
                         routes=int(batch["n"] - batch["unreached"]), unreached=int(batch["unreached"]), steps=int(batch["steps"]),
                         longest=int(batch["longest"]), batch_bytes=int(batch["device_bytes"]), load_bytes=int(load["device_bytes"]),
                         walk_bytes=int(ri["device_bytes"]), field_bytes=int(info["device_bytes"]),
                         label_bytes=info["headings"] * W * H * 8 + (W * H * 8 if info["headings"] == 4 else 0))
            r.release()
            cf.release()
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    hop = [b - a for a, b in zip(ms["costfield_compute"], ms["cfroute_compute"])]
    routed = statistics.median(ms["trace"])
    rec = dict(probe="cfroute", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, query="TO, soft, all exits", state=facts, ms={k: summary(v) for k, v in ms.items()},
               hop_plane_ms=summary(hop),
               astar_batch=dict(note="ms_extrapolated = ms_sample * live vehicles / sample: an EXTRAPOLATION", ms_sample=summary(astar["ms_sample"]),
                                ms_extrapolated=summary(astar["ms_extrapolated"]), sample=astar["sample"], found=astar["found"],
                                equal_to_route=astar["equal"], route_less=astar["route_less"], route_more=[0] * len(astar["sample"]),
                                extrapolated_over_trace=round(statistics.median(astar["ms_extrapolated"]) / routed, 1)),
               ms_per_tick={k: summary(v) for k, v in tick.items()})
    if args.parent_lib:
        p, t = tick["d_parent"], statistics.median(tick["d_this_cfroute_unused"])
        rec["unused_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["unused_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
