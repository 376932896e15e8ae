#!/usr/bin/env python3
"""What a cost field costs: the config-2 world at 4096^2 / 10^6 vehicles, timed

  (a) ts_costfield_compute in TO mode from one seed (the road cell nearest the map's centre) and from all "exits" (the
      world's highway exits where its tables have them, else its road cells on the map's edge), free-flow, soft and strict,
      at tiles 16 and 32 (TS_DEBUG_COSTFIELD_TILE), with the rounds and tile visits each took beside the times;
  (b) the route it replaces: ts_astar_batch from a random sample of road cells to the same single seed (soft), scaled by
      road cells / sample - an EXTRAPOLATION, nobody would wait for the real thing.  The sample starts at --sample and is
      cut down when a pilot of 50 queries says the whole of it would take more than --astar-seconds; the size used is
      recorded.  Every sampled path is priced under the step rule (numpy, here) and checked against the field at its start:
      never below the field, equal to it where turns cost nothing;
  (c) per tick with the feature never used, on a library built from the parent commit (--parent-lib, optional) and on this
      one, alternating inside every round with the legs swapping places: "unused" must sit inside the parent's own spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Medians
and the spread (min .. max) over the rounds are reported; the first compute of every engine is a warm-up.  No time was fixed
in advance.  Prints one JSON line and writes it to profiles/costfield_probe.json (or --out).

    python profiles/costfield_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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

MODES = {"free_flow": dict(free_flow=True), "soft": dict(soft=True), "strict": dict(soft=False)}
TILES = (16, 32)
DX, DY = np.array([0, 1, 0, -1]), np.array([1, 0, -1, 0])


def timed_ticks(api, steps):
    api.counters()
    t0 = time.perf_counter()
    api.step(steps)
    api.counters()
    return (time.perf_counter() - t0) * 1e3 / steps


def path_costs(p, maps, off, xy, starts):
    """The cost under the step rule (soft, with the flow) of every path of the CSR (off, xy), the start cell in front."""
    allowed, road, rtype, occ, stop, dens = maps
    rt = np.array([0.0, p.road_type_penalty_r1, p.road_type_penalty_r2, p.road_type_penalty_r3])
    out = np.full(len(off) - 1, -1, dtype=np.int64)
    for i in range(len(off) - 1):
        cells = xy[off[i]:off[i + 1]].astype(np.int64)
        if len(cells) == 0:
            continue
        if tuple(cells[0]) != tuple(starts[i]):
            cells = np.vstack([starts[i][None, :], cells])
        u, v = cells[:-1], cells[1:]
        d = np.where(v[:, 1] - u[:, 1] == 1, 0, np.where(v[:, 0] - u[:, 0] == 1, 1, np.where(v[:, 1] - u[:, 1] == -1, 2, 3)))
        assert np.array_equal(u + np.stack([DX[d], DY[d]], axis=1), v), "a path that does not step to a neighbour"
        assert ((allowed[u[:, 1], u[:, 0]] >> d) & 1).all(), "a path against the flow"
        c = np.ones(len(d))
        if p.turn_penalty_enabled:
            c[1:] += np.where(d[1:] != d[:-1], float(p.turn_penalty), 0.0)
        vy, vx = v[:, 1], v[:, 0]
        if p.dynamic_penalties_enabled:
            veh = np.trunc(p.obstacle_penalty_vehicle * (1.0 + p.dynamic_penalty_scale * dens[vy, vx].astype(np.float64)))
        else:
            veh = np.full(len(d), float(p.obstacle_penalty_vehicle))
        c += np.where(occ[vy, vx] == 1, veh, 0.0) + np.where(stop[vy, vx] == 1, float(p.obstacle_penalty_stop), 0.0)
        if p.road_type_penalties_enabled:
            c += np.where(road[vy, vx] == 1, rt[rtype[vy, vx] & 3], 0.0)
        out[i] = int(np.trunc(c).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--astar-seconds", type=float, default=40.0, help="what the sampled A* batch of one round may take")
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "costfield_probe.json"))
    args = ap.parse_args()
    import bench
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    W, H = int(tables["width"]), int(tables["height"])
    road_map = np.asarray(tables["is_road_map"])
    road = np.argwhere(road_map == 1)[:, ::-1].astype(np.int32)
    centre = road[np.argmin(np.abs(road[:, 0] - W // 2) + np.abs(road[:, 1] - H // 2))]
    if "highway_exits_xy" in tables and len(tables["highway_exits_xy"]):
        exits, exits_are = np.asarray(tables["highway_exits_xy"], dtype=np.int32).reshape(-1, 2), "highway exits"
    else:
        edge = (road[:, 0] == 0) | (road[:, 1] == 0) | (road[:, 0] == W - 1) | (road[:, 1] == H - 1)
        exits, exits_are = road[edge], "road cells on the map's edge (the synthetic world has no highway exits)"
    if len(exits) == 0:
        exits, exits_are = road[:: max(len(road) // 64, 1)][:64], "64 road cells spread over the map (no road reaches the edge)"
    seeds = {"one_seed": centre[None, :], "all_exits": exits}
    keys = [(s, m, t) for s in seeds for m in MODES for t in TILES]
    ms = {k: [] for k in keys}
    work = {}
    astar = dict(ms_extrapolated=[], ms_sample=[], sample=[], found=[], equal=[], field_less=[])
    tick = {k: [] for k in (["c_parent"] if args.parent_lib else []) + ["c_this_costfield_unused"]}
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
            # the fields, on the engine that just ran "unused" (its tick window is over)
            cf = api.costfield
            os.environ["TS_DEBUG_COSTFIELD_TILE"] = "32"
            cf.compute(seeds["one_seed"], mode="to", free_flow=True)          # warm-up
            for s, m, t in keys:
                os.environ["TS_DEBUG_COSTFIELD_TILE"] = str(t)
                t0 = time.perf_counter()
                info = cf.compute(seeds[s], mode="to", **MODES[m])
                ms[(s, m, t)].append((time.perf_counter() - t0) * 1e3)
                work[(s, m, t)] = dict(rounds=info["rounds"], tile_visits=info["tile_visits"], reached=info["reached"],
                                       max_value=info["max_value"], headings=info["headings"],
                                       tiles=(-(-W // t)) * (-(-H // t)))
            os.environ.pop("TS_DEBUG_COSTFIELD_TILE", None)
            # (b) the sampled A* batch to the same seed, against the soft field
            info = cf.compute(seeds["one_seed"], mode="to", soft=True)
            rng = np.random.default_rng(args.seed + rnd)
            n = min(args.sample, len(road))
            sample = road[rng.choice(len(road), size=n, replace=False)]
            q = lambda cells: [(int(x), int(y), int(centre[0]), int(centre[1]), 1, 0, 0x7FFFFFFF) for x, y in cells]
            t0 = time.perf_counter()
            api.astar_batch(q(sample[:50]))
            pilot = time.perf_counter() - t0
            n = int(max(50, min(n, args.astar_seconds / max(pilot / 50, 1e-6))))
            sample = sample[:n]
            t0 = time.perf_counter()
            off, xy = api.astar_batch(q(sample))
            t_batch = (time.perf_counter() - t0) * 1e3
            at_start = cf.gather("cost", sample).astype(np.int64)
            p = api.params_from_defaults(bench.POLICY)
            maps = (np.asarray(tables["allowed_dirs_map"]), road_map, np.asarray(tables["road_type_map"]),
                    api.map(capi.MAP_OCCUPANCY), api.map(capi.MAP_STOP), api.density())
            cost = path_costs(p, maps, off, xy, sample.astype(np.int64))
            has = cost >= 0
            same_cell = (sample == centre).all(axis=1)
            assert ((at_start[~has & ~same_cell] == 0xFFFFFFFF)).all(), "the batch found no path where the field has a value"
            assert (at_start[has] <= cost[has]).all(), "a path of the batch is cheaper than the field"
            turns_cost = bool(p.turn_penalty_enabled) and int(p.turn_penalty) > 0
            assert turns_cost or (at_start[has] == cost[has]).all(), "turns are free and the field is not the path's cost"
            astar["ms_sample"].append(t_batch)
            astar["ms_extrapolated"].append(t_batch * len(road) / n)
            astar["sample"].append(n)
            astar["found"].append(int(has.sum()))
            astar["equal"].append(int((at_start[has] == cost[has]).sum()))
            astar["field_less"].append(int((at_start[has] < cost[has]).sum()))
            facts = dict(road_cells=int(len(road)), exits=int(len(exits)), exits_are=exits_are, seed=[int(v) for v in centre],
                         live_vehicles=api.num_vehicles(), tick=info["tick"], turns_cost=turns_cost,
                         label_bytes=info["headings"] * W * H * 8 + (W * H * 8 if info["headings"] == 4 else 0),
                         result_bytes=info["device_bytes"])
            cf.release()
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    fields = {f"{s}/{m}/tile{t}": dict(ms=summary(ms[(s, m, t)]), **work[(s, m, t)],
                                      visits_per_tile_round=round(work[(s, m, t)]["tile_visits"] / max(work[(s, m, t)]["tiles"] * work[(s, m, t)]["rounds"], 1), 4))
              for s, m, t in keys}
    one_soft = statistics.median(ms[("one_seed", "soft", 32)])
    rec = dict(probe="costfield", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, state=facts, fields=fields,
               astar_batch=dict(note="ms_extrapolated = ms_sample * road cells / sample: an EXTRAPOLATION", ms_sample=summary(astar["ms_sample"]),
                                ms_extrapolated=summary(astar["ms_extrapolated"]), sample=astar["sample"], found=astar["found"],
                                equal_to_field=astar["equal"], field_less=astar["field_less"], field_more=[0] * len(astar["sample"]),
                                extrapolated_over_field=round(statistics.median(astar["ms_extrapolated"]) / one_soft, 1)),
               ms_per_tick={k: summary(v) for k, v in tick.items()})
    if args.parent_lib:
        p, t = tick["c_parent"], statistics.median(tick["c_this_costfield_unused"])
        rec["unused_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["unused_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
