#!/usr/bin/env python3
"""What jam detection costs: the config-2 world at 4096^2 / 10^6 vehicles, on the tick after the warm-up and the timed steps
(the record says how many vehicles stand there), timed

  (a) ts_jams_compute over the vehicles (min_ticks 1), FLOW and GRID, at TS_DEBUG_JAMS_TILE = 0 / 8 / 16 / 32;
  (b) the same for a dense mask on the device, occupancy > 0 (every cell a vehicle is on, standing or not);
  (c) ts_jams_groups on the FLOW result;
  (d) the host route it replaces: ts_download_vehicles plus tests/jams_expect.py (FLOW: the rule in numpy with a union-find)
      or scipy.ndimage.label (GRID, where scipy imports), on the same state, checked against the engine's records;
  (e) per tick with the feature never used, on a library built from the parent commit (--parent-lib, optional) and on this one,
      alternating inside every round with the legs swapping places: "unused" must sit inside the parent's own spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Each leg
is warmed up; medians and the spread (min .. max) over the rounds are reported.  Prints one JSON line and writes it to
profiles/jams_probe.json (or --out).

    python profiles/jams_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch          # before the engine library: the device mask is a torch tensor the engine reads in place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILES = (0, 8, 16, 32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg e)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jams_probe.json"))
    args = ap.parse_args()
    torch.cuda.init()
    import bench
    from tests import jams_expect as je
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    W, H = int(tables["width"]), int(tables["height"])
    keys = [f"{src}_{link}_tile{t}" for src in ("vehicles", "mask") for link in ("flow", "grid") for t in TILES]
    ms = {k: [] for k in keys}
    other = {k: [] for k in ("groups", "host_flow_numpy", "host_grid_scipy", "download_vehicles")}
    tick = {k: [] for k in (["e_parent"] if args.parent_lib else []) + ["e_this_jams_unused"]}
    facts = {}
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        legs = list(tick)
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):          # the legs swap places from round to round
            api = capi.CApi(libs["parent" if leg == "e_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            tick[leg].append(timed_ticks(api, args.steps))
            if leg == "e_parent":
                api.close()
                continue
            j = api.jams
            occ = torch.as_tensor((api.map(capi.MAP_OCCUPANCY) > 0).astype(np.uint8)).cuda()
            for src, mask in (("vehicles", None), ("mask", occ)):
                for link in ("flow", "grid"):
                    for t in TILES:
                        os.environ["TS_DEBUG_JAMS_TILE"] = str(t)
                        j.compute(1, link, mask=mask)
                        ms[f"{src}_{link}_tile{t}"].append(timed(lambda: j.compute(1, link, mask=mask), args.calls))
            os.environ.pop("TS_DEBUG_JAMS_TILE", None)
            dense = j.compute(1, "flow", mask=occ)
            # the host route on the same state, held against the engine's records
            t0 = time.perf_counter()
            rows = api.vehicles()
            t_rows = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            count = je.count_plane(rows, H, W, 1)
            lab = je.label(count, je.FLOW, tables["allowed_dirs_map"])
            cells = np.bincount(lab[lab >= 0])
            other["host_flow_numpy"].append(t_rows + (time.perf_counter() - t0) * 1e3)
            other["download_vehicles"].append(t_rows)
            info = j.compute(1, "flow")
            rec = j.records()
            assert info["n_jams"] == len(cells) and np.array_equal(rec["cells"], cells) and np.array_equal(j.plane("label"), lab), \
                "the host route and the engine disagree (FLOW)"
            other["groups"].append(timed(j.groups, args.calls))
            if ndimage is not None:
                t0 = time.perf_counter()
                rows = api.vehicles()
                glab, n = ndimage.label(je.count_plane(rows, H, W, 1) > 0)
                gcells = np.bincount(glab[glab > 0] - 1)
                other["host_grid_scipy"].append((time.perf_counter() - t0) * 1e3)
                ginfo = j.compute(1, "grid")
                assert ginfo["n_jams"] == n and np.array_equal(j.records()["cells"], gcells), "the host route and the engine disagree (GRID)"
            facts = dict(live_vehicles=int(len(rows)), standing_vehicles=info["standing_vehicles"], standing_cells=info["standing_cells"],
                         jams_flow=info["n_jams"], largest_flow=info["largest_cells"], occupied_cells=dense["standing_cells"],
                         jams_dense_flow=dense["n_jams"], largest_dense_flow=dense["largest_cells"], tick=info["tick"],
                         device_bytes=info["device_bytes"], light_groups=int(len(j.groups())))
            j.release()
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = dict(probe="jams", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, calls_per_window=args.calls,
               warmup=args.warmup, rounds=args.rounds, state=facts, ms_per_compute={k: summary(v) for k, v in ms.items()},
               best_tile={f"{src}_{link}": min(TILES, key=lambda t: med[f"{src}_{link}_tile{t}"]) for src in ("vehicles", "mask") for link in ("flow", "grid")},
               ms_per_call={k: summary(v) for k, v in other.items()},
               host_flow_over_compute=round(statistics.median(other["host_flow_numpy"]) / med["vehicles_flow_tile32"], 1),
               host_grid_over_compute=round(statistics.median(other["host_grid_scipy"]) / med["vehicles_grid_tile32"], 1) if other["host_grid_scipy"] else None,
               ms_per_tick={k: summary(v) for k, v in tick.items()})
    if args.parent_lib:
        p, t = tick["e_parent"], statistics.median(tick["e_this_jams_unused"])
        rec["unused_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["unused_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
