#!/usr/bin/env python3
"""What the trip log costs: the config-2 policy at 4096^2 / 10^6 vehicles, timed per tick

  (a) on a library built from the parent commit (--parent-lib, optional),
  (b) on this library with the log off,
  (c) with the log on, capacity 2 x 10^6 records,

plus the milliseconds of reading the whole log and of one OD reduction over 128 x 128-cell zones (1 024 of them at 4096^2).
The legs alternate inside every round on engines of their own (same workload, same seeds), each warmed up before its timed
window; the medians over the rounds and the spread (min .. max) of every leg are reported.  "Off" is judged against the parent inside the parent's own
spread; "on" is reported, not gated.  Prints one JSON line and writes it to profiles/triplog_probe.json (or --out).

    python profiles/triplog_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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


def timed_ticks(api, steps):
    """ms per tick over `steps` ticks; the window ends in a device synchronise (counters read back)."""
    api.counters()
    t0 = time.perf_counter()
    for _ in range(steps):
        api.step(1)
    api.counters()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=2_000_000)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplog_probe.json"))
    args = ap.parse_args()
    assert args.rounds >= 5, "the median of at least five runs"
    import bench
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    legs = (["a_parent"] if args.parent_lib else []) + ["b_off", "c_on"]
    ms = {leg: [] for leg in legs}
    read_ms, od_ms = [], []
    end_state = {}
    zone = (np.arange(args.size)[:, None] // 128 * (-(-args.size // 128)) + np.arange(args.size)[None, :] // 128).astype(np.int32)
    n_zones = int(zone.max()) + 1
    for rnd in range(args.rounds):
        for leg in legs:
            api = capi.CApi(libs["parent" if leg == "a_parent" else "this"], "ts_")
            if leg == "c_on":      # (on before the vehicles are placed, as the facade does it)
                create = api.create
                api.create = lambda *a, _c=create, _api=api, **k: (_c(*a, **k), _api.triplog_start(args.capacity))[0]
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            ms[leg].append(timed_ticks(api, args.steps))
            if leg == "c_on":
                info = api.triplog_info()
                t0 = time.perf_counter()
                rec = api.trips()
                read_ms.append((time.perf_counter() - t0) * 1e3)
                if n_zones <= capi.TRIPLOG_MAX_ZONES:
                    api.triplog_set_zones(zone, n_zones)
                    t0 = time.perf_counter()
                    od = api.triplog_od(["arrived"])
                    od_ms.append((time.perf_counter() - t0) * 1e3)
                    assert int(od["count"].sum()) + od["unzoned"] == int((rec["end_reason"] == capi.TRIP_END["arrived"]).sum())
                assert len(rec) == info["count"] == args.vehicles - api.num_vehicles() - info["dropped"], (len(rec), info)
                end_state["records"], end_state["groups"], end_state["device_bytes"] = info["count"], info["groups"], info["device_bytes"]
            # the run itself must not depend on the leg
            fp = (api.rng_fingerprint(capi.RNG_SCHEDULER), int(api.num_vehicles()), int(api.map(capi.MAP_OCCUPANCY).sum()))
            assert end_state.setdefault("fp", fp) == fp, f"{leg}: the run differs from the other legs"
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    rec = dict(probe="triplog", size=args.size, vehicles=args.vehicles, policy="config2", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, capacity=args.capacity, ms_per_tick={leg: summary(v) for leg, v in ms.items()},
               read_all_ms=summary(read_ms), od_128_cell_zones_ms=summary(od_ms), n_zones=n_zones,
               records=end_state.get("records"), groups=end_state.get("groups"), device_bytes=end_state.get("device_bytes"))
    b, c = (statistics.median(ms[k]) for k in ("b_off", "c_on"))
    rec["overhead_on_over_off_ms"] = round(c - b, 4)
    if args.parent_lib:
        a = ms["a_parent"]
        rec["off_minus_parent_ms"] = round(b - statistics.median(a), 4)
        rec["parent_spread_ms"] = round(max(a) - min(a), 4)
        rec["off_within_parent_spread"] = bool(min(a) <= b <= max(a))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
