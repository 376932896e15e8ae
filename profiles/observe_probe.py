#!/usr/bin/env python3
"""What traffic observation costs, and what it replaces: the config-2 policy at 4096^2 / 10^6 vehicles, timed per tick

  (a) on a library built from the parent commit (--parent-lib, optional),
  (b) on this library with observation off,
  (c) with all seven planes on,
  (d) with the only alternative there was: ts_download_vehicles after every tick,

plus the milliseconds of observe_pooled(factor 64) over the four ENTER planes and of observe_groups.  The legs alternate
inside every round on engines of their own (same workload, same seeds), each warmed up before its timed window; the medians
over the rounds and the spread (min .. max) of every leg are reported.  Prints one JSON line and writes it to
profiles/observe_probe.json (or --out).

    python profiles/observe_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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


def timed_ticks(api, steps, after_tick=None):
    """ms per tick over `steps` ticks; every tick ends in a device synchronise (counters read back)."""
    api.counters()
    t0 = time.perf_counter()
    for _ in range(steps):
        api.step(1)
        if after_tick:
            after_tick()
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
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observe_probe.json"))
    args = ap.parse_args()
    assert args.rounds >= 5, "the median of at least five runs"
    import bench
    from trafficsimulation_amd import _capi as capi
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    legs = (["a_parent"] if args.parent_lib else []) + ["b_off", "c_on", "d_download"]
    ms = {leg: [] for leg in legs}
    pooled_ms, groups_ms = [], []
    end_state = {}
    for rnd in range(args.rounds):
        for leg in legs:
            api = capi.CApi(libs["parent" if leg == "a_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            if leg == "c_on":
                api.observe_start()
            api.step(args.warmup)
            ms[leg].append(timed_ticks(api, args.steps, api.vehicles if leg == "d_download" else None))
            if leg == "c_on":
                t0 = time.perf_counter()
                flow = sum(api.observe_pooled(n, 64) for n in capi.OBS_ENTER)
                pooled_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                rows = api.observe_groups()
                groups_ms.append((time.perf_counter() - t0) * 1e3)
                steps_sum = int(api.vehicles()[:, capi.V_FIELDS.index("steps_traveled")].sum())
                assert int(flow.sum()) >= steps_sum > 0, (int(flow.sum()), steps_sum)      # (equal unless vehicles arrived and left)
                end_state["flow_cells"], end_state["groups"] = int(flow.sum()), int(len(rows))
            # the run itself must not depend on the leg
            fp = (api.rng_fingerprint(capi.RNG_SCHEDULER), int(api.num_vehicles()), int(api.map(capi.MAP_OCCUPANCY).sum()))
            assert end_state.setdefault("fp", fp) == fp, f"{leg}: the run differs from the other legs"
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v])
    rec = dict(probe="observe", size=args.size, vehicles=args.vehicles, policy="config2", steps=args.steps, warmup=args.warmup,
               rounds=args.rounds, ms_per_tick={leg: summary(v) for leg, v in ms.items()},
               pooled64_four_enter_planes_ms=summary(pooled_ms), groups_ms=summary(groups_ms), groups=end_state.get("groups"),
               plane_bytes=args.size * args.size * 4, planes_on=len(capi.OBS_PLANES),
               vehicle_rows_bytes_per_tick=args.vehicles * len(capi.V_FIELDS) * 4)
    b, c, d = (statistics.median(ms[k]) for k in ("b_off", "c_on", "d_download"))
    rec["overhead_on_over_off_ms"] = round(c - b, 4)
    rec["download_over_on"] = round(d / c, 2)
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
