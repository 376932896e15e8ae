#!/usr/bin/env python3
"""Step 0 of the host tail: from the per-entry records of a -DTS_TRACE_REPLAN build
(profiles/run_replan_trace.sh, the files replan_trace.py reads) and the host searcher's measured rate (profiles/tail_probe.py),
how many searches are in flight over a k_replan pass, and what handing the last T of them to host threads would save.

Per traced pass: the time at which at most 16 / 32 / 64 / 128 entries are still running and the expansions those entries end up
with; then, for every (T, floor) of a small grid, the predicted length of the pass

    max( t(T) + period + ceil(handed / threads) * longest host search + overhead ,  end of the last entry that is not handed over )

where t(T) is when T entries remain, `period` the expansions between two looks at the idle counter at the device's pace, an entry
is handed over when it has made `floor` expansions by then (linear in its own span), a host search starts from scratch at the
probe's microseconds per expansion with all threads busy, and `overhead` stands for the transfers and the re-run launch.

    python3 profiles/tail_gate.py --probe tail_probe.json rtrace_tick*.bin > profiles/r16_tail_gate.json
"""
import argparse
import json
import math
import sys

import numpy as np

PERIOD_EXP = 4096          # fresh expansions between two looks at the idle counter
OVERHEAD_MS = 5.0          # list read-back, path upload, the re-run's launch and its replayed policy code
SPREAD_MS = 39.5           # profiles/r15_bench_ab.json: base_spread_max_minus_min of ticks_between_sum_ms (sixteen ticks)


def load(path):
    a = np.fromfile(path, dtype=np.int32).reshape(-1, 4)
    t0 = a[:, 0].astype(np.uint32).astype(np.int64)
    t1 = a[:, 1].astype(np.uint32).astype(np.int64)
    ok = (t0 != 0) | (t1 != 0)
    a, t0, t1 = a[ok], t0[ok], t1[ok]
    base = t0.min()
    return (t0 - base) / 1e5, (t1 - base) / 1e5, a[:, 2].astype(np.int64)      # start, end in ms; expansions


def in_flight(s, e, exp):
    order = np.argsort(-e)
    out = {}
    for k in (16, 32, 64, 128):
        if len(e) <= k:
            continue
        last = order[:k]
        out[str(k)] = {"at_ms": round(float(e[order[k]]), 1), "expansions_min": int(exp[last].min()), "expansions_max": int(exp[last].max()),
                       "expansions_sum": int(exp[last].sum())}
    return out


def predict(s, e, exp, T, floor, us_host, threads, us_dev):
    if len(e) <= T:
        return float(e.max()), 0
    order = np.argsort(-e)
    t = float(e[order[T]])
    last = order[:T]
    span = np.maximum(e[last] - s[last], 1e-6)
    made = exp[last] * np.clip((t - s[last]) / span, 0.0, 1.0)
    handed = made >= floor
    n = int(handed.sum())
    if n == 0:
        return float(e.max()), 0
    host = math.ceil(n / threads) * float(exp[last][handed].max()) * us_host / 1e3
    rest = float(e[last][~handed].max()) if n < T else 0.0
    return max(t + PERIOD_EXP * us_dev / 1e3 + host + OVERHEAD_MS, rest), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", required=True, help="tail_probe.py's JSON: the host searcher's microseconds per expansion by thread count")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("traces", nargs="+")
    args = ap.parse_args()
    probe = json.load(open(args.probe))
    us_host = float(probe["threads"][str(args.threads)]["us_per_expansion"])
    ticks, grid = {}, {}
    for p in sorted(args.traces, key=lambda q: int(q.split("tick")[1].split(".")[0])):
        name = "tick_" + p.split("tick")[1].split(".")[0]
        s, e, exp = load(p)
        long = exp > 100000
        us_dev = float(((e - s)[long] * 1e3 / exp[long]).mean()) if long.any() else 1.7
        ticks[name] = {"entries": int(len(e)), "span_ms": round(float(e.max()), 1), "queue_empty_at_ms": round(float(s.max()), 1),
                       "device_us_per_expansion_of_searches_over_100000": round(us_dev, 2), "at_most_n_in_flight": in_flight(s, e, exp), "predicted_ms": {}}
        for T in (8, 16, 32, 48, 64, 96, 128, 256):
            for floor in (4096, 16384, 65536):
                ms, n = predict(s, e, exp, T, floor, us_host, args.threads, us_dev)
                key = f"T{T}_floor{floor}"
                ticks[name]["predicted_ms"][key] = [round(ms, 1), n]
                g = grid.setdefault(key, {"T": T, "floor": floor, "saving_ms": 0.0, "handed": 0})
                g["saving_ms"] += float(e.max()) - ms
                g["handed"] += n
    best = max(grid.values(), key=lambda g: g["saving_ms"])
    n_ticks = len(ticks)
    out = {
        "host_us_per_expansion": {k: v["us_per_expansion"] for k, v in probe["threads"].items()},
        "threads": args.threads, "period_expansions": PERIOD_EXP, "overhead_ms": OVERHEAD_MS,
        "ticks": ticks,
        "grid_saving_ms_over_the_traced_passes": {k: round(v["saving_ms"], 1) for k, v in grid.items()},
        "chosen": {"T": best["T"], "floor": best["floor"], "saving_ms_over_the_traced_passes": round(best["saving_ms"], 1),
                   "saving_ms_per_pass": round(best["saving_ms"] / max(n_ticks, 1), 1), "searches_handed_over": best["handed"]},
        "gate": {"traced_passes": n_ticks, "parent_spread_ms_of_sixteen_ticks": SPREAD_MS,
                 "threshold_ms": round(3 * SPREAD_MS * n_ticks / 16.0, 1),
                 "threshold_note": "three times the parent's spread on the sum of sixteen ticks between waves, scaled to the number of traced passes",
                 "passes": bool(best["saving_ms"] >= 3 * SPREAD_MS * n_ticks / 16.0)},
    }
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
