#!/usr/bin/env python3
"""What a frame costs: the config-2 policy at 4096^2 / 10^6 vehicles, timed

  (a) a full-map zoom-1 frame into the engine's device buffer (ts_render_device: pre-pass + frame kernel + synchronise);
  (b) the same frame to host memory (ts_render: (a) plus 64 MiB over the bus);
  (c) a shrink-4 overview of the whole map, to the device buffer;
  (d) a 512 x 512-cell window at zoom 4, to the device buffer;
  (e) the host route these replace: ts_download_map x 3 (stop, rain, occupancy) plus ts_download_vehicles, then the palette
      look-up of tests/render_expect.py's rule in vectorised numpy (cells, then one scatter of the vehicles' colours);
  (f) per tick with the renderer never configured, on a library built from the parent commit (--parent-lib, optional) and
      on this one, alternating inside every round: "off" must sit inside the parent's own round-to-round spread.

Every timing ends in a device synchronise (the entries synchronise themselves; the tick windows end in ts_counters).  Each
leg is warmed up; medians and the spread (min .. max) over the rounds are reported.  From the shapes the frame kernel's
bytes are N * (3 plane bytes + 1 dynamic byte + 4 pixel bytes) at zoom 1; the figure over (a)'s time is reported next to the
call's time (the call also holds the pre-pass and its launches, so the rate is a lower bound of the kernel's).  Prints one
JSON line and writes it to profiles/render_probe.json (or --out).

    python profiles/render_probe.py --parent-lib /path/to/parent/libtrafficsim_hip.so
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


def host_route(api, capi, type_plane, pal, vpal):
    """Download what a frame needs and compose the zoom-1 frame with numpy."""
    t0 = time.perf_counter()
    stop, rain, _occ = api.map(capi.MAP_STOP), api.map(capi.MAP_RAIN), api.map(capi.MAP_OCCUPANCY)
    rows = api.vehicles()
    t1 = time.perf_counter()
    frame = pal[type_plane, 0, (stop == 1).astype(np.intp), (rain > 0).astype(np.intp)]
    f = rows[:, capi.V_FIELDS.index("flags")]
    status = np.where(f & capi.F_COLLISION, 1, np.where(f & capi.F_MALFUNCTION, 2, np.where(f & capi.F_PARKED, 3, 0)))
    kind = np.where(f & (capi.F_OVERTAKING | capi.F_DETOUR), 1, 0)
    flash = 1 if api.counters().step_count % 2 == 0 else 0
    frame[rows[:, 2], rows[:, 1]] = vpal[kind, status, flash]
    return frame, (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--vehicles", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=20, help="frames per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtrafficsim_hip.so built from the parent commit (leg f)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_probe.json"))
    args = ap.parse_args()
    import bench
    from trafficsimulation_amd import _capi as capi, render as rn
    from trafficsimulation_amd._lib import load_library
    tables, routes, _ = bench.make_workload(args.size, args.vehicles, args.seed)
    libs = {"this": load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    W, H = int(tables["width"]), int(tables["height"])
    if "cell_type_map" in tables:
        type_plane, names = np.asarray(tables["cell_type_map"]).astype(np.uint8), rn.CELL_TYPE_NAMES
    else:
        type_plane = rn.fallback_type_plane(tables["is_road_map"], tables["intersection_map"], tables["light_ctrl_xy"], tables["light_xy"])
        names = rn.fallback_type_names()
    pal, vpal = rn.cell_palette(None, names), rn.vehicle_palette()
    layers = capi.RL_SIGNALS | capi.RL_RAIN | capi.RL_VEHICLES
    win = min(512, W, H)
    views = {"a_full_zoom1_device": rn.make_view(cells_w=W, cells_h=H, layers=layers),
             "c_shrink4_device": rn.make_view(cells_w=W, cells_h=H, shrink=4, layers=layers),
             "d_window512_zoom4_device": rn.make_view(x0=W // 3, y0=H // 3, cells_w=win, cells_h=win, zoom=4, layers=layers)}
    ms = {k: [] for k in list(views) + ["b_full_zoom1_host", "e_host_route", "e_of_which_downloads"]}
    tick = {k: [] for k in (["f_parent"] if args.parent_lib else []) + ["f_this_renderer_off"]}
    for rnd in range(args.rounds):
        print(f"[probe] round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
        for leg in tick:
            api = capi.CApi(libs["parent" if leg == "f_parent" else "this"], "ts_")
            bench.setup(api, tables, routes, args.seed, policy="config2")
            api.step(args.warmup)
            tick[leg].append(timed_ticks(api, args.steps))
            if leg == "f_parent":
                api.close()
                continue
            # the frames, on the engine that just ran "off" (its tick window is over: configuring now does not touch it)
            api.render_set_cells(type_plane, pal)
            api.render_set_vehicle_palette(vpal)
            ptr = ctypes.c_void_p()
            dev = api._ext("render_device")
            for name, v in views.items():
                for _ in range(args.warmup):
                    api._chk(dev(api.h, ctypes.byref(v), ctypes.byref(ptr)))
                ms[name].append(timed(lambda: api._chk(dev(api.h, ctypes.byref(v), ctypes.byref(ptr))), args.frames))
            full = views["a_full_zoom1_device"]
            host = np.zeros((H, W, 4), dtype=np.uint8)
            to_host = api._ext("render")
            for _ in range(2):
                api._chk(to_host(api.h, ctypes.byref(full), host.ctypes.data))
            ms["b_full_zoom1_host"].append(timed(lambda: api._chk(to_host(api.h, ctypes.byref(full), host.ctypes.data)), max(3, args.frames // 4)))
            frame, _, _ = host_route(api, capi, type_plane, pal, vpal)
            single = np.bincount(api.vehicles()[:, 2].astype(np.int64) * W + api.vehicles()[:, 1], minlength=W * H).reshape(H, W) <= 1
            assert np.array_equal(frame[single], host[single]), "the host route and the engine disagree on a cell with at most one vehicle"
            for _ in range(3):
                _, dl, total = host_route(api, capi, type_plane, pal, vpal)
                ms["e_of_which_downloads"].append(dl)
                ms["e_host_route"].append(total)
            api.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v]) if v else None
    frame_bytes = W * H * (3 + 1 + 4)
    a = statistics.median(ms["a_full_zoom1_device"])
    rec = dict(probe="render", size=args.size, vehicles=args.vehicles, policy="config2 (reduced)", steps=args.steps, frames_per_window=args.frames,
               warmup=args.warmup, rounds=args.rounds, ms_per_frame={k: summary(v) for k, v in ms.items()},
               ms_per_tick={k: summary(v) for k, v in tick.items()},
               frame_kernel_bytes_from_shapes=frame_bytes, a_bytes_over_call_time_GBps=round(frame_bytes / a / 1e6, 1),
               host_route_over_a=round(statistics.median(ms["e_host_route"]) / a, 1))
    if args.parent_lib:
        p, t = tick["f_parent"], statistics.median(tick["f_this_renderer_off"])
        rec["off_minus_parent_ms"] = round(t - statistics.median(p), 4)
        rec["parent_spread_ms"] = round(max(p) - min(p), 4)
        rec["off_within_parent_spread"] = bool(min(p) <= t <= max(p))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
