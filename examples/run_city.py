"""Headless run of the reference's city on the MI355X engine: `python examples/run_city.py --size 200 --seed 1 --ticks 500`.

Everything comes from (size, seed): worldgen builds the city the reference builds after `random.seed(seed)`, the engine's
traffic generator schedules day 0, then `model.step()` is CityModel.step().  Prints the traffic generator's statistics
every `--every` ticks, like the reference's console output.  Needs the HIP library and a GPU (no CPU fallback)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# config.py's values for what DynamicTrafficAgent, the service fleet and the city blocks read (config.py:238-253, 333-335)
TRAFFIC = dict(P_int=10000, P_thr=2400, dt=6, start_offset=6 * 3600, service_food=50, service_waste=50,
               max_load_food=50.0, max_load_waste=250.0, load_time=20, gradual=True, food_capacity_per_cell=2.0,
               waste_capacity_per_cell=1.5, food_consumption_ticks=50, waste_production_ticks=100)

def write_frame(path_stem, frame):
    """An (h, w, 4) RGBA frame as PNG through PIL where that imports, else as binary PPM (P6, RGB); returns the file's path."""
    try:
        from PIL import Image
    except ImportError:
        path = path_stem + ".ppm"
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
            f.write(frame[..., :3].tobytes())
        return path
    path = path_stem + ".png"
    Image.fromarray(frame[..., :3], "RGB").save(path)
    return path


def run(size, seed, ticks, every=50, engine=None, traffic=None, defaults=None, out=print, observe=False, trip_log=None,
        frames=None, frame_every=10, zoom=1, shrink=1, **world_kwargs):
    from trafficsimulation_amd.mesa_api import CityModel
    t0 = time.time()
    m = CityModel(size, size, seed=seed, defaults=defaults or {}, traffic=dict(TRAFFIC, **(traffic or {})), engine=engine,
                  trip_log=trip_log, **world_kwargs)
    out(f"city {m.width}x{m.height} seed {seed}: {len(m.intersection_light_groups)} light groups, {len(m.city_blocks)} blocks, "
        f"{len(m.get_start_blocks())} entries, built in {time.time() - t0:.1f} s")
    if observe:
        m.observe()      # traffic observation planes (include/trafficsim_observe.h), from the first tick on
    t0 = time.time()
    if frames:
        os.makedirs(frames, exist_ok=True)
    for t in range(1, ticks + 1):
        m.step()
        if frames and t % frame_every == 0:      # rendered on the device (include/trafficsim_render.h), one file per frame
            write_frame(os.path.join(frames, f"frame_{t:06d}"), m.render(zoom=zoom, shrink=shrink))
        if t % every == 0 or t == ticks:
            s = m.dynamic_traffic_generator.cached_stats
            out(f"tick {t:6d}  live {len(m.active_vehicle_agents):6d}  internal {s['live_internal']:5d}  through {s['live_through']:5d}  "
                f"service {s['live_service_food'] + s['live_service_waste']:3d}  parked {s['parked']:4d}  stuck {s['stuck']:4d}  "
                f"clouds {len(m.rains)}  {1e3 * (time.time() - t0) / t:.2f} ms/tick")
    return m


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=500)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--carve", action="store_true", help="carve_subblock_roads=True (BASELINE config 5 style)")
    ap.add_argument("--heatmap", metavar="OUT.npy", default=None, help="write the run's flow (cells entered), pooled 8 x 8, to this file")
    ap.add_argument("--trips", metavar="OUT.npy", default=None, help="write one record per finished trip (capi.TRIP_DTYPE) to this file")
    ap.add_argument("--trip-capacity", type=int, default=1 << 20, help="records the trip log holds (later ones are dropped and counted)")
    ap.add_argument("--demand", metavar="OUT.npy", default=None, help="write the planned load at the end of the run (remaining routes per cell, (H, W) uint32) to this file")
    ap.add_argument("--select-link", nargs=2, metavar=("X,Y", "OUT.npy"), default=None,
                    help="write the select-link load of cell (X, Y) at the end of the run (the remaining routes of the vehicles that will enter it, per cell, (H, W) uint32) to OUT.npy")
    ap.add_argument("--jams", metavar="OUT.npy", default=None,
                    help="write one record per jam at the end of the run (queues of standing vehicles, jams.JAM_DTYPE) to this file")
    ap.add_argument("--isochrone", nargs=2, metavar=("X,Y", "OUT.npy"), default=None,
                    help="write the travel cost from every cell to cell (X, Y) at the end of the run ((H, W) uint32, 0xFFFFFFFF: unreachable) to OUT.npy")
    ap.add_argument("--evacuate", metavar="OUT.npy", default=None,
                    help="write the load of every live vehicle's route to its nearest highway exit at the end of the run ((H, W) uint32) to this file")
    ap.add_argument("--frames", metavar="DIR", default=None, help="write a frame of the whole city into DIR every --frame-every ticks (PNG with PIL, else PPM)")
    ap.add_argument("--frame-every", type=int, default=10)
    ap.add_argument("--zoom", type=int, default=1, help="pixels per cell of the frames (1..64)")
    ap.add_argument("--shrink", type=int, default=1, help="cells per pixel of the frames (1..64; not together with --zoom)")
    a = ap.parse_args()
    kw = dict(carve_subblock_roads=True) if a.carve else {}
    m = run(a.size, a.seed, a.ticks, a.every, observe=bool(a.heatmap), trip_log=a.trip_capacity if a.trips else None,
            frames=a.frames, frame_every=a.frame_every, zoom=a.zoom, shrink=a.shrink, **kw)
    if a.heatmap:
        import numpy as np
        from trafficsimulation_amd import _capi as capi
        np.save(a.heatmap, sum(m.engine.observe_pooled(n, 8) for n in capi.OBS_ENTER))
    if a.demand:
        import numpy as np
        load = m.planned_load()      # computed on the device (include/trafficsim_demand.h): the whole remaining path, one bin
        np.save(a.demand, load["load"][0])
        y, x = divmod(int(load["load"][0].argmax()), m.width)
        print(f"planned load: {load['steps']} steps of {load['vehicles']} vehicles; busiest cell ({x}, {y}) with {int(load['load'][0, y, x])} planned entries")
    if a.select_link:
        import numpy as np
        x, y = (int(v) for v in a.select_link[0].split(","))
        # on the device (include/trafficsim_selectlink.h): whose routes cross the gate, then the demand walk over those vehicles alone
        link = m.select_link([[(x, y)]])
        load = m.select_link_load(any=1)
        np.save(a.select_link[1], load["load"][0])
        by_dir = ", ".join(f"{d} {int(n)}" for d, n in zip("NESW", link["cross"][0, 0]))
        print(f"select link ({x}, {y}): {link['crossing']} of {link['vehicles']} vehicles cross it {link['crossings']} times ({by_dir}); "
              f"their routes hold {load['steps']} steps")
    if a.jams:
        import numpy as np
        # on the device (include/trafficsim_jams.h): the connected components of the cells on which a vehicle stands
        found = m.jams()
        np.save(a.jams, found["jams"])
        big = found["jams"][0] if found["n"] else None
        print(f"jams: {found['n']} with {found['standing_vehicles']} standing vehicles on {found['standing_cells']} cells"
              + (f"; the largest has {int(big['cells'])} cells from ({int(big['x0'])}, {int(big['y0'])}) to ({int(big['x1'])}, {int(big['y1'])})" if big is not None else ""))
    if a.isochrone:
        import numpy as np
        x, y = (int(v) for v in a.isochrone[0].split(","))
        thr = [50, 100, 200, 500, 1000, 5000]
        iso = m.isochrones([(x, y)], thr)      # computed on the device (include/trafficsim_costfield.h): a soft TO field and its bands
        np.save(a.isochrone[1], m.engine.costfield.plane("cost"))
        print(f"cost to ({x}, {y}): {iso['reached']} cells reached in {iso['rounds']} rounds, farthest at {iso['max_value']}; road cells within "
              + ", ".join(f"{t}: {int(n)}" for t, n in zip(thr, iso["road_cells"])))
    if a.evacuate:
        import numpy as np
        # on the device (include/trafficsim_cfroute.h): the catchments of the exits, a route per vehicle, their summed load
        vehicles = list(m.active_vehicle_agents)
        zone = m.catchments("highway_exits")
        if vehicles:
            ev = m.assigned_load(m.highway_exits, vehicles)
            routes = m.routes_along(m.highway_exits, vehicles)
            np.save(a.evacuate, ev["load"])
            y, x = divmod(int(ev["load"].argmax()), m.width)
            by_exit = np.bincount(routes["owner"][routes["owner"] >= 0], minlength=zone["n"])
            print(f"evacuation: {ev['routes']} of {len(vehicles)} vehicles reach one of {zone['n']} exits in {ev['steps']} steps "
                  f"(longest route {routes['trace_longest']}); busiest cell ({x}, {y}) with {int(ev['load'][y, x])} entries; "
                  f"busiest exit {int(by_exit.argmax())} takes {int(by_exit.max())}")
        else:
            np.save(a.evacuate, np.zeros((m.height, m.width), dtype=np.uint32))
            print("evacuation: no live vehicles")
    if a.trips:
        import numpy as np
        rec, info = m.trips(), m.engine.triplog_info()
        np.save(a.trips, rec)
        od = m.od_matrix()
        o, d = divmod(int(od["count"].argmax()), len(od["zones"]))
        print(f"{len(rec)} trips logged ({info['dropped']} dropped), {int(od['count'].sum())} arrived between known zones; "
              f"busiest pair: {od['zones'][o]} -> {od['zones'][d]} ({int(od['count'][o, d])} trips)")
