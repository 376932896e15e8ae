#!/usr/bin/env python3
"""Golden frames of the reference's own portrayal layer (build container only; never runs on the GPU box).

Runs the reference's unmodified `CityModel.step()` through make_golden.run_scenario, so the trace arrays are the ordinary ones
(tests/trace_util.py replays them), and adds what a viewer would have drawn at a few ticks - every cell and every vehicle
asked for `get_portrayal()["Color"]`, as the Mesa page and the VisPy viewer do once per frame:

  frame_ticks    (T,) int32            ticks (0-based, after that tick's step) the frames belong to
  frame_steps    (T,) int32            CityModel.step_count at those ticks (the flash is step_count % 2 == 0)
  cells_rgb      (T, H, W, 3) uint8    the cell's colour, resolved by matplotlib
  vehicle_rgba   (T, H, W, 4) uint8    the colour of the last vehicle of grid.get_cell_list_contents per cell (what a
                                       CanvasGrid draws last), alpha 0 where the cell holds none
  ambiguous      (T, H, W) bool        cells that hold several vehicles whose colours differ
  cell_base_type_map (H, W) int8       the cell type whose ZONE_COLORS entry is the cell's base_color: cell_type_map, except on
                                       a ControlledRoad, which keeps the colour of the road it was carved from
                                       (city_model.py:1458) - there CellAgent.road_type
  service_idx    (n,) int32            spawn indices of the ServiceVehicleAgents seen at the frame ticks
  zone_names / zone_rgb, vehicle_names / vehicle_rgb
                                       Defaults.ZONE_COLORS and the six vehicle colours of Defaults, resolved to RGB

The frames are chosen after the run, from a capture of every tick, so that together they show every colour rule; the
script asserts that on the reference's output alone.  No file of the reference is touched.

Usage:  python tests/golden/make_golden_render.py all | <scenario>
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_lights import write_npz  # noqa: E402

SCENARIOS = {
    # everything a frame can show on one small map: queue-actuated lights (the default), rain with a high spawn chance, the
    # fault probabilities of faults_64_s9, the traffic generator, and a service fleet - its vehicles park while they service, and
    # they are the reference's only remove_on_arrival=False vehicles.  (Seeds 52 and 53 of this scenario end in the reference's
    # own "already added to scheduler" exception before a service vehicle has parked.)
    "render_city_64_s56": dict(size=64, seed=56, vehicles=60, ticks=240,
                               defaults={"RAIN_RADIUS_MIN": 8, "RAIN_RADIUS_MAX": 20, "RAIN_SPAWN_CHANCE": 0.3,
                                         "VEHICLE_MALFUNCTION_CHANCE": 0.004, "VEHICLE_MALFUNCTION_DURATION": 25,
                                         "VEHICLE_SIDESWIPE_COLLISION_CHANCE": 0.2, "VEHICLE_SIDESWIPE_COLLISION_DURATION": 30,
                                         "TOTAL_SERVICE_VEHICLES_FOOD": 600, "TOTAL_SERVICE_VEHICLES_WASTE": 600,
                                         "INTERNAL_POPULATION_TRAFFIC_PER_DAY": 8000, "PASSING_POPULATION_TRAFFIC_PER_DAY": 3000}),
}
N_FRAMES = (8, 12)
CELL_TAGS = ("ControlledRoadStop", "ControlledRoadGo", "TrafficLightStop", "TrafficLightGo", "IntersectionPending")
VEHICLE_TAGS = ("fault_flash0", "fault_flash1", "parked", "contraflow", "service")


def run(name):
    import numpy as np
    import matplotlib.colors as mcolors
    spec = SCENARIOS[name]
    mg.SCENARIOS[name] = dict(spec)
    mg._setup_paths()
    from Simulation.config import Defaults
    from Simulation.city_model import CityModel
    from Simulation.agents.vehicles.vehicle_base import VehicleAgent
    from Simulation.agents.vehicles.vehicle_service import ServiceVehicleAgent
    from Simulation.utilities.general import desaturate

    def rgb(color):
        return tuple(int(round(c * 255)) for c in mcolors.to_rgb(color))

    caps = []
    m_ref = {}
    mg_names = ["Wall", "Sidewalk", "Nothing", "R1", "R2", "R3", "Intersection", "BlockEntrance", "HighwayEntrance", "HighwayExit",
                "ControlledRoad", "TrafficLight", "Residential", "Office", "Market", "Leisure", "Other", "Empty"]   # world_tables' codes
    orig_step = CityModel.step

    def step(self):
        orig_step(self)
        m_ref["m"] = self
        self.cache_cell_portrayal = False      # (a viewer's cache of static cells: every cell is asked again here)
        H, W = self.height, self.width
        cells = np.zeros((H, W, 3), dtype=np.uint8)
        veh = np.zeros((H, W, 4), dtype=np.uint8)
        amb = np.zeros((H, W), dtype=bool)
        tags, service, n_veh_cells = set(), set(), 0
        flash = 1 if self.step_count % 2 == 0 else 0
        for x in range(W):
            for y in range(H):
                contents = self.grid.get_cell_list_contents([(x, y)])
                cell = self.get_cell_contents(x, y)[0]
                col = cell.get_portrayal()["Color"]
                cells[y, x] = rgb(col)
                raining = Defaults.RAIN_ENABLED and self.rain_map[y, x] > 0
                stop = self.stop_map[y, x] == 1
                if raining:
                    tags.add("rain_" + cell.cell_type)
                elif cell.cell_type == "ControlledRoad":
                    tags.add("ControlledRoadStop" if stop else "ControlledRoadGo")
                    assert col == (Defaults.ZONE_COLORS["ControlledRoadStop"] if stop else desaturate(cell.base_color, 0.75, 0.25))
                elif cell.cell_type == "TrafficLight":
                    tags.add("TrafficLightStop" if stop else "TrafficLightGo")
                elif cell.cell_type == "Intersection" and cell.intersection_group.pending_phase is not None:
                    tags.add("IntersectionPending")
                    assert col == Defaults.ZONE_COLORS["IntersectionPending"]
                vs = [a for a in contents if isinstance(a, VehicleAgent)]
                if not vs:
                    continue
                n_veh_cells += 1
                cols = [rgb(v.get_portrayal()["Color"]) for v in vs]
                veh[y, x] = cols[-1] + (255,)
                amb[y, x] = len(set(cols)) > 1
                top = vs[-1]
                for v in vs:
                    if isinstance(v, ServiceVehicleAgent):
                        service.add(v._g_idx)
                if top.is_in_collision or top.is_in_malfunction:
                    tags.add(f"fault_flash{flash}")
                elif top.is_parked:
                    tags.add("parked")
                if isinstance(top, ServiceVehicleAgent):
                    tags.add("service")
                elif top.is_overtaking or top.is_in_stuck_detour:
                    tags.add("contraflow")
        caps.append(dict(cells=cells, veh=veh, amb=amb, tags=tags, service=service, n_veh_cells=n_veh_cells,
                         step_count=int(self.step_count)))
    CityModel.step = step

    saved = {}
    real_savez = np.savez_compressed

    def keep(path, **arrays):   # (run_scenario reports the file's size: let it write, the file is replaced below)
        saved.update(arrays=arrays)
        real_savez(path, **arrays)
    np.savez_compressed = keep
    try:
        mg.run_scenario(name)
    finally:
        np.savez_compressed = real_savez
        CityModel.step = orig_step
    os.remove(os.path.join(HERE, f"trace_{name}.npz"))
    out = saved["arrays"]
    T = len(out["veh_off"]) - 1
    assert "raised_at_tick" not in out, f"{name}: tick {out['raised_at_tick']}: {out['raised_message']}"
    assert T == len(caps)

    # ---- the frames: a greedy cover of the colour rules, a consecutive pair for the flash, then spread out ----
    usable = [t for t in range(T) if caps[t]["n_veh_cells"] and caps[t]["amb"].sum() * 100 <= caps[t]["n_veh_cells"]]
    rain_types = set().union(*(c["tags"] for c in caps))
    rain_types = sorted(t for t in rain_types if t.startswith("rain_"))
    want = set(CELL_TAGS) | set(VEHICLE_TAGS) | set(rain_types[:4])
    chosen, covered = [], set()
    while want - covered:
        best = max(usable, key=lambda t: (len((caps[t]["tags"] & want) - covered), -t))
        gain = (caps[best]["tags"] & want) - covered
        assert gain, f"{name}: no tick of this run shows {sorted(want - covered)}"
        chosen.append(best)
        covered |= gain
    if not any(t + 1 in chosen for t in chosen):
        chosen.append(next(t + 1 for t in sorted(chosen) if t + 1 in usable and t + 1 not in chosen))
    spread = [t for t in usable[::max(1, len(usable) // N_FRAMES[0])] if t not in chosen]
    while len(chosen) < N_FRAMES[0]:
        chosen.append(spread.pop(len(spread) // 2))
    chosen = sorted(set(chosen))
    assert N_FRAMES[0] <= len(chosen) <= N_FRAMES[1], chosen

    out["frame_ticks"] = np.asarray(chosen, dtype=np.int32)
    out["frame_steps"] = np.asarray([caps[t]["step_count"] for t in chosen], dtype=np.int32)
    out["cells_rgb"] = np.stack([caps[t]["cells"] for t in chosen])
    out["vehicle_rgba"] = np.stack([caps[t]["veh"] for t in chosen])
    out["ambiguous"] = np.stack([caps[t]["amb"] for t in chosen])
    out["service_idx"] = np.asarray(sorted(set().union(*(caps[t]["service"] for t in chosen))), dtype=np.int32)
    base = np.asarray(out["cell_type_map"]).copy()
    for x in range(m_ref["m"].width):
        for y in range(m_ref["m"].height):
            cell = m_ref["m"].get_cell_contents(x, y)[0]
            if cell.cell_type == "ControlledRoad":
                base[y, x] = mg_names.index(cell.road_type)
            assert cell.base_color == Defaults.ZONE_COLORS[mg_names[base[y, x]]], (x, y, cell.cell_type)
    out["cell_base_type_map"] = base.astype(np.int8)
    zones = sorted(Defaults.ZONE_COLORS)
    out["zone_names"] = np.asarray(json.dumps(zones))
    out["zone_rgb"] = np.asarray([rgb(Defaults.ZONE_COLORS[z]) for z in zones], dtype=np.uint8)
    vnames = ["VEHICLE_BASE_COLOR", "VEHICLE_PARKED_COLOR", "VEHICLE_MALFUNCTION_COLOR", "VEHICLE_COLLISION_COLOR",
              "VEHICLE_CONTRAFLOW_OVERTAKE_COLOR", "SERVICE_VEHICLE_BASE_COLOR"]
    out["vehicle_names"] = np.asarray(json.dumps(vnames))
    out["vehicle_rgb"] = np.asarray([rgb(getattr(Defaults, v)) for v in vnames], dtype=np.uint8)

    # ---- coverage, on the reference run alone ----
    assert not Defaults.CHANGE_ASSIGNED_CELL_COLOR_ON_STOP and Defaults.AGENT_PORTRAYAL_LEVEL >= 1
    shown = set().union(*(caps[t]["tags"] for t in chosen))
    for tag in CELL_TAGS + VEHICLE_TAGS:
        assert tag in shown, f"{name}: the frames do not show {tag}"
    assert len([t for t in shown if t.startswith("rain_")]) >= 3, "fewer than three rain-tinted cell types"
    assert (np.diff(out["frame_ticks"]) == 1).any(), "no two consecutive frames"
    assert np.array_equal(out["frame_steps"], out["frame_ticks"] + 1), "step_count is not ticks stepped"
    for k, t in enumerate(chosen):
        assert out["ambiguous"][k].sum() * 100 <= caps[t]["n_veh_cells"], f"tick {t}: more than 1 % of the vehicle cells are ambiguous"
    path = os.path.join(HERE, f"{name}.npz")
    write_npz(path, out)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("trace_") and f.endswith(".npz"))
    size = os.path.getsize(path)
    assert size <= largest, f"{path}: {size} bytes, the largest fixture so far has {largest}"
    print(f"[{name}] frames at {chosen} show {sorted(shown)}; ambiguous cells {int(out['ambiguous'].sum())}; size={size}")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        for j in SCENARIOS:     # one process per scenario: Defaults are read at import time
            subprocess.run([sys.executable, os.path.abspath(__file__), j], check=True, cwd="/tmp")
    else:
        run(what)


if __name__ == "__main__":
    main()
