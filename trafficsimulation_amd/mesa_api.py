"""Mesa-shaped facade over the engine: the API surface that the reference's server, portrayal code
and Tornado handlers use (SURVEY.md §8(b) "API surface the Python facade must keep").

    model = CityModel(width=200, height=200, seed=1)        # the reference's world for that seed (worldgen), or
    model = CityModel(width=4096, height=4096, seed=1, world="synthetic")   # fast vectorised look-alike (citygen), or
    model = CityModel.from_tables(tables, seed=1)           # world tables captured elsewhere
    VehicleAgent("veh_1", model, start_cell, target_cell, population_type="through")
    model.step()                                            # CityModel.step (city_model.py:1831-1860)
    model.grid[x, y], model.schedule.agents, model.occupancy_map, agent.get_portrayal() ...

All state lives on the device; the Python objects are *views* that read a per-tick snapshot
(downloaded lazily, once per tick, the first time anything asks).  Host-side writes that the
reference's UI performs directly on numpy maps (cell.py:241-251: set_light_stop/go) are collected in
the host copy of stop_map and uploaded before the next tick.

Differences from the reference that a caller can observe:
  * `CityModel(width, height, seed=..., **ctor_kwargs)` builds the same world as the reference does after
    `random.seed(seed)` (trafficsimulation_amd.worldgen; the constructor keywords are the reference's) and hands
    the global stream on to the engine in the state world-gen left it in; `world="synthetic"` selects citygen.
  * individual `agent.step()` calls are not meaningful: agents are stepped on the device in the
    shuffled order.  `model.schedule.step()` therefore runs the decide + move phases of one tick.
  * with `traffic={...}` the engine's traffic generator spawns internal / through / service vehicles itself;
    they show up as VehicleAgent / ServiceVehicleAgent views (ids "V_<spawn index>" / "SV_<spawn index>": the
    reference's id strings are not kept on the device), `model.city_blocks` holds CityBlock views.
  * learning light controllers are not part of the engine.  Under TRAFFIC_LIGHT_AGENT_ALGORITHM = "EXTERNAL" (or the
    reference's name "NEIGHBOR_RL_BATCHED") the groups decide nothing themselves and the caller drives them between ticks:
    `model.light_states()`, `model.control_lights(actions)`, `model.request_phases(phases)`
    (include/trafficsim_lights_ext.h); the policy and its training are the caller's torch code.  "RL_A2C_BATCHED" and
    "GAT_DQN_BATCHED" select the environment side of those two controllers (include/trafficsim_lights_proto.h): their
    states, rewards and - `model.control_lights_q(q)` - GAT-DQN's epsilon-greedy step on the global stream; the learners
    (update_a2c, _train_dqn) stay the caller's.  The non-batched variants (NEIGHBOR_RL, GAT_DQN) draw and infer inside the
    shuffled schedule and are out of scope.
  * rain clouds are not exposed as agents (only `model.rain_map`).
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Optional

import numpy as np

from . import _capi as capi
from .world import build_engine

DIR_NAMES = ["N", "E", "S", "W"]
DIRECTION_ICONS = {"N": "↑", "S": "↓", "E": "→", "W": "←"}


def str_to_unique_int(s: str) -> int:
    """utilities/general.py:12-14."""
    return int(hashlib.md5(s.encode("utf-8")).hexdigest(), 16)


class Defaults:
    """The subset of config.py `Defaults` the facade reads; engine parameters are set through
    `CityModel(defaults={...})` with the reference's attribute names."""
    VEHICLE_BASE_COLOR = "black"
    VEHICLE_PARKED_COLOR = "aliceblue"
    VEHICLE_MALFUNCTION_COLOR = "yellow"
    VEHICLE_COLLISION_COLOR = "red"
    VEHICLE_CONTRAFLOW_OVERTAKE_COLOR = "orange"
    SERVICE_VEHICLE_BASE_COLOR = "darkolivegreen"
    AVAILABLE_CITY_BLOCKS = ["Residential", "Office", "Market", "Leisure", "Other"]
    AGENT_PORTRAYAL_LEVEL = 2
    ZONE_COLORS = {"Road": "saddlebrown", "Intersection": "yellow", "Nothing": "white", "TrafficLight": "lime",
                   "TrafficLightStop": "red", "ControlledRoad": "thistle", "ControlledRoadStop": "salmon",
                   # config.py:98-120, for worlds whose tables carry `cell_type_map` (worldgen)
                   "Residential": "cadetblue", "Office": "orange", "Market": "green", "Leisure": "palevioletred",
                   "Other": "darkkhaki", "Empty": "papayawhip", "Sidewalk": "grey", "Wall": "black", "R1": "dodgerblue",
                   "R2": "saddlebrown", "R3": "darkgreen", "IntersectionPending": "darkkhaki", "HighwayEntrance": "blue",
                   "HighwayExit": "royalblue", "BlockEntrance": "magenta"}


from .worldgen import CELL_TYPE_NAMES as _CELL_TYPE_NAMES


class CellAgent:
    """View of one grid cell (cell.py:11-60): type and directions come from the static maps."""

    def __init__(self, model: "CityModel", x: int, y: int):
        self.model = self.city_model = model
        self.position = self.pos = (x, y)
        self.id = f"Cell_{x}_{y}"
        self.unique_id = str_to_unique_int(self.id)
        self.light = None
        self.intersection_group = None
        self.controlled_blocks: List["CellAgent"] = []

    @property
    def cell_type(self) -> str:
        x, y = self.position
        m = self.model
        if m._cell_type_map is not None:          # the reference's own type strings (worldgen tables)
            return _CELL_TYPE_NAMES[int(m._cell_type_map[y, x])]
        if (x, y) in m._light_index:
            return "TrafficLight"
        if m.intersection_map[y, x]:
            return "Intersection"
        if (x, y) in m._controlled_cells:
            return "ControlledRoad"
        return "Road" if m.is_road_map[y, x] else "Nothing"

    @property
    def block_id(self):
        """CellAgent.block_id of block cells and block entrances (None elsewhere, or without a `block_id_map` table)."""
        m = self.model
        b = int(m._block_id_map[self.position[1], self.position[0]]) if m._block_id_map is not None else 0
        return b or None

    @property
    def block_type(self):
        b = self.block_id
        blk = self.model.city_blocks.get(b) if b else None
        return blk.block_type if blk is not None else None

    @property
    def road_type(self):
        ct = self.cell_type
        return ct if ct in ("R1", "R2", "R3") else None

    @property
    def directions(self) -> List[str]:
        x, y = self.position
        bits = int(self.model.allowed_dirs_map[y, x])
        return [DIR_NAMES[k] for k in range(4) if bits & (1 << k)]

    def get_position(self):
        return self.position

    # ---- names and predicates the UI's drop-downs use (cell.py:160-195) -------------------------------------------------
    def get_display_name(self):
        ct = self.cell_type
        x, y = self.position
        m = self.model
        if ct == "Intersection":
            return f"Intersection_{x}_{y}"                      # the custom_id place_cell gave it (city_model.py:240)
        if ct == "BlockEntrance":
            return f"BlockEntrance_{self.block_id}"
        if ct in ("HighwayEntrance", "HighwayExit"):            # _format_highway_label (cell.py:77-156)
            if y == 0:
                cardinal = "South"
            elif y == m.height - 1:
                cardinal = "North"
            elif x == 0:
                cardinal = "West"
            elif x == m.width - 1:
                cardinal = "East"
            else:
                cardinal = "Center"
            horizontal = cardinal in ("South", "North")
            # highway_id is "highway_horizontal" / "highway_vertical" (city_model.py:1413-1416): one id per orientation,
            # so the label's group index is always 1
            same = m.highway_entrances if ct == "HighwayEntrance" else m.highway_exits
            if horizontal:
                coll = sorted((c for c in same if c.position[1] == y), key=lambda c: c.position[0])
            else:
                coll = sorted((c for c in same if c.position[0] == x), key=lambda c: c.position[1])
            kind = "Entrance" if ct == "HighwayEntrance" else "Exit"
            return f"{'Horizontal' if horizontal else 'Vertical'}_1_{cardinal}_{kind}_{coll.index(self) + 1}"
        if ct == "TrafficLight" and self.intersection_group is not None:
            g = self.intersection_group
            return f"TrafficLight_I{g.id}_#{g.traffic_lights.index(self)}"
        return self.position

    def is_block_entrance(self):
        return self.cell_type == "BlockEntrance"

    def is_highway_entrance(self):
        return self.cell_type == "HighwayEntrance"

    def is_highway_exit(self):
        return self.cell_type == "HighwayExit"

    def is_controlled_road(self):
        return self.cell_type == "ControlledRoad"

    def set_light_stop(self):   # cell.py:241-245
        self.model._write_stop([self.position] + [c.position for c in self.controlled_blocks], 1)

    def set_light_go(self):     # cell.py:247-251
        self.model._write_stop([self.position] + [c.position for c in self.controlled_blocks], 0)

    def is_traffic_light(self):
        return self.cell_type == "TrafficLight"

    def get_portrayal(self):
        x, y = self.position
        ct = self.cell_type
        is_stop = self.model.stop_map[y, x] == 1
        # cell.py:274-299 through the table the device renderer uses (render.py): a name where the reference returns the
        # name, '#rrggbb' where it returns desaturate's output - one cell and one pixel cannot disagree
        from . import render as _render
        grp = self.intersection_group
        pend = ct == "Intersection" and grp is not None and grp.pending_phase is not None
        base = self.model._cell_base_type_map
        rt = f"ControlledRoad:{_CELL_TYPE_NAMES[int(base[y, x])]}" if ct == "ControlledRoad" and base is not None and self.model._cell_type_map is not None else ct
        color = _render.cell_color(rt, pend, bool(is_stop), bool(self.model.rain_map[y, x] > 0), self.model._render_defaults())
        p = {"Shape": "rect", "w": 1.0, "h": 1.0, "Filled": True, "Layer": 0, "Color": color, "Position": self.position}
        if ct == "ControlledRoad":
            p["Control State"] = "Stop" if is_stop else "Go"
        if self.block_id is not None:               # cell.py:316-317
            p["Block ID"] = self.block_id
        arrows = [DIRECTION_ICONS[d] for d in self.directions]
        if arrows:
            p["Directions"] = " ".join(arrows)
        return p


class VehicleAgent:
    """VehicleAgent(custom_id, model, start_cell, target_cell, population_type, vehicle_type)
    (vehicle_base.py:29-89).  Construction places the vehicle and plans its path on the device."""

    def __init__(self, custom_id, model: "CityModel", start_cell: CellAgent, target_cell: CellAgent,
                 population_type: str = "undefined", vehicle_type: str = "undefined", path=None):
        self.id = custom_id
        self.unique_id = str_to_unique_int(custom_id)
        self.model = self.city_model = model
        self.start_cell, self.target = start_cell, target_cell
        self.population_type, self.vehicle_type = population_type, vehicle_type
        self.base_color = Defaults.VEHICLE_BASE_COLOR
        if self.unique_id in model._vehicle_by_uid:
            raise Exception(f"Agent with unique id {self.unique_id!r} already added to scheduler")
        model._flush_host_writes()
        pop = [capi.POP.get(population_type, 0)]
        spawn_idx = model.engine.num_spawned()   # shared with the vehicles the engine's generator creates
        if path is None:
            model.engine.add_vehicles([start_cell.position], [target_cell.position], pop)
        else:
            model.engine.add_vehicles([start_cell.position], [target_cell.position], pop, [0, len(path)], path)
        self._spawn_idx = spawn_idx
        model._n_spawned = spawn_idx + 1
        model._vehicles[self._spawn_idx] = self
        model._vehicle_by_uid[self.unique_id] = self
        model._invalidate()

    @classmethod
    def _view(cls, model: "CityModel", spawn_idx: int, meta) -> "VehicleAgent":
        """A vehicle the engine's traffic generator created (dynamic_traffic_generator.py:398-430)."""
        vt = int(meta[capi.M_FIELDS.index("vehicle_type")])
        klass = ServiceVehicleAgent if vt else cls
        v = object.__new__(klass)
        v.id = f"{'SV' if vt else 'V'}_{spawn_idx}"
        v.unique_id = str_to_unique_int(v.id)
        v.model = v.city_model = model
        v.start_cell = None
        v._static_target = None if vt else model.cell(int(meta[2]), int(meta[3]))
        v.population_type = {1: "internal", 2: "through"}.get(int(meta[1]), "undefined")
        v.vehicle_type = {capi.TRIP_SERVICE_FOOD: "food", capi.TRIP_SERVICE_WASTE: "waste"}.get(vt, "undefined")
        v.base_color = Defaults.VEHICLE_BASE_COLOR
        v._spawn_idx = spawn_idx
        model._vehicles[spawn_idx] = v
        model._vehicle_by_uid[v.unique_id] = v
        return v

    @property
    def target(self):
        t = self.__dict__.get("_static_target")
        if t is not None:
            return t
        m = self.model._meta_row(self._spawn_idx)     # service vehicles change their target
        return None if m is None else self.model.cell(int(m[2]), int(m[3]))

    @target.setter
    def target(self, cell):
        self.__dict__["_static_target"] = cell

    # ---- live state (one row of the per-tick snapshot) --------------------------------------------
    def _row(self):
        return self.model._vehicle_row(self._spawn_idx)

    def _field(self, name):
        r = self._row()
        return None if r is None else int(r[capi.V_FIELDS.index(name)])

    @property
    def pos(self):
        r = self._row()
        return None if r is None else (int(r[1]), int(r[2]))   # None once removed, like MultiGrid.remove_agent

    @property
    def direction(self):
        d = self._field("direction")
        return None if d is None or d < 0 else DIR_NAMES[d]

    current_speed = property(lambda s: s._field("current_speed"))
    base_speed = property(lambda s: s._field("base_speed"))
    max_steps = property(lambda s: s._field("max_steps"))
    stuck_ticks = property(lambda s: s._field("stuck_ticks"))
    steps_traveled = property(lambda s: s._field("steps_traveled"))
    path_retry_cooldown = property(lambda s: s._field("cooldown"))

    def _flag(self, bit):
        f = self._field("flags")
        return bool(f & bit) if f is not None else False

    is_stuck = property(lambda s: s._flag(capi.F_STUCK))
    is_parked = property(lambda s: s._flag(capi.F_PARKED))
    is_in_collision = property(lambda s: s._flag(capi.F_COLLISION))
    is_in_malfunction = property(lambda s: s._flag(capi.F_MALFUNCTION))
    is_overtaking = property(lambda s: s._flag(capi.F_OVERTAKING))
    is_in_stuck_detour = property(lambda s: s._flag(capi.F_DETOUR))
    blocked_by_vehicle = property(lambda s: s._flag(capi.F_BLOCKED))

    @property
    def path(self):
        i = self.model._active_index(self._spawn_idx)
        return [] if i is None else [tuple(c) for c in self.model.engine.path(i).tolist()]

    def is_stranded(self):
        return self.is_in_collision or self.is_in_malfunction

    def get_current_direction(self):
        return self.direction

    def get_current_path(self):
        return self.path

    def get_target(self):
        return self.target.get_position()

    def get_vehicle_type_name(self):
        return "Vehicle"

    def get_description(self):
        return f"{self.population_type} Citizen"

    def step(self):
        raise NotImplementedError("vehicles are stepped on the device, in the shuffled order, by CityModel.step()")

    def get_portrayal(self):   # vehicle_base.py:817-865
        p = {"Shape": "circle", "r": 0.66, "Filled": True, "Layer": 1, "Color": self.base_color}
        base = Defaults.VEHICLE_CONTRAFLOW_OVERTAKE_COLOR if (self.is_overtaking or self.is_in_stuck_detour) else self.base_color
        flash_on = (self.model.step_count % 2) == 0
        if self.is_in_collision:
            p["Color"] = base if flash_on else Defaults.VEHICLE_COLLISION_COLOR
        elif self.is_in_malfunction:
            p["Color"] = base if flash_on else Defaults.VEHICLE_MALFUNCTION_COLOR
        elif self.is_parked:
            p["Color"] = base if flash_on else Defaults.VEHICLE_PARKED_COLOR
        else:
            p["Color"] = base
        p["Type"] = self.get_vehicle_type_name()
        p["Identifier"] = self.unique_id
        p["Description"] = self.get_description()
        p["Position"] = self.pos
        p["Direction"] = DIRECTION_ICONS.get(self.direction, "?")
        p["Speed"] = self.current_speed
        p["Current Destination"] = self.target.id if self.target else "None"
        flags = []
        if self.is_in_stuck_detour: flags.append("Detouring (Stuck)")
        if self.is_overtaking: flags.append("Overtaking")
        if self.is_in_malfunction: flags.append("Malfunctioning")
        if self.is_in_collision: flags.append("InCollision")
        if self.is_parked: flags.append("Parked")
        if (self.stuck_ticks or 0) > 0: flags.append(f"Stuck ({self.stuck_ticks})")
        p["Status"] = ", ".join(flags) if flags else "Ok"
        return p


class ServiceVehicleAgent(VehicleAgent):
    """View of a ServiceVehicleAgent (vehicle_service.py:13-158); created by the engine's traffic generator."""

    def __init__(self, custom_id, model: "CityModel", start_cell: CellAgent, service_type: str, max_load=None):
        """ServiceVehicleAgent(vid, model, entrance, sv_type) as the UI's CreateServiceVehicleHandler calls it
        (vehicle_control.py:182-206); the generator's own service vehicles arrive as views (VehicleAgent._view)."""
        if max_load is not None:
            raise NotImplementedError("max_load comes from Defaults (the handler never passes it)")
        self.id = custom_id
        self.unique_id = str_to_unique_int(custom_id)
        if self.unique_id in model._vehicle_by_uid:
            raise Exception(f"Agent with unique id {self.unique_id!r} already added to scheduler")
        self.model = self.city_model = model
        self.start_cell = start_cell
        self.population_type = "through"
        self.vehicle_type = service_type.lower()
        self.base_color = Defaults.VEHICLE_BASE_COLOR
        model._flush_host_writes()
        self._spawn_idx = model.engine.num_spawned()
        model.engine.add_service_vehicle(start_cell.position[0], start_cell.position[1],
                                         capi.TRIP_SERVICE_FOOD if self.vehicle_type == "food" else capi.TRIP_SERVICE_WASTE)
        model._n_spawned = self._spawn_idx + 1
        model._vehicles[self._spawn_idx] = self
        model._vehicle_by_uid[self.unique_id] = self
        model._invalidate()

    service_type = property(lambda s: "Food" if s.vehicle_type == "food" else "Waste")

    def _svc(self):
        return self.model._service_row(self._spawn_idx)

    @property
    def current_load(self):
        r = self._svc()
        return None if r is None else float(r[0])

    @property
    def max_load(self):
        r = self._svc()
        return None if r is None else float(r[1])

    @property
    def current_block(self):
        r = self._svc()
        blocks = list(self.model.city_blocks.values())
        return None if r is None or int(r[2]) < 0 or int(r[2]) >= len(blocks) else blocks[int(r[2])]

    @property
    def phase(self):
        m = self.model._meta_row(self._spawn_idx)
        return None if m is None else {0: "to_block", 1: "servicing", 2: "to_exit"}.get(int(m[5]))

    def _get_base_color(self):
        return Defaults.SERVICE_VEHICLE_BASE_COLOR

    def get_vehicle_type_name(self):
        return f"{self.service_type}ServiceVehicle"

    def get_description(self):
        return f"{self.service_type}-Service Vehicle ({self.current_load:.1f}/{self.max_load})"

    def get_portrayal(self):
        p = super().get_portrayal()
        b = self.current_block
        p["Destination Block"] = f"{b.id}, {b.block_type}" if b else "None"
        return p


class CityBlock:
    """View of a CityBlock (city_block.py:14-150): stock lives in the engine."""

    def __init__(self, model: "CityModel", index: int, block_type: str, inner_cells: int, entrances, block_id=None):
        self.model = self.city_model = model
        self.index = index
        self.block_id = int(block_id) if block_id is not None else index + 1   # key in model.city_blocks (city_model.py:1743)
        self.id = f"CB_{self.block_id}"                                          # custom_id of _spawn_city_block (1729)
        self.unique_id = str_to_unique_int(self.id)
        self.block_type = block_type
        self._n_inner = int(inner_cells)
        self._entrances = list(entrances)
        sv = model._service_cfg
        self.max_food_units = self._n_inner * sv.get("food_capacity_per_cell", 2.0)
        self.max_waste_units = self._n_inner * sv.get("waste_capacity_per_cell", 1.5)

    def get_entrances(self):
        return self._entrances

    def get_food_units(self):
        return float(self.model._block_rows()[self.index, 0])

    def get_waste_units(self):
        return float(self.model._block_rows()[self.index, 1])

    def needs_food(self):
        return self.block_type in ("Market", "Leisure")        # Defaults.CITY_BLOCK_THAT_NEED_FOOD

    def produces_waste(self):
        return True                                             # Defaults.CITY_BLOCK_THAT_PRODUCE_WASTE = all types

    def food_shortage(self):
        return self.max_food_units - self.get_food_units()

    def waste_surplus(self):
        return self.get_waste_units()

    def step(self):
        raise NotImplementedError("city blocks are stepped by CityModel.step()")

    def __repr__(self):
        return (f"<CityBlock {self.id} | {self.block_type} | Food {self.get_food_units():.1f}/{self.max_food_units}, "
                f"Waste {self.get_waste_units():.1f}/{self.max_waste_units}>")


class IntersectionLightGroup:
    """View of one light group (intersection_light_group.py:30-116)."""

    def __init__(self, model: "CityModel", index: int, lights: List[CellAgent], cells: List[CellAgent]):
        self.model = self.city_model = model
        self.index = index
        self.id = f"Intersection_{index + 1}"
        self.unique_id = str_to_unique_int(self.id)
        self.traffic_lights = lights
        self.intersection_cells = cells

    def _f(self, name):
        return int(self.model._group_rows()[self.index, capi.G_FIELDS.index(name)])

    @property
    def current_phase(self):
        v = self._f("current_phase")
        return None if v < 0 else v

    @property
    def pending_phase(self):
        v = self._f("pending_phase")
        return None if v < 0 else v

    queue_timer = property(lambda s: s._f("queue_timer"))
    gap_timer = property(lambda s: s._f("gap_timer"))
    fixed_time_timer = property(lambda s: s._f("fixed_time_timer"))
    ns_pressure = property(lambda s: s._f("ns_pressure"))
    ew_pressure = property(lambda s: s._f("ew_pressure"))
    # external light control only (intersection_light_group.py:91-92)
    _rl_phase = property(lambda s: int(s.model._light_controller()[s.index, 0]))
    rl_timer = property(lambda s: int(s.model._light_controller()[s.index, 1]))
    epsilon = property(lambda s: float(s.model._light_epsilon()[s.index]))      # GAT_DQN_BATCHED (intersection_light_group.py:102)

    # ---- links (intersection_light_group.py:293-307) --------------------------------------------------------------
    def get_opposite_traffic_lights(self):
        """{"N-S": [...], "W-E": [...]}; like the reference, the first call re-runs populate_links() for the group."""
        m = self.model
        m.engine.group_links(self.index, True)
        t = m.tables
        ns = np.asarray(t["g_ns_lights"])[int(t["g_ns_lights_off"][self.index]):int(t["g_ns_lights_off"][self.index + 1])]
        ew = np.asarray(t["g_ew_lights"])[int(t["g_ew_lights_off"][self.index]):int(t["g_ew_lights_off"][self.index + 1])]
        return {"N-S": [m.traffic_lights[int(i)] for i in ns], "W-E": [m.traffic_lights[int(i)] for i in ew]}

    def get_neighbor_groups(self):
        """{direction: group}: the table as the constructor left it until the links are re-populated."""
        m = self.model
        key = "g_neighbors" if m.engine.group_links(self.index, False) else "g_neighbors_ctor"
        nb = np.asarray(m.tables.get(key, m.tables["g_neighbors"])).reshape(-1, 4, 2)[self.index]
        return {DIR_NAMES[int(d)]: m.intersection_light_groups[int(g)] for d, g in nb if d >= 0 and g >= 0}

    def get_intermediate_groups(self):
        """Groups lying between this one and a neighbour without closing all lanes (the reference keeps a set; a list in
        ascending group order here).  Needs the `g_intermediate*` tables (worldgen and make_golden's `worlds` job write
        them; trace fixtures captured earlier do not hold them)."""
        m = self.model
        key = "g_intermediate" if m.engine.group_links(self.index, False) else "g_intermediate_ctor"
        if key not in m.tables:
            raise NotImplementedError("these world tables carry no intermediate-group lists")
        off = np.asarray(m.tables[key + "_off"])
        return [m.intersection_light_groups[int(g)] for g in np.asarray(m.tables[key])[int(off[self.index]):int(off[self.index + 1])]]

    def set_all_go_with_neighbors_and_intermediate(self):     # 332-337
        self.set_all_go_with_neighbors()
        for g in self.get_intermediate_groups():
            g.set_all_go()

    def set_all_stop_with_neighbors_and_intermediate(self):   # 339-344
        self.set_all_stop_with_neighbors()
        for g in self.get_intermediate_groups():
            g.set_all_stop()

    def set_all_go_with_neighbors(self):      # 322-325
        self.set_all_go()
        for g in self.get_neighbor_groups().values():
            g.set_all_go()

    def set_all_stop_with_neighbors(self):    # 327-330
        self.set_all_stop()
        for g in self.get_neighbor_groups().values():
            g.set_all_stop()

    def set_all_stop(self):     # intersection_light_group.py:316-317
        for tl in self.traffic_lights:
            tl.set_light_stop()

    def set_all_go(self):
        for tl in self.traffic_lights:
            tl.set_light_go()

    def step(self):
        raise NotImplementedError("light groups are stepped on the device by CityModel.step()")


class _TrafficStats:
    """dynamic_traffic_generator.py:102-131 counters, read from the engine."""
    _FIELDS = ("stuck", "collisions", "malfunctions", "overtaking", "in_stuck_detour", "parked", "live_internal",
               "live_through", "count_completed_internal", "count_completed_through", "total_distance_internal",
               "total_distance_through", "errored_internal", "errored_through", "total_duration_internal",
               "total_duration_through", "elapsed", "created_internal", "created_through", "created_service_food",
               "created_service_waste", "live_service_food", "live_service_waste")

    def __init__(self, model):
        self._model = model
        self.unique_id = "DTA"

    def __getattr__(self, name):
        if name in _TrafficStats._FIELDS:
            return getattr(self._model._counters(), name)
        raise AttributeError(name)

    @property
    def cached_stats(self) -> Dict[str, object]:
        """DynamicTrafficAgent.cached_stats (dynamic_traffic_generator.py:525-648): refreshed inside the generator's own step
        every STATISTICS_UPDATE_INTERVAL ticks, read by ui_modules/traffic_statistics.py between updates; empty before the
        first update, like the reference's.  A generator without any population to spawn is not stepped as an agent of
        its own by the engine (nothing it does could be seen): its counters are served as they are then."""
        cs = self._model.engine.cached_stats()
        if cs or self._model._traffic_armed:
            return cs
        c = self._model._counters()
        return {f: getattr(c, f) for f in _TrafficStats._FIELDS}


class _RainManager:
    """What the RainControl card and the /spawn_rain handler use of RainManager (rain_control.py:22-73)."""

    def __init__(self, model):
        self._model = model
        self.unique_id = "RainManager"

    cooldown = property(lambda s: int(s._model.engine.rain_info().cooldown))
    counter = property(lambda s: int(s._model.engine.rain_info().counter))

    def add_random_rain(self):
        self._model._flush_host_writes()
        self._model.engine.rain_spawn()
        self._model._invalidate()

    def step(self):
        raise NotImplementedError("the rain manager is stepped by CityModel.step()")


class _Grid:
    """MultiGrid view: grid[x, y] -> [CellAgent, vehicles in arrival order...]."""

    def __init__(self, model):
        self.model, self.width, self.height = model, model.width, model.height

    def __getitem__(self, xy):
        x, y = xy
        return [self.model.cell(x, y)] + self.model._vehicles_at(x, y)

    def coord_iter(self):
        for x in range(self.width):
            for y in range(self.height):
                yield self[x, y], (x, y)

    def out_of_bounds(self, pos):
        return not self.model.in_bounds(*pos)


class _Schedule:
    """RandomActivation view: .agents in insertion order, .step() = one device tick."""

    def __init__(self, model):
        self.model = model
        self.steps = 0

    @property
    def agents(self):
        m = self.model
        return list(m.intersection_light_groups) + list(m.city_blocks.values()) \
            + ([m.dynamic_traffic_generator] if m.dynamic_traffic_generator else []) + m.active_vehicle_agents

    def get_agent_count(self):
        return self.model.engine.num_scheduled()

    def step(self):
        m = self.model
        m._flush_host_writes()
        m.engine.step(1)
        m._invalidate()
        self.steps += 1


class CityModel:
    """CityModel (city_model.py:26-205) on the device engine."""

    def __init__(self, width=200, height=200, seed=None, defaults: Optional[dict] = None, tables: Optional[dict] = None,
                 engine: Optional[capi.CApi] = None, global_seed: Optional[int] = None, global_state=None,
                 sched_state=None, traffic: Optional[dict] = None, world: str = "reference", trip_log: Optional[int] = None,
                 **world_kwargs):
        import random as _random
        self._seed = seed if seed is not None else _random.random()
        if traffic is not None and "gradual_city_block_resources" in world_kwargs:   # ctor kwarg -> CityBlock mode (city_model.py:50, 1735)
            traffic = dict(traffic, gradual=bool(world_kwargs["gradual_city_block_resources"]))
        if tables is None and world == "synthetic":
            from . import citygen
            tables = citygen.generate(width, height, seed=seed if seed is not None else 1, **world_kwargs)
        elif tables is None:
            # CityModel.__init__'s build sequence (city_model.py:124-148) draws from the global `random` stream; the
            # engine's global stream continues from where that leaves it, as the reference's agents would
            from . import worldgen
            d = defaults or {}
            algo = d.get("TRAFFIC_LIGHT_AGENT_ALGORITHM")
            if capi.LIGHT_ALGORITHMS.get(algo) == capi.LIGHT_ALGORITHMS["EXTERNAL"] or algo in capi.LIGHT_PROTOCOLS:
                world_kwargs = dict(world_kwargs, approach_road_types=True)   # (penalty_score of the state vector)
            world_kwargs = dict(world_kwargs, cell_base_types=True)           # (the renderer's palette: render.type_plane)
            tables = worldgen.generate_world(width, height, seed=global_seed if global_seed is not None else self._seed,
                                             rain_enabled=bool(d.get("RAIN_ENABLED", True)), enable_traffic=traffic is not None,
                                             block_entrance_road_level=int(d.get("BLOCK_ENTRANCE_ROAD_LEVEL", 0)), **world_kwargs)
            if global_state is None:
                global_state = tables["global_rng_state"]
        self.width, self.height = int(tables["width"]), int(tables["height"])
        if engine is None:
            from ._lib import new_engine
            engine = new_engine()                   # the HIP engine; raises loudly when it is unavailable
        self.engine = engine
        self.tables = tables
        sched_seed = self._seed if isinstance(self._seed, int) else int(self._seed * 2 ** 53)
        gseed = global_seed if global_seed is not None else sched_seed
        # random.setstate()-style states take precedence over integer seeds (exact replays of a reference run)
        build_engine(engine, tables, defaults=defaults or {}, global_seed=gseed, sched_seed=sched_seed,
                     global_state=global_state, sched_state=sched_state)
        # trip_log=capacity: the trip log (include/trafficsim_triplog.h) is on before the first vehicle is placed, so every
        # record knows its origin
        if trip_log is not None:
            engine.triplog_start(int(trip_log))
        # DynamicTrafficAgent("DTA", self) (city_model.py:203-204): traffic = {"P_int", "P_thr", "start_offset",
        # "service_food", "service_waste", ...} arms the engine's generator; it draws day 0 from the global stream now
        self._service_cfg = dict(traffic or {})
        self._traffic_armed = traffic is not None
        self._defaults = dict(defaults or {})
        if traffic is not None:
            engine.set_traffic_generator(tables, internal_per_day=traffic.get("P_int", 10000),
                                         passing_per_day=traffic.get("P_thr", 2400),
                                         start_offset_seconds=traffic.get("start_offset", 6 * 3600), service=traffic)
        self.allowed_dirs_map = np.asarray(tables["allowed_dirs_map"], dtype=np.uint8)
        self.is_road_map = np.asarray(tables["is_road_map"], dtype=np.int8)
        self.road_type_map = np.asarray(tables["road_type_map"], dtype=np.int8)
        self.intersection_map = np.asarray(tables["intersection_map"], dtype=np.int8)
        self._cell_type_map = np.asarray(tables["cell_type_map"]) if "cell_type_map" in tables else None
        self._block_id_map = np.asarray(tables["block_id_map"]) if "block_id_map" in tables else None
        self._cell_base_type_map = np.asarray(tables["cell_base_type_map"]) if "cell_base_type_map" in tables else None
        self._stop_host = np.zeros((self.height, self.width), dtype=np.int8)
        self._stop_dirty = False
        self.step_count = 0
        self._n_spawned = 0
        self._vehicles: Dict[int, VehicleAgent] = {}
        self._vehicle_by_uid: Dict[int, VehicleAgent] = {}
        self._cells: Dict[tuple, CellAgent] = {}
        self._snap = None
        self._render_ready = False      # the renderer's tables go to the engine on the first render() of every model
        self.user_selected_traffic_light = self.user_selected_intersection = self.user_selected_opposite = None
        # lights / groups
        lxy = np.asarray(tables["light_xy"]).reshape(-1, 2)
        self._light_index = {(int(x), int(y)): i for i, (x, y) in enumerate(lxy)}
        self.traffic_lights = [self.cell(int(x), int(y)) for x, y in lxy]
        coff, cxy = np.asarray(tables["light_ctrl_off"]), np.asarray(tables["light_ctrl_xy"]).reshape(-1, 2)
        self._controlled_cells = set()
        self.controlled_roads = []
        for i, tl in enumerate(self.traffic_lights):
            for x, y in cxy[coff[i]:coff[i + 1]]:
                c = self.cell(int(x), int(y))
                c.light = tl
                tl.controlled_blocks.append(c)
                if (int(x), int(y)) not in self._controlled_cells:
                    self._controlled_cells.add((int(x), int(y)))
                    self.controlled_roads.append(c)
        goff = np.asarray(tables["g_light_off"])
        ioff, ixy = np.asarray(tables["g_icell_off"]), np.asarray(tables["g_icell_xy"]).reshape(-1, 2)
        self.intersection_light_groups = []
        for g in range(len(goff) - 1):
            lights = self.traffic_lights[goff[g]:goff[g + 1]]
            cells = [self.cell(int(x), int(y)) for x, y in ixy[ioff[g]:ioff[g + 1]]]
            grp = IntersectionLightGroup(self, g, lights, cells)
            for c in lights + cells:
                c.intersection_group = grp
            self.intersection_light_groups.append(grp)
        self.dynamic_traffic_generator = _TrafficStats(self) if 3 in np.asarray(tables["schedule_kinds0"]) else None
        self.grid = _Grid(self)
        self.schedule = _Schedule(self)
        self.city_blocks = {}
        if 2 in np.asarray(tables["schedule_kinds0"]):
            self.rain_manager = _RainManager(self)
        if "blk_type" in tables and 1 in np.asarray(tables["schedule_kinds0"]):
            eoff, exy = np.asarray(tables["blk_entr_off"]), np.asarray(tables["blk_entr_xy"]).reshape(-1, 2)
            inner = np.asarray(tables.get("blk_inner_cells", np.zeros(len(eoff) - 1)))
            ids = np.asarray(tables["blk_id"]) if "blk_id" in tables else np.arange(1, len(eoff))
            for b, t in enumerate(np.asarray(tables["blk_type"])):
                cb = CityBlock(self, b, Defaults.AVAILABLE_CITY_BLOCKS[int(t)], int(inner[b]),
                               [self.cell(int(x), int(y)) for x, y in exy[eoff[b]:eoff[b + 1]]], block_id=int(ids[b]))
                self.city_blocks[cb.block_id] = cb       # keyed by block_id like the reference's dict
        self.block_entrances = [self.cell(int(x), int(y)) for x, y in np.asarray(tables.get("block_entrances_xy", np.zeros((0, 2)))).reshape(-1, 2)]
        self.highway_entrances = [self.cell(int(x), int(y)) for x, y in np.asarray(tables.get("highway_entrances_xy", np.zeros((0, 2)))).reshape(-1, 2)]
        self.highway_exits = [self.cell(int(x), int(y)) for x, y in np.asarray(tables.get("highway_exits_xy", np.zeros((0, 2)))).reshape(-1, 2)]

    @classmethod
    def from_tables(cls, tables: dict, seed=None, **kw):
        return cls(tables=tables, seed=seed, **kw)

    # ---- stepping ------------------------------------------------------------------------------
    def step(self):
        """city_model.py:1831-1860: density -> decide -> schedule.step() -> step_count += 1."""
        self.schedule.step()
        self.step_count += 1

    def run_parallel_decide(self):   # fused into the engine tick (city_model.py:1811-1829)
        pass

    def _update_density_map(self):   # materialised on demand by the engine (city_model.py:1764-1778)
        pass

    @property
    def density_map(self):
        self._flush_host_writes()
        return self.engine.density()

    # ---- snapshot plumbing -----------------------------------------------------------------------
    def _invalidate(self):
        self._snap = None

    def _snapshot(self):
        if self._snap is None:
            rows = self.engine.vehicles()
            by_spawn = {int(r[0]): i for i, r in enumerate(rows)}
            cells: Dict[tuple, list] = {}
            for r in rows:
                cells.setdefault((int(r[1]), int(r[2])), []).append(int(r[0]))
            self._snap = dict(rows=rows, by_spawn=by_spawn, cells=cells, maps={}, groups=None, counters=None,
                              meta=None, service=None, blocks=None)
            self._n_spawned = self.engine.num_spawned()
        return self._snap

    def _meta_row(self, spawn_idx):
        s = self._snapshot()
        if s["meta"] is None:
            s["meta"] = self.engine.vehicle_meta()
        i = s["by_spawn"].get(spawn_idx)
        return None if i is None else s["meta"][i]

    def _service_row(self, spawn_idx):
        s = self._snapshot()
        if s["service"] is None:
            idx, loads, blk = self.engine.service_vehicles()
            s["service"] = {int(i): (loads[k, 0], loads[k, 1], int(blk[k])) for k, i in enumerate(idx)}
        return s["service"].get(spawn_idx)

    def _block_rows(self):
        s = self._snapshot()
        if s["blocks"] is None:
            s["blocks"] = self.engine.blocks()
        return s["blocks"]

    rain_map = property(lambda s: s._map(capi.MAP_RAIN))

    @property
    def rains(self):
        """city_model.rains as far as its callers go: they only take its length (rain_control.py:33, 67;
        traffic_statistics.py:216)."""
        return [None] * int(self.engine.rain_info().n_rains)

    def _vehicle_row(self, spawn_idx):
        s = self._snapshot()
        i = s["by_spawn"].get(spawn_idx)
        return None if i is None else s["rows"][i]

    def _active_index(self, spawn_idx):
        return self._snapshot()["by_spawn"].get(spawn_idx)

    def _vehicle_view(self, spawn_idx):
        v = self._vehicles.get(spawn_idx)
        if v is None:   # spawned by the engine's traffic generator
            v = VehicleAgent._view(self, spawn_idx, self._meta_row(spawn_idx))
        return v

    def _vehicles_at(self, x, y):
        return [self._vehicle_view(i) for i in self._snapshot()["cells"].get((x, y), [])]

    def _group_rows(self):
        s = self._snapshot()
        if s["groups"] is None:
            s["groups"] = self.engine.groups()
        return s["groups"]

    def _light_controller(self):
        s = self._snapshot()
        if s.get("light_ctrl") is None:
            s["light_ctrl"] = self.engine.lights_controller()
        return s["light_ctrl"]

    def _light_epsilon(self):
        s = self._snapshot()
        if s.get("light_eps") is None:
            s["light_eps"] = self.engine.lights_proto_controller()
        return s["light_eps"]

    def _light_protocol(self) -> int:
        """0: the simple protocol; 1 / 2: RL_A2C_BATCHED / GAT_DQN_BATCHED (include/trafficsim_lights_proto.h)"""
        return capi.LIGHT_PROTOCOLS.get((self._defaults or {}).get("TRAFFIC_LIGHT_AGENT_ALGORITHM"), 0)

    # ---- external light control (include/trafficsim_lights_ext.h, _lights_proto.h), between two step() calls ----------
    def light_states(self, to_host: bool = True):
        """The state vector of every light group, (G, SRL_INPUT_DIMENSIONS) float32, as the reference's get_rl_state
        builds it (rl_simple.py:95-143).  Calling it again before control_lights or step returns the same vectors.
        Under RL_A2C_BATCHED: (G, 13) as rl_a2c.get_rl_state; under GAT_DQN_BATCHED: (features (G, 5, 9), mask (G, 5)) as
        rl_gatdqn.get_gat_state.  to_host=False computes them on the device only (engine.lights_device() /
        lights_proto_device() hold them) and returns None."""
        self._flush_host_writes()
        if self._light_protocol():
            return self.engine.lights_proto_observe(to_host=to_host)
        return self.engine.lights_observe(to_host=to_host)

    def control_lights_q(self, q, want_next: bool = True, to_host: bool = True):
        """GAT_DQN_BATCHED: the reference's epsilon-greedy step on q (G, 2) - numpy or a float32 torch tensor on the engine's
        device - which draws from the global `random` stream like rl_gatdqn.py:289-292.  Returns (actions, rewards, next
        features), (actions, rewards) with want_next=False, None with to_host=False (everything stays in
        engine.lights_proto_device())."""
        self._flush_host_writes()
        out = self.engine.lights_proto_act_q(q, want_next=want_next, to_host=to_host)
        self._invalidate()
        return out

    def control_lights(self, actions, to_host: bool = True):
        """One action per group (0 keep, 1 ask for the other phase; numpy, a sequence or an int8 torch tensor on the
        engine's device): the reference's action protocol (rl_simple.py:226-236).  Returns the next-state vectors; under
        RL_A2C_BATCHED the rewards, under GAT_DQN_BATCHED (rewards, next features) - nothing is drawn.  to_host=False
        brings nothing down and returns None."""
        self._flush_host_writes()
        if self._light_protocol():
            out = self.engine.lights_proto_act(actions, to_host=to_host)
        else:
            out = self.engine.lights_act(actions, want_next=to_host)
        self._invalidate()
        return out

    def request_phases(self, phases) -> None:
        """apply_phase(phase) on every group whose entry is 0 or 1 (-1 = none), for controllers of any other kind."""
        self._flush_host_writes()
        self.engine.lights_request(phases)
        self._invalidate()

    def _counters(self):
        s = self._snapshot()
        if s["counters"] is None:
            s["counters"] = self.engine.counters()
        return s["counters"]

    def _map(self, which):
        s = self._snapshot()
        if which not in s["maps"]:
            s["maps"][which] = self.engine.map(which)
        return s["maps"][which]

    occupancy_map = property(lambda s: s._map(capi.MAP_OCCUPANCY))
    stuck_map = property(lambda s: s._map(capi.MAP_STUCK))

    @property
    def stop_map(self):
        return self._stop_host if self._stop_dirty else self._map(capi.MAP_STOP)

    def _write_stop(self, cells, value):
        if not self._stop_dirty:
            self._stop_host = self._map(capi.MAP_STOP).copy()
            self._stop_dirty = True
        for (x, y) in cells:
            self._stop_host[y, x] = value

    def _flush_host_writes(self):
        if self._stop_dirty:
            self.engine.upload_map(capi.MAP_STOP, self._stop_host)
            self._stop_dirty = False
            self._invalidate()

    # ---- route queries on the current state (include/trafficsim_astar_batch.h) -----------------------
    def find_paths(self, starts, goals, soft_obstacles=False, ignore_flow=False, maximum_steps=None):
        """Routes for many (start, goal) pairs on the model's current maps, all searches in one device launch: a list with
        one path per pair - (x, y) tuples without the start cell, [] for "no path" - each equal to what the pathfinder
        operator (`pathfinding.astar_hip`, i.e. `astar_numba`) returns for that pair.  The simulation is not disturbed."""
        starts = np.asarray(starts, dtype=np.int64).reshape(-1, 2) if len(starts) else np.zeros((0, 2), np.int64)
        goals = np.asarray(goals, dtype=np.int64).reshape(-1, 2) if len(goals) else np.zeros((0, 2), np.int64)
        if len(starts) != len(goals):
            raise ValueError(f"starts and goals must pair up: {len(starts)} starts, {len(goals)} goals")
        self._flush_host_writes()
        q = np.zeros((len(starts), 7), dtype=np.int64)
        q[:, 0:2], q[:, 2:4] = starts, goals
        q[:, 4], q[:, 5] = int(bool(soft_obstacles)), int(bool(ignore_flow))
        q[:, 6] = 0x7FFFFFFF if maximum_steps is None else int(min(maximum_steps, 0x7FFFFFFF))
        off, xy = self.engine.astar_batch(q)
        self._invalidate()          # (the A* counters moved)
        cells = list(map(tuple, xy.tolist()))
        return [cells[off[i]:off[i + 1]] for i in range(len(starts))]

    # ---- traffic observation (include/trafficsim_observe.h) ------------------------------------------
    def observe(self, planes=None):
        """Start accumulating per-cell observation planes on the device (default: all of `capi.OBS_PLANES`), from the next
        step on; `planes=()` or False stops it.  Observation changes nothing the run computes and is not carried by save /
        load / deepcopy / pickle: the model those give has observation off."""
        if planes is False or (isinstance(planes, (list, tuple)) and len(planes) == 0):
            self.engine.observe_stop()
        else:
            self.engine.observe_start(planes)

    def observations(self) -> dict:
        """{plane name: (H, W) uint32} for the planes held, plus "ticks"; with the four ENTER planes also "flow" (their sum,
        uint64: how often a vehicle entered the cell), with SPEED and PRESENT also "mean_speed" (float64, NaN where no
        vehicle was ever seen)."""
        info = self.engine.observe_info()
        out = {name: self.engine.observe_plane(name) for name in info["planes"]}
        if all(n in out for n in capi.OBS_ENTER):
            out["flow"] = sum(out[n].astype(np.uint64) for n in capi.OBS_ENTER)
        if "speed" in out and "present" in out:
            present = out["present"].astype(np.float64)
            out["mean_speed"] = np.divide(out["speed"].astype(np.float64), present, out=np.full(present.shape, np.nan), where=present > 0)
        out["ticks"] = info["ticks"]
        return out

    # ---- trip log (include/trafficsim_triplog.h) ----------------------------------------------------
    def trips(self) -> np.ndarray:
        """One `capi.TRIP_DTYPE` record per vehicle that has left since the model was built with `trip_log=capacity`, in the
        log's canonical order (tick by tick, ascending spawn index inside a tick).  Like observation the log is not carried by
        save / load / deepcopy / pickle: the model those give has the log off."""
        return self.engine.trips()

    def _block_zones(self):
        """(zone plane (H, W) int32, zone names): one zone per city block, made of the block's entrances, then one for the
        highway entrances and one for the highway exits."""
        t = self.tables
        zone = np.full((self.height, self.width), -1, dtype=np.int32)
        names = []
        if "blk_entr_off" in t:
            eoff, exy = np.asarray(t["blk_entr_off"]), np.asarray(t["blk_entr_xy"]).reshape(-1, 2)
            ids = np.asarray(t["blk_id"]) if "blk_id" in t else np.arange(1, len(eoff))
            for b in range(len(eoff) - 1):
                xy = exy[eoff[b]:eoff[b + 1]]
                zone[xy[:, 1], xy[:, 0]] = len(names)
                names.append(f"block_{int(ids[b])}")
        for key, name in (("highway_entrances_xy", "highway_entrances"), ("highway_exits_xy", "highway_exits")):
            xy = np.asarray(t.get(key, np.zeros((0, 2))), dtype=np.int64).reshape(-1, 2)
            zone[xy[:, 1], xy[:, 0]] = len(names)
            names.append(name)
        return zone, names

    def od_matrix(self, by: str = "block", reasons=("arrived",)) -> dict:
        """Origin / destination matrix of the logged trips whose end reason is in `reasons` (`capi.TRIP_END` names), summed
        on the device: {"zones": names, "count": (Z, Z) uint64 indexed [origin zone, destination zone], "mean_duration" and
        "mean_distance": (Z, Z) float64, NaN where no trip was counted, "unzoned": trips with an unknown origin or an end
        outside every zone}.  `by="block"`: one zone per city block (its entrances), one for all highway entrances, one for
        all highway exits."""
        if by != "block":
            raise ValueError(f"od_matrix: unknown zoning {by!r} (only 'block')")
        zone, names = self._block_zones()
        if len(names) > capi.TRIPLOG_MAX_ZONES:
            raise ValueError(f"od_matrix: {len(names)} zones, the engine takes {capi.TRIPLOG_MAX_ZONES}")
        self.engine.triplog_set_zones(zone, len(names))
        od = self.engine.triplog_od(reasons)
        n = od["count"].astype(np.float64)
        nan = np.full(n.shape, np.nan)
        return {"zones": names, "count": od["count"], "unzoned": od["unzoned"],
                "mean_duration": np.divide(od["duration"], n, out=nan.copy(), where=n > 0),
                "mean_distance": np.divide(od["distance"].astype(np.float64), n, out=nan.copy(), where=n > 0)}

    def intersection_report(self) -> List[dict]:
        """Per light group, over the ticks observed: vehicle-ticks waiting on the N-S and on the W-E approaches (and the
        vehicle-ticks present there), and the throughput - entries into the intersection's cells, in all and by direction."""
        rows = self.engine.observe_groups()
        ticks = self.engine.observe_info()["ticks"]
        f = capi.OG_FIELDS.index
        out = []
        for g, r in enumerate(rows):
            by_dir = {d: int(r[f("enter_" + d.lower())]) for d in "NESW"}
            out.append({"group": self.intersection_light_groups[g].id if g < len(self.intersection_light_groups) else g,
                        "index": g, "ticks": ticks,
                        "waiting_ns": int(r[f("ns_waiting")]), "waiting_ew": int(r[f("ew_waiting")]),
                        "present_ns": int(r[f("ns_present")]), "present_ew": int(r[f("ew_present")]),
                        "throughput": sum(by_dir.values()), "throughput_by_direction": by_dir})
        return out

    # ---- route demand (include/trafficsim_demand.h) ---------------------------------------------------
    def _demand_compute(self, bins, bin_cells, open_tail, vehicles, select=None) -> dict:
        """`select`: a byte mask over the spawn indices handed out so far, in place of `vehicles` (select_link_load)."""
        self._flush_host_writes()
        if vehicles is not None:
            select = np.zeros(self.engine.num_spawned(), dtype=np.uint8)
            idx = np.asarray([v._spawn_idx if hasattr(v, "_spawn_idx") else int(v) for v in vehicles], dtype=np.int64)
            if len(idx) and (idx.min() < 0 or idx.max() >= len(select)):
                raise ValueError("planned_load: a vehicle is not a spawn index handed out so far")
            select[idx] = 1
        return self.engine.demand_compute(bins, bin_cells, open_tail, select)

    def planned_load(self, bins: int = 1, bin_cells: int = 1, open_tail: bool = True, vehicles=None, pooled=None) -> dict:
        """Where traffic is going: the remaining main path of every live vehicle (or of `vehicles`: vehicle agents or spawn
        indices) counted per cell on the device.  Step k of a path (k = 0: the vehicle's next cell) goes to bin k // bin_cells;
        steps beyond the last bin go to the last one (`open_tail`) or are left out.  Returns {"load": (bins, H, W) uint32 (uint64,
        (bins, ceil(H / pooled), ceil(W / pooled)), with `pooled`: sums over pooled x pooled blocks), "by_direction":
        (bins, 4, H, W) by the direction N E S W of the step into the cell} and the fields of `engine.demand_info()`.  A snapshot
        of the state between two steps: not updated by step() and not carried by save / load / deepcopy / pickle."""
        return self._planned_planes(self._demand_compute(bins, bin_cells, open_tail, vehicles), pooled)

    def _planned_planes(self, info, pooled) -> dict:
        """planned_load()'s result from the info of the compute that just ran."""
        eng, nb = self.engine, info["n_bins"]
        if pooled is None:
            load = np.stack([eng.demand_plane(b) for b in range(nb)])
            by_dir = np.stack([np.stack([eng.demand_plane(b, d) for d in range(4)]) for b in range(nb)])
        else:
            load = np.stack([eng.demand_pooled(pooled, b) for b in range(nb)])
            by_dir = np.stack([np.stack([eng.demand_pooled(pooled, b, d) for d in range(4)]) for b in range(nb)])
        return dict(info, load=load, by_direction=by_dir)

    def intersection_demand(self, bins: int = 1, bin_cells: int = 1, open_tail: bool = True, vehicles=None) -> List[dict]:
        """Per light group, keyed like intersection_report(): the planned entries into its N-S and W-E approach cells and into
        the intersection's cells (in all and by direction), one number per bin (lists of `bins` ints)."""
        info = self._demand_compute(bins, bin_cells, open_tail, vehicles)
        rows = self.engine.demand_groups()
        f = capi.DG_FIELDS.index
        out = []
        for g, r in enumerate(rows):
            by_dir = {d: [int(v) for v in r[:, f("enter_" + d.lower())]] for d in "NESW"}
            out.append({"group": self.intersection_light_groups[g].id if g < len(self.intersection_light_groups) else g,
                        "index": g, "tick": info["tick"], "bins": info["n_bins"], "bin_cells": info["bin_cells"],
                        "planned_ns": [int(v) for v in r[:, f("ns_in")]], "planned_ew": [int(v) for v in r[:, f("ew_in")]],
                        "planned_throughput": [sum(by_dir[d][b] for d in "NESW") for b in range(info["n_bins"])],
                        "planned_throughput_by_direction": by_dir})
        return out

    # ---- select-link analysis (include/trafficsim_selectlink.h) ------------------------------------------
    def gate_of_group(self, group, which: str = "ns_in") -> list:
        """A gate made of a light group's cells, from the CSR tables intersection_demand() reads: its N-S approach cells
        (`"ns_in"`), its W-E approach cells (`"ew_in"`) or the intersection's own cells (`"cells"`), open to all directions.
        `group`: an IntersectionLightGroup or its index."""
        keys = {"ns_in": "g_ns_in", "ew_in": "g_ew_in", "cells": "g_icell"}
        if which not in keys:
            raise ValueError(f"gate_of_group: unknown part {which!r} (one of {sorted(keys)})")
        g = int(getattr(group, "index", group))
        off = np.asarray(self.tables[keys[which] + "_off"])
        if not 0 <= g < len(off) - 1:
            raise ValueError(f"gate_of_group: no light group {g}")
        xy = np.asarray(self.tables[keys[which] + "_xy"]).reshape(-1, 2)[off[g]:off[g + 1]]
        return [(int(x), int(y)) for x, y in xy]

    def select_link(self, gates, bins: int = 1, bin_cells: int = 1, open_tail: bool = True) -> dict:
        """Whose routes go through here: the remaining main path of every live vehicle walked over `gates` on the device.
        `gates`: a list of gates, each a list of (x, y) cells - open to every direction - or (x, y, "NESW"-subset): the
        directions of the step into the cell that count.  Bins as for planned_load().  Returns {"cross": (G, bins, 4) uint64
        crossings by gate, bin and direction N E S W, "pair": (G, G) uint64 vehicles whose routes cross both gates (the
        diagonal: the gate's vehicles)} and the fields of `engine.selectlink.info()` ("vehicles", "crossing", "crossings", ...).
        The result stays in the engine for select_link_vehicles / _load / _od.  A snapshot of the state between two steps: not
        updated by step() and not carried by save / load / deepcopy / pickle (the model those give has neither gates nor a
        result)."""
        self._flush_host_writes()
        sl = self.engine.selectlink
        sl.set_gates(gates)
        info = sl.compute(bins, bin_cells, open_tail)
        cross, pair = sl.tables()
        return dict(info, cross=cross, pair=pair)

    def select_link_vehicles(self, any: int = 0, all: int = 0, none: int = 0) -> list:
        """The agents, of the vehicles the last select_link() walked, whose gate mask meets (any == 0 or mask & any) and
        mask & all == all and mask & none == 0 (bit g: gate g), in spawn order; vehicles that have left since are left out."""
        sel, _ = self.engine.selectlink.select(any, all, none)
        live = {int(r[0]) for r in self._snapshot()["rows"]}
        return [self._vehicle_view(int(i)) for i in np.nonzero(sel)[0] if int(i) in live]

    def select_link_load(self, any: int = 0, all: int = 0, none: int = 0, bins: int = 1, bin_cells: int = 1, open_tail: bool = True,
                         pooled=None) -> dict:
        """planned_load() of the vehicles that selection picks, with its bins, bin_cells, open_tail and pooled: the mask goes
        from the select-link result to the demand walk as it is, and the load is of the routes as they are now."""
        sel, _ = self.engine.selectlink.select(any, all, none)
        mask = np.zeros(self.engine.num_spawned(), dtype=np.uint8)     # (vehicles spawned since the compute are not selected)
        mask[:len(sel)] = sel
        return self._planned_planes(self._demand_compute(bins, bin_cells, open_tail, None, mask), pooled)

    def select_link_od(self, any: int = 0, all: int = 0, none: int = 0) -> dict:
        """Where the selected vehicles were and where they were going when select_link() ran, by the zones of od_matrix():
        {"zones": names, "count": (Z, Z) int64 indexed [zone of the cell, zone of the goal], "unzoned"}."""
        zone, names = self._block_zones()
        sl = self.engine.selectlink
        if len(names) > capi.TRIPLOG_MAX_ZONES:
            raise ValueError(f"select_link_od: {len(names)} zones, the engine takes {capi.TRIPLOG_MAX_ZONES}")
        sl.set_zones(zone, len(names))
        count, unzoned = sl.od(any, all, none)
        return {"zones": names, "count": count, "unzoned": unzoned}

    # ---- jam detection (include/trafficsim_jams.h) -------------------------------------------------------
    def jams(self, min_ticks: int = 1, link: str = "flow", top: Optional[int] = None) -> dict:
        """Where the jams are now: the connected components of the cells on which a vehicle has stood for at least `min_ticks`
        ticks (parked ones aside), labelled on the device.  `link`: "flow" joins 4-neighbours one of which may drive to the
        other, "grid" all 4-neighbours.  Returns {"jams": the jams.JAM_DTYPE records sorted by (cells descending, root
        ascending) and cut to the `top` largest, "label": (H, W) int32, the jam number of every cell (the number a record had
        before the sort: `"number"` holds it per sorted record), -1 where there is none, "n": the number of jams} and the
        fields of `engine.jams.info()` ("standing_vehicles", "standing_cells", "largest_cells", "tick", ...).  The result stays
        in the engine for queue_report / jam_vehicles / jam_load.  A snapshot of the state between two steps: not updated by
        step() and not carried by save / load / deepcopy / pickle (the model those give has no result)."""
        self._flush_host_writes()
        jm = self.engine.jams
        info = jm.compute(min_ticks, link)
        rec = jm.records()
        order = np.lexsort((np.arange(len(rec)), -rec["cells"].astype(np.int64)))
        if top is not None:
            order = order[:max(int(top), 0)]
        return dict(info, jams=rec[order], number=order.astype(np.int32), label=jm.plane("label"), n=info["n_jams"])

    def queue_report(self, min_ticks: int = 1, link: str = "flow") -> List[dict]:
        """Per light group, keyed like intersection_report(): the queues that reach its N-S and W-E approach cells, each whole
        - their cells, vehicles, largest extent, longest wait and number - and the standing cells inside its box."""
        self._flush_host_writes()
        jm = self.engine.jams
        info = jm.compute(min_ticks, link)
        from .jams import JG_FIELDS
        f = JG_FIELDS.index
        out = []
        for g, r in enumerate(jm.groups()):
            row = {"group": self.intersection_light_groups[g].id if g < len(self.intersection_light_groups) else g,
                   "index": g, "tick": info["tick"], "box_cells": int(r[f("box_cells")])}
            for ax in ("ns", "ew"):
                row.update({f"queue_{ax}": int(r[f(ax + "_cells")]), f"queue_vehicles_{ax}": int(r[f(ax + "_vehicles")]),
                            f"queue_extent_{ax}": int(r[f(ax + "_extent")]), f"longest_wait_{ax}": int(r[f(ax + "_stuck_max")]),
                            f"jams_{ax}": int(r[f(ax + "_jams")])})
            out.append(row)
        return out

    def jam_vehicles(self, jam: int) -> list:
        """The agents standing in jam `jam` (its number in the label plane) of the last jams() / queue_report(), in spawn
        order; vehicles that have left since are left out."""
        per_vehicle = self.engine.jams.vehicles()
        if int(jam) < 0:
            raise ValueError(f"jam_vehicles: {jam} is no jam number")
        live = {int(r[0]) for r in self._snapshot()["rows"]}
        return [self._vehicle_view(int(i)) for i in np.nonzero(per_vehicle == int(jam))[0] if int(i) in live]

    def jam_load(self, jam: int, **planned_load_arguments) -> dict:
        """Where the vehicles of that jam are going: planned_load(vehicles=jam_vehicles(jam), ...)."""
        return self.planned_load(vehicles=self.jam_vehicles(jam), **planned_load_arguments)

    # ---- cost fields (include/trafficsim_costfield.h) --------------------------------------------------
    @staticmethod
    def _seed_cells(seeds) -> np.ndarray:
        """(n, 2) int32 (x, y) of `seeds`: (x, y) pairs, cells or vehicle agents (where they stand now), or a mix."""
        out = []
        for s in seeds:
            pos = s.pos if hasattr(s, "pos") else s
            if pos is None:
                raise ValueError(f"cost field: {s!r} has no position (a vehicle that has left?)")
            out.append((int(pos[0]), int(pos[1])))
        return np.asarray(out, dtype=np.int32).reshape(-1, 2)

    def cost_field(self, seeds, mode: str = "to", seed_cost=None, **modes) -> dict:
        """What the network costs right now: the cheapest travel cost, under the pathfinder's own cost rule and the traffic as
        it is, from every cell to its nearest seed (`mode="to"`) or from the seeds to every cell (`"from"`), computed on the
        device.  `seeds`: (x, y) pairs, cells or vehicle agents; `modes`: soft (default True), ignore_flow, free_flow, max_cost.
        Returns {"cost": (H, W) uint32 (0xFFFFFFFF: unreachable), "owner": (H, W) int32 index into "seeds" of the seed that
        attains it (-1: unreachable), "seeds": (n, 2)} and the fields of `engine.costfield.info()`.  A snapshot of the state
        between two steps: not updated by step() and not carried by save / load / deepcopy / pickle."""
        self._flush_host_writes()
        xy = self._seed_cells(seeds)
        cf = self.engine.costfield
        info = cf.compute(xy, seed_cost, mode=mode, **modes)
        return dict(info, cost=cf.plane("cost"), owner=cf.plane("owner"), seeds=xy)

    def catchments(self, kind="highway_exits", **modes) -> dict:
        """Which exit, entrance or depot is the nearest one for every cell: the owner plane of the TO field seeded at the
        highway exits (`kind="highway_exits"`), the block entrances (`"block_entrances"`) or the given cells.  Returns
        {"zone": (H, W) int32, "n": the number of seeds, "seeds": (n, 2), "cost": the value plane}; with at most
        capi.TRIPLOG_MAX_ZONES seeds, `engine.triplog_set_zones(zone, n)` takes the plane as it is."""
        if isinstance(kind, str):
            if kind not in ("highway_exits", "block_entrances"):
                raise ValueError(f"catchments: unknown kind {kind!r} ('highway_exits', 'block_entrances' or a list of cells)")
            kind = self.highway_exits if kind == "highway_exits" else self.block_entrances
        f = self.cost_field(kind, mode="to", **modes)
        return {"zone": f["owner"], "n": len(f["seeds"]), "seeds": f["seeds"], "cost": f["cost"]}

    def isochrones(self, seeds, thresholds, mode: str = "to", **modes) -> dict:
        """Isochrone areas of `seeds`: for every ascending threshold the number of road cells whose cost is at most it, counted
        on the device.  Returns {"thresholds", "road_cells": uint64 per threshold} and the fields of `engine.costfield.info()`;
        the planes stay on the device (engine.costfield.plane / gather / device read them)."""
        self._flush_host_writes()
        cf = self.engine.costfield
        info = cf.compute(self._seed_cells(seeds), mode=mode, **modes)
        thr = np.asarray(thresholds, dtype=np.uint32).reshape(-1)
        return dict(info, thresholds=thr, road_cells=cf.bands(thr))

    # ---- routes along a cost field (include/trafficsim_cfroute.h) ---------------------------------------
    def _route_starts(self, starts):
        """((n, 2) int32 cells, int8 headings) of `starts`: (x, y) pairs and cells have no heading, a vehicle agent stands
        where it is now and is held with the heading it drives with."""
        self._flush_host_writes()
        xy = self._seed_cells(starts)
        head = np.full(len(xy), -1, dtype=np.int8)
        for i, s in enumerate(starts):
            if hasattr(s, "_spawn_idx"):
                d = s._field("direction")
                head[i] = d if d is not None and 0 <= d <= 3 else -1
        return xy, head

    def routes_along(self, seeds, starts, mode: str = "to", seed_cost=None, **modes) -> dict:
        """Shortest routes read off a cost field, all in one launch: from every start to its nearest seed (`mode="to"`; a
        vehicle agent's route honours the heading it has now) or from the nearest seed to every start (`"from"`), under the
        pathfinder's cost rule and the traffic as it is.  `seeds`, `starts`: (x, y) pairs, cells or vehicle agents; `modes` as
        for cost_field().  Returns {"routes": a list of (k, 2) int32 arrays of (x, y) cells, each without its first cell as
        A* paths are, "dirs": the same routes as direction bytes with their CSR offsets "off", "cost": uint32 per route
        (0xFFFFFFFF: no route), "owner": int32 index into "seeds" (-1: none), "seeds", "starts", "headings"} and the fields of
        `engine.costfield.routes.info()`.  The cost field of the seeds stays the engine's result."""
        seed_xy = self._seed_cells(seeds)
        xy, head = self._route_starts(starts)
        r = self.engine.costfield.routes
        r.compute(seed_xy, seed_cost, mode=mode, **modes)
        r.trace(xy, head if mode == "to" else None)
        off, dirs, cost, owner = r.routes()
        _, cells = r.cells()
        return dict(r.info(), routes=[cells[off[i]:off[i + 1]] for i in range(len(xy))], off=off, dirs=dirs, cost=cost, owner=owner,
                    seeds=seed_xy, starts=xy, headings=head)

    def assigned_load(self, seeds, starts, weights=None, mode: str = "to", seed_cost=None, **modes) -> dict:
        """All-or-nothing assignment: every start sends `weights` units (default 1) down its route to the nearest seed, summed
        per cell on the device without materialising the routes.  Returns {"load": (H, W) uint32, "by_direction": (4, H, W)
        by the direction N E S W of the step into the cell - field for field what planned_load() and the ENTER planes of
        observe() hold -, "routes", "unreached", "steps"} and the fields of `engine.costfield.routes.info()`."""
        seed_xy = self._seed_cells(seeds)
        xy, head = self._route_starts(starts)
        r = self.engine.costfield.routes
        r.compute(seed_xy, seed_cost, mode=mode, **modes)
        load = r.load(xy, head if mode == "to" else None, weights)
        return dict(r.info(), **{k: load[k] for k in ("routes", "unreached", "steps")}, load=r.load_plane(),
                    by_direction=np.stack([r.load_plane(d) for d in range(4)]), seeds=seed_xy, starts=xy)

    # ---- getters used by the UI (city_model.py:1965-2149) ------------------------------------------
    # ---- device renderer (include/trafficsim_render.h) ---------------------------------------------------
    def _render_defaults(self):
        """`Defaults` with the colour settings CityModel(defaults={...}) overrode (ZONE_COLORS, VEHICLE_*_COLOR, ...)."""
        over = {k: v for k, v in self._defaults.items() if k == "ZONE_COLORS" or k.endswith("_COLOR") or k == "CHANGE_ASSIGNED_CELL_COLOR_ON_STOP"}
        if not over:
            return Defaults
        if "ZONE_COLORS" in over:
            over["ZONE_COLORS"] = dict(Defaults.ZONE_COLORS, **over["ZONE_COLORS"])
        return type("Defaults", (Defaults,), over)

    def render_type_plane(self):
        """(type codes (H, W) uint8, type names): the `cell_type_map` table where the world has one, else the plane
        CellAgent.cell_type's fallback derives (light, intersection, controlled road, road, nothing), vectorised."""
        from . import render as _render
        if self._cell_type_map is not None:
            return _render.type_plane(self._cell_type_map, self._cell_base_type_map), _render.RENDER_TYPE_NAMES
        return (_render.fallback_type_plane(self.is_road_map, self.intersection_map, sorted(self._controlled_cells),
                                            sorted(self._light_index)), _render.fallback_type_names())

    def render(self, x0=0, y0=0, w=None, h=None, zoom=1, shrink=1, layers=("signals", "rain", "vehicles"), heat=None,
               heat_max=None, routes=None, flip_y=True, device=False, background=(0, 0, 0), vehicle_radius_256=None):
        """One RGBA8 frame of the cells [x0, x0 + w) x [y0, y0 + h) (default: the whole map) rendered on the device: an
        (h', w', 4) uint8 array, or with device=True a torch tensor over the engine's frame buffer (valid until the next
        render).  `layers`: names of capi.RENDER_LAYERS or a TS_RL_* mask; `heat`: an observation plane name or "flow" (adds
        the heat layer; the plane must be observed, see observe()), scaled to `heat_max` (default: the plane's maximum,
        at least 1); `routes`: vehicles or spawn indices whose remaining paths to draw (adds the routes layer).  flip_y=True
        puts the largest y in row 0, the way a CanvasGrid shows the city.  The colour tables (render.py) go to the engine
        on the first call."""
        from . import render as _render
        eng = self.engine
        self._flush_host_writes()
        if not self._render_ready:
            d = self._render_defaults()
            plane, names = self.render_type_plane()
            eng.render_set_cells(plane, _render.cell_palette(d, names))
            eng.render_set_vehicle_palette(_render.vehicle_palette(d))
            eng.render_set_heat_lut(_render.heat_lut())
            self._render_ready = True
        mask = capi.render_layer_mask(layers)
        if heat is not None:
            mask |= capi.RL_HEAT
            if heat_max is None:
                planes = capi.OBS_ENTER if heat == "flow" else [heat]
                heat_max = max(1, int(sum(eng.observe_plane(p).astype(np.uint64) for p in planes).max()))
        if routes is not None:
            mask |= capi.RL_ROUTES
            eng.render_set_routes([int(getattr(v, "_spawn_idx", v)) for v in routes])
        view = _render.make_view(x0=x0, y0=y0, cells_w=self.width - x0 if w is None else w, cells_h=self.height - y0 if h is None else h,
                                 zoom=zoom, shrink=shrink, layers=mask, flip_y=flip_y, heat_plane=heat if heat is not None else 0,
                                 heat_max=heat_max if heat_max is not None else 1, background=background,
                                 vehicle_radius_256=capi.RENDER_DEFAULT_RADIUS if vehicle_radius_256 is None else vehicle_radius_256)
        return eng.render_device(view) if device else eng.render(view)

    @property
    def active_vehicle_agents(self):
        rows = self._snapshot()["rows"]
        return [self._vehicle_view(int(r[0])) for r in rows]

    def cell(self, x, y) -> CellAgent:
        c = self._cells.get((x, y))
        if c is None:
            c = self._cells[(x, y)] = CellAgent(self, x, y)
        return c

    def remove_vehicle(self, vehicle, population_type: str = "undefined", vehicle_type: str = "undefined"):
        """city_model.py:1920-1941 - between ticks: the vehicle leaves the grid, the schedule and the decide order
        As in the reference the live counters follow `population_type` as the caller passes it ('internal' / 'through'; the
        default 'undefined' leaves them alone); `vehicle_type` only concerns service vehicles, which the host cannot remove."""
        self.engine.remove_vehicle(vehicle._spawn_idx, capi.POP.get(population_type, capi.POP["undefined"]))
        self._vehicles.pop(vehicle._spawn_idx, None)
        self._invalidate()

    def get_cell_contents(self, x, y):
        return self.grid[x, y] if self.in_bounds(x, y) else []

    def in_bounds(self, x, y):
        return 0 <= x < self.width and 0 <= y < self.height

    def get_width(self):
        return self.width

    def get_height(self):
        return self.height

    def get_traffic_lights(self):
        return self.traffic_lights

    def get_controlled_roads(self):
        return self.controlled_roads

    def get_intersection_light_groups(self):
        return self.intersection_light_groups

    def get_block_entrances(self):
        return self.block_entrances

    def get_highway_entrances(self):
        return self.highway_entrances

    def get_highway_exits(self):
        return self.highway_exits

    def get_start_blocks(self):
        return list(self.block_entrances) + list(self.highway_entrances)

    def get_exit_blocks(self):
        return list(self.block_entrances) + list(self.highway_exits)

    def get_valid_exits(self, entry_cell):
        """city_model.py:2118-2149.  For a HighwayEntrance the reference filters with `not _are_adjacent(...)`, and
        `_are_adjacent` returns a Manhattan distance (2092-2099): nothing passes, the list is empty."""
        if entry_cell in self.block_entrances:
            return [be for be in self.block_entrances if be is not entry_cell] + list(self.highway_exits)
        return []

    # ---- city-block queries (city_model.py:2017-2087): views over the engine's block stock -------------------------
    @staticmethod
    def _sort_blocks(blocks, by):
        if by == "food":
            return sorted(blocks, key=lambda b: b.get_food_units())
        if by == "waste":
            return sorted(blocks, key=lambda b: -b.get_waste_units())
        return blocks

    def get_all_city_blocks(self, sort_by="unsorted"):
        return self._sort_blocks(list(self.city_blocks.values()), sort_by)

    def get_blocks_needing_food(self, sort_by="unsorted"):
        return self._sort_blocks([b for b in self.city_blocks.values() if b.needs_food()], sort_by)

    def get_blocks_producing_waste(self, sort_by="unsorted"):
        return self._sort_blocks([b for b in self.city_blocks.values() if b.produces_waste()], sort_by)

    def get_city_blocks_by_types(self, block_types, sort_by="unsorted"):
        if block_types is None:
            subset = list(self.city_blocks.values())
        else:
            wanted = {block_types} if isinstance(block_types, str) else set(block_types)
            subset = [b for b in self.city_blocks.values() if b.block_type in wanted]
        return self._sort_blocks(subset, sort_by)

    def get_city_blocks_by_type(self, block_type, sort_by="unsorted"):
        return self.get_city_blocks_by_types([block_type], sort_by)

    def get_residential_city_blocks(self, sort_by="unsorted"):
        return self.get_city_blocks_by_types("Residential", sort_by)

    def get_office_city_blocks(self, sort_by="unsorted"):
        return self.get_city_blocks_by_types("Office", sort_by)

    def get_market_city_blocks(self, sort_by="unsorted"):
        return self.get_city_blocks_by_types("Market", sort_by)

    def get_leisure_city_blocks(self, sort_by="unsorted"):
        return self.get_city_blocks_by_types("Leisure", sort_by)

    def get_other_city_blocks(self, sort_by="unsorted"):
        return self.get_city_blocks_by_types("Other", sort_by)

    def get_block_most_in_need_of_food(self):
        needy = self.get_blocks_needing_food(sort_by="food")
        return needy[0] if needy else None

    def get_block_most_in_need_of_waste_pickup(self):
        dirty = self.get_blocks_producing_waste(sort_by="waste")
        return dirty[0] if dirty else None

    def is_type(self, x, y, ctype):       # city_model.py:1803-1805
        return self.in_bounds(x, y) and self.cell(x, y).cell_type == ctype

    @staticmethod
    def next_cell_in_direction(x, y, d):  # city_model.py:1015-1024
        dx, dy = {"N": (0, 1), "S": (0, -1), "E": (1, 0), "W": (-1, 0)}.get(d, (0, 0))
        return x + dx, y + dy

    def set_traffic_lights_go(self):      # city_model.py:1995-1997
        for tl in self.traffic_lights:
            tl.set_light_go()

    def set_traffic_lights_stop(self):    # city_model.py:1999-2001
        for tl in self.traffic_lights:
            tl.set_light_stop()

    def close(self):
        self.engine.close()

    # ---- checkpoints (include/trafficsim_checkpoint.h): save / load, copy.deepcopy and pickle --------------------------
    def _checkpoint_state(self) -> dict:
        """Everything a second model needs: the world tables, the constructor's settings, the facade's own state and the
        engine's blob."""
        import json
        self._flush_host_writes()
        blob = self.engine.checkpoint_save()
        vs = sorted(self._vehicles.items())
        def xy(c):
            return (-1, -1) if c is None else (int(c.position[0]), int(c.position[1]))
        config = dict(defaults=self._defaults, traffic=self._service_cfg if self._traffic_armed else None, seed=self._seed,
                      step_count=int(self.step_count), n_spawned=int(self._n_spawned))
        st = {"t/" + k: np.asarray(v) for k, v in self.tables.items()}
        st.update({
            "config_json": np.asarray(json.dumps(config)),
            "veh_spawn": np.asarray([i for i, _ in vs], dtype=np.int64),
            "veh_id": np.asarray([str(v.id) for _, v in vs], dtype=str),
            "veh_kind": np.asarray([1 if isinstance(v, ServiceVehicleAgent) else 0 for _, v in vs], dtype=np.int8),
            "veh_pop": np.asarray([str(v.population_type) for _, v in vs], dtype=str),
            "veh_type": np.asarray([str(v.vehicle_type) for _, v in vs], dtype=str),
            "veh_start": np.asarray([xy(v.__dict__.get("start_cell")) for _, v in vs], dtype=np.int32).reshape(-1, 2),
            "veh_target": np.asarray([xy(v.__dict__.get("_static_target")) for _, v in vs], dtype=np.int32).reshape(-1, 2),
            "engine_blob": np.frombuffer(blob, dtype=np.uint8),
        })
        return st

    def _restore(self, st, engine: Optional[capi.CApi] = None):
        """__init__ from a _checkpoint_state (the world from its tables: no world-gen), then the blob."""
        import json
        cfg = json.loads(str(np.asarray(st["config_json"])))
        tables = {k[2:]: np.asarray(st[k]) for k in st if k.startswith("t/")}
        CityModel.__init__(self, tables=tables, seed=cfg["seed"], defaults=cfg["defaults"], traffic=cfg["traffic"], engine=engine)
        self.engine.checkpoint_load(np.asarray(st["engine_blob"], dtype=np.uint8))
        self.step_count, self._n_spawned = int(cfg["step_count"]), int(cfg["n_spawned"])
        for k, i in enumerate(np.asarray(st["veh_spawn"])):
            klass = ServiceVehicleAgent if int(st["veh_kind"][k]) else VehicleAgent
            v = object.__new__(klass)
            v.id = str(st["veh_id"][k])
            v.unique_id = str_to_unique_int(v.id)
            v.model = v.city_model = self
            sx, sy = (int(q) for q in st["veh_start"][k])
            v.start_cell = None if sx < 0 else self.cell(sx, sy)
            tx, ty = (int(q) for q in st["veh_target"][k])
            if tx >= 0 or klass is VehicleAgent:
                v._static_target = None if tx < 0 else self.cell(tx, ty)
            v.population_type, v.vehicle_type = str(st["veh_pop"][k]), str(st["veh_type"][k])
            v.base_color = Defaults.VEHICLE_BASE_COLOR
            v._spawn_idx = int(i)
            self._vehicles[v._spawn_idx] = v
            self._vehicle_by_uid[v.unique_id] = v
        self._invalidate()
        return self

    def save(self, path) -> None:
        """One .npz (no pickled objects) from which CityModel.load resumes this run exactly."""
        with open(path, "wb") as f:
            np.savez(f, **self._checkpoint_state())

    @classmethod
    def load(cls, path, engine: Optional[capi.CApi] = None) -> "CityModel":
        """The model `save` wrote: the engine is rebuilt from the stored world tables (world-gen does not run) and takes
        the stored state; stepping it continues the saved run bit for bit."""
        with np.load(path, allow_pickle=False) as z:
            st = {k: z[k] for k in z.files}
        return cls.__new__(cls)._restore(st, engine)

    def __deepcopy__(self, memo):
        """A second model with an engine of its own (same library), in the state of this one."""
        other = type(self).__new__(type(self))
        memo[id(self)] = other
        return other._restore(self._checkpoint_state(), capi.CApi(self.engine.lib, self.engine.prefix))

    def __getstate__(self):
        return self._checkpoint_state()

    def __setstate__(self, st):
        self._restore(st)


def agent_portrayal(agent):
    """visualization/agent_portrayal.py:18-52: dispatch on the agent's own get_portrayal()."""
    if agent is None or not hasattr(agent, "get_portrayal"):
        return None
    return agent.get_portrayal()
