"""What a cost field (include/trafficsim_costfield.h) must hold, straight from its definition: the step rule of
astar_numba.py:171-226 and a heapq Dijkstra over (cell, heading) with labels (cost, seed index), so that value and owner come
out of one lexicographic minimum.  Plain Python on purpose - nothing here shares code with the engine."""
import heapq

import numpy as np

INF = 0x3F3F3F3F
UNREACHABLE = 0xFFFFFFFF
DX, DY = (0, 1, 0, -1), (1, 0, -1, 0)      # N: y + 1, E: x + 1, S: y - 1, W: x - 1
HEADINGS = (-1, 0, 1, 2, 3)

# config.py's values of the constants astar_numba.py binds (tests/golden/make_golden.py COST_DEFAULTS)
COST_DEFAULTS = dict(VEHICLE_CONTRAFLOW_PENALTY=5000, VEHICLE_OBSTACLE_PENALTY_VEHICLE=1000, VEHICLE_OBSTACLE_PENALTY_STOP=500,
                     VEHICLE_ROAD_TYPES_PENALTIES_ENABLED=True, VEHICLE_ROAD_TYPES_PENALTY_R1=0.5,
                     VEHICLE_ROAD_TYPES_PENALTY_R2=5, VEHICLE_ROAD_TYPES_PENALTY_R3=50.0, VEHICLE_TURN_PENALTY_ENABLED=True,
                     VEHICLE_TURN_PENALTY=10, VEHICLE_DYNAMIC_PENALTIES_ENABLED=True, VEHICLE_DYNAMIC_PENALTY_SCALE=4.0)


class Rule:
    """The step rule on one set of maps and constants."""

    def __init__(self, consts, allowed, is_road, road_type, occupancy, stop, density):
        c = dict(COST_DEFAULTS, **{k: v for k, v in consts.items() if k in COST_DEFAULTS})
        self.turn_on, self.turn = bool(c["VEHICLE_TURN_PENALTY_ENABLED"]), c["VEHICLE_TURN_PENALTY"]
        self.contra, self.veh, self.stop_pen = c["VEHICLE_CONTRAFLOW_PENALTY"], c["VEHICLE_OBSTACLE_PENALTY_VEHICLE"], c["VEHICLE_OBSTACLE_PENALTY_STOP"]
        self.rt_on = bool(c["VEHICLE_ROAD_TYPES_PENALTIES_ENABLED"])
        self.rt = (0, c["VEHICLE_ROAD_TYPES_PENALTY_R1"], c["VEHICLE_ROAD_TYPES_PENALTY_R2"], c["VEHICLE_ROAD_TYPES_PENALTY_R3"])
        self.dyn, self.scale = bool(c["VEHICLE_DYNAMIC_PENALTIES_ENABLED"]), float(c["VEHICLE_DYNAMIC_PENALTY_SCALE"])
        self.H, self.W = np.asarray(allowed).shape
        as_list = lambda a: np.asarray(a).tolist()
        self.allowed, self.is_road, self.road_type = as_list(allowed), as_list(is_road), as_list(road_type)
        self.occ, self.stop = as_list(occupancy), as_list(stop)
        self.density = np.asarray(density, dtype=np.float64).tolist()       # (a float32 map, widened exactly)

    @classmethod
    def from_params(cls, p, *maps):
        """... from a TsParams."""
        return cls(dict(VEHICLE_CONTRAFLOW_PENALTY=int(p.contraflow_penalty), VEHICLE_OBSTACLE_PENALTY_VEHICLE=int(p.obstacle_penalty_vehicle),
                        VEHICLE_OBSTACLE_PENALTY_STOP=int(p.obstacle_penalty_stop),
                        VEHICLE_ROAD_TYPES_PENALTIES_ENABLED=bool(p.road_type_penalties_enabled),
                        VEHICLE_ROAD_TYPES_PENALTY_R1=float(p.road_type_penalty_r1), VEHICLE_ROAD_TYPES_PENALTY_R2=float(p.road_type_penalty_r2),
                        VEHICLE_ROAD_TYPES_PENALTY_R3=float(p.road_type_penalty_r3), VEHICLE_TURN_PENALTY_ENABLED=bool(p.turn_penalty_enabled),
                        VEHICLE_TURN_PENALTY=int(p.turn_penalty), VEHICLE_DYNAMIC_PENALTIES_ENABLED=bool(p.dynamic_penalties_enabled),
                        VEHICLE_DYNAMIC_PENALTY_SCALE=float(p.dynamic_penalty_scale)), *maps)

    def step(self, x, y, d, p, soft=True, ignore_flow=False, free_flow=False):
        """The cost of the step from (x, y) in direction d after heading p (-1: none), None when there is no such step."""
        nx, ny = x + DX[d], y + DY[d]
        if not (0 <= nx < self.W and 0 <= ny < self.H):
            return None
        c = 1.0
        if self.turn_on and p != -1 and d != p:
            c += self.turn
        if not (self.allowed[y][x] >> d) & 1:
            if ignore_flow and self.is_road[ny][nx] == 1:
                c += self.contra
            else:
                return None
        if not free_flow:
            if self.occ[ny][nx] == 1:
                if not soft:
                    return None
                c += int(self.veh * (1.0 + self.scale * self.density[ny][nx])) if self.dyn else self.veh
            if self.stop[ny][nx] == 1:
                if not soft:
                    return None
                c += self.stop_pen
        if self.rt_on and self.is_road[ny][nx] == 1:
            c += self.rt[self.road_type[ny][nx] & 3]
        return int(c)

    def path_cost(self, cells, **modes):
        """The cost of the path through `cells` ((x, y), the start first), None when one of its steps does not exist."""
        total, p = 0, -1
        for (x, y), (nx, ny) in zip(cells[:-1], cells[1:]):
            d = [(DX[k], DY[k]) for k in range(4)].index((nx - x, ny - y))
            c = self.step(x, y, d, p, **modes)
            if c is None:
                return None
            total, p = total + c, d
        return total


def field(rule, seeds, seed_cost=None, mode="to", soft=True, ignore_flow=False, free_flow=False, max_cost=0):
    """(value plane (H, W) uint32, owner plane (H, W) int32) of the definition."""
    modes = dict(soft=soft, ignore_flow=ignore_flow, free_flow=free_flow)
    limit = min(INF, max_cost + 1) if max_cost else INF
    seeds = [(int(x), int(y)) for x, y in np.asarray(seeds).reshape(-1, 2)]
    costs = [0] * len(seeds) if seed_cost is None else [int(c) for c in seed_cost]
    best, heap = {}, []

    def offer(label, state):
        if label[0] < limit and label < best.get(state, (limit, 0)):
            best[state] = label
            heapq.heappush(heap, (label, state))

    for i, ((x, y), c) in enumerate(zip(seeds, costs)):
        # FROM: a seed has no heading.  TO: arriving at a seed ends the path whatever the heading was
        for p in ((-1,) if mode == "from" else HEADINGS):
            offer((c, i), (x, y, p))
    while heap:
        label, (x, y, p) = heapq.heappop(heap)
        if best[(x, y, p)] != label:
            continue
        if mode == "from":       # (x, y) was reached with heading p: step on
            for d in range(4):
                c = rule.step(x, y, d, p, **modes)
                if c is not None:
                    offer((label[0] + c, label[1]), (x + DX[d], y + DY[d], d))
        elif p != -1:            # the label of "at (x, y), having arrived with heading p": who steps into (x, y) in direction p?
            ux, uy = x - DX[p], y - DY[p]
            if 0 <= ux < rule.W and 0 <= uy < rule.H:
                for q in HEADINGS:
                    c = rule.step(ux, uy, p, q, **modes)
                    if c is not None:
                        offer((label[0] + c, label[1]), (ux, uy, q))
    value = np.full((rule.H, rule.W), UNREACHABLE, dtype=np.uint32)
    owner = np.full((rule.H, rule.W), -1, dtype=np.int32)
    cell = {}
    for (x, y, p), label in best.items():
        if (mode == "from" or p == -1) and label < cell.get((x, y), (limit, 0)):
            cell[(x, y)] = label
    for (x, y), (c, i) in cell.items():
        value[y, x], owner[y, x] = c, i
    return value, owner
