"""Every device extension switched on next to one trace replay, and one bundle of their outputs per check tick.

`Sidecar(api, tr)` turns on observation (all seven planes), the trip log, the renderer (tables, palettes, heat LUT, a route
list) on an engine that was set up from trace `tr`; `Sidecar.check(t)`, called after tick t, asserts the rules that need
nothing but the engine's own downloads and the trace (paths against the rows' CRCs, demand against download_path, the route
layer against download_path, observation growth against the rows, the trip log against the rows; then, unless
`analyses=False`, the cost field of the trace's highway exits and the routes and load of the live vehicles along it against
tests/costfield_expect.py and tests/cfroute_expect.py on the engine's own map downloads, and select-link over gate sets taken
from the demand plane just verified against tests/selectlink_expect.py on download_path) and returns a bundle: a dict of
numpy arrays holding every output.  The simulation state of a trace replay is the reference's whichever way the engine
computes it (other searcher, other build, host tail, collected pool, sharded ranks), so the bundles of two replays of one
trace are equal byte for byte - `assert_same_bundles`.  tests/test_gpu_ext_paths.py runs the matrix.

No pytest in here: the worker scripts of the sharded runs import this module.  `check_query` and `read_planes` are the route
demand checks of tests/test_gpu_demand.py, which imports them back; the checks of one cost-field, route or select-link call
are in tests/ext_rules.py."""
import numpy as np

from tests import cfroute_expect as re_
from tests import costfield_expect as ce
from tests import demand_expect as de
from tests import ext_rules as er
from tests import observe_util as ou
from tests import render_expect as rx
from tests import selectlink_expect as se
from tests import triplog_util as tu
from tests.trace_util import replay_and_compare
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import render as rn

V = ou.V
SAMPLED, ENTER = slice(0, 3), slice(3, 7)
DEMAND_QUERIES = [(1, 1, 1), (4, 16, 1)]
ROUTE_RGBA = (1, 2, 3, 255)            # weight 255: a route cell is exactly this colour
BG = (17, 34, 51, 0)
CHECK_EVERY = 10
# the cost field and its routes: every check tick from the trace's highway exits, exit k at cost k % 4
FIELD_A = dict(mode="to", soft=True)                               # (the density path: ensure_density runs, density_valid goes)
FIELD_B = dict(mode="from", soft=False, ignore_flow=True)
# select-link: the gate sets A and B of the whole-path demand plane under the demand queries and one without the open tail
SELECTLINK_QUERIES = DEMAND_QUERIES + [(3, 8, 0)]
SELECT = dict(any=0b101, none=0b10)
N_ZONES = 7
FAR_STEP = 16                          # a first crossing at step 16 or later lies beyond the path's first pool word
GC_MIN_CELLS = 17                      # cells driven since a path was written: a collection has dropped its first word
# config1_64_s11 (generator_ticks, pinned on the CPU by tests/test_ext_sidecar.py): by tick 260 the rows show 102 vehicles
# spawned (50 were placed before tick 0) and a service vehicle parked after tick 225
GENERATOR_TRACE, GENERATOR_T, GENERATOR_SPAWNED, GENERATOR_PARKED_AT = "config1_64_s11", 260, 102, 225
# the fixtures of each light-control family in whose recorded runs searches run inside ticks (light_fixtures_with_searches,
# pinned on the CPU by tests/test_ext_sidecar.py); the GAT one is driven through act_q, whose epsilon-greedy draws come from
# the global stream on the host
LIGHTS_EXT_FIXTURE, LIGHTS_PROTO_FIXTURE = "lights_ext_stuck_96_s43", "lights_gat_96_s49"


def read_planes(api, n_bins):
    return np.stack([np.stack([api.demand_plane(b, d) for d in range(4)]) for b in range(n_bins)])


def check_query(api, tr, veh, query, ctx, tick):
    """One compute of `query` against the numpy rule on `veh`: every plane, the direction sums, pooled reads, the group rows
    and the totals."""
    n_bins, bin_cells, open_tail = query
    H, W = int(tr["height"]), int(tr["width"])
    want = de.planes(H, W, veh, n_bins, bin_cells, bool(open_tail))
    info = api.demand_compute(n_bins, bin_cells, bool(open_tail))
    ctx = f"{ctx}, query {query}"
    assert info == api.demand_info(), ctx
    assert (info["n_bins"], info["bin_cells"], info["open_tail"], info["selected"]) == (n_bins, bin_cells, bool(open_tail), False), ctx
    assert (info["width"], info["height"], info["tick"], info["vehicles"]) == (W, H, tick, len(veh)), ctx
    assert info["device_bytes"] == n_bins * 4 * H * W * 4, ctx
    got = read_planes(api, n_bins)
    assert np.array_equal(got, want), f"{ctx}: planes differ at [bin, dir, y, x] {np.argwhere(got != want)[:4].tolist()}"
    assert info["bin_steps"] == [int(want[b].sum()) for b in range(n_bins)] and info["steps"] == int(want.sum()), ctx
    for b in range(n_bins):
        assert np.array_equal(api.demand_plane(b), want[b].sum(axis=0, dtype=np.uint32)), f"{ctx}: bin {b}, the sum of the directions"
    for f in (1, 7, 64):
        b = n_bins - 1
        assert np.array_equal(api.demand_pooled(f, b), ou.pooled(want[b].sum(axis=0, dtype=np.uint32), f)), f"{ctx}: pooled by {f}"
        assert np.array_equal(api.demand_pooled(f, 0, "E"), ou.pooled(want[0, 1], f)), f"{ctx}: E plane pooled by {f}"
    assert np.array_equal(api.demand_groups(), de.group_rows(tr, want)), f"{ctx}: group rows"


# ---- what the fixtures alone decide (checked on the CPU by tests/test_ext_sidecar.py) ------------------------------------
def ticks_of(tr):
    """The ticks a mode replays: the whole trace where it has at most 80, otherwise the first 60."""
    T = ou.n_ticks(tr)
    return T if T <= 80 else 60


def check_ticks(T):
    """After every 10th tick and after the last."""
    return [t for t in range(T) if t % CHECK_EVERY == CHECK_EVERY - 1 or t == T - 1]


def spawned_by(tr, t):
    """Vehicles placed up to and including tick t, as far as the rows show them (spawn indices are handed out in order)."""
    n0 = len(tr["v_start_xy"])
    rows = tr["veh_rows"][:tr["veh_off"][t + 1]]
    return max(n0, int(rows[:, V["spawn_idx"]].max()) + 1 if len(rows) else 0)


def first_parked_tick(tr):
    """The first tick after which a row carries F_PARKED (a service vehicle standing at its block), or None."""
    for t in range(ou.n_ticks(tr)):
        if ((ou.rows_at(tr, t)[:, V["flags"]] & capi.F_PARKED) != 0).any():
            return t
    return None


def generator_ticks(tr):
    """(T, vehicles spawned by T, first tick with a parked vehicle): T is the smallest multiple of 10 by which the rows show
    more than twice the initial population spawned and a parked service vehicle; None where the trace never gets there."""
    n0, parked = len(tr["v_start_xy"]), first_parked_tick(tr)
    if parked is None:
        return None
    for T in range(CHECK_EVERY, ou.n_ticks(tr) + 1, CHECK_EVERY):
        if spawned_by(tr, T - 1) > 2 * n0 and parked < T:
            return T, spawned_by(tr, T - 1), parked
    return None


def since_written(tr, ticks):
    """{check tick: the most cells a vehicle alive after it has driven since its path was last written}, from the rows alone.
    A trace without searches (astar_per_tick is 0 throughout): every path was written at spawn, so that is steps_traveled.
    A trace with searches: every path computation resets the vehicle's cooldown to PATHFINDING_COOLDOWN
    (ou.keeps_its_path), so a row whose cooldown is not that value after a tick kept its path through the tick; a row that
    carries it counts as rewritten there (a lower bound).  17 cells or more: under a collection per tick the path has lost
    its first word and path_cur stands inside a word."""
    searches = int(np.sum(tr["astar_per_tick"])) > 0
    pc = ou.cooldown_param(tr)
    written = {}
    out = {}
    due = set(check_ticks(ticks))
    for t in range(ticks):
        rows = ou.rows_at(tr, t)
        for r in rows:
            v, s = int(r[V["spawn_idx"]]), int(r[V["steps_traveled"]])
            if v not in written:
                written[v] = 0
            if searches and int(r[V["cooldown"]]) == pc:
                written[v] = s
        if t in due and len(rows):
            out[t] = max(int(r[V["steps_traveled"]]) - written[int(r[V["spawn_idx"]])] for r in rows)
    return out


def light_fixtures_with_searches(names):
    """The light-control fixtures in whose recorded run searches ran inside ticks."""
    from trafficsimulation_amd.world import load_trace
    from tests.trace_util import trace_path
    return [n for n in names if int(np.sum(load_trace(trace_path(n))["astar_per_tick"])) > 0]


def zone_plane(tr):
    """The OD zones of a trace's map: road cell number k (row-major over the whole map) lies in zone k % 7, other cells in none."""
    H, W = int(tr["height"]), int(tr["width"])
    cell = np.arange(H * W, dtype=np.int32).reshape(H, W)
    return np.where(np.asarray(tr["is_road_map"]) == 1, cell % N_ZONES, -1).astype(np.int32)


def walk_conditions(wants):
    """What the select-link expectations {(gate set "A" / "B", query): se.walk result} of one tick say about the cases:
    two_gates - a vehicle crosses two gates or more; far_first - a first crossing at step 16 or later; cut_tail - a vehicle
    with fewer crossings under the query without the open tail than under whole paths."""
    open_, cut = DEMAND_QUERIES[0], SELECTLINK_QUERIES[-1]
    return dict(two_gates=any(bin(int(m)).count("1") >= 2 for k in "AB" for m in wants[k, open_]["mask"]),
                far_first=bool(any((wants[k, q]["first_step"] >= FAR_STEP).any() for k in "AB" for q in SELECTLINK_QUERIES)),
                cut_tail=bool(any((wants[k, cut]["crossings"] < wants[k, open_]["crossings"]).any() for k in "AB")))


def field_conditions(tr, t):
    """What the fixture alone says about the cost-field queries after tick t, computed with zero density (costs depend on the
    density, reachability does not): (road cells, cells query A reaches, cells query B reaches, road cells B reaches, live
    vehicles, live vehicles on a cell that A does not reach).  The cells reached can outnumber the road cells: flow bits
    lead onto cells that are no road."""
    H, W = int(tr["height"]), int(tr["width"])
    occ, stop = (np.unpackbits(tr[k][t])[:H * W].reshape(H, W) for k in ("occ_t", "stop_t"))
    rule = ce.Rule(tr["defaults_json"], tr["allowed_dirs_map"], tr["is_road_map"], tr["road_type_map"], occ, stop, np.zeros((H, W)))
    seeds = np.asarray(tr["highway_exits_xy"], dtype=np.int32).reshape(-1, 2)
    cost = [k % 4 for k in range(len(seeds))]
    a, _ = ce.field(rule, seeds, cost, **FIELD_A)
    b, _ = ce.field(rule, seeds, cost, **FIELD_B)
    rows = ou.rows_at(tr, t)
    at = a[rows[:, V["y"]], rows[:, V["x"]]]
    road = np.asarray(tr["is_road_map"]) == 1
    return (int(road.sum()), int((a != ce.UNREACHABLE).sum()), int((b != ce.UNREACHABLE).sum()), int((b[road] != ce.UNREACHABLE).sum()),
            len(rows), int((at == ce.UNREACHABLE).sum()))


def replay_tick(api, tr, t):
    """trace_util.replay_and_compare over the one tick t (the slice of the trace as a trace of its own)."""
    sub = dict(tr)
    for k in ("occ_t", "stop_t", "stuck_t", "rain_t", "grp_rows", "nsched_t", "rng_rows", "cnt_rows", "blk_rows"):
        if k in sub:
            sub[k] = tr[k][t:t + 1]
    off = np.asarray(tr["veh_off"])
    sub["veh_rows"], sub["veh_off"] = tr["veh_rows"][off[t]:off[t + 1]], off[t:t + 2] - off[t]
    sub.pop("raised_at_tick", None)
    assert replay_and_compare(api, sub, ticks=1) == 1


def type_tables(tables):
    """(type plane, cell palette) of a world: from its cell_type_map, or the facade's fallback where the trace has none."""
    if "cell_type_map" in tables:
        return rn.type_plane(tables["cell_type_map"], tables.get("cell_base_type_map")), rn.cell_palette()
    plane = rn.fallback_type_plane(tables["is_road_map"], tables["intersection_map"], tables["light_ctrl_xy"], tables["light_xy"])
    return plane, rn.cell_palette(type_names=rn.fallback_type_names())


class Sidecar:
    def __init__(self, api, tr, tables=None, fixture_paths=False, analyses=True):
        """`api` is set up from `tr` and has not stepped.  `tables` (default: the trace) holds the world tables the renderer
        is configured from.  fixture_paths: the trace's vehicles keep their spawn-time paths (explicit paths, no search):
        demand is held to de.fixture_vehicles instead of download_path.  analyses: the cost field, its routes and select-link
        are checked and bundled too (the trace must have highway exits)."""
        self.api, self.tr, self.fixture_paths, self.analyses = api, tr, fixture_paths, analyses
        tables = tr if tables is None else tables
        self.tables = tables
        self.H, self.W = int(tr["height"]), int(tr["width"])
        if analyses:
            self.seeds = np.asarray(tr["highway_exits_xy"], dtype=np.int32).reshape(-1, 2)
            self.seed_cost = [k % 4 for k in range(len(self.seeds))]
            self.params = api.params_from_defaults(tr["defaults_json"])
            self.zones = zone_plane(tr)
            api.selectlink.set_zones(self.zones, N_ZONES)
            self.last_walk = None                                  # (the expectation of set A, whole paths, at the last check)
        api.observe_start()
        ever = spawned_by(tr, ou.n_ticks(tr) - 1)
        api.triplog_start(-(-ever // 64) * 64)
        plane, pal = type_tables(tables)
        api.render_set_cells(plane, pal)
        api.render_set_vehicle_palette(rn.vehicle_palette())
        api.render_set_heat_lut(rn.heat_lut())
        live = [int(v) for v in api.vehicles()[:, V["spawn_idx"]]]
        seq = tu.sequence(tr)
        leaver = [int(seq[0, 1])] if len(seq) and int(seq[0, 1]) in live else []
        self.routes = sorted(set(live[::3] + leaver))
        self.leaver = leaver[0] if leaver else None
        api.render_set_routes(self.routes, ROUTE_RGBA)
        self.last = -1                                             # the tick of the previous check
        self.planes = np.zeros((7, self.H, self.W), dtype=np.uint32)
        self.steps = {v: 0 for v in live}                          # steps_traveled at the previous check
        self.n_records = 0
        # fields / routes: planes and routes held to the expectation; n_spawned and conditions: one entry per check tick
        self.stats = {"checks": 0, "paths": 0, "fields_compared": 0, "routes_compared": 0, "selectlink_computes": 0,
                      "n_spawned": [], "conditions": []}

    def views(self):
        W, H = self.W, self.H
        common = dict(layers=capi.RL_ALL, heat_plane="present", heat_max=5, background=BG)
        return {"full": rn.make_view(cells_w=W, cells_h=H, **common),
                "shrunk": rn.make_view(cells_w=W, cells_h=H, shrink=4, **common),
                "window": rn.make_view(x0=(W - 7) | 1, y0=H - 5, cells_w=11, cells_h=9, zoom=3, **common)}

    def check(self, t, last=False):
        """The rules and the bundle after tick t; `last`: the run's last check tick, at which the analyses also trace query
        B's routes and load a second weight vector (every mode's wall time had more than doubled with them at every check)."""
        api, tr, H, W = self.api, self.tr, self.H, self.W
        ctx = f"tick {t}"
        out = {}
        rows = api.vehicles()
        # paths: download_path is the path the row's CRC and length speak of
        paths = [api.path(k) for k in range(len(rows))]
        for k, r in enumerate(rows):
            assert len(paths[k]) == int(r[V["path_len"]]), f"{ctx}: vehicle {int(r[0])}: {len(paths[k])} cells downloaded, the row has {int(r[V['path_len']])}"
            crc = capi.path_crc(paths[k]) if len(paths[k]) else 0
            assert crc == int(r[V["path_crc"]]) & 0xFFFFFFFF, f"{ctx}: vehicle {int(r[0])}: the downloaded path has another CRC than the row"
        self.stats["paths"] += len(rows)
        out["path_len"] = np.asarray([len(p) for p in paths], dtype=np.int64)
        out["path_xy"] = np.concatenate(paths + [np.zeros((0, 2), np.int32)]).astype(np.int32)
        # demand
        veh = [(int(r[V["x"]]), int(r[V["y"]]), paths[k]) for k, r in enumerate(rows)]
        if self.fixture_paths:
            fveh, _ = de.fixture_vehicles(tr, t)
            assert len(fveh) == len(veh) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(veh, fveh)), \
                f"{ctx}: download_path is not the rest of the spawn-time path"
            veh = fveh
        for q in DEMAND_QUERIES:
            check_query(api, tr, veh, q, ctx, t + 1)
            info = api.demand_info()
            out[f"demand_{q[0]}_{q[1]}"] = read_planes(api, q[0])
            out[f"demand_totals_{q[0]}_{q[1]}"] = np.asarray([info["steps"], info["vehicles"]] + list(info["bin_steps"]), dtype=np.int64)
            out[f"demand_groups_{q[0]}_{q[1]}"] = api.demand_groups()
            out[f"demand_pooled7_{q[0]}_{q[1]}"] = api.demand_pooled(7)
        # routes: the layer alone, over the whole map
        frame = api.render(rn.make_view(cells_w=W, cells_h=H, layers=capi.RL_ROUTES, background=BG))
        got = (frame[..., :3] == np.asarray(ROUTE_RGBA[:3], dtype=np.uint8)).all(axis=2)
        pos_of = {int(s): k for k, s in enumerate(rows[:, V["spawn_idx"]])}
        want = np.zeros((H, W), dtype=bool)
        for v in self.routes:
            if v in pos_of:
                want |= rx.mask_of(paths[pos_of[v]], H, W)
        assert np.array_equal(got, want), f"{ctx}: the route layer is not the downloaded paths at (y, x) {np.argwhere(got != want)[:4].tolist()}"
        out["frame_routes"] = frame
        for name, view in self.views().items():
            out[f"frame_{name}"] = api.render(view)
        # observation
        planes = ou.read_planes(api)
        want_s = self.planes[SAMPLED].copy()
        for u in range(self.last + 1, t + 1):
            want_s += ou.sampled_delta(tr, u)
        for k in range(3):
            assert np.array_equal(planes[k], want_s[k]), f"{ctx}: plane {capi.OBS_PLANES[k]} did not grow by what the rows of ticks {self.last + 1} .. {t} add"
        rec = api.trips()
        ended = rec[self.n_records:]
        now = {int(r[V["spawn_idx"]]): int(r[V["steps_traveled"]]) for r in rows}
        moved = sum(s - self.steps.get(v, 0) for v, s in now.items())
        moved += sum(int(r["distance"]) - self.steps.get(int(r["spawn_idx"]), 0) for r in ended)
        grown = int(planes[ENTER].astype(np.int64).sum()) - int(self.planes[ENTER].astype(np.int64).sum())
        assert grown == moved, f"{ctx}: the ENTER planes grew by {grown}, steps_traveled and the finished trips by {moved}"
        out["observe"] = planes
        # trip log
        seq = np.stack([rec["end_step"], rec["spawn_idx"]], axis=1).astype(np.int64).reshape(-1, 2)
        want_seq = tu.sequence(tr, t + 1)
        assert np.array_equal(seq, want_seq), f"{ctx}: the trip log's (end_step, spawn_idx) is not the rows' sequence"
        out["trips"] = np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()
        if self.analyses:
            # (after everything above, whose keys keep their bytes; the demand result is left as the last query above left it)
            before = api.counters()
            self.check_fields(t, rows, out, last)
            self.check_selectlink(t, rows, veh, out)
            api.demand_compute(*DEMAND_QUERIES[-1][:2], bool(DEMAND_QUERIES[-1][2]))
            after = api.counters()
            for f in ("astar_calls", "astar_expansions", "astar_relaxations", "step_count"):
                assert getattr(before, f) == getattr(after, f), f"{ctx}: the analyses moved the counter {f}"
        self.last, self.planes, self.steps, self.n_records = t, planes, now, len(rec)
        self.stats["checks"] += 1
        return out

    def check_fields(self, t, rows, out, last):
        """The cost field of the highway exits and the routes along it on the engine's maps as they are after tick t: query A
        (TO, soft) with the live vehicles' routes under their headings and the load they make, query B (FROM, strict, against
        the flow) and, at the last check tick, the routes that arrive at the vehicles and the load under a second weight
        vector."""
        api, H, W = self.api, self.H, self.W
        r = api.costfield.routes
        rule = er.rule_of(api, self.params, self.tables)
        seeds, cost = self.seeds, self.seed_cost
        starts = np.ascontiguousarray(rows[:, [V["x"], V["y"]]].astype(np.int32))
        heads = np.maximum(rows[:, V["direction"]], -1).astype(np.int8)
        spawn = rows[:, V["spawn_idx"]]
        for tag, q, hd in (("a", FIELD_A, heads), ("b", FIELD_B, None)):
            ctx = f"tick {t}: field {tag.upper()} {q}"
            routed = len(starts) > 0 and (tag == "a" or last)
            want_v, want_o = ce.field(rule, seeds, cost, **q)
            info = r.compute(seeds, cost, **q)
            got_v, got_o = api.costfield.plane("cost"), api.costfield.plane("owner")
            assert np.array_equal(got_v, want_v), f"{ctx}: values differ at (y, x) {np.argwhere(got_v != want_v)[:4].tolist()}"
            assert np.array_equal(got_o, want_o), f"{ctx}: owners differ at (y, x) {np.argwhere(got_o != want_o)[:4].tolist()}"
            finite = want_v != ce.UNREACHABLE
            assert info["reached"] == int(finite.sum()) and info["max_value"] == (int(want_v[finite].max()) if finite.any() else 0), ctx
            assert (info["tick"], info["n_seeds"], info["mode"], info["headings"]) == (t + 1, len(seeds), q["mode"], re_.headings(rule)), ctx
            out[f"field_{tag}_cost"], out[f"field_{tag}_owner"] = got_v, got_o
            out[f"field_{tag}_totals"] = np.asarray([info["reached"], info["max_value"]], dtype=np.int64)
            self.stats["fields_compared"] += 1
            if not (routed or tag == "a"):
                continue
            L, hops, nh = er.expectation(rule, seeds, cost, q)
            got_h = er.download_hops(api)
            assert np.array_equal(got_h, hops), f"{ctx}: hop plane differs at (y, x) {np.argwhere(got_h != hops)[:4].tolist()}"
            if tag == "a":
                out["field_a_hops"] = got_h
            if not routed:
                continue
            totals = []
            want = re_.batch(hops, L, q["mode"], nh, starts, hd)
            traced = er.check_batch(api, want, starts, hd, q["mode"], ctx)
            for name, a in zip(("off", "dirs", "cost", "owner"), r.routes()):
                out[f"routes_{tag}_{name}"] = a
            totals += [traced["n"], traced["steps"], traced["longest"], traced["unreached"]]
            self.stats["routes_compared"] += len(starts)
            if tag == "a":
                loads = [("unit", None)] + ([("weighted", ((spawn.astype(np.int64) * 37) % 1001).astype(np.uint32))] if last else [])
                for wname, weights in loads:
                    load = r.load(starts, hd, weights)
                    exp = re_.load_planes((H, W), q["mode"], starts, want[0], want[1], weights)
                    got = np.stack([r.load_plane(d) for d in range(4)])
                    assert np.array_equal(got, exp), f"{ctx}: load planes, {wname} weights, differ at [dir, y, x] {np.argwhere(got != exp)[:4].tolist()}"
                    assert np.array_equal(r.load_plane(), exp.sum(axis=0, dtype=np.uint32)), f"{ctx}: the device sum of the load planes, {wname} weights"
                    unreached = int((want[3] == -1).sum())
                    assert (load["steps"], load["unreached"], load["routes"]) == (int(exp.sum(dtype=np.uint64)), unreached, len(starts) - unreached), \
                        f"{ctx}: load totals, {wname} weights: {load}"
                    out[f"load_{wname}"] = got
                    totals += [load["steps"], load["routes"], load["unreached"]]
            out[f"routes_{tag}_totals"] = np.asarray(totals, dtype=np.int64)

    def check_selectlink(self, t, rows, veh, out):
        """Select-link over the gate sets of the whole-path demand plane just verified: every array against the walk of
        download_path, the cross table against the engine's own demand planes, a selection through ts_demand_compute, OD."""
        api, tr, H, W = self.api, self.tr, self.H, self.W
        s = api.selectlink
        spawn = rows[:, V["spawn_idx"]].astype(np.int64)
        n = api.num_spawned()
        self.stats["n_spawned"].append(n)
        sets = se.gate_sets(out["demand_1_1"][0], tr["is_road_map"])
        wants = {}
        for name, gates in zip("AB", sets):
            s.set_gates(gates)
            for q in SELECTLINK_QUERIES:
                ctx = f"tick {t}: select-link, set {name}, query {q}"
                want = wants[name, q] = se.walk(H, W, veh, spawn, n, gates, q[0], q[1], bool(q[2]))
                got = er.check_result(s, want, gates, q, t + 1, ctx)
                self.stats["selectlink_computes"] += 1
                key = f"demand_{q[0]}_{q[1]}"
                if q in DEMAND_QUERIES:
                    planes = out[key]
                else:
                    api.demand_compute(q[0], q[1], bool(q[2]))
                    planes = read_planes(api, q[0])
                assert np.array_equal(got["cross"], se.from_planes(planes, gates)), f"{ctx}: cross is not the demand planes summed over the gates' cells"
                for k in ("mask", "crossings", "first_step", "first_gate", "cross", "pair"):
                    out[f"selectlink_{name}_{q[0]}_{q[1]}_{k}"] = got[k]
                out[f"selectlink_{name}_{q[0]}_{q[1]}_totals"] = np.asarray([got["t_vehicles"], got["t_crossing"], got["t_crossings"]], dtype=np.int64)
        # a selection over set A, whole paths: its load through ts_demand_compute, its OD counts
        whole = wants["A", DEMAND_QUERIES[0]]
        ctx = f"tick {t}: select-link, set A, selection {SELECT}"
        s.set_gates(sets[0])
        s.compute(*DEMAND_QUERIES[0][:2], bool(DEMAND_QUERIES[0][2]))
        self.stats["selectlink_computes"] += 1
        sel, count = s.select(**SELECT)
        rule = se.selected(whole, **SELECT)
        assert sel.dtype == np.uint8 and np.array_equal(sel, rule) and count == int(rule.sum()), f"{ctx}: the select bytes"
        picked = [v for v, i in zip(veh, spawn) if rule[i]]
        info = api.demand_compute(4, 16, True, select=sel)
        assert info["selected"] and info["vehicles"] == count, ctx
        got = read_planes(api, 4)
        assert np.array_equal(got, de.planes(H, W, picked, 4, 16, True)), f"{ctx}: the demand planes of the selected vehicles"
        pos, goal = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
        pos[spawn] = rows[:, [V["x"], V["y"]]]
        goal[spawn] = api.vehicle_meta()[:, [capi.M_FIELDS.index("target_x"), capi.M_FIELDS.index("target_y")]]
        for tag, kw in (("all", {}), ("sel", SELECT)):
            counts, unzoned = s.od(**kw)
            w_counts, w_unzoned = se.od(se.selected(whole, **kw), pos, goal, self.zones, N_ZONES)
            assert counts.dtype == np.int64 and np.array_equal(counts, w_counts) and unzoned == w_unzoned, f"{ctx}: OD counts ({tag})"
            out[f"selectlink_od_{tag}"] = np.concatenate([counts.ravel(), [unzoned]]).astype(np.int64)
        out["selectlink_select"] = sel
        # what the expectation alone says about the cases (asserted by covered())
        self.stats["conditions"].append(walk_conditions(wants))
        self.last_walk = dict(whole, spawn=spawn)

    def covered(self):
        """The analyses ran, and on cases that can tell a wrong walk from a right one - from the expectation alone, at the last
        check tick: a vehicle crosses two gates or more, a first crossing lies beyond the path's first pool word, and a
        vehicle has fewer crossings without the open tail than with it."""
        st = self.stats
        assert st["fields_compared"] > 0 and st["routes_compared"] > 0 and st["selectlink_computes"] > 0, st
        last = st["conditions"][-1]
        assert last["two_gates"], "at the last check tick no vehicle crosses two gates"
        assert last["far_first"], f"at the last check tick no first crossing lies at step {FAR_STEP} or later"
        assert last["cut_tail"], f"at the last check tick query {SELECTLINK_QUERIES[-1]} cuts no crossing off"


def run_trace(api, tr, ticks, sidecar):
    """Replay ticks [0, ticks) one at a time, every tick against the trace; the bundles of the check ticks, in order."""
    due = set(check_ticks(ticks))
    bundles = []
    for t in range(ticks):
        replay_tick(api, tr, t)
        if t in due:
            bundles.append(sidecar.check(t, last=t == ticks - 1))
    if sidecar.analyses:
        sidecar.covered()
    return bundles


def flatten(bundles):
    """A list of bundles as one dict for np.savez."""
    return {f"{i:03d}/{k}": v for i, b in enumerate(bundles) for k, v in b.items()}


def assert_same_bundles(got, want, ctx):
    """Two flattened bundle lists, byte for byte."""
    assert sorted(got) == sorted(want), f"{ctx}: bundles hold {sorted(set(got) ^ set(want))[:6]} on one side only"
    for k in sorted(want):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{ctx}: {k} differs from the default mode's"
