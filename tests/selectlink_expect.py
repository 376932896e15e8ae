"""Expected select-link results (include/trafficsim_selectlink.h) in numpy - no engine.

The rule, restated: a gate is a set of (cell, direction mask) pairs, the mask bits being N 1, E 2, S 4, W 8 and a bit the
direction of the step *into* the cell (N is y + 1).  A (cell, direction) belongs to at most one gate.  Every vehicle contributes
the cells of its remaining main path (what ts_download_path returns: without the cell it stands on, step k = 0 being its next
cell); for k < n_bins * bin_cells the bin is k // bin_cells, a later step counts in the last bin when open_tail is set and does
not exist for the query otherwise.  Step k of vehicle v into cell c in direction d is a crossing of gate g when (c, d) belongs
to g.  Per vehicle, by spawn index: `mask` (the gates it crosses), `crossings`, `first_step` (the smallest counted k that is a
crossing) and `first_gate` (that step's gate), 0 / 0 / -1 / -1 for a spawn index that is no live vehicle.  Totals:
cross[gate][bin][dir], pair[a][b] = the vehicles crossing both a and b, the vehicles walked, those with a mask, the sum of
cross.  A vehicle is selected by (any, all, none) when it was walked and (any == 0 or mask & any) and mask & all == all and
mask & none == 0.

`walk` takes the vehicles as (x, y, cells) triples with their spawn indices, as demand_expect.fixture_vehicles and
engine_vehicles give them; gates are lists of (x, y) or (x, y, "NESW"-subset), as selectlink.SelectLink.set_gates takes them."""
import numpy as np

from tests import demand_expect as de

DIR_BIT = {"N": 1, "E": 2, "S": 4, "W": 8}
QUERIES = de.QUERIES


def gate_plane(H, W, gates):
    """(4, H, W) int8: the gate of a step into (y, x) in direction d, -1 for none."""
    plane = np.full((4, H, W), -1, dtype=np.int8)
    for g, gate in enumerate(gates):
        for cell in gate:
            x, y = int(cell[0]), int(cell[1])
            dirs = cell[2] if len(cell) > 2 else "NESW"
            for ch in dirs:
                d = "NESW".index(ch)
                assert plane[d, y, x] == -1, f"({x}, {y}, {ch}) is claimed twice"
                plane[d, y, x] = g
    return plane


def walk(H, W, vehicles, spawn, n_spawned, gates, n_bins=1, bin_cells=1, open_tail=True):
    """The whole result as a dict: "mask" uint32, "crossings" uint32, "first_step" int32, "first_gate" int8 (n_spawned each),
    "walked" bool, "cross" (G, n_bins, 4) uint64, "pair" (G, G) uint64, and the totals "t_vehicles", "t_crossing", "t_crossings"."""
    G = len(gates)
    gp = gate_plane(H, W, gates)
    r = {"mask": np.zeros(n_spawned, np.uint32), "crossings": np.zeros(n_spawned, np.uint32),
         "first_step": np.full(n_spawned, -1, np.int32), "first_gate": np.full(n_spawned, -1, np.int8),
         "walked": np.zeros(n_spawned, bool), "cross": np.zeros((G, n_bins, 4), np.uint64), "pair": np.zeros((G, G), np.uint64)}
    for (x, y, cells), s in zip(vehicles, spawn):
        s = int(s)
        r["walked"][s] = True
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        if len(cells) == 0:
            continue
        prev = np.vstack([[[x, y]], cells[:-1]])
        dx, dy = cells[:, 0] - prev[:, 0], cells[:, 1] - prev[:, 1]
        assert np.all(np.abs(dx) + np.abs(dy) == 1), "a path step that is no move to a 4-neighbour"
        d = np.where(dy == 1, 0, np.where(dx == 1, 1, np.where(dy == -1, 2, 3)))
        k = np.arange(len(cells))
        b = k // bin_cells
        keep = b < n_bins
        if open_tail:
            b, keep = np.minimum(b, n_bins - 1), np.ones(len(cells), dtype=bool)
        g = gp[d, cells[:, 1], cells[:, 0]].astype(np.int64)
        hit = keep & (g >= 0)
        if not hit.any():
            continue
        np.add.at(r["cross"], (g[hit], b[hit], d[hit]), 1)
        mask = 0
        for gg in np.unique(g[hit]):
            mask |= 1 << int(gg)
        r["mask"][s] = mask
        r["crossings"][s] = int(hit.sum())
        first = int(np.argmax(hit))
        r["first_step"][s], r["first_gate"][s] = first, g[first]
        on = [a for a in range(G) if mask >> a & 1]
        for a in on:
            for c in on:
                r["pair"][a, c] += 1
    r["t_vehicles"] = int(r["walked"].sum())
    r["t_crossing"] = int((r["mask"] != 0).sum())
    r["t_crossings"] = int(r["cross"].sum())
    return r


def selected(r, any=0, all=0, none=0):
    """The select bytes (uint8, n_spawned) of a result."""
    m = r["mask"].astype(np.int64)
    ok = r["walked"] & ((m & any) != 0 if any else True) & ((m & all) == all) & ((m & none) == 0)
    return ok.astype(np.uint8)


def od(sel, pos_xy, goal_xy, zones, n_zones):
    """(counts (Z, Z) int64, unzoned) of the spawn indices with a select byte: pos_xy / goal_xy are (n_spawned, 2), whatever
    they hold for the unselected."""
    counts, unzoned = np.zeros((n_zones, n_zones), dtype=np.int64), 0
    H, W = zones.shape

    def zone_of(x, y):          # (a cell outside the map has no zone)
        return int(zones[y, x]) if 0 <= x < W and 0 <= y < H else -1
    for s in np.nonzero(sel)[0]:
        zo, zd = zone_of(*pos_xy[s]), zone_of(*goal_xy[s])
        if zo < 0 or zd < 0:
            unzoned += 1
        else:
            counts[zo, zd] += 1
    return counts, unzoned


def from_planes(planes, gates):
    """cross (G, n_bins, 4) from demand planes (n_bins, 4, H, W): the planes summed over every gate's accepting cells."""
    out = np.zeros((len(gates), planes.shape[0], 4), dtype=np.uint64)
    for g, gate in enumerate(gates):
        for cell in gate:
            for ch in (cell[2] if len(cell) > 2 else "NESW"):
                d = "NESW".index(ch)
                out[g, :, d] += planes[:, d, int(cell[1]), int(cell[0])].astype(np.uint64)
    return out


def top_cells(load, n=32):
    """The n most loaded cells of an (H, W) plane as (x, y), taken with a stable sort."""
    order = np.argsort(-load.astype(np.int64).ravel(), kind="stable")[:n]
    return [(int(i % load.shape[1]), int(i // load.shape[1])) for i in order]


def gate_sets(whole, is_road):
    """The two gate sets derived from the whole-path demand planes `whole` (4, H, W) themselves.
    A: the 32 most loaded cells as single-cell gates open to all directions.
    B: 8 gates of 4 such cells each, every cell open only to its most used direction, and a ninth gate on the first road cell
    (row-major) that no route enters."""
    load = whole.astype(np.int64).sum(axis=0)
    top = top_cells(load)
    A = [[(x, y)] for x, y in top]
    B = [[(x, y, "NESW"[int(np.argmax(whole[:, y, x]))]) for x, y in top[4 * g:4 * g + 4]] for g in range(8)]
    ys, xs = np.nonzero((np.asarray(is_road) == 1) & (load == 0))
    B.append([(int(xs[0]), int(ys[0]))])
    return A, B


GATE31 = 1 << 31


def gate31_selections(mask):
    """Three selections over a 32-gate set, one with each of any, all and none doing work and gate 31 in each: any = gate 31 or
    gate 1; all = gate 31 and the gate its vehicles cross most often besides it; any = the gate whose vehicles split most evenly
    into those that cross gate 31 too and those that do not, without gate 31."""
    hit31, miss31 = mask[(mask & GATE31) != 0], mask[(mask & GATE31) == 0]
    assert len(hit31), "no route crosses gate 31"
    both = [int((hit31 >> g & 1).sum()) for g in range(31)]
    split = int(np.argmax([min(both[g], int((miss31 >> g & 1).sum())) for g in range(31)]))
    return [dict(any=GATE31 | 2), dict(all=GATE31 | 1 << int(np.argmax(both))), dict(any=1 << split, none=GATE31)]
