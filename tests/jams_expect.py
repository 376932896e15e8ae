"""The jam rule of include/trafficsim_jams.h in plain numpy with a union-find: the count plane of vehicle rows, the components
of a count plane under the GRID or FLOW links, the records, the per-vehicle array, the group rows, and the masks the tests
label.  No engine, no pytest."""
import numpy as np

from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd.jams import JAM_DTYPE, JG_FIELDS

V = {n: i for i, n in enumerate(capi.V_FIELDS)}
GRID, FLOW = 0, 1
TILE = 8          # the smallest tile side of the device's LDS stage: what "across a tile border" means for the masks


def standing_rows(rows, min_ticks=1):
    """The rows (ts_download_vehicles) of the standing vehicles."""
    rows = np.asarray(rows).reshape(-1, len(capi.V_FIELDS))
    return rows[(rows[:, V["stuck_ticks"]] >= min_ticks) & ((rows[:, V["flags"]] & capi.F_PARKED) == 0)]


def count_plane(rows, H, W, min_ticks=1):
    out = np.zeros((H, W), dtype=np.uint32)
    st = standing_rows(rows, min_ticks)
    np.add.at(out, (st[:, V["y"]], st[:, V["x"]]), 1)
    return out


def fixture_rows(tr, block):
    """Block `block` of a trace's veh_rows: the state after block + 1 steps."""
    return np.asarray(tr["veh_rows"][tr["veh_off"][block]:tr["veh_off"][block + 1]])


def _find(parent, c):
    r = c
    while parent[r] != r:
        r = parent[r]
    while parent[c] != r:
        parent[c], c = r, parent[c]
    return r


def label(count, link, allowed=None):
    """(H, W) int32 jam numbers of a count plane, -1 where nothing stands: union-find over the E and N links, the smaller root
    wins, jams numbered by ascending root."""
    count = np.asarray(count)
    H, W = count.shape
    st = count > 0
    al = (np.asarray(allowed).astype(np.int64) & 15) if allowed is not None else np.zeros((H, W), dtype=np.int64)
    parent = np.arange(H * W)
    ys, xs = np.nonzero(st)
    for y, x in zip(ys.tolist(), xs.tolist()):
        for d, (dx, dy) in ((1, (1, 0)), (0, (0, 1))):          # E, N (N is cell + width)
            nx, ny = x + dx, y + dy
            if nx >= W or ny >= H or not st[ny, nx]:
                continue
            if link == FLOW and not (al[y, x] >> d & 1 or al[ny, nx] >> ((d + 2) & 3) & 1):
                continue
            a, b = _find(parent, y * W + x), _find(parent, ny * W + nx)
            if a != b:
                parent[max(a, b)] = min(a, b)
    out = np.full(H * W, -1, dtype=np.int32)
    cells = (ys * W + xs).tolist()
    roots = np.array([_find(parent, c) for c in cells], dtype=np.int64)
    out[cells] = np.searchsorted(np.unique(roots), roots)
    return out.reshape(H, W)


def records(lab, count, inter=None, rows=None, min_ticks=1):
    """JAM_DTYPE records of a label plane; `rows`: the vehicle rows behind a count plane made of vehicles (None: mask mode)."""
    lab, count = np.asarray(lab), np.asarray(count)
    H, W = lab.shape
    n = int(lab.max()) + 1 if lab.size else 0
    rec = np.zeros(max(n, 0), dtype=JAM_DTYPE)
    ys, xs = np.nonzero(lab >= 0)
    js = lab[ys, xs]
    for j in range(n):
        m = js == j
        y, x = ys[m], xs[m]
        root = int((y * W + x).min())
        r = rec[j]
        r["root_x"], r["root_y"], r["cells"], r["vehicles"] = root % W, root // W, len(x), int(count[y, x].astype(np.int64).sum())
        r["x0"], r["y0"], r["x1"], r["y1"] = x.min(), y.min(), x.max(), y.max()
        r["extent"] = max(int(x.max() - x.min()), int(y.max() - y.min())) + 1
        r["inter_cells"] = int((np.asarray(inter)[y, x] != 0).sum()) if inter is not None else 0
    if rows is not None:
        for row in standing_rows(rows, min_ticks):
            r = rec[lab[row[V["y"]], row[V["x"]]]]
            r["stuck_max"] = max(int(r["stuck_max"]), int(row[V["stuck_ticks"]]))
            r["stuck_sum"] += int(row[V["stuck_ticks"]])
    return rec


def per_vehicle(lab, rows, n_spawned, min_ticks=1):
    out = np.full(n_spawned, -1, dtype=np.int32)
    if rows is not None:
        st = standing_rows(rows, min_ticks)
        out[st[:, V["spawn_idx"]]] = lab[st[:, V["y"]], st[:, V["x"]]]
    return out


def group_lists(tr, g):
    """The three CSR lists of group g as (x, y) arrays: ns_in, ew_in, the intersection's cells."""
    return [np.asarray(tr[k + "_xy"]).reshape(-1, 2)[tr[k + "_off"][g]:tr[k + "_off"][g + 1]] for k in ("g_ns_in", "g_ew_in", "g_icell")]


def group_rows(tr, lab, rec):
    """[G][JG_FIELDS] int64 from the trace's own g_*_xy tables."""
    G = len(tr["g_icell_off"]) - 1
    out = np.zeros((G, len(JG_FIELDS)), dtype=np.int64)
    f = JG_FIELDS.index
    for g in range(G):
        ns, ew, box = group_lists(tr, g)
        for ax, xy in (("ns", ns), ("ew", ew)):
            js = sorted({int(j) for j in lab[xy[:, 1], xy[:, 0]] if j >= 0})
            out[g, f(ax + "_jams")] = len(js)
            out[g, f(ax + "_cells")] = sum(int(rec[j]["cells"]) for j in js)
            out[g, f(ax + "_vehicles")] = sum(int(rec[j]["vehicles"]) for j in js)
            out[g, f(ax + "_stuck_max")] = max([int(rec[j]["stuck_max"]) for j in js], default=0)
            out[g, f(ax + "_extent")] = max([int(rec[j]["extent"]) for j in js], default=0)
        jb = lab[box[:, 1], box[:, 0]]
        out[g, f("box_jams")], out[g, f("box_cells")] = len({int(j) for j in jb if j >= 0}), int((jb >= 0).sum())
    return out


def expect(count, link, allowed, inter, rows=None, n_spawned=0, min_ticks=1, tr=None):
    """Everything a compute leaves, from a count plane: {"label", "count", "records", "vehicles", "groups" (with `tr`),
    "info": the totals of TsJamInfo}."""
    lab = label(count, link, allowed)
    rec = records(lab, count, inter, rows, min_ticks)
    out = {"label": lab, "count": np.asarray(count, dtype=np.uint32), "records": rec, "vehicles": per_vehicle(lab, rows, n_spawned, min_ticks),
           "info": {"n_jams": len(rec), "standing_cells": int((lab >= 0).sum()), "standing_vehicles": int(np.asarray(count, dtype=np.int64).sum()),
                    "largest_cells": int(rec["cells"].max()) if len(rec) else 0}}
    if tr is not None:
        out["groups"] = group_rows(tr, lab, rec)
    return out


def _spiral(H, W):
    """One path from the corner inwards, a free cell between its turns: it turns where the cell ahead is outside, set, or the
    one behind that is set."""
    sp = np.zeros((H, W), dtype=np.uint8)
    inside = lambda x, y: 0 <= x < W and 0 <= y < H
    may = lambda x, y, dx, dy: inside(x + dx, y + dy) and not sp[y + dy, x + dx] and not (inside(x + 2 * dx, y + 2 * dy) and sp[y + 2 * dy, x + 2 * dx])
    x, y, dx, dy = 0, 0, 1, 0
    sp[0, 0] = 1
    while True:
        if not may(x, y, dx, dy):
            dx, dy = -dy, dx
            if not may(x, y, dx, dy):
                return sp
        x, y = x + dx, y + dy
        sp[y, x] = 1


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def masks(H, W, seed=5):
    """{name: (H, W) uint8} - the shapes that try the labelling: see tests/test_jams_expect.py for what each one must give."""
    rng = np.random.RandomState(seed)
    z = lambda: np.zeros((H, W), dtype=np.uint8)
    out = {"empty": z(), "full": z() + 1}
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = ((xx + yy) % 2 == 0).astype(np.uint8)
    s = z()                                           # boustrophedon: every second row whole, joined at alternating ends
    s[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        s[y, W - 1 if k % 2 == 0 else 0] = 1
    out["serpentine"] = s
    sp = _spiral(H, W)
    out["spiral"] = sp
    c = z()                                           # comb: teeth in tile row 0 (columns 0, 2, 4, ...), the spine in tile row 1
    c[0:TILE, 0::2] = 1
    c[TILE, :] = 1
    out["comb"] = c
    d = z()                                           # diagonal pairs, one across the tile corner (7, 7) / (8, 8): they stay apart
    for x, y in ((2, 2), (3, 3), (TILE - 1, TILE - 1), (TILE, TILE), (20, 5), (21, 4)):
        d[y, x] = 1
    out["diagonals"] = d
    k = z()
    k[0, 0] = k[0, W - 1] = k[H - 1, 0] = k[H - 1, W - 1] = 1
    out["corners"] = k
    p = z()                                           # a pair across every tile border, in both orientations, apart from each other
    for ty in range(0, H, TILE):
        for tx in range(TILE, W, TILE):
            if ty + 3 < H:
                p[ty + 3, tx - 1] = p[ty + 3, tx] = 1
    for ty in range(TILE, H, TILE):
        for tx in range(0, W, TILE):
            if tx + 5 < W and tx + 5 != tx + TILE - 1:
                p[ty - 1, tx + 5] = p[ty, tx + 5] = 1
    out["border_pairs"] = p
    b = (rng.rand(H, W) < 0.4).astype(np.uint8)      # bytes 1 and 255 mixed
    b[b > 0] = np.where(rng.rand(int(b.sum())) < 0.5, 1, 255)
    out["bytes"] = b
    return out


def random_masks(H, W):
    """Seeded random masks at density 0.1, 0.5 and 0.59 (just under the site-percolation threshold 0.5927: large, tortuous
    clusters)."""
    return {f"random_{p}": (np.random.RandomState(int(p * 100)).rand(H, W) < p).astype(np.uint8) for p in (0.1, 0.5, 0.59)}
