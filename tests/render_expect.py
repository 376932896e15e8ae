"""A numpy statement of the renderer's pixel rule (include/trafficsim_render.h), independent of the engine's code: what a
frame must hold, given the state a caller can download and the tables it uploaded.  Everything is integer arithmetic, so
every comparison against it is an equality.

    state = {"W", "H",
             "type": uint8 (H, W) or None, "cell_pal": uint8 (n, 2, 2, 2, 4),
             "veh_pal": uint8 (3, 4, 2, 4) or None, "lut": uint8 (256, 4) or None,
             "stop": int (H, W) stop_map, "rain": int (H, W) rain_map, "pend": bool (H, W),
             "top": int (H, W), kind * 4 + status of the cell's top vehicle, -1 = none,
             "route": bool (H, W), "route_rgba": 4 ints,
             "heat": uint64 (H, W) (the plane, or the sum of the four ENTER planes), "step_count": int}
    view  = dict(x0, y0, cells_w, cells_h, zoom, shrink, layers, flip_y, heat_max, vehicle_radius_256, background)
"""
import os

import numpy as np

from tests.trace_util import GOLDEN

RENDER_FIXTURES = ["render_city_64_s56"]


def fixture_path(name):
    return os.path.join(GOLDEN, f"{name}.npz")


SIGNALS, RAIN, VEHICLES, HEAT, ROUTES = 1, 2, 4, 8, 16
ALL = 31


def blend(c, o):
    """c = (c * (255 - A) + o * A + 127) / 255 per colour channel: c (..., 3), o (..., 4) with A = o[..., 3]."""
    c = c.astype(np.int64)
    o = np.asarray(o).astype(np.int64)
    a = o[..., 3:4]
    return (c * (255 - a) + o[..., :3] * a + 127) // 255


def compose(state, layers, heat_max):
    """Steps 1 to 4 per map cell: (colour (H, W, 3) after cell, heat and route; vehicle colour (H, W, 3); has vehicle (H, W))."""
    H, W = state["H"], state["W"]
    sig = 1 if layers & SIGNALS else 0
    pend = state["pend"].astype(np.int64) * sig
    stop = (np.asarray(state["stop"]) == 1).astype(np.int64) * sig
    rain = (np.asarray(state["rain"]) > 0).astype(np.int64) * (1 if layers & RAIN else 0)
    pal = np.asarray(state["cell_pal"]).reshape(-1, 4)
    idx = ((state["type"].astype(np.int64) * 2 + pend) * 2 + stop) * 2 + rain
    col = pal[idx][..., :3].astype(np.int64)
    if layers & HEAT:
        i = np.minimum(255, np.asarray(state["heat"]).astype(np.uint64) * np.uint64(255) // np.uint64(heat_max)).astype(np.int64)
        col = blend(col, np.asarray(state["lut"])[i])
    if layers & ROUTES:
        routed = blend(col, np.broadcast_to(np.asarray(state["route_rgba"]), (H, W, 4)))
        col = np.where(state["route"][..., None], routed, col)
    has = np.zeros((H, W), dtype=bool)
    vcol = np.zeros((H, W, 3), dtype=np.int64)
    if layers & VEHICLES:
        top = np.asarray(state["top"])
        has = top >= 0
        flash = 1 if state["step_count"] % 2 == 0 else 0
        vp = np.asarray(state["veh_pal"]).reshape(12, 2, 4)
        vcol = vp[np.maximum(top, 0), flash][..., :3].astype(np.int64)
    return col, vcol, has


def frame_size(view):
    z, s = view.get("zoom", 1), view.get("shrink", 1)
    if s > 1:
        return -(-view["cells_w"] // s), -(-view["cells_h"] // s)
    return view["cells_w"] * z, view["cells_h"] * z


def render(state, view):
    """The frame as uint8 (h, w, 4)."""
    H, W = state["H"], state["W"]
    z, s = view.get("zoom", 1), view.get("shrink", 1)
    layers = view.get("layers", SIGNALS | RAIN | VEHICLES)
    bg = np.asarray(list(view.get("background", (0, 0, 0, 255)))[:3], dtype=np.int64)
    R = view.get("vehicle_radius_256", 169)
    ow, oh = frame_size(view)
    drawn = state.get("type") is not None
    if drawn:
        col, vcol, has = compose(state, layers, view.get("heat_max", 1))
    if s == 1:
        r, p = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
        vr = oh - 1 - r if view.get("flip_y") else r
        y, j = view["y0"] + vr // z, vr % z
        x, i = view["x0"] + p // z, p % z
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H) & drawn
        out = np.broadcast_to(bg, (oh, ow, 3)).copy()
        if drawn:
            xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
            # (at zoom 1 the vehicle fills its cell)
            disc = ((2 * i + 1 - z) ** 2 + (2 * j + 1 - z) ** 2).astype(np.int64) * 65536 <= (2 * R * z) ** 2 if z > 1 else True
            c = np.where((has[yc, xc] & disc)[..., None], vcol[yc, xc], col[yc, xc])
            out = np.where(inside[..., None], c, out)
    else:
        vy, vx = np.meshgrid(np.arange(oh * s), np.arange(ow * s), indexing="ij")   # cells of the view, padded to whole boxes
        y, x = view["y0"] + vy, view["x0"] + vx
        inside = (vx < view["cells_w"]) & (vy < view["cells_h"]) & (x >= 0) & (x < W) & (y >= 0) & (y < H) & drawn
        cells = np.broadcast_to(bg, (oh * s, ow * s, 3)).copy()
        if drawn:
            xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
            c = np.where(has[yc, xc][..., None], vcol[yc, xc], col[yc, xc])
            cells = np.where(inside[..., None], c, cells)
        sums = cells.reshape(oh, s, ow, s, 3).sum(axis=(1, 3))
        out = (sums + (s * s) // 2) // (s * s)
        if view.get("flip_y"):
            out = out[::-1]
    return np.concatenate([out, np.full((oh, ow, 1), 255, dtype=np.int64)], axis=2).astype(np.uint8)


# ---- the state of a frame from what a caller can download -----------------------------------------------------------

def mask_of(xy, H, W):
    m = np.zeros((H, W), dtype=bool)
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    m[xy[:, 1], xy[:, 0]] = True
    return m


def pending_mask(tables, pending_phase, H, W):
    """The intersection cells (g_icell CSR of the light tables) of every group whose pending phase is not None (-1)."""
    off, xy = np.asarray(tables["g_icell_off"]), np.asarray(tables["g_icell_xy"]).reshape(-1, 2)
    m = np.zeros((H, W), dtype=bool)
    for g in np.nonzero(np.asarray(pending_phase) >= 0)[0]:
        c = xy[off[g]:off[g + 1]]
        m[c[:, 1], c[:, 0]] = True
    return m


def vehicle_code(flags, service):
    """kind * 4 + status (include/trafficsim_render.h): kind 2 service, else 1 overtaking (32) or detour (64), else 0;
    status, first match: 1 collision (8), 2 malfunction (16), 3 parked (4)."""
    f = np.asarray(flags).astype(np.int64)
    status = np.where(f & 8, 1, np.where(f & 16, 2, np.where(f & 4, 3, 0)))
    kind = np.where(np.asarray(service, dtype=bool), 2, np.where(f & (32 | 64), 1, 0))
    return kind * 4 + status


class TopTracker:
    """Which vehicle is the tail of each cell's list.  A vehicle is appended to its cell's list when it is placed and every
    time it moves, so the tail of a cell is the vehicle that entered it last.  Fed the vehicle rows after every tick, this
    keeps the tick each vehicle entered its cell; where several vehicles of one cell entered in the same tick the host cannot
    tell their order, and `top` reports the cell in `tied` with the candidates' codes."""

    def __init__(self):
        self.where = {}   # spawn index -> ((x, y), tick entered)
        self.tick = 0

    def update(self, spawn_idx, x, y):
        self.tick += 1
        new = {}
        for v, vx, vy in zip(np.asarray(spawn_idx).tolist(), np.asarray(x).tolist(), np.asarray(y).tolist()):
            old = self.where.get(v)
            new[v] = old if old is not None and old[0] == (vx, vy) else ((vx, vy), self.tick)
        self.where = new

    def top(self, spawn_idx, codes, H, W):
        """(top (H, W) int, -1 = none; tied {(x, y): set of codes}) for the vehicles of the last update."""
        best = {}
        for v, code in zip(np.asarray(spawn_idx).tolist(), np.asarray(codes).tolist()):
            cell, t = self.where[v]
            b = best.get(cell)
            if b is None or t > b[0]:
                best[cell] = (t, [code])
            elif t == b[0]:
                b[1].append(code)
        top = np.full((H, W), -1, dtype=np.int64)
        tied = {}
        for (x, y), (_, cs) in best.items():
            top[y, x] = cs[0]
            if len(set(cs)) > 1:
                tied[(x, y)] = set(cs)
        return top, tied
