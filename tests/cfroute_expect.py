"""What the hop plane, the routes and the load of include/trafficsim_cfroute.h must hold, straight from the header's rule: a
heapq Dijkstra over (cell, heading) that keeps the label (cost, seed index) of every state, the hop rule on those labels,
the walk along the plane and the load of a set of walks.  Plain Python on purpose - it shares the step rule (`Rule`) with
the cost-field expectation and nothing with the engine."""
import heapq

import numpy as np

from tests.costfield_expect import Rule  # noqa: F401  (the step rule every function here takes)

INF = 0x3F3F3F3F
UNREACHABLE = 0xFFFFFFFF
DX, DY = (0, 1, 0, -1), (1, 0, -1, 0)      # N: y + 1, E: x + 1, S: y - 1, W: x - 1
HEADINGS = (-1, 0, 1, 2, 3)
STOP, NONE = 4, 7


def headings(rule) -> int:
    """States per cell the engine keeps: 4 when a turn costs something, else 1."""
    return 4 if rule.turn_on and rule.turn > 0 else 1


def _seeds(seeds, seed_cost):
    seeds = [(int(x), int(y)) for x, y in np.asarray(seeds).reshape(-1, 2)]
    return seeds, ([0] * len(seeds) if seed_cost is None else [int(c) for c in seed_cost])


def labels(rule, seeds, seed_cost=None, mode="to", soft=True, ignore_flow=False, free_flow=False, max_cost=0) -> dict:
    """{(x, y, p): (cost, seed index)} of every state that has a label; p = -1 is "no heading"."""
    modes = dict(soft=soft, ignore_flow=ignore_flow, free_flow=free_flow)
    limit = min(INF, max_cost + 1) if max_cost else INF
    seeds, costs = _seeds(seeds, seed_cost)
    best, heap = {}, []

    def offer(label, state):
        if label[0] < limit and label < best.get(state, (limit, 0)):
            best[state] = label
            heapq.heappush(heap, (label, state))

    for i, ((x, y), c) in enumerate(zip(seeds, costs)):
        for p in ((-1,) if mode == "from" else HEADINGS):
            offer((c, i), (x, y, p))
    while heap:
        label, (x, y, p) = heapq.heappop(heap)
        if best[(x, y, p)] != label:
            continue
        if mode == "from":
            for d in range(4):
                c = rule.step(x, y, d, p, **modes)
                if c is not None:
                    offer((label[0] + c, label[1]), (x + DX[d], y + DY[d], d))
        elif p != -1:
            ux, uy = x - DX[p], y - DY[p]
            if 0 <= ux < rule.W and 0 <= uy < rule.H:
                for q in HEADINGS:
                    c = rule.step(ux, uy, p, q, **modes)
                    if c is not None:
                        offer((label[0] + c, label[1]), (ux, uy, q))
    return best


def cell_label(L, x, y, mode):
    """The label of the cell: TO its "no heading" state's, FROM the smallest of its five; None without one."""
    if mode == "to":
        return L.get((x, y, -1))
    found = [L[(x, y, p)] for p in HEADINGS if (x, y, p) in L]
    return min(found) if found else None


def planes(rule, L, mode):
    """(value plane (H, W) uint32, owner plane (H, W) int32) formed from the labels."""
    value = np.full((rule.H, rule.W), UNREACHABLE, dtype=np.uint32)
    owner = np.full((rule.H, rule.W), -1, dtype=np.int32)
    for y in range(rule.H):
        for x in range(rule.W):
            l = cell_label(L, x, y, mode)
            if l is not None:
                value[y, x], owner[y, x] = l
    return value, owner


def _plus(label, c):
    return None if label is None or c is None else (label[0] + c, label[1])


def hop_plane(rule, L, seeds, seed_cost=None, mode="to", soft=True, ignore_flow=False, free_flow=False, max_cost=0) -> np.ndarray:
    """The (H, W) uint16 hop plane of the labels L, field k at bits 3k .. 3k + 2 (the header's rule)."""
    modes = dict(soft=soft, ignore_flow=ignore_flow, free_flow=free_flow)
    seeds, costs = _seeds(seeds, seed_cost)
    on_cell = {}
    for i, (xy, c) in enumerate(zip(seeds, costs)):
        on_cell.setdefault(xy, set()).add((c, i))
    nh = headings(rule)
    out = np.zeros((rule.H, rule.W), dtype=np.uint16)
    for y in range(rule.H):
        for x in range(rule.W):
            f = [NONE] * 5
            if mode == "to":
                for k, p in enumerate(HEADINGS):
                    l = L.get((x, y, p))
                    if l is None:
                        continue
                    if l in on_cell.get((x, y), ()):
                        f[k] = STOP
                        continue
                    for d in range(4):
                        if _plus(L.get((x + DX[d], y + DY[d], d)), rule.step(x, y, d, p, **modes)) == l:
                            f[k] = d
                            break
            elif nh == 1:
                # one label and one decision per cell, in all five fields
                l = cell_label(L, x, y, mode)
                v = NONE
                if l is not None:
                    if L.get((x, y, -1)) == l:
                        v = STOP
                    else:
                        for d in range(4):
                            ux, uy = x - DX[d], y - DY[d]
                            if 0 <= ux < rule.W and 0 <= uy < rule.H and \
                                    _plus(cell_label(L, ux, uy, mode), rule.step(ux, uy, d, -1, **modes)) == l:
                                v = d
                                break
                f = [v] * 5
            else:
                l = cell_label(L, x, y, mode)
                if l is not None:
                    f[0] = STOP if L.get((x, y, -1)) == l else min(d for d in range(4) if L.get((x, y, d)) == l)
                for d in range(4):
                    ld = L.get((x, y, d))
                    ux, uy = x - DX[d], y - DY[d]
                    if ld is None or not (0 <= ux < rule.W and 0 <= uy < rule.H):
                        continue
                    if _plus(L.get((ux, uy, -1)), rule.step(ux, uy, d, -1, **modes)) == ld:
                        f[1 + d] = STOP
                        continue
                    for h in range(4):
                        if _plus(L.get((ux, uy, h)), rule.step(ux, uy, d, h, **modes)) == ld:
                            f[1 + d] = h
                            break
            out[y, x] = sum(v << (3 * k) for k, v in enumerate(f))
    return out


def field_of(hops, x, y, k) -> int:
    return (int(hops[y, x]) >> (3 * k)) & 7


def walk(hops, mode, nh, start, heading=-1):
    """The direction bytes of the route of `start` in travel order, None where there is none.  TO: from the start, held with
    `heading`; FROM: to the start."""
    H, W = hops.shape
    x, y = int(start[0]), int(start[1])
    dirs, cap = [], 5 * H * W
    if mode == "to":
        p = int(heading)
        while True:
            d = field_of(hops, x, y, p + 1)
            if d == STOP:
                return dirs
            if d == NONE and not dirs:
                return None
            assert d < 4 and len(dirs) < cap, "the plane leads nowhere"
            x, y, p = x + DX[d], y + DY[d], d
            assert 0 <= x < W and 0 <= y < H
            dirs.append(d)
    assert int(heading) == -1, "a FROM route ends at its start: no heading"
    d = field_of(hops, x, y, 0)
    while True:
        if d == STOP:
            return dirs[::-1]
        if d == NONE and not dirs:
            return None
        assert d < 4 and len(dirs) < cap, "the plane leads nowhere"
        dirs.append(d)
        ux, uy = x - DX[d], y - DY[d]
        assert 0 <= ux < W and 0 <= uy < H
        d = field_of(hops, x, y, 1 + d) if nh == 4 else field_of(hops, ux, uy, 0)
        x, y = ux, uy


def route(hops, L, mode, nh, start, heading=-1):
    """(dirs, cost, owner) of a start: the walk, and the label of its state (TO) or of its cell (FROM); ([], UNREACHABLE,
    -1) where there is no route."""
    x, y = int(start[0]), int(start[1])
    dirs = walk(hops, mode, nh, start, heading)
    l = L.get((x, y, int(heading))) if mode == "to" else cell_label(L, x, y, mode)
    assert (dirs is None) == (l is None)
    return ([], UNREACHABLE, -1) if dirs is None else (dirs, l[0], l[1])


def cells_of(start, dirs, mode):
    """The cells of a route, its first one first: TO it starts at `start`, FROM it ends there."""
    x, y = int(start[0]), int(start[1])
    if mode != "to":
        x, y = x - sum(DX[d] for d in dirs), y - sum(DY[d] for d in dirs)
    out = [(x, y)]
    for d in dirs:
        x, y = x + DX[d], y + DY[d]
        out.append((x, y))
    return out


def batch(hops, L, mode, nh, starts, heads=None):
    """(off int64[n + 1], dirs uint8, cost uint32[n], owner int32[n]) of many starts: what ts_cfroute_read returns."""
    starts = np.asarray(starts).reshape(-1, 2)
    heads = [-1] * len(starts) if heads is None else [int(h) for h in heads]
    off, dirs, cost, owner = [0], [], [], []
    for s, h in zip(starts.tolist(), heads):
        d, c, o = route(hops, L, mode, nh, s, h)
        dirs += d
        off.append(len(dirs))
        cost.append(c)
        owner.append(o)
    return (np.asarray(off, dtype=np.int64), np.asarray(dirs, dtype=np.uint8), np.asarray(cost, dtype=np.uint32),
            np.asarray(owner, dtype=np.int32))


def load_planes(shape, mode, starts, off, dirs, weights=None):
    """The four (H, W) uint32 planes of a batch: the step into a cell in direction d adds the start's weight to plane d there."""
    starts = np.asarray(starts).reshape(-1, 2)
    w = np.ones(len(starts), dtype=np.uint32) if weights is None else np.asarray(weights, dtype=np.uint32)
    at = [[], [], []]
    wt = []
    for i, s in enumerate(starts.tolist()):
        d = [int(v) for v in dirs[off[i]:off[i + 1]]]
        for k, (x, y) in zip(d, cells_of(s, d, mode)[1:]):
            at[0].append(k), at[1].append(y), at[2].append(x), wt.append(w[i])
    out = np.zeros((4,) + tuple(shape), dtype=np.uint32)
    if wt:
        np.add.at(out, tuple(np.asarray(a, dtype=np.int64) for a in at), np.asarray(wt, dtype=np.uint32))
    return out
