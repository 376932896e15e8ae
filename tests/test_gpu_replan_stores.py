"""The search loop's lane-predicated stores and its packed coordinates (csrc/astar.h: astar_loop).

Every lane of a masked store stores: the idle ones to a spare - slot LDS_HEAP of the LDS heap and of its dir bytes, and the
record behind the last node of the searcher's table.  A heap entry carries its cell as y << 16 | x.  What could go wrong: a
spare that is a real record (node 0, the last node, the next searcher's first), a dummy record that a later search of the same
table reads, a spare LDS slot that the hand-over between the LDS form and the HBM-spill form of the loop counts as a heap slot,
x and y swapped or clipped on a map that is not square.  Every path is compared with the CPU oracle's."""
import ctypes
import functools

import numpy as np
import pytest

from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import _lib
from trafficsimulation_amd import citygen
from trafficsimulation_amd.world import build_engine, load_trace
from tests.engine_util import small_engine
from tests.trace_util import setup_from_trace, trace_path

pytestmark = pytest.mark.gpu

BUILDS = {"shipped": _lib.new_engine, "smallheap": small_engine}
WARM_TICKS = 6          # vehicles on the road and lights red before the queries: strict and soft searches differ


@functools.lru_cache(maxsize=None)
def trace(name):
    return load_trace(trace_path(name))


def node_order(tr):
    """(x, y) of every search node in the engine's numbering (ts_create: roads, cells with flow bits and the cells those bits
    point at, in the 8 x 8-tiled order of the snapshot)."""
    W, H = int(tr["width"]), int(tr["height"])
    a = np.asarray(tr["allowed_dirs_map"]).astype(np.int32) & 15
    node = (np.asarray(tr["is_road_map"]) == 1) | (a != 0)
    node[1:, :] |= (a[:-1, :] & 1) != 0       # N: y + 1
    node[:, 1:] |= (a[:, :-1] & 2) != 0       # E: x + 1
    node[:-1, :] |= (a[1:, :] & 4) != 0       # S: y - 1
    node[:, :-1] |= (a[:, 1:] & 8) != 0       # W: x - 1
    ys, xs = np.nonzero(node)
    key = ((ys >> 3) * ((W + 7) // 8) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    o = np.argsort(key, kind="stable")
    return xs[o], ys[o], node


def with_neighbours(x, y, node):
    H, W = node.shape
    out = [(int(x), int(y))]
    for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        if 0 <= x + dx < W and 0 <= y + dy < H and node[y + dy, x + dx]:
            out.append((int(x + dx), int(y + dy)))
    return out


def pair_queries(cells_a, cells_b):
    """Every ordered pair of distinct cells, strict and soft."""
    cells = list(dict.fromkeys(cells_a + cells_b))
    return np.array([(sx, sy, gx, gy, soft, 0, 0x7FFFFFFF) for soft in (0, 1) for (sx, sy) in cells for (gx, gy) in cells
                     if (sx, sy) != (gx, gy)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def oracle_answers(name, key):
    """The oracle's paths for the queries of `key` on the maps of trace `name` after WARM_TICKS ticks (computed once)."""
    from oracle import pyoracle
    q = QUERIES[key](trace(name))
    c = setup_from_trace(pyoracle.load(), trace(name), explicit_paths=False)
    try:
        c.step(WARM_TICKS)
        want = [c.astar(*(int(v) for v in a[:4]), bool(a[4]), bool(a[5]), int(a[6])) for a in q]
        maps = [c.map(m).copy() for m in (capi.MAP_OCCUPANCY, capi.MAP_STOP)]
    finally:
        c.close()
    return q, want, maps


def end_node_queries(tr):
    xs, ys, node = node_order(tr)
    return pair_queries(with_neighbours(xs[0], ys[0], node), with_neighbours(xs[-1], ys[-1], node))


def last_line_queries(tr):
    """Starts and goals on column W - 1 and on row H - 1, and on the first column and row across the map from them."""
    W, H = int(tr["width"]), int(tr["height"])
    xs, ys, node = node_order(tr)
    pick = lambda m: [(int(x), int(y)) for x, y in zip(xs[m][:3], ys[m][:3])]
    col, row = pick(xs == W - 1), pick(ys == H - 1)
    assert col and row, "the fixture has no search node on its last column / row"
    return pair_queries(col + row, pick(xs == 0)[:2] + pick(ys == 0)[:2])


QUERIES = {"end_nodes": end_node_queries, "last_lines": last_line_queries}


def engine_at_queries(build, name, maps):
    h = setup_from_trace(BUILDS[build](), trace(name), explicit_paths=False)
    try:
        h.step(WARM_TICKS)
        assert np.array_equal(h.map(capi.MAP_OCCUPANCY), maps[0]) and np.array_equal(h.map(capi.MAP_STOP), maps[1])
    except BaseException:
        h.close()
        raise
    return h


def assert_batch(h, q, want, ctx):
    off, xy = h.astar_batch(q)
    assert len(off) == len(q) + 1
    for i, a in enumerate(q):
        assert np.array_equal(xy[off[i]:off[i + 1]], want[i]), f"{ctx}: query {i} {a.tolist()}"


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", ["full_64_s1", "ragged_100x75_s33"])
def test_spare_table_record(monkeypatch, name, build):
    """Searches that start and end on node 0, on the last node (the record in front of the spare) and on their neighbours: on
    every searcher slot a batch gets, then all of them one after the other on a single slot's table."""
    q, want, maps = oracle_answers(name, "end_nodes")
    found = [sum(len(w) > 0 for w, a in zip(want, q) if a[4] == soft) for soft in (0, 1)]
    print(f"{name}: {len(q)} queries, paths found on the oracle: strict {found[0]}, soft {found[1]}")
    # (the condition on the input: some searches of either kind find their way; the others flood everything they can reach
    # before they answer [] - and read every record they stored)
    assert len(q) >= 24 and found[0] >= 4 and found[1] >= 4, found
    h = engine_at_queries(build, name, maps)
    try:
        assert_batch(h, q, want, f"{name} {build}")
    finally:
        h.close()
    monkeypatch.setenv("TS_ASTAR_SLOTS", "1")
    h = engine_at_queries(build, name, maps)
    try:
        assert_batch(h, q, want, f"{name} {build} one slot")
        assert h.debug_batch_info()["last_waves"] == 1
        assert_batch(h, q[::-1], want[::-1], f"{name} {build} one slot, second batch")
    finally:
        h.close()


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", ["rect_64x112_s19", "rect_96x64_s18"])
def test_packed_coordinates(name, build):
    """A map taller than wide and one wider than tall; queries from and to the last column and the last row."""
    tr = trace(name)
    W, H = int(tr["width"]), int(tr["height"])
    assert (W, H) in ((64, 112), (96, 64))
    q, want, maps = oracle_answers(name, "last_lines")
    on_col = sum(len(w) > 0 for w, a in zip(want, q) if W - 1 in (a[0], a[2]))
    on_row = sum(len(w) > 0 for w, a in zip(want, q) if H - 1 in (a[1], a[3]))
    print(f"{name}: {len(q)} queries; paths found from / to column {W - 1}: {on_col}, row {H - 1}: {on_row}")
    assert on_col >= 4 and on_row >= 4, (on_col, on_row)             # (the condition on the input)
    h = engine_at_queries(build, name, maps)
    try:
        assert_batch(h, q, want, f"{name} {build}")
        for i in range(0, len(q), 7):                                 # (ts_astar's own kernel, a few of them)
            a = q[i]
            one = h.astar(*(int(v) for v in a[:4]), bool(a[4]), bool(a[5]), int(a[6]))
            assert np.array_equal(one, want[i]), f"{name} {build}: query {i} {a.tolist()} (ts_astar)"
    finally:
        h.close()


# ---- the spare LDS slot where the two forms of the loop hand over ---------------------------------------------------------------
# The small-heap build keeps 128 heap slots in LDS (csrc/Makefile).  The LDS form hands over when a turn starts with more than
# LDS_HEAP - 4 entries, the spill form hands back below LDS_HEAP - 96.  A search whose heap peaks within a few entries of
# LDS_HEAP fills the slots next to the spare one; one that peaks far above it crosses the band upwards and comes back down.
SMALL_LDS_HEAP = 128
# a dense 128 x 128 city (blocks of 3 .. 6 cells: heaps of some hundred entries), 200 vehicles, six ticks old
BOUNDARY_CITY = dict(wall_thickness=2, min_block_spacing=3, max_block_spacing=6)
BOUNDARY_SEED, BOUNDARY_VEHICLES, BOUNDARY_TICKS, POOL_SEED, POOL = 3, 200, 6, 1, 1500
# Query i of the seeded pool (soft when i is odd) and the deepest heap of its search, as the CPU oracle built with -DTSO_STATS
# reports it (the largest heap_size + 1 at a push): the first 24 of the pool that peak within +-8 of LDS_HEAP and the first 24
# that peak above LDS_HEAP + 96.  Measured on the CPU alone; a change to citygen or to the pool has to measure again.
NEAR = [(29, 132), (93, 135), (147, 121), (161, 131), (177, 125), (347, 122), (355, 135), (375, 123), (383, 132), (403, 135),
        (503, 128), (509, 127), (563, 130), (739, 129), (923, 135), (1005, 133), (1039, 129), (1099, 128), (1103, 121), (1135, 132),
        (1143, 132), (1183, 125), (1297, 124), (1327, 125)]
ABOVE = [(33, 239), (35, 312), (43, 243), (67, 241), (69, 268), (71, 245), (83, 312), (85, 294), (89, 245), (103, 233), (109, 236),
         (111, 238), (115, 283), (117, 246), (125, 236), (129, 307), (141, 232), (143, 261), (165, 261), (175, 237), (185, 234),
         (189, 250), (195, 254), (199, 230)]
assert sum(abs(p - SMALL_LDS_HEAP) <= 8 for _, p in NEAR) >= 20 and sum(p > SMALL_LDS_HEAP + 96 for _, p in ABOVE) >= 20


def boundary_engine(api):
    tb = citygen.generate(128, 128, seed=BOUNDARY_SEED, **BOUNDARY_CITY)
    s, g, off, dirs = citygen.make_routes(tb, BOUNDARY_VEHICLES, seed=BOUNDARY_SEED + 1, min_len=10, max_len=70)
    build_engine(api, tb, defaults={"RAIN_ENABLED": False}, global_seed=11, sched_seed=12)
    api.add_vehicles_dirs(s, g, np.full(len(s), capi.POP["through"], np.int32), off, dirs)
    api.step(BOUNDARY_TICKS)
    ys, xs = np.nonzero(np.asarray(tb["is_road_map"]) == 1)
    ab = np.random.RandomState(POOL_SEED).randint(len(xs), size=(POOL, 2))
    queries = {i: (int(xs[ab[i, 0]]), int(ys[ab[i, 0]]), int(xs[ab[i, 1]]), int(ys[ab[i, 1]]), bool(i % 2), False, 0x7FFFFFFF)
               for i, _ in NEAR + ABOVE}
    return api, queries


def test_spare_lds_slot_at_the_hand_over():
    """Road-to-road queries one at a time on the small-heap build: every path is the oracle's, and the deepest heap of every
    search (ts_debug_read, word 4; the word is cleared by loading a checkpoint before each query) is the one the CPU measured."""
    from oracle import pyoracle
    c, queries = boundary_engine(pyoracle.load())
    try:
        want = {i: c.astar(*a) for i, a in queries.items()}
        maps = [c.map(m).copy() for m in (capi.MAP_OCCUPANCY, capi.MAP_STOP)]
    finally:
        c.close()
    assert all(len(w) > 0 for w in want.values())
    h, _ = boundary_engine(small_engine())
    try:
        assert np.array_equal(h.map(capi.MAP_OCCUPANCY), maps[0]) and np.array_equal(h.map(capi.MAP_STOP), maps[1])
        blob = h.checkpoint_save()
        dbg = (ctypes.c_int32 * 8)()
        peaks = {}
        for i, a in queries.items():
            h.checkpoint_load(blob)
            got = h.astar(*a)
            assert h.lib.ts_debug_read(h.h, dbg) == 0
            peaks[i] = int(dbg[4])
            assert np.array_equal(got, want[i]), f"query {i} {a}: path differs (deepest heap {peaks[i]})"
        print("deepest heaps, near:", [peaks[i] for i, _ in NEAR], "above:", [peaks[i] for i, _ in ABOVE])
        # the coverage floor: the hand-over band is crossed both ways, and often
        assert sum(abs(peaks[i] - SMALL_LDS_HEAP) <= 8 for i, _ in NEAR) >= 20
        assert sum(peaks[i] > SMALL_LDS_HEAP + 96 for i, _ in ABOVE) >= 20
        assert [peaks[i] for i, _ in NEAR + ABOVE] == [p for _, p in NEAR + ABOVE]
        assert ((int(dbg[6]) & 0xFFFFFFFF) | (int(dbg[7]) << 32)) > 0      # (the last search spent expansions in the spill form)
    finally:
        h.close()
