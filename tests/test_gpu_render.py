"""The device renderer (include/trafficsim_render.h) on the GPU: frames against the reference's own portrayal colours
(tests/golden/render_*.npz), against the numpy statement of the pixel rule (tests/render_expect.py) over many views, the heat
and route layers, the device-side frame buffer, a run that rendering does not change, and every refusal."""

import numpy as np
import pytest

from tests import procs
from tests.engine_util import assert_same_state, full_state, refused
from tests.render_expect import RENDER_FIXTURES, fixture_path
from tests.render_scene import BG, Scene, to_view
from tests.trace_util import replay_and_compare, setup_from_trace, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import render as rn
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace

pytestmark = pytest.mark.gpu

WORLDS = {"render": (fixture_path(RENDER_FIXTURES[0]), None), "ragged": (trace_path("ragged_100x75_s33"), 40)}


@pytest.fixture(scope="module", params=list(WORLDS))
def scene(request):
    path, ticks = WORLDS[request.param]
    if ticks is None:                      # the render fixture: up to its first flash-parity pair of frame ticks
        ft = np.asarray(load_trace(path)["frame_ticks"])
        ticks = int(ft[np.nonzero(np.diff(ft) == 1)[0][0]]) + 1
    s = Scene(path, ticks)
    rows = s.rows()
    plen = rows[:, capi.V_FIELDS.index("path_len")]
    s.set_routes([int(v) for v in rows[np.argsort(-plen)[:6], 0]])
    yield s
    s.api.close()


def views_of(W, H, vx, vy):
    """The views of the issue for a W x H map; (vx, vy) is a cell that holds a vehicle."""
    full = dict(x0=0, y0=0, cells_w=W, cells_h=H)
    xo = (W - 7) | 1
    out = [dict(full), dict(full, flip_y=True),
           dict(x0=xo, y0=H - 5, cells_w=11, cells_h=9, zoom=3),                # over the right and top edges, 33 pixels wide
           dict(x0=xo, y0=H - 5, cells_w=11, cells_h=9, zoom=3, flip_y=True),
           dict(x0=-3, y0=-5, cells_w=13, cells_h=11, zoom=8),                  # over the left and bottom edges
           dict(x0=vx - 2, y0=vy - 1, cells_w=5, cells_h=3, zoom=16, vehicle_radius_256=128),
           dict(x0=vx - 2, y0=vy - 1, cells_w=5, cells_h=3, zoom=16, vehicle_radius_256=255),
           dict(x0=vx - 1, y0=vy - 1, cells_w=3, cells_h=3, zoom=5),            # an odd zoom at the default radius
           dict(full, shrink=2), dict(full, shrink=3), dict(full, shrink=7), dict(full, shrink=7, flip_y=True),
           dict(x0=-5, y0=3, cells_w=W + 9, cells_h=H, shrink=3),
           dict(full, shrink=64),
           dict(x0=vx, y0=vy, cells_w=1, cells_h=1), dict(x0=vx, y0=vy, cells_w=1, cells_h=1, zoom=64),
           dict(x0=W + 5, y0=-40, cells_w=9, cells_h=7), dict(x0=W + 5, y0=-40, cells_w=9, cells_h=7, shrink=2)]
    return out


def test_engine_equals_the_pixel_rule_on_every_view(scene):
    rows = scene.rows()
    assert len(rows) > 0
    vx, vy = int(rows[0, 1]), int(rows[0, 2])
    st = scene.state("present")
    assert (st["top"] >= 0).sum() > 10 and st["route"].any()
    for view in views_of(scene.W, scene.H, vx, vy):
        for layers in (None, capi.RL_ALL):
            got = scene.check(dict(view, layers=layers, heat_plane="present", heat_max=5), st)
        if view["x0"] > scene.W:
            assert (got[..., :3] == np.asarray(BG[:3])).all() and (got[..., 3] == 255).all()


@pytest.mark.parametrize("layers", [0, capi.RL_SIGNALS, capi.RL_RAIN, capi.RL_VEHICLES, capi.RL_HEAT, capi.RL_ROUTES, capi.RL_ALL])
def test_each_layer_alone_and_all_together(scene, layers):
    st = scene.state("present")
    frames = [scene.check(dict(x0=0, y0=0, cells_w=scene.W, cells_h=scene.H, layers=layers, heat_plane="present", heat_max=9, **kw), st)
              for kw in (dict(), dict(zoom=2), dict(shrink=2))]
    base = scene.api.render(rn.make_view(cells_w=scene.W, cells_h=scene.H, layers=0, background=BG))
    assert (frames[0][..., 3] == 255).all()
    if layers in (capi.RL_VEHICLES, capi.RL_HEAT, capi.RL_ROUTES, capi.RL_ALL):
        assert not np.array_equal(frames[0], base), "the layer draws nothing"


def test_flash_parity_changes_stranded_vehicles_only(scene):
    """Two consecutive ticks: both are frames of the rule (the flash bit is step_count % 2 == 0)."""
    full = dict(x0=0, y0=0, cells_w=scene.W, cells_h=scene.H, layers=capi.RL_VEHICLES)
    scene.check(full)
    scene.step()
    scene.check(full)
    scene.set_routes(scene.routes)


@pytest.mark.parametrize("plane,heat_max", [("present", 40), ("waiting", 3), ("flow", 12), ("flow", 1), ("speed", 0xFFFFFFFF)])
def test_heat(scene, plane, heat_max):
    st = scene.state(plane)
    if plane != "waiting":                                  # (heat_max = 1: values above 1 exercise the clamp at 255)
        assert st["heat"].max() > (1 if heat_max == 1 else 0), "nothing observed on this plane"
    for kw in (dict(), dict(zoom=3, cells_w=21, x0=5), dict(shrink=3)):
        scene.check(dict(dict(x0=0, y0=0, cells_w=scene.W, cells_h=scene.H, layers=capi.RL_HEAT, heat_plane=plane, heat_max=heat_max), **kw), st)


def test_routes_are_the_downloaded_paths(scene):
    api = scene.api
    rows = scene.rows()
    plen = rows[:, capi.V_FIELDS.index("path_len")]
    live = set(int(v) for v in rows[:, 0])
    gone = [v for v in range(api.num_spawned()) if v not in live]
    long_ones, empty = rows[plen > 64, 0], rows[plen == 0, 0]
    old = list(scene.routes)
    colour = (1, 2, 3, 255)                                # weight 255: a route cell is exactly this colour
    full = rn.make_view(cells_w=scene.W, cells_h=scene.H, layers=capi.RL_ROUTES, background=BG)
    try:
        cases = {"several": [int(v) for v in rows[:5, 0]]}
        if len(long_ones):
            cases["longer than 64 steps"] = [int(long_ones[0])]
        if len(empty):
            cases["empty path"] = [int(empty[0])]
        if gone:
            cases["a removed vehicle among live ones"] = [int(rows[0, 0]), gone[0], int(rows[-1, 0])]
            cases["only a removed vehicle"] = [gone[-1]]
        cases["the same vehicle twice"] = [int(rows[0, 0])] * 2
        cases["cleared"] = []
        for what, ids in cases.items():
            api.render_set_routes(ids, colour)
            assert api.render_info()["n_routes"] == len(ids)
            got = (api.render(full)[..., :3] == np.asarray(colour[:3])).all(axis=2)
            want = scene.path_mask(ids)
            assert np.array_equal(got, want), f"{what}: {np.argwhere(got != want)[:4].tolist()}"
            if what in ("several", "longer than 64 steps"):
                assert want.any()
            if what in ("empty path", "only a removed vehicle", "cleared"):
                assert not want.any()
        assert len(long_ones) or scene.W != 100, "the ragged world is expected to hold a path longer than 64 steps"
        refused(capi.TS_E_INVALID, lambda: api.render_set_routes([api.num_spawned()], colour))
    finally:
        scene.set_routes(old)


# ---- the reference's own frames ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDER_FIXTURES)
def test_reference_frames(name):
    """Replay the fixture; at every frame tick the full-map zoom-1 frame is what the reference's get_portrayal() colours
    give: the vehicle's colour where a vehicle is drawn last in the cell, the cell's colour elsewhere."""
    tr = load_trace(fixture_path(name))
    H, W = int(tr["height"]), int(tr["width"])
    api = new_engine()
    setup_from_trace(api, tr)
    api.render_set_cells(rn.type_plane(tr["cell_type_map"], tr["cell_base_type_map"]), rn.cell_palette())
    api.render_set_vehicle_palette(rn.vehicle_palette())
    view = rn.make_view(cells_w=W, cells_h=H)
    done = 0
    for k, t in enumerate(np.asarray(tr["frame_ticks"]).tolist()):
        replay_and_compare_from(api, tr, done, t + 1)
        done = t + 1
        got = api.render(view)
        veh = tr["vehicle_rgba"][k]
        want = np.where(veh[..., 3:4] > 0, veh[..., :3], tr["cells_rgb"][k])
        ok = (got[..., :3] == want).all(axis=2) | tr["ambiguous"][k]
        assert ok.all(), f"tick {t}: {np.argwhere(~ok)[:5].tolist()} differ, e.g. got {got[tuple(np.argwhere(~ok)[0])]}"
        cells_only = api.render(rn.make_view(cells_w=W, cells_h=H, layers=capi.RL_SIGNALS | capi.RL_RAIN))
        assert np.array_equal(cells_only[..., :3], tr["cells_rgb"][k]), f"tick {t}: cell colours"
    api.close()


def replay_and_compare_from(api, tr, t0, t1):
    """trace_util.replay_and_compare over ticks [t0, t1): the slice of the trace as a trace of its own."""
    if t1 <= t0:
        return
    sub = dict(tr)
    for k in ("occ_t", "stop_t", "stuck_t", "rain_t", "grp_rows", "nsched_t", "rng_rows", "cnt_rows", "blk_rows"):
        if k in sub:
            sub[k] = tr[k][t0:]
    off = np.asarray(tr["veh_off"])
    sub["veh_rows"], sub["veh_off"] = tr["veh_rows"][off[t0]:], off[t0:] - off[t0]
    sub.pop("raised_at_tick", None)
    replay_and_compare(api, sub, ticks=t1 - t0)


# ---- the frame buffer on the device ----------------------------------------------------------------------------------------
DEVICE_SCRIPT = r'''
import numpy as np
from trafficsimulation_amd import _capi as capi, render as rn
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace
from tests.trace_util import setup_from_trace, trace_path
tr = load_trace(trace_path("ragged_100x75_s33"))
api = new_engine()
setup_from_trace(api, tr)
api.render_set_cells(np.asarray(tr["cell_type_map"]).astype(np.uint8), rn.cell_palette())
api.render_set_vehicle_palette(rn.vehicle_palette())
api.step(10)
small = rn.make_view(cells_w=100, cells_h=75)
a = api.render_device(small)
assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == (75, 100, 4)
assert np.array_equal(a.cpu().numpy(), api.render(small))
p0 = a.data_ptr()
api.step(1)
b = api.render_device(small)
assert b.data_ptr() == p0, "the buffer moved between two frames of one size"
assert np.array_equal(b.cpu().numpy(), api.render(small))
bytes0 = api.render_info()["device_bytes"]
big = rn.make_view(cells_w=100, cells_h=75, zoom=4)
c = api.render_device(big)
assert tuple(c.shape) == (300, 400, 4) and api.render_info()["device_bytes"] >= bytes0 + (16 - 1) * 100 * 75 * 4
assert np.array_equal(c.cpu().numpy(), api.render(big))
d = api.render_device(small)                      # (a smaller frame afterwards reuses the grown buffer)
assert d.data_ptr() == c.data_ptr() and np.array_equal(d.cpu().numpy(), api.render(small))
info = api.render_info()
assert info["frames"] == 8 and (info["last_w"], info["last_h"]) == (100, 75)
api.close()
'''


def test_device_output():
    """render_device(): a torch tensor over the engine's own frame buffer.  In a process of its own that imports torch before
    it loads the engine, like the observe_device test."""
    procs.run_python(DEVICE_SCRIPT, torch_first=True, timeout=300)


# ---- rendering changes nothing --------------------------------------------------------------------------------------------
def test_purity():
    """One run renders every tick with all layers, the other never configures the renderer: identical state, identical
    checkpoint bytes.  (Observation, which the heat layer needs, is not simulation state either: both runs observe.)"""
    path = fixture_path(RENDER_FIXTURES[0])
    a, b = Scene(path, 0), Scene(path, 0, configure=False)
    b.api.observe_start()
    assert a.api.render_info()["n_types"] == len(rn.RENDER_TYPE_NAMES) and b.api.render_info() == {
        "n_types": 0, "has_vehicle_palette": False, "has_heat_lut": False, "n_routes": 0, "last_w": 0, "last_h": 0, "frames": 0,
        "device_bytes": 0}
    view = rn.make_view(cells_w=a.W, cells_h=a.H, layers=capi.RL_ALL, heat_plane="flow", heat_max=4, zoom=2)
    for t in range(60):
        a.api.step(1)
        b.api.step(1)
        rows = a.api.vehicles()
        a.api.render_set_routes(rows[:8, 0])
        a.api.render(view)
    assert_same_state(full_state(a.api), full_state(b.api), "rendered every tick")
    assert a.api.render_info()["frames"] == 60
    a.api.close()
    b.api.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_frame_buffer_alone():
    s = Scene(trace_path("ragged_100x75_s33"), 5, configure=False)
    api, W, H = s.api, s.W, s.H
    ok = dict(x0=0, y0=0, cells_w=W, cells_h=H, layers=0, background=BG)
    before_cells = api.render(to_view(ok))
    assert (before_cells[..., :3] == np.asarray(BG[:3])).all(), "before ts_render_set_cells every cell is background"
    api.render_set_cells(s.type, s.cell_pal)
    frame = api.render(to_view(ok))
    frames0 = api.render_info()["frames"]

    def refused_views(code, *views):
        refused(code, *(lambda view=view: api.render(to_view(dict(ok, **view))) for view in views))

    refused_views(capi.TS_E_INVALID, dict(zoom=0), dict(zoom=65), dict(shrink=0), dict(shrink=65), dict(zoom=2, shrink=2), dict(cells_w=0), dict(cells_h=-1),
                  dict(layers=32), dict(vehicle_radius_256=-1), dict(layers=capi.RL_HEAT, heat_plane=8), dict(layers=capi.RL_HEAT, heat_plane=-1),
                  dict(layers=capi.RL_HEAT, heat_plane=0, heat_max=0))
    refused_views(capi.TS_E_CAPACITY, dict(cells_w=8193))
    refused_views(capi.TS_E_CAPACITY, dict(cells_h=129, zoom=64))
    refused_views(capi.TS_E_CAPACITY, dict(cells_w=8192 * 64 + 1, shrink=64))
    refused_views(capi.TS_E_STATE, dict(layers=capi.RL_VEHICLES))                       # no vehicle palette
    refused_views(capi.TS_E_STATE, dict(layers=capi.RL_HEAT, heat_plane=0, heat_max=1))  # no LUT
    api.render_set_heat_lut(s.lut)
    refused_views(capi.TS_E_STATE, dict(layers=capi.RL_HEAT, heat_plane=0, heat_max=1))  # not observed
    api.observe_start(["present", "enter_n"])
    refused_views(capi.TS_E_STATE, dict(layers=capi.RL_HEAT, heat_plane="waiting", heat_max=1))
    refused_views(capi.TS_E_STATE, dict(layers=capi.RL_HEAT, heat_plane="flow", heat_max=1))   # flow needs all four ENTER planes
    refused(capi.TS_E_INVALID, lambda: api.render_set_routes([-1]))
    refused(capi.TS_E_INVALID, lambda: api.render_set_routes([api.num_spawned()]))
    refused(capi.TS_E_INVALID, lambda: api.render_set_routes(list(range(1)) * 4097))
    refused(capi.TS_E_INVALID, lambda: api.render_set_cells(np.full((H, W), len(rn.RENDER_TYPE_NAMES), dtype=np.uint8), s.cell_pal))
    # null pointers, straight at the C entries
    lib, h = api.lib, api.h
    v = to_view(ok)
    import ctypes as C
    assert api._ext("render")(h, None, frame.ctypes.data) == capi.TS_E_INVALID
    assert api._ext("render")(h, C.byref(v), None) == capi.TS_E_INVALID
    assert api._ext("render_device")(h, C.byref(v), None) == capi.TS_E_INVALID
    assert api._ext("render_set_cells")(h, None, len(s.cell_pal), s.cell_pal.ctypes.data) == capi.TS_E_INVALID
    assert api._ext("render_set_vehicle_palette")(h, None) == capi.TS_E_INVALID
    assert api._ext("render_set_heat_lut")(h, None) == capi.TS_E_INVALID
    assert api._ext("render_info")(h, None) == capi.TS_E_INVALID
    info = api.render_info()
    assert info["frames"] == frames0 and (info["last_w"], info["last_h"]) == (W, H)
    # the frame buffer still holds the last good frame: a device-side copy of it, read through a second good frame's pointer
    # being the same buffer is what test_device_output shows; here the bytes, through the one entry that hands them out
    procs.run_python(REFUSAL_SCRIPT, torch_first=True, timeout=300)
    api.close()


REFUSAL_SCRIPT = r'''
import numpy as np
from trafficsimulation_amd import _capi as capi, render as rn
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace
from tests.trace_util import setup_from_trace, trace_path
tr = load_trace(trace_path("ragged_100x75_s33"))
api = new_engine()
setup_from_trace(api, tr)
api.render_set_cells(np.asarray(tr["cell_type_map"]).astype(np.uint8), rn.cell_palette())
api.step(3)
good = rn.make_view(cells_w=100, cells_h=75, layers=capi.RL_SIGNALS)
t = api.render_device(good)
before = t.cpu().numpy().copy()
for bad in (rn.make_view(cells_w=100, cells_h=75, zoom=65), rn.make_view(cells_w=9000, cells_h=75),
            rn.make_view(cells_w=100, cells_h=75, layers=capi.RL_VEHICLES),
            rn.make_view(cells_w=100, cells_h=75, layers=capi.RL_HEAT, heat_plane="present", heat_max=1)):
    try:
        api.render_device(bad)
    except capi.EngineError:
        pass
    else:
        raise SystemExit("a bad view was rendered")
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), before), "a refused call wrote to the frame buffer"
assert api.render_info()["frames"] == 1
api.close()
'''
