"""Jam detection on the device (include/trafficsim_jams.h) against tests/jams_expect.py: every output on four fixtures in both
link modes, two thresholds and the four tile sides; the tie to the WAITING plane of the observation; every mask from a host
pointer and from a device tensor; refusals and state; the snapshot and its purity; two sharded ranks."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import jams_expect as je
from tests import procs
from tests.engine_util import assert_same_deep_state, deep_state, engine_for, refused
from tests.lights_ext_expect import Stepper
from tests.test_jams_expect import FIXTURES, all_masks
from tests.trace_util import setup_from_trace, trace_path
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import jams as jm
from trafficsimulation_amd._lib import new_engine
from trafficsimulation_amd.world import load_trace

pytestmark = pytest.mark.gpu

TILES = (0, 8, 16, 32)
DEFAULT_TILE = 0           # no tile stage: what profiles/jams_probe.py found ahead (README.md)
LINKS = {"grid": je.GRID, "flow": je.FLOW}


def read_all(j):
    """Every output of the result held, and the totals of its info."""
    i = j.info()
    return {"records": j.records(), "vehicles": j.vehicles(), "label": j.plane("label"), "count": j.plane("count"), "groups": j.groups(),
            "info": {k: i[k] for k in ("n_jams", "standing_cells", "standing_vehicles", "largest_cells")}}


def same(got, want, ctx):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{ctx}: {k}"
        else:
            assert g == w, f"{ctx}: {k}: {g} != {w}"


def as_bytes(r):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def replayed(name, block):
    """(engine, trace) of a fixture after block + 1 steps: its rows are block `block` of the trace's.  Kept for the module:
    a compute changes nothing."""
    api, tr = engine_for(name)
    if "rl_action" in tr:
        Stepper(api, lambda t: (api.lights_observe(), api.lights_act(tr["rl_action"][t]))).step(block + 1)
    else:
        api.step(block + 1)
    assert np.array_equal(api.vehicles(), je.fixture_rows(tr, block)), f"{name}: the engine is not at block {block}"
    return api, tr


def expectation(api, tr, link, min_ticks):
    """... formed from the rows the engine downloads."""
    rows = api.vehicles()
    return je.expect(je.count_plane(rows, api.H, api.W, min_ticks), link, tr["allowed_dirs_map"], tr["intersection_map"], rows,
                     api.num_spawned(), min_ticks, tr=tr)


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_ticks", [1, 3])
@pytest.mark.parametrize("link", ["grid", "flow"])
@pytest.mark.parametrize("name,block", FIXTURES)
def test_fixture_expectation(name, block, link, min_ticks, monkeypatch):
    api, tr = replayed(name, block)
    want = expectation(api, tr, LINKS[link], min_ticks)
    assert want["info"]["n_jams"] > 0 and want["groups"].any()
    seen = []
    for tile in TILES:
        monkeypatch.setenv("TS_DEBUG_JAMS_TILE", str(tile))
        info = api.jams.compute(min_ticks, link)
        assert (info["held"], info["tile"], info["min_ticks"], info["link"], info["source"]) == (True, tile, min_ticks, LINKS[link], 0)
        assert (info["n_spawned"], info["tick"], info["width"], info["height"]) == (api.num_spawned(), block + 1, api.W, api.H)
        got = read_all(api.jams)
        same(got, want, f"{name} {link} min_ticks {min_ticks} tile {tile}")
        seen.append(as_bytes(got))
    assert all(s == seen[0] for s in seen), "the bytes depend on the tile side"
    monkeypatch.setenv("TS_DEBUG_JAMS_TILE", "24")        # (any other value: the default)
    assert api.jams.compute(min_ticks, link)["tile"] == DEFAULT_TILE


# ---- 2. the tie to observation ----------------------------------------------------------------------------------------------------
def test_the_count_plane_is_the_growth_of_the_waiting_plane():
    api, tr = engine_for("carfollow_96_s2")
    api.step(42)
    api.observe_start()
    w0, g0 = api.observe_plane("waiting").astype(np.int64), api.observe_groups()
    api.step(1)
    grown, g1 = api.observe_plane("waiting").astype(np.int64) - w0, api.observe_groups()
    api.jams.compute(1, "grid")
    count = api.jams.plane("count").astype(np.int64)
    assert np.array_equal(count, grown) and count.sum() > 100
    ns = capi.OG_FIELDS.index("ns_waiting")
    for g in range(len(g1)):
        xy = je.group_lists(tr, g)[0]
        assert int(count[xy[:, 1], xy[:, 0]].sum()) == int(g1[g, ns] - g0[g, ns]), f"group {g}"
    assert (g1[:, ns] - g0[:, ns]).sum() > 0
    api.close()


# ---- 3. masks ---------------------------------------------------------------------------------------------------------------------
def synthetic_engine(shape):
    """An engine on a 40 x 40 map without vehicles: seeded random flow bits and intersection cells."""
    rng = np.random.RandomState(40)
    allowed = rng.randint(0, 16, shape).astype(np.int8)
    inter = (rng.rand(*shape) < 0.2).astype(np.int8)
    z = np.zeros(shape, dtype=np.int8)
    api = new_engine()
    api.create(allowed, z + 1, z, inter, api.default_params())
    return api, {"allowed_dirs_map": allowed, "intersection_map": inter}


def mask_engine(shape):
    if shape == (40, 40):
        return synthetic_engine(shape)
    api, tr = engine_for("ragged_100x75_s33")
    return api, tr


@pytest.mark.parametrize("shape", [(40, 40), (75, 100)])
def test_masks_from_a_host_pointer(shape, monkeypatch):
    api, tr = mask_engine(shape)
    for name, m in all_masks(shape).items():
        for link in LINKS:
            e = je.expect(m.astype(np.uint32), LINKS[link], tr["allowed_dirs_map"], tr["intersection_map"], None, api.num_spawned())
            seen = []
            for tile in TILES:
                monkeypatch.setenv("TS_DEBUG_JAMS_TILE", str(tile))
                info = api.jams.compute(7, link, mask=m)
                assert (info["source"], info["mask_on_device"], info["tile"]) == (1, False, tile)
                got = read_all(api.jams)
                got.pop("groups")
                same(got, e, f"{shape} {name} {link} tile {tile}")
                seen.append(as_bytes(got))
            assert all(s == seen[0] for s in seen), f"{name} {link}: the bytes depend on the tile side"
    api.close()


MASK_SCRIPT = r'''
import numpy as np
from tests import jams_expect as je
from tests.test_jams_expect import all_masks
from tests.test_gpu_jams import LINKS, TILES, mask_engine, read_all, same
for shape in ((40, 40), (75, 100)):
    api, tr = mask_engine(shape)
    for name, m in all_masks(shape).items():
        t = torch.as_tensor(m).cuda()
        for link in LINKS:
            e = je.expect(m.astype(np.uint32), LINKS[link], tr["allowed_dirs_map"], tr["intersection_map"], None, api.num_spawned())
            for tile in TILES:
                os.environ["TS_DEBUG_JAMS_TILE"] = str(tile)
                info = api.jams.compute(1, link, mask=t)
                assert (info["source"], info["mask_on_device"], info["tile"]) == (1, True, tile)
                got = read_all(api.jams)
                got.pop("groups")
                same(got, e, "%%s %%s %%s tile %%d from the device" %% (shape, name, link, tile))
    j = api.jams
    lab, cnt, rec, veh = j.device("label"), j.device("count"), j.device("records"), j.device("vehicles")
    assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == shape and np.array_equal(lab.cpu().numpy(), j.plane("label"))
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), j.plane("count"))
    assert rec.cpu().numpy().tobytes() == j.records().tobytes() and rec.shape[0] == j.info()["n_jams"] > 0
    assert tuple(veh.shape) == (api.num_spawned(),) and (veh.cpu().numpy() == -1).all()
    api.close()
'''


def test_masks_from_a_device_tensor():
    """Every mask as a uint8 tensor on the engine's device, and the four device views, in a process of its own that imports
    torch before it loads the engine."""
    procs.run_python(MASK_SCRIPT, torch_first=True, timeout=300)


# ---- 4. refusals and state -----------------------------------------------------------------------------------------------------------
def raw_compute(api, null_query=False, **kw):
    q = jm.TsJamQuery(min_ticks=1, link=1)
    for k, v in kw.items():
        setattr(q, k, v)
    return api.jams._ext("jams_compute")(api.h, None if null_query else ctypes.byref(q), None)


def test_refusals_and_state(monkeypatch):
    monkeypatch.delenv("TS_DEBUG_JAMS_TILE", raising=False)
    api, tr = replayed("carfollow_96_s2", 42)
    j = api.jams
    j.release()
    j.release()                                          # (nothing to free: fine)
    reads = (j.records, j.vehicles, j.plane, lambda: j.plane("count"), j.groups, j.device, lambda: j.records(0, 0))
    refused(capi.TS_E_STATE, *reads)
    i = j.info()
    assert (i["held"], i["n_jams"], i["device_bytes"], i["width"], i["height"]) == (False, 0, 0, api.W, api.H)
    info = j.compute(1, "flow")
    assert info["tile"] == DEFAULT_TILE and info["device_bytes"] >= 2 * 4 * api.W * api.H + 56 * info["n_jams"] + 4 * api.num_spawned()
    held, held_info = as_bytes(read_all(j)), j.info()
    some = np.ones((api.H, api.W), dtype=np.uint8)
    bad = [lambda: raw_compute(api, null_query=True), lambda: raw_compute(api, min_ticks=0), lambda: raw_compute(api, min_ticks=-5),
           lambda: raw_compute(api, link=2), lambda: raw_compute(api, link=-1), lambda: raw_compute(api, source=2),
           lambda: raw_compute(api, source=-1), lambda: raw_compute(api, source=1), lambda: raw_compute(api, source=1, mask=some.ctypes.data, mask_on_device=2)]
    for k, call in enumerate(bad):
        assert call() == capi.TS_E_INVALID, k
        assert as_bytes(read_all(j)) == held and j.info() == held_info, f"refused compute {k} changed the result"
    n, ns = info["n_jams"], info["n_spawned"]
    buf = np.zeros(max(n, ns) + 8, dtype=jm.JAM_DTYPE)
    rec, veh, dl, dev, grp = (j._ext(f"jams_{e}") for e in ("records", "vehicles", "download", "device", "groups"))
    ptr = ctypes.c_void_p()
    for k, rc in enumerate([rec(api.h, -1, 1, buf.ctypes.data), rec(api.h, 0, n + 1, buf.ctypes.data), rec(api.h, n, 1, buf.ctypes.data),
                            rec(api.h, 0, -1, buf.ctypes.data), rec(api.h, 0, 1, None), veh(api.h, -1, 1, buf.ctypes.data),
                            veh(api.h, 1, ns, buf.ctypes.data), veh(api.h, 0, 1, None), dl(api.h, 2, buf.ctypes.data), dl(api.h, -1, buf.ctypes.data),
                            dl(api.h, 0, None), dev(api.h, 4, ctypes.byref(ptr)), dev(api.h, -1, ctypes.byref(ptr)), dev(api.h, 0, None),
                            grp(api.h, None), j._ext("jams_info")(api.h, None)]):
        assert rc == capi.TS_E_INVALID, k
    assert len(j.records(n, 0)) == 0 and len(j.records(0, 0)) == 0 and len(j.vehicles(ns, 0)) == 0
    assert np.array_equal(j.records(3, 4), j.records()[3:7]) and np.array_equal(j.vehicles(5, 9), j.vehicles()[5:14])
    assert as_bytes(read_all(j)) == held
    # a result with zero jams
    zero = j.compute(10 ** 6, "grid")
    assert (zero["held"], zero["n_jams"], zero["standing_cells"], zero["standing_vehicles"], zero["largest_cells"]) == (True, 0, 0, 0, 0)
    assert len(j.records()) == 0 and (j.vehicles() == -1).all() and (j.plane("label") == -1).all() and not j.plane("count").any()
    assert not j.groups().any() and j.groups().shape == (len(tr["g_icell_off"]) - 1, len(jm.JG_FIELDS))
    empty = j.compute(1, "flow", mask=np.zeros((api.H, api.W), dtype=np.uint8))
    assert empty["n_jams"] == 0 and empty["source"] == 1
    j.release()
    refused(capi.TS_E_STATE, *reads)
    assert not j.info()["held"] and j.info()["device_bytes"] == 0


# ---- 5. snapshot and non-interference ----------------------------------------------------------------------------------------------
def test_computing_before_every_tick_changes_nothing():
    name, T = "full_96_s8", 30
    plain, tr = engine_for(name)
    plain.step(T)
    busy, _ = engine_for(name)
    j = busy.jams
    for t in range(T):
        before = busy.checkpoint_save()
        j.compute(1 + t % 3, "flow")
        assert busy.checkpoint_save() == before, f"tick {t}: a compute changed the checkpoint bytes"
        busy.step(1)
    assert j.info()["n_jams"] > 0
    assert_same_deep_state(deep_state(plain), deep_state(busy), "jams computed before every tick")
    assert plain.checkpoint_save() == busy.checkpoint_save()
    cp, cb = plain.counters(), busy.counters()
    assert (cp.astar_calls, cp.astar_expansions, cp.astar_relaxations) == (cb.astar_calls, cb.astar_expansions, cb.astar_relaxations)
    assert cb.astar_calls > 0
    # the result survives ten ticks byte for byte, and a checkpoint load
    j.compute(1, "flow")
    held, info = as_bytes(read_all(j)), j.info()
    assert info["tick"] == T
    blob = busy.checkpoint_save()
    busy.step(10)
    assert as_bytes(read_all(j)) == held and j.info() == info, "ts_step touched the result"
    busy.checkpoint_load(blob)
    assert as_bytes(read_all(j)) == held and j.info() == info, "a checkpoint load touched the result"
    fresh = new_engine()
    setup_from_trace(fresh, tr)
    fresh.checkpoint_load(blob)
    assert not fresh.jams.info()["held"]
    refused(capi.TS_E_STATE, fresh.jams.records)
    for e in (plain, busy, fresh):
        e.close()


# ---- 6. sharded mode ------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import numpy as np
from tests.engine_util import engine_for
from tests.test_gpu_jams import read_all
api, tr = engine_for(%(trace)r)
sr = tdist.ShardedReplans().attach(api)
api.step(%(ticks)d)
assert sr.calls > 0
api.jams.compute(1, "flow")
got = read_all(api.jams)
res["info"] = got.pop("info")
np.savez(os.path.join(OUTDIR, "jams%%d.npz" %% rank), **got)
api.close()
'''


def test_sharded_ranks_compute_the_single_engines_bytes():
    """Two ranks with sharded replanning: both ranks' records, planes, per-vehicle arrays and group rows equal the single
    engine's.  The other engine paths (quads, small heap, host tail, collected pool) differ only in how paths are stored, which
    jam detection does not read - it reads pos, stuck_ticks, flags and the static byte -, so this one two-rank run is the
    path test."""
    name, ticks = "full_96_s8", 30
    ranks, saved, _ = procs.run_ranks(WORKER, 2, timeout=600, trace=name, ticks=ticks)
    api, tr = engine_for(name)
    api.step(ticks)
    api.jams.compute(1, "flow")
    single = read_all(api.jams)
    same(single, expectation(api, tr, je.FLOW, 1), "single engine")
    assert single["info"]["n_jams"] > 10
    for r in range(2):
        assert ranks[r]["info"] == single["info"], r
        for k, v in saved[f"jams{r}.npz"].items():
            assert v.dtype == single[k].dtype and np.array_equal(v, single[k]), f"rank {r}: {k}"
    api.close()
