"""The engine-side rules of the cost-field, cost-field-route and select-link tests that more than one module needs: one call of
the extension held against the expectation (tests/costfield_expect.py, tests/cfroute_expect.py, tests/selectlink_expect.py).
tests/test_gpu_costfield.py, tests/test_gpu_cfroute.py and tests/test_gpu_selectlink.py import them back; tests/ext_sidecar.py
runs them on every engine path.  No pytest in here: the worker scripts of the sharded runs import this module."""
import ctypes

import numpy as np

from tests import cfroute_expect as re_
from tests import costfield_expect as ce
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import cfroute as cr


# ---- cost fields ------------------------------------------------------------------------------------------------------------
def rule_of(api, params, tables):
    """The step rule on the engine's maps as they are now (the density map is download_density's)."""
    return ce.Rule.from_params(params, tables["allowed_dirs_map"], tables["is_road_map"], tables["road_type_map"],
                               api.map(capi.MAP_OCCUPANCY), api.map(capi.MAP_STOP), api.density())


# ---- routes along a cost field ----------------------------------------------------------------------------------------------
def modes_of(q):
    return dict(mode=q.get("mode", "to"), soft=q.get("soft", True), ignore_flow=q.get("ignore_flow", False),
                free_flow=q.get("free_flow", False), max_cost=q.get("max_cost", 0))


def expectation(rule, seeds, cost, q):
    """(labels, hop plane, states per cell) of a query."""
    L = re_.labels(rule, seeds, cost, **modes_of(q))
    return L, re_.hop_plane(rule, L, seeds, cost, **modes_of(q)), re_.headings(rule)


def expand(starts, off, dirs, mode):
    """The cells of every route of a batch without its first one, in one (steps, 2) array."""
    out = []
    for i, s in enumerate(np.asarray(starts).reshape(-1, 2).tolist()):
        out += re_.cells_of(s, [int(d) for d in dirs[off[i]:off[i + 1]]], mode)[1:]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def check_batch(api, want, starts, heads, mode, ctx):
    """trace() the starts and compare the whole batch, and cells(), with the expectation `want`."""
    r = api.costfield.routes
    info = r.trace(starts, heads)
    off, dirs, cost, owner = r.routes()
    for name, got, exp in zip(("off", "dirs", "cost", "owner"), (off, dirs, cost, owner), want):
        assert got.dtype == exp.dtype and np.array_equal(got, exp), f"{ctx}: {name} differs at {np.argwhere(got != exp)[:4].ravel().tolist() if got.shape == exp.shape else (got.shape, exp.shape)}"
    coff, xy = r.cells()
    assert np.array_equal(coff, off) and np.array_equal(xy, expand(starts, off, dirs, mode)), f"{ctx}: cells()"
    lens = np.diff(want[0])
    assert info["n"] == len(lens) and info["steps"] == int(want[0][-1]) and info["longest"] == int(lens.max())
    assert info["unreached"] == int((want[3] == -1).sum())
    return info


def download_hops(api):
    """The hop plane held as an (H, W) uint16 host array, without torch: ts_cfroute_device waits for the engine's stream and hands
    out the plane's device pointer, and the HIP runtime that the engine library itself is linked against (looked up through the
    library's own handle, so it is the one the engine allocates with) copies H * W * 2 bytes from there."""
    ptr = ctypes.c_void_p()
    api._chk(api.costfield.routes._ext("cfroute_device")(api.h, cr.CFR_HOPS, ctypes.byref(ptr)))
    out = np.zeros((api.H, api.W), dtype=np.uint16)
    copy = api.lib.hipMemcpy
    copy.restype, copy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    err = copy(out.ctypes.data, ptr, out.nbytes, 2)              # hipMemcpyDeviceToHost
    assert err == 0, f"hipMemcpy of the hop plane: HIP error {err}"
    return out


# ---- select-link ------------------------------------------------------------------------------------------------------------
def read_result(s):
    """Everything a result holds, as one dict of arrays and ints."""
    v, (cross, pair), info = s.vehicles(), s.tables(), s.info()
    return {"mask": v["mask"], "crossings": v["crossings"], "first_step": v["first_step"], "first_gate": v["first_gate"],
            "cross": cross, "pair": pair, "t_vehicles": info["vehicles"], "t_crossing": info["crossing"], "t_crossings": info["crossings"]}


def check_result(s, want, gates, query, tick, ctx):
    """One compute of `query` over the gates held against the rule's result `want`."""
    info = s.compute(*query[:2], bool(query[2]))
    assert info == s.info(), ctx
    assert (info["held"], info["n_bins"], info["bin_cells"], info["open_tail"]) == (True, query[0], query[1], bool(query[2])), ctx
    assert (info["n_gates"], info["n_gate_cells"], info["tick"]) == (len(gates), sum(len(g) for g in gates), tick), ctx
    assert (info["width"], info["height"], info["n_spawned"]) == (s.api.W, s.api.H, len(want["mask"])), ctx
    got = read_result(s)
    for k in ("mask", "crossings", "first_step", "first_gate", "cross", "pair"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{ctx}: {k} differs at {np.argwhere(got[k] != want[k])[:4].tolist()}"
    for k in ("t_vehicles", "t_crossing", "t_crossings"):
        assert got[k] == want[k], f"{ctx}: {k}: {got[k]} != {want[k]}"
    return got
