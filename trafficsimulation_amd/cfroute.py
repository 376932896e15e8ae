"""Routes along a cost field (include/trafficsim_cfroute.h): the hop plane a compute leaves, the routes of many starts in one
launch and the load they put on the network, on the device.  The entries form a group of their own, in the shape of a
`_capi.ENTRIES` value, bound on first use by `costfield.CostField._ext`'s rule; `CApi.costfield.routes` hands out a
`RouteField`."""
import ctypes as C

import numpy as np

from . import _capi as capi
from . import costfield as cf

CFR_STOP, CFR_NONE = 4, 7
CFR_HOPS, CFR_OFF, CFR_DIRS, CFR_COST, CFR_OWNER = 0, 1, 2, 3, 4
CFR_MAX_STARTS = 1 << 24
PARTS = {"hops": (CFR_HOPS, "int16"), "off": (CFR_OFF, "int64"), "dirs": (CFR_DIRS, "uint8"), "cost": (CFR_COST, "int32"),
         "owner": (CFR_OWNER, "int32")}


class TsCfRouteBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("unreached", C.c_int32), ("steps", C.c_int64), ("longest", C.c_int64), ("tick", C.c_int64),
                ("device_bytes", C.c_uint64)]


class TsCfRouteLoadInfo(C.Structure):
    _fields_ = [("routes", C.c_int64), ("unreached", C.c_int64), ("steps", C.c_uint64), ("tick", C.c_int64),
                ("device_bytes", C.c_uint64)]


class TsCfRouteInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("held", "mode", "headings", "n_seeds", "width", "height")] + [
        ("tick", C.c_int64), ("device_bytes", C.c_uint64), ("trace_n", C.c_int32), ("trace_unreached", C.c_int32),
        ("trace_steps", C.c_int64), ("trace_longest", C.c_int64), ("trace_tick", C.c_int64), ("trace_device_bytes", C.c_uint64),
        ("load_routes", C.c_int64), ("load_unreached", C.c_int64), ("load_steps", C.c_uint64), ("load_tick", C.c_int64),
        ("load_device_bytes", C.c_uint64)]


_H, _P, _I32 = C.c_void_p, C.c_void_p, C.c_int32
ENTRIES = ("cost-field routes", {
    "cfroute_compute": [_H, C.POINTER(cf.TsCostFieldQuery), C.POINTER(cf.TsCostFieldInfo)],
    "cfroute_info": [_H, C.POINTER(TsCfRouteInfo)],
    "cfroute_trace": [_H, _I32, _P, _P, C.POINTER(TsCfRouteBatch)],
    "cfroute_read": [_H, _I32, _I32, _P, _P, _P, _P],
    "cfroute_cells": [_H, _I32, _I32, _P, _P],
    "cfroute_device": [_H, _I32, C.POINTER(C.c_void_p)],
    "cfroute_load": [_H, _I32, _P, _P, _P, C.POINTER(TsCfRouteLoadInfo)],
    "cfroute_load_download": [_H, _I32, _P],
    "cfroute_load_device": [_H, _I32, C.POINTER(C.c_void_p)],
    "cfroute_release": [_H],
})


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class RouteField:
    """The cost-field route entries of one engine (`api`: its CApi)."""

    def __init__(self, api):
        self.api = api

    def _ext(self, name: str):
        """An entry of ENTRIES, bound on first use: one binding per function object; the CPU oracle has none of them."""
        api = self.api
        phrase, entries = ENTRIES
        fn = getattr(api.lib, api.prefix + name, None) if api.prefix == "ts_" else None
        if fn is None:
            raise capi.EngineError(capi.TS_E_UNSUPPORTED, f"{api.prefix}{name}: this engine has no {phrase}")
        if fn.argtypes is None:
            fn.restype, fn.argtypes = C.c_int, entries[name]
        return fn

    @property
    def available(self) -> bool:
        return self.api.prefix == "ts_" and hasattr(self.api.lib, "ts_cfroute_compute")

    def compute(self, seeds, seed_cost=None, mode="to", soft=True, ignore_flow=False, free_flow=False, max_cost=0) -> dict:
        """`CostField.compute` with the same arguments and the same result - the planes `api.costfield` reads afterwards -
        and the hop plane of that field, which `trace` and `load` walk."""
        return cf.CostField(self.api)._compute(self._ext("cfroute_compute"), seeds, seed_cost, mode, soft, ignore_flow, free_flow, max_cost)

    def info(self) -> dict:
        """"held" (a hop plane exists), its "mode", "headings", "n_seeds", "tick" and "device_bytes", "width", "height", and
        the figures of the last trace ("trace_n", "trace_unreached", "trace_steps", "trace_longest", "trace_tick",
        "trace_device_bytes") and the last load ("load_routes", "load_unreached", "load_steps", "load_tick",
        "load_device_bytes")."""
        info = TsCfRouteInfo()
        self.api._chk(self._ext("cfroute_info")(self.api.h, C.byref(info)))
        d = capi._info_dict(info)
        d["held"] = bool(d["held"])
        d["mode"] = ("to" if d["mode"] == cf.CF_TO else "from") if d["held"] else None
        return d

    @staticmethod
    def _starts(starts, headings, weights=None):
        xy = capi._i32(starts).reshape(-1, 2)
        head = None if headings is None else np.ascontiguousarray(np.asarray(headings, dtype=np.int8).reshape(-1))
        w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.uint32).reshape(-1))
        for name, a in (("headings", head), ("weights", w)):
            if a is not None and len(a) != len(xy):
                raise ValueError(f"{len(a)} {name} for {len(xy)} starts")
        return xy, head, w

    def trace(self, starts, headings=None) -> dict:
        """The routes of the (n, 2) (x, y) cells `starts` along the hop plane, as the batch `routes` and `cells` read.  With a
        TO field `headings` (n values, -1: none, 0..3: N E S W) are the headings the starts are held with; with a FROM field
        they must be None or -1.  Returns {"n", "unreached", "steps", "longest", "tick", "device_bytes"}."""
        fn = self._ext("cfroute_trace")
        xy, head, _ = self._starts(starts, headings)
        out = TsCfRouteBatch()
        self.api._chk(fn(self.api.h, len(xy), _ptr(xy), _ptr(head), C.byref(out)))
        return capi._info_dict(out)

    def _range(self, first, n):
        total = self.info()["trace_n"]
        return int(first), (max(total - int(first), 0) if n is None else int(n))

    def routes(self, first=0, n=None):
        """Routes first .. first + n - 1 of the batch (n None: to its end) -> (off int64[n + 1], dirs uint8[off[n]], cost
        uint32[n], owner int32[n]): one direction byte per step (N 0, E 1, S 2, W 3), in travel order."""
        fn = self._ext("cfroute_read")
        first, n = self._range(first, n)
        off = np.zeros(n + 1, dtype=np.int64)
        cost, owner = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        self.api._chk(fn(self.api.h, first, n, off.ctypes.data, None, _ptr(cost), _ptr(owner)))
        dirs = np.zeros(int(off[-1]), dtype=np.uint8)
        if dirs.size:
            self.api._chk(fn(self.api.h, first, n, None, dirs.ctypes.data, None, None))
        return off, dirs, cost, owner

    def cells(self, first=0, n=None):
        """The same routes as cells -> (off int64[n + 1], xy int32[off[n], 2]), every route without its first cell, expanded
        on the device."""
        fn = self._ext("cfroute_cells")
        first, n = self._range(first, n)
        off = np.zeros(n + 1, dtype=np.int64)
        self.api._chk(fn(self.api.h, first, n, off.ctypes.data, None))
        xy = np.zeros((int(off[-1]), 2), dtype=np.int32)
        if xy.size:
            self.api._chk(fn(self.api.h, first, n, None, xy.ctypes.data))
        return off, xy

    def load(self, starts, headings=None, weights=None) -> dict:
        """All-or-nothing assignment: every start sends its weight (None: 1) down its route; the four planes stay on the
        device for `load_plane`.  Returns {"routes", "unreached", "steps", "tick", "device_bytes"}."""
        fn = self._ext("cfroute_load")
        xy, head, w = self._starts(starts, headings, weights)
        out = TsCfRouteLoadInfo()
        self.api._chk(fn(self.api.h, len(xy), _ptr(xy), _ptr(head), _ptr(w), C.byref(out)))
        return capi._info_dict(out)

    def load_plane(self, dir=None) -> np.ndarray:
        """(H, W) uint32: the load that enters every cell in direction `dir` (0..3), or with None the four summed on the
        device."""
        out = np.zeros((self.api.H, self.api.W), dtype=np.uint32)
        self.api._chk(self._ext("cfroute_load_download")(self.api.h, -1 if dir is None else int(dir), out.ctypes.data))
        return out

    def device(self, which="hops", device=None):
        """A torch tensor over the engine's own device memory (no copy): "hops" (H, W) int16 (the bits of the uint16 plane),
        "off" int64[n + 1], "dirs" uint8[steps], "cost" int32[n] (the bits of the uint32 costs), "owner" int32[n] of the
        batch, or "load" (4, H, W) int32.  Valid until the next compute, trace, load or release; torch must have been
        imported before the engine library was loaded."""
        ptr = C.c_void_p()
        if which == "load":
            self.api._chk(self._ext("cfroute_load_device")(self.api.h, 0, C.byref(ptr)))
            dtype, shape = "int32", (4, self.api.H, self.api.W)
        else:
            if which not in PARTS:
                raise ValueError(f"unknown part {which!r} (one of {sorted(PARTS) + ['load']})")
            code, dtype = PARTS[which]
            self.api._chk(self._ext("cfroute_device")(self.api.h, code, C.byref(ptr)))
            i = self.info()
            shape = {"hops": (self.api.H, self.api.W), "off": (i["trace_n"] + 1,), "dirs": (i["trace_steps"],)}.get(which, (i["trace_n"],))
        return self.api._device_view("costfield.routes.device", "use routes / cells / load_plane for host arrays", ptr.value, dtype, shape, device)

    def release(self):
        """Free the hop plane, the batch and the load planes; the cost field stays."""
        self.api._chk(self._ext("cfroute_release")(self.api.h))
