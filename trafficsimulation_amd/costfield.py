"""Cost fields (include/trafficsim_costfield.h): the travel cost from a set of seed cells to every cell, or from every cell
to the nearest seed, and the seed that attains it, computed on the device.  The entries form a group of their own, in the
shape of a `_capi.ENTRIES` value, bound on first use by `CApi._ext`'s rules; `CApi.costfield` hands out a `CostField`."""
import ctypes as C

import numpy as np

from . import _capi as capi

CF_FROM, CF_TO = 0, 1
CF_VALUE, CF_OWNER = 0, 1
CF_MAX_SEEDS, CF_MAX_BANDS = 1 << 20, 1024
CF_UNREACHABLE = 0xFFFFFFFF
CF_INF = 0x3F3F3F3F          # the reference's INF: values of this much or more do not exist
MODES = {"from": CF_FROM, "to": CF_TO}
PLANES = {"cost": CF_VALUE, "value": CF_VALUE, "owner": CF_OWNER}


class TsCostFieldQuery(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "soft_obstacles", "ignore_flow", "free_flow")] + [
        ("max_cost", C.c_uint32), ("n_seeds", C.c_int32), ("seed_xy", C.c_void_p), ("seed_cost", C.c_void_p), ("reserved", C.c_int64)]


class TsCostFieldInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "soft_obstacles", "ignore_flow", "free_flow")] + [
        ("max_cost", C.c_uint32)] + [(n, C.c_int32) for n in ("n_seeds", "width", "height", "tile", "headings")] + [
        ("tick", C.c_int64), ("reached", C.c_int64), ("max_value", C.c_uint32), ("rounds", C.c_int32), ("tile_visits", C.c_int64),
        ("device_bytes", C.c_uint64)]


_H, _P, _I32 = C.c_void_p, C.c_void_p, C.c_int32
ENTRIES = ("cost field", {
    "costfield_compute": [_H, C.POINTER(TsCostFieldQuery), C.POINTER(TsCostFieldInfo)],
    "costfield_info": [_H, C.POINTER(TsCostFieldInfo)],
    "costfield_download": [_H, _I32, _P],
    "costfield_gather": [_H, _I32, _I32, _P, _P],
    "costfield_bands": [_H, _I32, _P, _P],
    "costfield_device": [_H, _I32, C.POINTER(C.c_void_p)],
    "costfield_release": [_H],
})


def _which(which) -> int:
    if isinstance(which, str):
        if which not in PLANES:
            raise ValueError(f"unknown plane {which!r} (one of {sorted(PLANES)})")
        return PLANES[which]
    return int(which)


class CostField:
    """The cost-field entries of one engine (`api`: its CApi)."""

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
        return self.api.prefix == "ts_" and hasattr(self.api.lib, "ts_costfield_compute")

    @property
    def routes(self):
        """The routes along this engine's cost field, as a cfroute.RouteField (a view like this one)."""
        from .cfroute import RouteField
        return RouteField(self.api)

    @staticmethod
    def _info(info: TsCostFieldInfo) -> dict:
        d = capi._info_dict(info)
        d["mode"] = "to" if d["mode"] == CF_TO else "from"
        for k in ("soft_obstacles", "ignore_flow", "free_flow"):
            d[k] = bool(d[k])
        return d

    def compute(self, seeds, seed_cost=None, mode="to", soft=True, ignore_flow=False, free_flow=False, max_cost=0) -> dict:
        """The field of the engine's current maps.  `seeds`: (n, 2) (x, y) cells; `seed_cost`: n costs added to what leaves
        from (`mode="from"`) or arrives at (`"to"`) each seed, None: all 0; `soft`: occupied and red cells cost their
        penalties (else they cannot be entered); `ignore_flow`: steps against the flow at the contraflow penalty;
        `free_flow`: occupancy and lights are not looked at; `max_cost`: values above it are unreachable (0: no limit).
        Returns info()."""
        return self._compute(self._ext("costfield_compute"), seeds, seed_cost, mode, soft, ignore_flow, free_flow, max_cost)

    def _compute(self, fn, seeds, seed_cost, mode, soft, ignore_flow, free_flow, max_cost) -> dict:
        """compute() through the entry `fn` (cfroute.RouteField.compute: the same query, and a hop plane)."""
        if mode not in MODES:
            raise ValueError(f"unknown mode {mode!r} ('from' or 'to')")
        xy = capi._i32(seeds).reshape(-1, 2)
        q = TsCostFieldQuery(mode=MODES[mode], soft_obstacles=int(bool(soft)), ignore_flow=int(bool(ignore_flow)),
                             free_flow=int(bool(free_flow)), max_cost=int(max_cost), n_seeds=len(xy))
        keep = xy if len(xy) else np.zeros((1, 2), dtype=np.int32)       # (no seeds still reaches the engine's refusal)
        q.seed_xy = keep.ctypes.data
        cost = None
        if seed_cost is not None:
            cost = capi._i32(seed_cost).reshape(-1)
            if len(cost) != len(xy):
                raise ValueError(f"{len(cost)} seed costs for {len(xy)} seeds")
            q.seed_cost = cost.ctypes.data if len(cost) else None
        info = TsCostFieldInfo()
        self.api._chk(fn(self.api.h, C.byref(q), C.byref(info)))
        del keep, cost
        return self._info(info)

    def info(self) -> dict:
        """The query of the result held ("mode", "soft_obstacles", "ignore_flow", "free_flow", "max_cost", "n_seeds": 0 when
        there is none), "width", "height", "tile", "headings", "tick", "reached", "max_value", "rounds", "tile_visits",
        "device_bytes"."""
        info = TsCostFieldInfo()
        self.api._chk(self._ext("costfield_info")(self.api.h, C.byref(info)))
        return self._info(info)

    def plane(self, which="cost") -> np.ndarray:
        """The value plane ("cost" or 0: (H, W) uint32, CF_UNREACHABLE where no path exists) or the owner plane ("owner" or 1:
        (H, W) int32 seed indices, -1 where unreachable)."""
        w = _which(which)
        out = np.zeros((self.api.H, self.api.W), dtype=np.int32 if w == CF_OWNER else np.uint32)
        self.api._chk(self._ext("costfield_download")(self.api.h, w, out.ctypes.data))
        return out

    def gather(self, which, xy) -> np.ndarray:
        """The plane at the (n, 2) cells `xy`, read on the device."""
        fn, w = self._ext("costfield_gather"), _which(which)
        cells = capi._i32(xy).reshape(-1, 2)
        out = np.zeros(len(cells), dtype=np.int32 if w == CF_OWNER else np.uint32)
        self.api._chk(fn(self.api.h, w, len(cells), cells.ctypes.data if len(cells) else None, out.ctypes.data if len(cells) else None))
        return out

    def bands(self, thresholds) -> np.ndarray:
        """Isochrone areas: for every ascending threshold the number of road cells whose value is <= it (uint64), reduced on
        the device."""
        fn = self._ext("costfield_bands")
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.uint32).reshape(-1))
        out = np.zeros(max(len(thr), 1), dtype=np.uint64)
        self.api._chk(fn(self.api.h, len(thr), thr.ctypes.data if len(thr) else None, out.ctypes.data))
        return out[:len(thr)]

    def device(self, which="cost", device=None):
        """A plane as an (H, W) int32 torch tensor over the engine's own device memory (no copy; the value plane's bits are
        its uint32 values; valid until the next compute, release or close).  torch must have been imported before the engine
        library was loaded, as for observe_device."""
        ptr = C.c_void_p()
        self.api._chk(self._ext("costfield_device")(self.api.h, _which(which), C.byref(ptr)))
        return self.api._device_view("costfield.device", "use costfield.plane for a host array", ptr.value, "int32",
                                     (self.api.H, self.api.W), device)

    def release(self):
        """Free the planes; there is no result afterwards."""
        self.api._chk(self._ext("costfield_release")(self.api.h))
