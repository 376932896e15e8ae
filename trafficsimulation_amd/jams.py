"""Jam detection (include/trafficsim_jams.h): the queues of standing vehicles as connected components of the grid, labelled on
the device.  The entries form a group of their own, in the shape of a `_capi.ENTRIES` value, bound on first use by the rule of
`costfield.CostField._ext`; `CApi.jams` hands out a `Jams`."""
import ctypes as C

import numpy as np

from . import _capi as capi

LINK = {"grid": 0, "flow": 1}
SOURCE = {"vehicles": 0, "mask": 1}
WHICH = {"label": 0, "count": 1, "records": 2, "vehicles": 3}
JG_FIELDS = ["ns_jams", "ns_cells", "ns_vehicles", "ns_stuck_max", "ns_extent", "ew_jams", "ew_cells", "ew_vehicles",
             "ew_stuck_max", "ew_extent", "box_jams", "box_cells"]
JAM_DTYPE = np.dtype([("root_x", np.int32), ("root_y", np.int32), ("cells", np.int32), ("vehicles", np.uint32), ("x0", np.int32),
                      ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("extent", np.int32), ("inter_cells", np.int32),
                      ("stuck_max", np.int32), ("reserved", np.int32), ("stuck_sum", np.int64)])


class TsJamQuery(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("min_ticks", "link", "source", "mask_on_device")] + [("mask", C.c_void_p)]


class TsJamRecord(C.Structure):
    _fields_ = [(n, C.c_uint32 if n == "vehicles" else C.c_int32) for n in JAM_DTYPE.names[:-1]] + [("stuck_sum", C.c_int64)]


class TsJamInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("min_ticks", "link", "source", "mask_on_device", "held", "width", "height", "n_spawned",
                                         "n_jams", "standing_cells", "largest_cells", "tile")] + [
        ("tick", C.c_int64), ("standing_vehicles", C.c_int64), ("device_bytes", C.c_uint64)]


_H, _P, _I32 = C.c_void_p, C.c_void_p, C.c_int32
ENTRIES = ("jam detection", {
    "jams_compute": [_H, C.POINTER(TsJamQuery), C.POINTER(TsJamInfo)],
    "jams_info": [_H, C.POINTER(TsJamInfo)],
    "jams_records": [_H, _I32, _I32, _P],
    "jams_vehicles": [_H, _I32, _I32, _P],
    "jams_download": [_H, _I32, _P],
    "jams_groups": [_H, _P],
    "jams_device": [_H, _I32, C.POINTER(C.c_void_p)],
    "jams_release": [_H],
})


def _name(table: dict, what: str, v) -> int:
    if isinstance(v, str):
        if v not in table:
            raise ValueError(f"unknown {what} {v!r} (one of {sorted(table)})")
        return table[v]
    return max(min(int(v), 0x7FFFFFFF), -0x80000000)


class Jams:
    """The jam-detection entries of one engine (`api`: its CApi)."""

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
        return self.api.prefix == "ts_" and hasattr(self.api.lib, "ts_jams_compute")

    @staticmethod
    def _info(info: TsJamInfo) -> dict:
        d = capi._info_dict(info)
        for k in ("held", "mask_on_device"):
            d[k] = bool(d[k])
        return d

    def compute(self, min_ticks: int = 1, link="flow", mask=None) -> dict:
        """Label the jams of the state as it is now: the connected components ("grid": of 4-neighbours, "flow": of 4-neighbours
        one of which may drive to the other) of the cells that hold a vehicle with stuck_ticks >= min_ticks that is not parked -
        or, with `mask` ((H, W) bytes: a numpy array, or a uint8 torch tensor on the engine's device, read there), of the cells
        whose byte is not 0.  Returns info()."""
        fn = self._ext("jams_compute")
        q = TsJamQuery(min_ticks=max(min(int(min_ticks), 0x7FFFFFFF), -0x80000000), link=_name(LINK, "link", link))
        keep = None
        if mask is not None:
            q.source = SOURCE["mask"]
            shape = (self.api.H, self.api.W)
            if hasattr(mask, "data_ptr"):
                q.mask_on_device = int(self.api._own_tensor(mask, "jams.compute", "uint8", shape))
                keep = mask
                q.mask = mask.data_ptr() or None
            else:
                keep = np.ascontiguousarray(mask, dtype=np.uint8)
                if keep.shape != shape:
                    raise ValueError(f"the mask must be {shape}, got {keep.shape}")
                q.mask = keep.ctypes.data
        info = TsJamInfo()
        self.api._chk(fn(self.api.h, C.byref(q), C.byref(info)))
        del keep
        return self._info(info)

    def info(self) -> dict:
        """{"min_ticks", "link", "source", "mask_on_device", "held", "width", "height", "n_spawned", "n_jams", "standing_cells",
        "largest_cells", "tile", "tick", "standing_vehicles", "device_bytes"}."""
        info = TsJamInfo()
        self.api._chk(self._ext("jams_info")(self.api.h, C.byref(info)))
        return self._info(info)

    def _range(self, first, n, total):
        if n is None:
            n = max(total - int(first), 0)
        return max(min(int(first), 0x7FFFFFFF), -1), max(min(int(n), 0x7FFFFFFF), -1)

    def records(self, first: int = 0, n=None) -> np.ndarray:
        """Jams [first, first + n) (default: all from `first` on) as JAM_DTYPE records, in ascending order of their roots."""
        fn = self._ext("jams_records")
        first, n = self._range(first, n, self.info()["n_jams"])
        out = np.zeros(max(n, 1), dtype=JAM_DTYPE)
        self.api._chk(fn(self.api.h, first, n, out.ctypes.data))
        return out[:max(n, 0)]

    def vehicles(self, first: int = 0, n=None) -> np.ndarray:
        """int32 by spawn index over [first, first + n): the jam a standing vehicle stands in, -1 for every other index."""
        fn = self._ext("jams_vehicles")
        first, n = self._range(first, n, self.info()["n_spawned"])
        out = np.zeros(max(n, 1), dtype=np.int32)
        self.api._chk(fn(self.api.h, first, n, out.ctypes.data))
        return out[:max(n, 0)]

    def plane(self, which="label") -> np.ndarray:
        """"label": (H, W) int32, the jam number, -1 where there is none; "count": (H, W) uint32."""
        fn = self._ext("jams_download")
        w = _name({"label": 0, "count": 1}, "plane", which)
        out = np.zeros((self.api.H, self.api.W), dtype=np.uint32 if w == WHICH["count"] else np.int32)
        self.api._chk(fn(self.api.h, w, out.ctypes.data))
        return out

    def groups(self) -> np.ndarray:
        """[G][JG_FIELDS] int64: per light group and axis the distinct jams that touch its ns_in / ew_in cells, the sums of
        their cells and vehicles, their largest stuck_max and extent; the distinct jams and the standing cells in its box."""
        fn = self._ext("jams_groups")
        n = self.api._chk(self.api._f("num_groups")(self.api.h))
        out = np.zeros((max(n, 1), len(JG_FIELDS)), dtype=np.int64)
        self.api._chk(fn(self.api.h, out.ctypes.data))
        return out[:n]

    def device(self, which="label", device=None):
        """A plane ("label", "count": (H, W)), the records ("records": (n_jams, 14) int32 words of JAM_DTYPE) or the per-vehicle
        array ("vehicles": n_spawned) as an int32 torch tensor over the engine's own device memory (no copy; valid until the next
        compute, release or close).  torch must have been imported before the engine library was loaded, as for observe_device."""
        fn = self._ext("jams_device")
        w = _name(WHICH, "array", which)
        ptr = C.c_void_p()
        self.api._chk(fn(self.api.h, w, C.byref(ptr)))
        i = self.info()
        shape = {WHICH["records"]: (i["n_jams"], JAM_DTYPE.itemsize // 4), WHICH["vehicles"]: (i["n_spawned"],)}.get(w, (self.api.H, self.api.W))
        return self.api._device_view("jams.device", "use jams.records, vehicles or plane for host arrays", ptr.value, "int32", shape, device)

    def release(self):
        """Free the result."""
        self.api._chk(self._ext("jams_release")(self.api.h))
