"""Select-link analysis (include/trafficsim_selectlink.h): which planned routes cross a set of gates, when they arrive, and from
where to where they go, computed on the device.  The entries form a group of their own, in the shape of a `_capi.ENTRIES` value,
bound on first use by the rule of `costfield.CostField._ext`; `CApi.selectlink` hands out a `SelectLink`.

Gate masks are uint32 everywhere: gate 31 is the sign bit of an int32 view."""
import ctypes as C

import numpy as np

from . import _capi as capi

SL_MAX_GATES, SL_MAX_CELLS, SL_MAX_ZONES = 32, 1 << 20, 1024
SL_DIR_ALL = 15
DIR_BITS = {"N": 1, "E": 2, "S": 4, "W": 8}
WHICH = {"mask": 0, "first_step": 1, "first_gate": 2, "crossings": 3, "select": 4, "gates": 5}
_WHICH_DTYPE = {0: "int32", 1: "int32", 2: "int8", 3: "int32", 4: "uint8", 5: "int32"}
VEHICLE_DTYPE = np.dtype([("mask", np.uint32), ("crossings", np.uint32), ("first_step", np.int32), ("first_gate", np.int8)])


class TsSelectLinkQuery(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_bins", "bin_cells", "open_tail", "reserved")]


class TsSelectLinkInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_gates", "n_gate_cells", "held", "n_bins", "bin_cells", "open_tail", "n_spawned", "n_zones",
                                         "width", "height")] + [
        ("tick", C.c_int64), ("vehicles", C.c_int64), ("crossing", C.c_int64), ("crossings", C.c_uint64), ("device_bytes", C.c_uint64)]


_H, _P, _I32, _U32 = C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32
ENTRIES = ("select-link analysis", {
    "selectlink_set_gates": [_H, _I32, _P, _P, _P],
    "selectlink_compute": [_H, C.POINTER(TsSelectLinkQuery), C.POINTER(TsSelectLinkInfo)],
    "selectlink_info": [_H, C.POINTER(TsSelectLinkInfo)],
    "selectlink_tables": [_H, _P, _P],
    "selectlink_vehicles": [_H, _I32, _I32, _P, _P, _P, _P],
    "selectlink_select": [_H, _U32, _U32, _U32, _P, C.POINTER(C.c_int64)],
    "selectlink_set_zones": [_H, _P, _I32],
    "selectlink_od": [_H, _U32, _U32, _U32, _P, C.POINTER(C.c_int64)],
    "selectlink_device": [_H, _I32, C.POINTER(C.c_void_p)],
    "selectlink_release": [_H],
})


def dir_mask(dirs) -> int:
    """The direction mask of a "NESW" subset (or of a mask already)."""
    if isinstance(dirs, str):
        if not dirs or any(ch not in DIR_BITS for ch in dirs.upper()):
            raise ValueError(f"unknown directions {dirs!r} (a non-empty subset of 'NESW')")
        return sum({DIR_BITS[ch] for ch in dirs.upper()})
    return int(dirs)


def gate_tables(gates):
    """(gate_off int32[G + 1], cells_xy int32[n][2], dir_mask uint8[n]) of a list of gates, each a list of (x, y) - open to
    all four directions - or (x, y, "NESW"-subset or mask)."""
    off, xy, dm = [0], [], []
    for gate in gates:
        for cell in gate:
            xy.append((int(cell[0]), int(cell[1])))
            dm.append(dir_mask(cell[2]) if len(cell) > 2 else SL_DIR_ALL)
        off.append(len(xy))
    if any(not 0 <= m <= 255 for m in dm):
        raise ValueError("a direction mask is one byte")
    return capi._i32(off), capi._i32(xy).reshape(-1, 2), np.asarray(dm, dtype=np.uint8)


def _u32(v) -> int:
    v = int(v)
    if not 0 <= v <= 0xFFFFFFFF:
        raise ValueError(f"a gate mask is a uint32, got {v}")
    return v


class SelectLink:
    """The select-link entries of one engine (`api`: its CApi)."""

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
        return self.api.prefix == "ts_" and hasattr(self.api.lib, "ts_selectlink_compute")

    @staticmethod
    def _info(info: TsSelectLinkInfo) -> dict:
        d = capi._info_dict(info)
        for k in ("held", "open_tail"):
            d[k] = bool(d[k])
        return d

    def set_gates(self, gates):
        """Make `gates` the set held (see gate_tables); drops the result."""
        fn = self._ext("selectlink_set_gates")
        off, xy, dm = gate_tables(gates)
        keep_xy = xy if len(xy) else np.zeros((1, 2), dtype=np.int32)      # (no cells still reaches the engine's refusal)
        keep_dm = dm if len(dm) else np.zeros(1, dtype=np.uint8)
        self.api._chk(fn(self.api.h, len(off) - 1, off.ctypes.data, keep_xy.ctypes.data, keep_dm.ctypes.data))

    def compute(self, n_bins: int = 1, bin_cells: int = 1, open_tail: bool = True) -> dict:
        """Walk every live vehicle's remaining main path over the gates held: step k is in bin k // bin_cells, steps beyond the
        last bin count in it (`open_tail`) or do not exist for the query.  Returns info()."""
        fn = self._ext("selectlink_compute")
        q = TsSelectLinkQuery(n_bins=int(n_bins), bin_cells=int(bin_cells), open_tail=int(bool(open_tail)))
        info = TsSelectLinkInfo()
        self.api._chk(fn(self.api.h, C.byref(q), C.byref(info)))
        return self._info(info)

    def info(self) -> dict:
        """{"n_gates", "n_gate_cells", "held", "n_bins", "bin_cells", "open_tail", "n_spawned", "n_zones", "width", "height",
        "tick", "vehicles", "crossing", "crossings", "device_bytes"}."""
        info = TsSelectLinkInfo()
        self.api._chk(self._ext("selectlink_info")(self.api.h, C.byref(info)))
        return self._info(info)

    def tables(self):
        """(cross (G, bins, 4) uint64: crossings by gate, bin and direction; pair (G, G) uint64: vehicles crossing both gates)."""
        fn = self._ext("selectlink_tables")
        i = self.info()
        G, B = i["n_gates"], i["n_bins"]
        cross, pair = np.zeros((max(G, 1), max(B, 1), 4), dtype=np.uint64), np.zeros((max(G, 1), max(G, 1)), dtype=np.uint64)
        self.api._chk(fn(self.api.h, cross.ctypes.data, pair.ctypes.data))
        return cross[:G, :B], pair[:G, :G]

    def vehicles(self, first: int = 0, n=None) -> np.ndarray:
        """Spawn indices [first, first + n) (default: all from `first` on) as VEHICLE_DTYPE records."""
        fn = self._ext("selectlink_vehicles")
        if n is None:
            n = max(self.info()["n_spawned"] - int(first), 0)
        first, n = max(min(int(first), 0x7FFFFFFF), -1), max(min(int(n), 0x7FFFFFFF), -1)
        k = max(n, 1)
        m, fs, fg, cr = np.zeros(k, np.uint32), np.zeros(k, np.int32), np.zeros(k, np.int8), np.zeros(k, np.uint32)
        self.api._chk(fn(self.api.h, first, n, m.ctypes.data, fs.ctypes.data, fg.ctypes.data, cr.ctypes.data))
        out = np.zeros(max(n, 0), dtype=VEHICLE_DTYPE)
        out["mask"], out["crossings"], out["first_step"], out["first_gate"] = m[:len(out)], cr[:len(out)], fs[:len(out)], fg[:len(out)]
        return out

    def select(self, any: int = 0, all: int = 0, none: int = 0):
        """(select bytes uint8[n_spawned], number selected) of the vehicles walked with
        (any == 0 or mask & any) and mask & all == all and mask & none == 0; the bytes stay on the device for device("select")."""
        fn = self._ext("selectlink_select")
        any, all, none = _u32(any), _u32(all), _u32(none)
        dst = np.zeros(max(self.info()["n_spawned"], 1), dtype=np.uint8)
        count = C.c_int64()
        self.api._chk(fn(self.api.h, any, all, none, dst.ctypes.data, C.byref(count)))
        return dst[:self.info()["n_spawned"]], int(count.value)

    def set_zones(self, zone_of_cell, n_zones: int):
        """One (H, W) int32 plane: the zone 0 .. n_zones - 1 of every cell, -1 = none.  n_zones = 0 drops the plane."""
        fn = self._ext("selectlink_set_zones")
        z = None
        if zone_of_cell is not None:
            z = np.ascontiguousarray(zone_of_cell, dtype=np.int32)
            if z.shape != (self.api.H, self.api.W):
                raise ValueError(f"the zone plane must be ({self.api.H}, {self.api.W}), got {z.shape}")
        self.api._chk(fn(self.api.h, z.ctypes.data if z is not None else None, max(min(int(n_zones), 0x7FFFFFFF), -1)))

    def od(self, any: int = 0, all: int = 0, none: int = 0):
        """(counts (Z, Z) int64 indexed [zone(cell at the compute), zone(goal at the compute)], unzoned) of the selected."""
        fn = self._ext("selectlink_od")
        any, all, none = _u32(any), _u32(all), _u32(none)
        nz = self.info()["n_zones"]
        counts, unzoned = np.zeros((max(nz, 1), max(nz, 1)), dtype=np.int64), C.c_int64()
        self.api._chk(fn(self.api.h, any, all, none, counts.ctypes.data, C.byref(unzoned)))
        return counts[:nz, :nz], int(unzoned.value)

    def device(self, which="mask", device=None):
        """A per-vehicle array ("mask", "first_step", "first_gate", "crossings", "select": n_spawned elements) or the gate plane
        ("gates": (H, W)) as a torch tensor over the engine's own device memory (no copy; uint32 values come as the bits of an
        int32 tensor; valid until the next set_gates, compute, release or close).  torch must have been imported before the
        engine library was loaded, as for observe_device."""
        fn = self._ext("selectlink_device")
        if isinstance(which, str):
            if which not in WHICH:
                raise ValueError(f"unknown array {which!r} (one of {sorted(WHICH)})")
            which = WHICH[which]
        w = int(which)
        ptr = C.c_void_p()
        self.api._chk(fn(self.api.h, w, C.byref(ptr)))
        shape = (self.api.H, self.api.W) if w == WHICH["gates"] else (self.info()["n_spawned"],)
        return self.api._device_view("selectlink.device", "use selectlink.vehicles or select for host arrays", ptr.value,
                                     _WHICH_DTYPE.get(w, "int32"), shape, device)

    def release(self):
        """Free gates, result and zone plane."""
        self.api._chk(self._ext("selectlink_release")(self.api.h))
