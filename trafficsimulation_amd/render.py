"""Colour semantics of the device renderer (include/trafficsim_render.h).

The engine looks colours up and knows nothing about them; this module states the reference's rules once, as tables:

  * `cell_palette`     cell.py:274-299 - per cell type and (pending, stop, rain), the colour CellAgent.get_portrayal() returns
  * `vehicle_palette`  vehicle_base.py:793-836, vehicle_service.py:142 - per (kind, status, flash)
  * `desaturate`       utilities/general.py:17-57, with its truncating int(x * 255) hex step
  * `heat_lut`         a default look-up table for the heat overlay (an engine-side addition: the reference has none)

Colour names resolve through CSS_COLORS, the CSS names `Defaults` uses (what matplotlib's to_rgb gives for them).
"""
from __future__ import annotations

import colorsys
from typing import Optional, Sequence

import numpy as np

from . import _capi as capi
from .worldgen import CELL_TYPE_NAMES

CSS_COLORS = {
    "aliceblue": "#f0f8ff", "black": "#000000", "blue": "#0000ff", "cadetblue": "#5f9ea0", "darkgreen": "#006400",
    "darkkhaki": "#bdb76b", "darkolivegreen": "#556b2f", "dodgerblue": "#1e90ff", "green": "#008000", "grey": "#808080",
    "gray": "#808080", "lime": "#00ff00", "magenta": "#ff00ff", "orange": "#ffa500", "palevioletred": "#db7093",
    "papayawhip": "#ffefd5", "red": "#ff0000", "royalblue": "#4169e1", "saddlebrown": "#8b4513", "salmon": "#fa8072",
    "thistle": "#d8bfd8", "white": "#ffffff", "yellow": "#ffff00",
}

# Type codes of the renderer's type plane.  A ControlledRoad keeps the base colour of the road it was carved from
# (city_model.py:1458), so its "go" colour depends on that road's type: codes 0..17 are the `cell_type_map` codes, and a
# controlled road whose original type is known (the `cell_base_type_map` table) has code 18 + that type.
RENDER_TYPE_NAMES = tuple(CELL_TYPE_NAMES) + tuple(f"ControlledRoad:{n}" for n in CELL_TYPE_NAMES)


def type_plane(cell_type_map, cell_base_type_map=None) -> np.ndarray:
    """uint8 [H][W] of codes into RENDER_TYPE_NAMES from the world tables.  Without `cell_base_type_map` (older tables) a
    controlled road has the plain "ControlledRoad" code, whose base colour is ZONE_COLORS["ControlledRoad"]."""
    ct = np.asarray(cell_type_map).astype(np.int64)
    if cell_base_type_map is None:
        return ct.astype(np.uint8)
    base = np.asarray(cell_base_type_map).astype(np.int64)
    controlled = ct == CELL_TYPE_NAMES.index("ControlledRoad")
    return np.where(controlled & (base != ct), len(CELL_TYPE_NAMES) + base, ct).astype(np.uint8)


# the vehicle palette's axes (include/trafficsim_render.h)
VEHICLE_KINDS = ("plain", "contraflow", "service")
VEHICLE_STATUS = ("ok", "collision", "malfunction", "parked")


def _defaults(defaults):
    if defaults is None:
        from .mesa_api import Defaults
        return Defaults
    return defaults


def to_rgb(color: str):
    """(r, g, b) as integers 0..255 of a CSS name from CSS_COLORS or a '#rrggbb' string."""
    h = color if color.startswith("#") else CSS_COLORS.get(color.lower())
    if h is None:
        raise ValueError(f"unknown colour name {color!r} (CSS_COLORS holds the names Defaults uses; '#rrggbb' always works)")
    if len(h) != 7:
        raise ValueError(f"colour {color!r} is not '#rrggbb'")
    return tuple(int(h[i:i + 2], 16) for i in (1, 3, 5))


def to_hex(color: str) -> str:
    return "#{:02x}{:02x}{:02x}".format(*to_rgb(color))


def desaturate(color: str, sat_factor: float = 0.5, light_factor: float = 0.0) -> str:
    """utilities/general.py:27-57: scale the HLS saturation, shift the lightness (clamped to 0..1), back to a hex string
    whose channels are int(x * 255) - truncated, not rounded."""
    r, g, b = (c / 255.0 for c in to_rgb(color))
    h, l, s = colorsys.rgb_to_hls(r, g, b)
    s *= sat_factor
    l = max(0.0, min(1.0, l + light_factor))
    r2, g2, b2 = colorsys.hls_to_rgb(h, l, s)
    return "#{:02x}{:02x}{:02x}".format(int(r2 * 255), int(g2 * 255), int(b2 * 255))


def check_defaults(defaults=None) -> None:
    """CHANGE_ASSIGNED_CELL_COLOR_ON_STOP=True tints road cells that have a light assigned; no table of the engine says which
    cells those are, so it is refused."""
    if getattr(_defaults(defaults), "CHANGE_ASSIGNED_CELL_COLOR_ON_STOP", False):
        raise capi.EngineError(capi.TS_E_UNSUPPORTED, "CHANGE_ASSIGNED_CELL_COLOR_ON_STOP=True: no table says which road cells "
                                                      "have an assigned light")


def cell_color(type_name: str, pend: bool, stop: bool, rain: bool, defaults=None) -> str:
    """The string CellAgent.get_portrayal()["Color"] holds (cell.py:274-299): a colour name where the reference returns the
    name, '#rrggbb' where it returns desaturate's output."""
    zc = _defaults(defaults).ZONE_COLORS
    if type_name.startswith("ControlledRoad:"):          # base_color of the road it was carved from (city_model.py:1458)
        type_name, color = "ControlledRoad", zc.get(type_name.split(":", 1)[1], "white")
    else:
        color = zc.get(type_name, "white")
    if type_name == "ControlledRoad":
        color = zc["ControlledRoadStop"] if stop else desaturate(color, sat_factor=0.75, light_factor=0.25)
    if type_name == "TrafficLight":
        color = zc["TrafficLightStop"] if stop else zc["TrafficLight"]
    if type_name == "Intersection" and pend:
        color = zc["IntersectionPending"]
    if rain:
        color = desaturate(color, sat_factor=0.95, light_factor=-0.05)
    return color


def cell_palette(defaults=None, type_names: Sequence[str] = RENDER_TYPE_NAMES) -> np.ndarray:
    """uint8 [n_types][2 pend][2 stop][2 rain][4] for ts_render_set_cells; type code = index into type_names (default:
    RENDER_TYPE_NAMES, the codes type_plane() gives)."""
    check_defaults(defaults)
    pal = np.zeros((len(type_names), 2, 2, 2, 4), dtype=np.uint8)
    pal[..., 3] = 255
    for t, name in enumerate(type_names):
        for pend in (0, 1):
            for stop in (0, 1):
                for rain in (0, 1):
                    pal[t, pend, stop, rain, :3] = to_rgb(cell_color(name, bool(pend), bool(stop), bool(rain), defaults))
    return pal


def vehicle_color(kind: int, status: int, flash: int, defaults=None) -> str:
    """vehicle_base.py:793-836: the base colour (service vehicles keep theirs whatever else is set; contraflow = overtaking
    or in a stuck detour) while the flash is on or nothing is wrong, else the status colour."""
    d = _defaults(defaults)
    base = (d.VEHICLE_BASE_COLOR, d.VEHICLE_CONTRAFLOW_OVERTAKE_COLOR, d.SERVICE_VEHICLE_BASE_COLOR)[kind]
    alt = (None, d.VEHICLE_COLLISION_COLOR, d.VEHICLE_MALFUNCTION_COLOR, d.VEHICLE_PARKED_COLOR)[status]
    return base if (flash or alt is None) else alt


def vehicle_palette(defaults=None) -> np.ndarray:
    """uint8 [3 kind][4 status][2 flash][4] for ts_render_set_vehicle_palette."""
    pal = np.zeros((3, 4, 2, 4), dtype=np.uint8)
    pal[..., 3] = 255
    for kind in range(3):
        for status in range(4):
            for flash in (0, 1):
                pal[kind, status, flash, :3] = to_rgb(vehicle_color(kind, status, flash, defaults))
    return pal


def vehicle_code(flags) -> np.ndarray:
    """kind * 4 + status of TS_V_FLAGS / meta rows, vectorised: the index into vehicle_palette().reshape(12, 2, 4).  `flags`
    carries the public TS_F_* bits; service vehicles are told by `service` in vehicle_codes below."""
    f = np.asarray(flags).astype(np.int64)
    status = np.where(f & capi.F_COLLISION, 1, np.where(f & capi.F_MALFUNCTION, 2, np.where(f & capi.F_PARKED, 3, 0)))
    kind = np.where(f & (capi.F_OVERTAKING | capi.F_DETOUR), 1, 0)
    return kind * 4 + status


def vehicle_codes(flags, service) -> np.ndarray:
    """vehicle_code with the service kind: `service` is true for ServiceVehicleAgents (kind 2 whatever else is set)."""
    c = vehicle_code(flags)
    return np.where(np.asarray(service, dtype=bool), 8 + c % 4, c)


def heat_lut() -> np.ndarray:
    """uint8 [256][4]: a default ramp for the heat overlay, from transparent dark blue over red to opaque-ish yellow.  Entry 0
    has weight 0: a cell nothing was observed in keeps its colour."""
    i = np.arange(256, dtype=np.int64)
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[:, 0] = np.clip(i * 3, 0, 255)
    lut[:, 1] = np.clip(i * 3 - 255, 0, 255)
    lut[:, 2] = np.clip(128 - i * 2, 0, 255)
    lut[:, 3] = np.where(i == 0, 0, np.clip(64 + i, 0, 230))
    return lut


def fallback_type_names():
    """Type names of worlds without a `cell_type_map` table, in the order of fallback_type_plane's codes."""
    return ("Nothing", "Road", "Intersection", "ControlledRoad", "TrafficLight")


def fallback_type_plane(is_road, intersection, controlled_xy, light_xy) -> np.ndarray:
    """uint8 [H][W] of codes into fallback_type_names(), by the facade's own order of tests (CellAgent.cell_type): light,
    intersection, controlled road, road, nothing."""
    is_road = np.asarray(is_road)
    plane = np.where(is_road != 0, 1, 0).astype(np.uint8)
    for xy, code in ((controlled_xy, 3),):
        xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
        plane[xy[:, 1], xy[:, 0]] = code
    plane[np.asarray(intersection) != 0] = 2
    xy = np.asarray(light_xy, dtype=np.int64).reshape(-1, 2)
    plane[xy[:, 1], xy[:, 0]] = 4
    return plane


def make_view(x0=0, y0=0, cells_w=1, cells_h=1, zoom=1, shrink=1, layers=None, flip_y=False, heat_plane=0, heat_max=1,
              vehicle_radius_256=capi.RENDER_DEFAULT_RADIUS, background=(0, 0, 0, 255)) -> "capi.TsRenderView":
    """A TsRenderView; `layers` is a TS_RL_* mask or names from capi.RENDER_LAYERS (default: signals, rain, vehicles)."""
    v = capi.TsRenderView()
    v.x0, v.y0, v.cells_w, v.cells_h, v.zoom, v.shrink = int(x0), int(y0), int(cells_w), int(cells_h), int(zoom), int(shrink)
    v.layers = capi.render_layer_mask(layers)
    v.flip_y = 1 if flip_y else 0
    v.heat_plane = capi.CApi._heat_plane(heat_plane)
    v.heat_max = int(heat_max)
    v.vehicle_radius_256 = int(vehicle_radius_256)
    bg = tuple(background) + (255,) * (4 - len(tuple(background)))
    for k in range(4):
        v.background[k] = int(bg[k])
    return v
