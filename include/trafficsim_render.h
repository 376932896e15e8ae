/*
 * trafficsim_render.h - a device renderer: RGBA8 frames of cells, lights, rain, vehicles, a heat overlay and drawn routes.
 *
 * An engine-side extension of trafficsim.h, in the shape of trafficsim_observe.h.  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no renderer.  The engine knows no colour semantics: the caller uploads a static type code per
 * cell and palettes indexed by (type, pending, stop, rain) and (kind, status, flash); trafficsimulation_amd/render.py
 * builds the reference's tables (cell.py:274-299, vehicle_base.py:817-836).  A type code is whatever the caller wants a
 * colour for: render.py uses the cell_type_map codes plus one code per original road type of a ControlledRoad.
 *
 * A frame is RGBA8, row-major, alpha 255.  With zoom it is cells_w * zoom by cells_h * zoom pixels, with shrink
 * ceil(cells_w / shrink) by ceil(cells_h / shrink).  Row 0 is the view's smallest y, like the [y, x] planes of
 * trafficsim.h; with flip_y row 0 is the largest y.
 *
 * The pixel rule (exact integer arithmetic), per cell (x, y) of the view, in this order:
 *   1 cell     t = type_plane[y][x]; stop = (stop_map == 1), 0 without TS_RL_SIGNALS; pend = 1 on the intersection cells of
 *              a light group whose pending phase is not None, 0 without TS_RL_SIGNALS; rain = (rain_map > 0), 0 without
 *              TS_RL_RAIN.  c = cell_palette[((t * 2 + pend) * 2 + stop) * 2 + rain].  A cell outside the map, or any cell
 *              before ts_render_set_cells, takes `background` and nothing else is drawn on it.
 *   2 heat     (TS_RL_HEAT) i = min(255, value * 255 / heat_max) in 64 bits, value from the observation plane heat_plane
 *              (TS_OBS_NPLANES: the four ENTER planes summed in 64 bits);
 *              c = (c * (255 - A) + lut[i] * A + 127) / 255 per channel, A = lut[i][3].
 *   3 route    (TS_RL_ROUTES) the same blend with the route colour on every cell of the remaining path of a listed live
 *              vehicle: exactly the cells ts_download_path returns for it.
 *   4 vehicle  (TS_RL_VEHICLES) the top vehicle of the cell is the tail of its MultiGrid list (the one a CanvasGrid draws
 *              last); parked and servicing vehicles count.  kind: 2 service, else 1 overtaking or in a stuck detour, else 0.
 *              status, first match: 1 collision, 2 malfunction, 3 parked, else 0.  flash = (step_count % 2 == 0), with
 *              TsCounters::step_count.  At zoom z pixel (i, j) of the cell takes vehicle_palette[kind][status][flash] if
 *              ((2i+1-z)^2 + (2j+1-z)^2) * 65536 <= (2 * R * z)^2, R = vehicle_radius_256, in 64 bits.  At zoom 1 and under
 *              shrink the vehicle fills its cell.
 *   5 scale    zoom replicates; shrink s gives (sum + s^2 / 2) / (s^2) per channel over the composed colours of the s x s
 *              cells of the box, cells outside the view or the map counting as `background`.
 *
 * The renderer never changes what a run computes and is not part of a checkpoint: ts_checkpoint_save gives identical bytes
 * with and without it, and a handle built from a checkpoint starts without tables.  In sharded mode
 * (ts_set_replan_sharding) every rank can render its replicated state; nothing is exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_INVALID   a null pointer, a bad view (see TsRenderView), n_types outside 1..64, a type code >= n_types, a route
 *                    id outside 0..ts_num_spawned-1, n outside 0..TS_RENDER_MAX_ROUTES.
 *   - TS_E_STATE     TS_RL_HEAT without that plane observed or without a LUT, TS_RL_VEHICLES without a vehicle palette.
 *   - TS_E_CAPACITY  a frame wider or taller than TS_RENDER_MAX_SIDE.
 *   - TS_E_DEVICE    no device memory.
 *   A refused call writes nothing and leaves the previous frame buffer as it was.
 */
#ifndef TRAFFICSIM_RENDER_H
#define TRAFFICSIM_RENDER_H

#include "trafficsim.h"
#include "trafficsim_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TS_RL_SIGNALS = 1,   /* stop and pending bits of the cell colour */
  TS_RL_RAIN = 2,      /* rain bit of the cell colour */
  TS_RL_VEHICLES = 4,
  TS_RL_HEAT = 8,
  TS_RL_ROUTES = 16,
  TS_RL_ALL = 31
};

enum {
  TS_RENDER_MAX_TYPES = 64,
  TS_RENDER_MAX_ROUTES = 4096,
  TS_RENDER_MAX_SCALE = 64,
  TS_RENDER_MAX_SIDE = 8192,
  TS_RENDER_DEFAULT_RADIUS = 169 /* the reference's r = 0.66 */
};

typedef struct TsRenderView {
  int32_t x0, y0, cells_w, cells_h; /* the viewed rectangle of cells (cells_w, cells_h >= 1; |x0|, |y0| <= 2^24); it may extend past the map */
  int32_t zoom;                     /* 1..64 pixels per cell */
  int32_t shrink;                   /* 1..64 cells per pixel; at most one of zoom and shrink is above 1 */
  uint32_t layers;                  /* TS_RL_* bits; cells are always drawn */
  int32_t flip_y;
  int32_t heat_plane;               /* TS_OBS_* index, or TS_OBS_NPLANES for flow (read under TS_RL_HEAT only) */
  uint32_t heat_max;                /* > 0 (under TS_RL_HEAT) */
  int32_t vehicle_radius_256;       /* 0..65535, radius in 1/256 of a cell */
  uint8_t background[4];
} TsRenderView;

typedef struct TsRenderInfo {
  int32_t n_types;             /* 0: ts_render_set_cells has not been called */
  int32_t has_vehicle_palette;
  int32_t has_heat_lut;
  int32_t n_routes;
  int32_t last_w, last_h;      /* pixels of the last frame (0: none yet) */
  int64_t frames;              /* frames rendered */
  uint64_t device_bytes;       /* device memory held by tables, the dynamic plane and the frame buffer */
} TsRenderInfo;

/* type_plane[height][width], every code < n_types; cell_palette[n_types][2 pend][2 stop][2 rain][4] RGBA. */
int ts_render_set_cells(ts_handle h, const uint8_t* type_plane, int32_t n_types, const uint8_t* cell_palette);

/* pal[3 kind][4 status][2 flash][4] RGBA. */
int ts_render_set_vehicle_palette(ts_handle h, const uint8_t* pal);

/* lut[256][4] RGBA, A = blend weight. */
int ts_render_set_heat_lut(ts_handle h, const uint8_t* lut);

/* The vehicles whose remaining paths TS_RL_ROUTES draws, by spawn index; n = 0 clears the list.  Vehicles no longer alive
 * are skipped at render time. */
int ts_render_set_routes(ts_handle h, int32_t n, const int32_t* spawn_idx, const uint8_t rgba[4]);

/* Frame size of a view (no handle: pure arithmetic).  TS_E_INVALID for a bad view, TS_E_CAPACITY above the size limit. */
int ts_render_size(const TsRenderView* v, int32_t* out_w, int32_t* out_h);

/* Render into host memory: dst[out_h][out_w][4]. */
int ts_render(ts_handle h, const TsRenderView* v, uint8_t* dst);

/* Render into the engine's own frame buffer (grown on demand) and return its device pointer; the frame is complete when the
 * call returns.  Valid until the next ts_render / ts_render_device or ts_destroy. */
int ts_render_device(ts_handle h, const TsRenderView* v, void** ptr);

int ts_render_info(ts_handle h, TsRenderInfo* out);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_RENDER_H */
