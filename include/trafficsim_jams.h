/*
 * trafficsim_jams.h - jam detection: the queues of standing vehicles as connected components of the grid, labelled on the
 * device between two ticks, with one record per jam, the jam of every vehicle and one row per light group.
 *
 * An engine-side extension of trafficsim.h (the reference keeps no such tables).  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no jam detection.
 *
 * The rule
 *   - a standing vehicle is a row of ts_download_vehicles at the time of the call with stuck_ticks >= min_ticks and
 *     (flags & TS_F_PARKED) == 0.  At min_ticks = 1 this is exactly the rule of the TS_OBS_WAITING plane.
 *   - the count plane (uint32[height][width]): with TS_JAM_VEHICLES the number of standing vehicles on the cell; with
 *     TS_JAM_MASK the caller's byte for the cell (0..255) - the compute then reads no vehicle.
 *   - a standing cell is a cell whose count is greater than 0.
 *   - two standing cells u and v that are 4-neighbours, d being the direction u -> v (N 0 = cell + width, E 1, S 2, W 3, as
 *     in the TS_OBS_ENTER planes; the allowed_dirs_map bits are N 1, E 2, S 4, W 8), are linked
 *       TS_JAM_GRID  always;
 *       TS_JAM_FLOW  when allowed_dirs[u] has d or allowed_dirs[v] has the opposite of d.  Lanes of opposite directions
 *                    that lie side by side do not merge; a standing vehicle on a cell without flow bits whose neighbours
 *                    do not point at it is a jam of its own.
 *     Diagonal neighbours are never linked.
 *   - a jam is a connected component of standing cells under the links.  Its root is its smallest cell index
 *     y * width + x; jams are numbered 0 .. n_jams - 1 by ascending root.  The result is canonical: it does not depend on
 *     the order in which threads ran, nor on TS_DEBUG_JAMS_TILE.
 *
 * Per jam (TsJamRecord, ts_jams_records): the root, the number of cells, the sum of their counts, the inclusive bounding
 * box, extent = max(x1 - x0, y1 - y0) + 1, the cells with the intersection bit (a blocked box), and the largest and the
 * summed stuck_ticks over the jam's standing vehicles (both 0 in mask mode).
 *
 * Per vehicle, by spawn index over the ts_num_spawned of the compute (ts_jams_vehicles): int32 jam, the jam of the cell a
 * standing vehicle stands on; -1 for every other index, and -1 everywhere in mask mode.
 *
 * Planes (ts_jams_download): TS_JAM_PLANE_LABEL int32, the jam number, -1 where there is none; TS_JAM_PLANE_COUNT uint32.
 *
 * Per light group (ts_jams_groups): int64 rows[ts_num_groups][TS_JG_NFIELDS], over the CSR tables ts_observe_groups and
 * ts_demand_groups use.  For each axis (the ns_in cells, then the ew_in cells) take the distinct jams with at least one
 * cell in the list: their number, the sum of their cells, the sum of their vehicles, the largest stuck_max, the largest
 * extent.  A jam counts once per (group, axis), however many of the list's cells it covers.  The sums include the whole
 * queue behind the approach cells, which waiting_ns / waiting_ew of the observation do not.  BOX_JAMS and BOX_CELLS are
 * the distinct jams and the standing cells among the group's intersection cells.
 *
 * The result is a snapshot.  ts_step neither updates nor clears it.  It is not simulation state and not part of a
 * checkpoint: ts_checkpoint_save gives the same bytes with and without a result, ts_checkpoint_load leaves the target's
 * result alone; a new handle has none.  Computing it changes nothing a run computes.
 *
 * Sharded mode (ts_set_replan_sharding): vehicle state is replicated, so every rank computes the same bytes and nothing
 * is exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_INVALID   a null pointer; min_ticks < 1; an unknown link or source; mask mode without a mask; a range outside
 *                    [0, n] (n = n_jams for records, n_spawned for vehicles); an unknown `which`.
 *   - TS_E_STATE     a read (records, vehicles, download, groups, device) before any compute or after ts_jams_release.
 *                    ts_jams_info is never TS_E_STATE.
 *   - TS_E_DEVICE    no device memory: everything a compute needs is allocated before anything of the previous result goes.
 *   - TS_E_CAPACITY  one of the capped loops of the labelling hit its cap (a tile sweep count above T * T + 1, a find of
 *                    more than height * width hops, a union of more than height * width rounds); nothing is published.
 *   Every refused compute leaves the previous result readable and unchanged.
 *
 * TS_DEBUG_JAMS_TILE=0|8|16|32 (read by ts_jams_compute; default 0, and 0 for any other value) sets the side of the
 * tiles that are labelled in LDS before the global merge; 0 skips that stage, so that the merge does every union.  Results
 * do not depend on it.
 */
#ifndef TRAFFICSIM_JAMS_H
#define TRAFFICSIM_JAMS_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TS_JAM_GRID = 0, TS_JAM_FLOW = 1 };
enum { TS_JAM_VEHICLES = 0, TS_JAM_MASK = 1 };
/* `which` of ts_jams_download (the two planes) and of ts_jams_device (all four) */
enum { TS_JAM_PLANE_LABEL = 0, TS_JAM_PLANE_COUNT = 1, TS_JAM_RECORDS = 2, TS_JAM_VEHICLE_JAM = 3 };

/* ts_jams_groups: one row per light group, field for field beside TS_OG_* and TS_DG_* */
enum {
  TS_JG_NS_JAMS = 0,      /* distinct jams with a cell among the group's ns_in cells */
  TS_JG_NS_CELLS = 1,     /* the sum of their cells */
  TS_JG_NS_VEHICLES = 2,  /* the sum of their vehicles */
  TS_JG_NS_STUCK_MAX = 3, /* the largest of their stuck_max */
  TS_JG_NS_EXTENT = 4,    /* the largest of their extents */
  TS_JG_EW_JAMS = 5,      /* the same five over the ew_in cells */
  TS_JG_EW_CELLS = 6,
  TS_JG_EW_VEHICLES = 7,
  TS_JG_EW_STUCK_MAX = 8,
  TS_JG_EW_EXTENT = 9,
  TS_JG_BOX_JAMS = 10,    /* distinct jams with a cell among the group's intersection_cells */
  TS_JG_BOX_CELLS = 11,   /* the standing cells among them */
  TS_JG_NFIELDS = 12
};

typedef struct TsJamQuery {
  int32_t min_ticks;      /* at least 1 */
  int32_t link;           /* TS_JAM_GRID or TS_JAM_FLOW */
  int32_t source;         /* TS_JAM_VEHICLES or TS_JAM_MASK */
  int32_t mask_on_device; /* 1: `mask` is a device pointer (read on the engine's stream) */
  const uint8_t* mask;    /* TS_JAM_MASK: [height * width] bytes, the count of every cell; ignored otherwise */
} TsJamQuery;

typedef struct TsJamRecord {
  int32_t root_x, root_y; /* the jam's smallest cell */
  int32_t cells;
  uint32_t vehicles;      /* the sum of the counts */
  int32_t x0, y0, x1, y1; /* the inclusive bounding box */
  int32_t extent;         /* max(x1 - x0, y1 - y0) + 1 */
  int32_t inter_cells;    /* cells with the intersection bit */
  int32_t stuck_max;      /* over the jam's standing vehicles; 0 in mask mode */
  int32_t reserved;       /* 0 */
  int64_t stuck_sum;      /* ... their sum */
} TsJamRecord;

typedef struct TsJamInfo {
  int32_t min_ticks, link, source, mask_on_device; /* the query of the result held */
  int32_t held;                                    /* 1: there is a result; 0: every field but width, height is 0 */
  int32_t width, height;
  int32_t n_spawned;      /* ts_num_spawned at the compute: the length of the per-vehicle array */
  int32_t n_jams;
  int32_t standing_cells;
  int32_t largest_cells;  /* the cells of the largest jam */
  int32_t tile;           /* the tile side the result was computed with (0: no tile stage) */
  int64_t tick;           /* TsCounters::step_count at the compute */
  int64_t standing_vehicles; /* the sum of the count plane */
  uint64_t device_bytes;  /* device memory held by the result */
} TsJamInfo;

/* Label the jams of the state as it is now and make that the result, in place of the previous one.  `out` may be NULL;
 * otherwise it receives what ts_jams_info would. */
int ts_jams_compute(ts_handle h, const TsJamQuery* q, TsJamInfo* out);

/* Never TS_E_STATE: without a result `held` is 0. */
int ts_jams_info(ts_handle h, TsJamInfo* out);

/* Records first .. first + n - 1, in the jams' order. */
int ts_jams_records(ts_handle h, int32_t first, int32_t n, TsJamRecord* dst);

/* Spawn indices first .. first + n - 1 of the per-vehicle array. */
int ts_jams_vehicles(ts_handle h, int32_t first, int32_t n, int32_t* dst);

/* One plane to the host: TS_JAM_PLANE_LABEL (int32[height * width]) or TS_JAM_PLANE_COUNT (uint32[height * width]). */
int ts_jams_download(ts_handle h, int32_t which, void* dst);

/* rows[ts_num_groups][TS_JG_NFIELDS]. */
int ts_jams_groups(ts_handle h, int64_t* rows);

/* Device pointer of a plane, of the records (TsJamRecord[n_jams]) or of the per-vehicle array (int32_t[n_spawned]), owned by
 * the engine; valid until the next compute, release or ts_destroy.  Waits for the engine's stream. */
int ts_jams_device(ts_handle h, int32_t which, void** ptr);

/* Free the result.  TS_OK when there was nothing to free. */
int ts_jams_release(ts_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_JAMS_H */
