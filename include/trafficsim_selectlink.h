/*
 * trafficsim_selectlink.h - select-link analysis: which planned routes cross a set of gates, when, and from where to where
 * they go, computed on the device.  Over several links at once it is screen-line or cordon analysis.
 *
 * An engine-side extension of trafficsim.h (the reference keeps no such tables).  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no select-link analysis.
 *
 * The rule
 *   - a gate is a set of (cell, direction mask) pairs.  The mask bits are N 1, E 2, S 4, W 8; a bit is the direction of
 *     the step *into* the cell, in the convention of the TS_OBS_ENTER planes and of ts_demand_compute: N is cell + width.
 *   - a set holds 1 .. TS_SL_MAX_GATES gates and up to TS_SL_MAX_CELLS cells in all.  A (cell, direction) pair belongs to at
 *     most one gate; one cell may belong to different gates for different directions (two screen lines that meet in an
 *     intersection).
 *   - the vehicles and their steps are exactly those of ts_demand_compute (trafficsim_demand.h): the vehicles are the rows
 *     of ts_download_vehicles at the time of the call, the steps of a vehicle are the cells ts_download_path returns for
 *     it now, step k = 0 being its next cell.  The cell a vehicle stands on never counts; auxiliary paths do not count.
 *   - (n_bins, bin_cells, open_tail) mean what they mean there: step k < n_bins * bin_cells is in bin k / bin_cells; a
 *     later step counts in the last bin with open_tail and does not exist for the query without it.  (1, 64, 0) asks
 *     "who comes through within the next 64 steps".
 *   - step k of vehicle v into cell c in direction d is a crossing of gate g when (c, d) belongs to g.
 *
 * Per vehicle, by spawn index (ts_selectlink_vehicles)
 *   mask        uint32  the gates it crosses (bit g: gate g)
 *   crossings   uint32  its crossings
 *   first_step  int32   the smallest counted k that is a crossing, -1 when there is none
 *   first_gate  int8    the gate of that step, -1 when there is none
 *   A spawn index that was no live vehicle at the compute reads 0 / 0 / -1 / -1.
 *
 * Totals, formed while the walk runs (ts_selectlink_tables, TsSelectLinkInfo)
 *   cross[n_gates][n_bins][4]  uint64  crossings by gate, bin and direction.  By construction cross[g][b][d] is the sum of
 *                                      demand plane [b][d] over the cells of g that accept d.
 *   pair[n_gates][n_gates]     uint64  the vehicles whose routes cross both gates; the diagonal is the vehicles crossing
 *                                      the gate.  The order of the two crossings is not kept.
 *   vehicles / crossing / crossings    the vehicles walked, those of them whose mask is not 0, the sum of cross.
 *
 * Selection (any, all, none): three gate masks.  A vehicle is selected when it was walked and
 *   (any == 0 || (mask & any)) && (mask & all) == all && (mask & none) == 0.
 * (0, 0, 0) selects every vehicle walked.  The select bytes - one per spawn index over the n_spawned of the compute, 1 for
 * selected, 0 otherwise - are what TsDemandQuery::select takes, from the host or with select_on_device = 1 through
 * ts_selectlink_device(TS_SL_SELECT): select-link load is ts_demand_compute with that mask (while ts_num_spawned is still
 * the n_spawned of the compute).  After a compute the bytes on the device hold the selection (0, 0, 0).
 *
 * The result is a snapshot.  The compute keeps a copy of the position and goal of every vehicle it walked, so every read
 * (vehicles, tables, select, od) is a function of the result and the zone plane alone, whatever the engine has done since:
 * ticks, spawns, removals, a collection of the path pool.  Computing it changes nothing a run computes.  It is not
 * simulation state and not part of a checkpoint; ts_checkpoint_load leaves gates, result and zones of the target as they
 * are; a new handle has neither gates nor a result.
 *
 * Sharded mode (ts_set_replan_sharding): vehicle state and paths are replicated, so every rank computes the same
 * result and nothing is exchanged (tests/test_gpu_ext_paths.py runs it on two ranks).
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_INVALID  a null pointer; n_gates outside 1..32; a gate_off that does not start at 0 or is not monotone; an empty
 *                   gate; more than TS_SL_MAX_CELLS cells; a cell outside the map; a direction mask of 0 or above 15; a
 *                   (cell, direction) claimed twice, inside one gate or by two; a query outside ts_demand_compute's limits;
 *                   a range outside [0, n_spawned at the compute]; a selection bit at or above n_gates; `which` out of
 *                   range; n_zones outside 0..1024.
 *   - TS_E_STATE    a compute before any gates; a read (tables, vehicles, select, od, device other than TS_SL_GATES) before
 *                   a compute, after a ts_selectlink_set_gates or after ts_selectlink_release; od without a zone plane;
 *                   device(TS_SL_GATES) without gates.
 *   - TS_E_DEVICE   no device memory: everything a call needs is allocated before anything of the previous gates or
 *                   result goes.
 *   A refused call leaves gates, result and zones as they were.  A ts_selectlink_set_gates that succeeds drops the result.
 *
 * TS_DEBUG_SELECTLINK_TEAM=8|16|32|64 and TS_DEBUG_SELECTLINK_CHUNK=n (read by ts_selectlink_compute) set the lanes per
 * vehicle and the path steps a team covers per iteration (1..65536, rounded up to a multiple of the team).  Results depend
 * on neither.
 */
#ifndef TRAFFICSIM_SELECTLINK_H
#define TRAFFICSIM_SELECTLINK_H

#include "trafficsim_demand.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TS_SL_MAX_GATES = 32, TS_SL_MAX_CELLS = 1048576, TS_SL_MAX_ZONES = 1024 };
enum { TS_SL_DIR_N = 1, TS_SL_DIR_E = 2, TS_SL_DIR_S = 4, TS_SL_DIR_W = 8, TS_SL_DIR_ALL = 15 };
/* `which` of ts_selectlink_device */
enum { TS_SL_MASK = 0, TS_SL_FIRST_STEP = 1, TS_SL_FIRST_GATE = 2, TS_SL_CROSSINGS = 3, TS_SL_SELECT = 4, TS_SL_GATES = 5 };

typedef struct TsSelectLinkQuery {
  int32_t n_bins;    /* 1..TS_DEMAND_MAX_BINS */
  int32_t bin_cells; /* path steps per bin, at least 1 */
  int32_t open_tail; /* 1: steps beyond the last bin count in the last bin; 0: they do not exist for this query */
  int32_t reserved;  /* 0 */
} TsSelectLinkQuery;

typedef struct TsSelectLinkInfo {
  int32_t n_gates, n_gate_cells;        /* the gates held; both 0: there are none */
  int32_t held;                         /* 1: there is a result; 0: the query, n_spawned, tick and the three totals are 0 */
  int32_t n_bins, bin_cells, open_tail; /* the query of the result held */
  int32_t n_spawned;                    /* ts_num_spawned at the compute: the length of the per-vehicle arrays */
  int32_t n_zones;                      /* of the zone plane held, 0: none */
  int32_t width, height;
  int64_t tick;          /* TsCounters::step_count at the compute */
  int64_t vehicles;      /* vehicles walked */
  int64_t crossing;      /* vehicles whose mask is not 0 */
  uint64_t crossings;    /* sum of cross */
  uint64_t device_bytes; /* device memory held by the gate plane, the result, the totals and the zone plane */
} TsSelectLinkInfo;

/* Make n_gates gates the set held, in place of the previous one: gate g is cells gate_off[g] .. gate_off[g + 1] - 1 of
 * cells_xy ((x, y) pairs) with their dir_mask bytes.  The checks run on the host before the device is touched.  Drops the
 * result. */
int ts_selectlink_set_gates(ts_handle h, int32_t n_gates, const int32_t* gate_off, const int32_t* cells_xy, const uint8_t* dir_mask);

/* Walk every live vehicle's remaining main path over the gates held and make that the result, in place of the previous
 * one.  `out` may be NULL; otherwise it receives what ts_selectlink_info would. */
int ts_selectlink_compute(ts_handle h, const TsSelectLinkQuery* q, TsSelectLinkInfo* out);

/* Never TS_E_STATE: without gates, a result or zones their fields are 0. */
int ts_selectlink_info(ts_handle h, TsSelectLinkInfo* out);

/* cross[n_gates][n_bins][4] and pair[n_gates][n_gates]; either may be NULL. */
int ts_selectlink_tables(ts_handle h, uint64_t* cross, uint64_t* pair);

/* Spawn indices first .. first + n - 1 of the per-vehicle arrays; any destination may be NULL. */
int ts_selectlink_vehicles(ts_handle h, int32_t first, int32_t n, uint32_t* mask, int32_t* first_step, int8_t* first_gate, uint32_t* crossings);

/* Form the select bytes of (any, all, none) on the device, where they stay; dst (host, n_spawned bytes) and count (the
 * number selected) may be NULL. */
int ts_selectlink_select(ts_handle h, uint32_t any, uint32_t all, uint32_t none, uint8_t* dst, int64_t* count);

/* ts_triplog_set_zones' contract with a plane of its own: int32[height * width], -1 = no zone, else 0 .. n_zones - 1;
 * n_zones is 1 .. TS_SL_MAX_ZONES; n_zones = 0 drops the plane (zone_of_cell may be NULL then). */
int ts_selectlink_set_zones(ts_handle h, const int32_t* zone_of_cell, int32_t n_zones);

/* counts[n_zones][n_zones]: the selected vehicles by [zone(cell at the compute)][zone(goal at the compute)].  A selected
 * vehicle with either end outside every zone adds 1 to *unzoned (may be NULL) and nothing to counts. */
int ts_selectlink_od(ts_handle h, uint32_t any, uint32_t all, uint32_t none, int64_t* counts, int64_t* unzoned);

/* Device pointer of a per-vehicle array (uint32_t mask[n_spawned], int32_t first_step, int8_t first_gate, uint32_t
 * crossings, uint8_t select) or of the gate plane (uint32_t[height * width]: byte d = 1 + the gate of a step entering in
 * direction d, 0 = none), owned by the engine; valid until the next set_gates, compute, release or ts_destroy.  Waits for
 * the engine's stream. */
int ts_selectlink_device(ts_handle h, int32_t which, void** ptr);

/* Free gates, result and zone plane.  TS_OK when there was nothing to free. */
int ts_selectlink_release(ts_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_SELECTLINK_H */
