/*
 * trafficsim_costfield.h - cost fields: the travel cost from a set of seed cells to every cell of the map, or from every
 * cell to the nearest seed, with the seed that attains it (a catchment), computed on the device.
 *
 * An engine-side extension of trafficsim.h (the reference answers one pair per search).  Implemented by
 * libtrafficsim_hip.so only; the CPU oracle has no cost field.
 *
 * A plane is [height][width], row-major, indexed [y * width + x] like every map of trafficsim.h: the value plane is
 * uint32_t, the owner plane int32_t.
 *
 * Maps
 *   the ones ts_astar would see if it were called now: a fresh density map from the current occupancy, the occupancy and
 *   stop maps as they are, the static planes.  Like ts_astar and ts_astar_batch a compute drops the cached density planes
 *   and the A* snapshot afterwards; it does not move the A* counters.
 *
 * Step rule (astar_numba.py:171-226 on TsParams)
 *   A step goes from cell u = (x, y) in direction d (N 0: y + 1, E 1: x + 1, S 2: y - 1, W 3: x - 1) to v; p is the
 *   previous heading, -1 for none.
 *   - v outside the map: no step.
 *   - c = 1.
 *   - c += turn_penalty when turn_penalty_enabled and p != -1 and d != p.
 *   - when allowed_dirs_map[u] lacks bit d: with ignore_flow and is_road_map[v] == 1, c += contraflow_penalty;
 *     otherwise no step.
 *   - unless free_flow:
 *       occupancy[v] == 1: soft, c += int(obstacle_penalty_vehicle * (1 + dynamic_penalty_scale * density[v])) under
 *                          dynamic_penalties_enabled, else c += obstacle_penalty_vehicle; strict, no step.
 *       stop[v] == 1:      soft, c += obstacle_penalty_stop; strict, no step.
 *   - when road_type_penalties_enabled and is_road_map[v] == 1: c += the penalty of road_type_map[v].
 *   - the step costs int(c), the integer the reference stores into `dist` (for an integer g, int(g + c) = g + int(c): with
 *     R1 = 0.5 a step onto an R1 road costs 1).
 *   The cost of a path is the sum of its step costs; its first step has p = -1.
 *
 * Field values
 *   - TS_CF_FROM: value(c) = min over seeds s and paths s -> c of seed_cost[s] + cost(path).
 *   - TS_CF_TO:   value(c) = min over seeds s and paths c -> s of cost(path) + seed_cost[s].
 *   - a path of no steps counts: a seed's value is at most its seed_cost.
 *   - the heading is part of the state: the minimum is exact over (cell, heading), which the reference's A* is not when
 *     turns cost something (its paths can cost more than the field says, never less).
 *   - a value of 0x3F3F3F3F or more (the reference's INF), or above a non-zero max_cost, is unreachable: TS_CF_UNREACHABLE.
 *   - owner(c) is the smallest seed index among the seeds that attain value(c), -1 where c is unreachable.  Several seeds
 *     may share a cell.
 *
 * The result is a snapshot and not simulation state: ts_step neither updates nor clears it (TsCostFieldInfo::tick says
 * which tick it belongs to), ts_checkpoint_save gives identical bytes with and without it, ts_checkpoint_load leaves it
 * alone, a handle built from a checkpoint starts without one.  Computing it changes nothing a run computes.
 *
 * Sharded mode (ts_set_replan_sharding): the maps are replicated, so every rank computes identical planes; nothing is
 * exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_UNSUPPORTED  parameters whose penalties are not all multiples of 0.5 (the kernels work in half units, as the
 *                       quad searcher does); an engine created with respect_awareness unless the query has free_flow (a
 *                       field has no single start to cast a field of view from).
 *   - TS_E_INVALID      a null pointer; n_seeds < 1 or above TS_CF_MAX_SEEDS; a seed outside the map; a seed_cost that is
 *                       negative or 0x3F3F3F3F or more; a mode or flag other than those below, reserved other than 0; a
 *                       `which` other than 0 or 1; a gathered cell outside the map; thresholds that descend, or more than
 *                       TS_CF_MAX_BANDS of them.
 *   - TS_E_STATE        a read (download, gather, bands, device) before any compute, or after ts_costfield_release.
 *   - TS_E_CAPACITY     the relaxation did not settle within as many rounds as there are states (values only decrease, so
 *                       this cannot happen).
 *   A compute that is refused, for whatever reason, leaves the previous result readable and unchanged.
 *
 * TS_DEBUG_COSTFIELD_TILE=8|16|32 (read by ts_costfield_compute; default and every other value: 32) sets the side of the
 * tiles a workgroup relaxes, so that a small map spans many tiles.  Results do not depend on it.
 */
#ifndef TRAFFICSIM_COSTFIELD_H
#define TRAFFICSIM_COSTFIELD_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TS_CF_FROM = 0, TS_CF_TO = 1 };
enum { TS_CF_VALUE = 0, TS_CF_OWNER = 1 };   /* `which` */
enum { TS_CF_MAX_SEEDS = 1048576, TS_CF_MAX_BANDS = 1024 };
#define TS_CF_UNREACHABLE 0xFFFFFFFFu

typedef struct TsCostFieldQuery {
  int32_t mode;           /* TS_CF_FROM or TS_CF_TO */
  int32_t soft_obstacles; /* 1: occupied and red cells cost their penalties; 0: they cannot be entered */
  int32_t ignore_flow;    /* 1: steps against the flow onto road cells, at contraflow_penalty */
  int32_t free_flow;      /* 1: occupancy and stop are not looked at */
  uint32_t max_cost;      /* 0: none; else values above it are unreachable */
  int32_t n_seeds;        /* 1..TS_CF_MAX_SEEDS */
  const int32_t* seed_xy;   /* n_seeds (x, y) pairs */
  const int32_t* seed_cost; /* NULL: all 0; else n_seeds costs in [0, 0x3F3F3F3F) */
  int64_t reserved;       /* 0 */
} TsCostFieldQuery;

typedef struct TsCostFieldInfo {
  int32_t mode, soft_obstacles, ignore_flow, free_flow; /* the query of the result held */
  uint32_t max_cost;
  int32_t n_seeds;       /* 0: there is no result */
  int32_t width, height;
  int32_t tile;          /* side of the tiles the compute relaxed */
  int32_t headings;      /* states per cell: 4 when turns cost something, else 1 */
  int64_t tick;          /* TsCounters::step_count at the compute */
  int64_t reached;       /* cells with a finite value */
  uint32_t max_value;    /* the largest finite value, 0 when nothing was reached */
  int32_t rounds;        /* launches of the tile kernel */
  int64_t tile_visits;   /* tiles relaxed, summed over the rounds */
  uint64_t device_bytes; /* device memory held by the two planes */
} TsCostFieldInfo;

/* Compute the field of the engine's current maps and make it the result, in place of the previous one.  `out` may be NULL;
 * otherwise it receives what ts_costfield_info would. */
int ts_costfield_compute(ts_handle h, const TsCostFieldQuery* q, TsCostFieldInfo* out);

/* Never TS_E_STATE: without a result everything but width and height is 0. */
int ts_costfield_info(ts_handle h, TsCostFieldInfo* out);

/* Copy a plane to host memory: dst[height * width], uint32_t values (which 0) or int32_t owners (which 1). */
int ts_costfield_download(ts_handle h, int32_t which, void* dst);

/* Read n cells of a plane on the device: xy holds n (x, y) pairs, out receives n 4-byte elements of the plane's type. */
int ts_costfield_gather(ts_handle h, int32_t which, int32_t n, const int32_t* xy, void* out);

/* Isochrone areas: counts[k] = the number of road cells (is_road_map == 1) whose value is <= thresholds[k], reduced on the
 * device.  The thresholds ascend (equal neighbours are allowed); 1..TS_CF_MAX_BANDS of them. */
int ts_costfield_bands(ts_handle h, int32_t n, const uint32_t* thresholds, uint64_t* counts);

/* Device pointer of a plane, owned by the engine; valid until the next ts_costfield_compute, ts_costfield_release or
 * ts_destroy.  The call waits for the engine's stream. */
int ts_costfield_device(ts_handle h, int32_t which, void** ptr);

/* Free the planes; there is no result afterwards.  TS_OK when there was none. */
int ts_costfield_release(ts_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_COSTFIELD_H */
