/*
 * trafficsim_cfroute.h - routes along a cost field: the decision an optimal route takes in every state of every cell (the
 * hop plane), the routes of many starts in one launch, and the load those routes put on the network (all-or-nothing
 * assignment of a set of starts to their nearest seeds), on the device.
 *
 * An engine-side extension of trafficsim_costfield.h, whose queries, modes and step rule it shares.  Implemented by
 * libtrafficsim_hip.so only; the CPU oracle has no cost-field routes.
 *
 * ts_cfroute_compute is ts_costfield_compute - same query, same refusals, same value and owner planes, which the
 * ts_costfield_* reads see afterwards - and, while the labels of the relaxation still exist, one more kernel that writes
 * the hop plane.
 *
 * Labels
 *   L(c, p) is the 64-bit label (value << 32) | seed of the settled field in state (c, p): cell c held with heading p, p =
 *   none, N, E, S, W.  No label: the state is unreachable.
 *   - TS_CF_TO:   L(c, p) = the cheapest way from c to a seed for a vehicle that arrived at c with heading p (none: the first
 *                 step is free of the turn penalty).  A seed i offers (seed_cost[i], i) to all five states of its cell.
 *   - TS_CF_FROM: L(c, d) = the cheapest way to arrive at c moving in direction d; L(c, none) = the smallest (seed_cost[i], i)
 *                 of the seeds on c.  The label of the cell is the smallest of the five.
 *   The value and owner planes are the two halves of L(c, none) (TO) and of the cell's label (FROM).
 *   step(u, d, p) is the step rule of trafficsim_costfield.h in the kernels' half units, (base2 + turn2 * [p != none and
 *   p != d]) >> 1: an exact integer, at least 1.
 *
 * The hop plane: one uint16_t per cell, [height][width], five 3-bit fields; field k lies at bits 3k .. 3k + 2, bit 15 is 0.
 *   TS_CF_TO    field 0: state (c, none); field 1 + p: state (c, p).  The value is
 *                 4  when some seed i on c has (seed_cost[i], i) == L(c, p): the route ends here;
 *                 d  otherwise, the smallest d for which the step c -> v in direction d after heading p exists under the
 *                    query's modes and L(v, d) + step(c, d, p) == L(c, p) - both halves of the label: the route ends at
 *                    the seed that owns the state;
 *                 7  when the state has no label.
 *   TS_CF_FROM  field 0, the cell itself:
 *                 4  when L(c, none) is the cell's label (its value is its own seed's);
 *                 d  otherwise, the smallest d with L(c, d) equal to the cell's label: the heading a route arrives with;
 *                 7  when the cell has no label.
 *               field 1 + d, "arrived with heading d", the state the predecessor cell u = c - off[d] was held with:
 *                 4  when L(u, none) + step(u, d, none) == L(c, d): u is a seed, which has no heading;
 *                 h  otherwise, the smallest h with L(u, h) + step(u, d, h) == L(c, d);
 *                 7  when (c, d) has no label.
 *   With TsCostFieldInfo::headings == 1 (no turn costs anything) a cell has one label and one decision, and all five fields
 *   hold it: TO as above; FROM 4 when the cell's label is a seed's on it, else the smallest d for which the step u -> c exists
 *   and L(u) + step == L(c), else 7.  A FROM walk then reads field 0 of every cell it comes to.
 *   Every step costs at least 1, so values strictly fall along a route (TO) or back along it (FROM): following the plane
 *   ends after fewer steps than there are states.
 *
 * Routes (ts_cfroute_trace)
 *   One route per start, as direction bytes (N 0, E 1, S 2, W 3 - what ts_add_vehicles_dirs takes), CSR in start order.
 *   - TO: from the start cell, held with start_heading (-1: none), to the seed that owns that state.  cost = L(c0, p0), so
 *     without a heading it is the value plane at the start.
 *   - FROM: from the owner seed to the start cell, in travel order (the seed's first step first).  Headings must be NULL or
 *     -1.  cost and owner are the two planes at the start.
 *   - no route: cost TS_CF_UNREACHABLE, owner -1, no steps.  A start on its own seed: no steps, that seed's cost.
 *
 * Load (ts_cfroute_load)
 *   Every start sends `weight` units down its route: the step into cell c in direction d adds the weight to plane d at c -
 *   the convention of the ENTER planes of trafficsim_observe.h and of ts_demand_compute.  Four uint32_t planes
 *   [4][height][width]; a sum of weights that wraps a uint32_t cell is the caller's responsibility.  The routes are not
 *   materialised.
 *
 * None of this is simulation state: ts_step, checkpoints and handles built from them treat it like the cost field itself.
 * Sharded mode: the maps are replicated, every rank computes the same plane and routes, nothing is exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread.
 *   - ts_cfroute_compute refuses what ts_costfield_compute refuses, with the same codes; refused, it leaves the previous
 *     field, the previous hop plane and the last batch as they were.
 *   - a plain ts_costfield_compute or ts_costfield_release drops the hop plane (its field is gone); the last batch and the
 *     load planes stay readable.
 *   - TS_E_STATE     a trace, a load or the hop plane's pointer without a hop plane; a read without a batch or a load.
 *   - TS_E_INVALID   a null pointer; n outside 1..TS_CFR_MAX_STARTS; a start outside the map; a heading outside -1..3, or
 *                    other than -1 with a FROM field; a range outside the batch; `which` or `dir` out of range.
 *   - TS_E_CAPACITY  a walk left the map or took more steps than there are states (a valid plane cannot do that): nothing
 *                    is published.
 *   - TS_E_DEVICE    no device memory for the result: the previous one stays.
 */
#ifndef TRAFFICSIM_CFROUTE_H
#define TRAFFICSIM_CFROUTE_H

#include "trafficsim_costfield.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TS_CFR_STOP = 4, TS_CFR_NONE = 7 };   /* values of a hop field besides the directions 0..3 */
enum { TS_CFR_HOPS = 0, TS_CFR_OFF = 1, TS_CFR_DIRS = 2, TS_CFR_COST = 3, TS_CFR_OWNER = 4 };   /* `which` */
enum { TS_CFR_MAX_STARTS = 16777216 };

typedef struct TsCfRouteBatch {
  int32_t n;             /* routes in the batch */
  int32_t unreached;     /* starts without a route */
  int64_t steps;         /* direction bytes of all routes: off[n] */
  int64_t longest;       /* steps of the longest route */
  int64_t tick;          /* of the hop plane walked */
  uint64_t device_bytes; /* device memory held by the batch */
} TsCfRouteBatch;

typedef struct TsCfRouteLoadInfo {
  int64_t routes;        /* starts with a route (of no steps, on a seed, included) */
  int64_t unreached;     /* starts without one */
  uint64_t steps;        /* the sum of the four planes: steps of all routes, weights applied */
  int64_t tick;          /* of the hop plane walked */
  uint64_t device_bytes; /* device memory held by the four planes */
} TsCfRouteLoadInfo;

typedef struct TsCfRouteInfo {
  int32_t held;          /* 1: there is a hop plane */
  int32_t mode;          /* TS_CF_FROM or TS_CF_TO: the field it belongs to */
  int32_t headings;      /* TsCostFieldInfo::headings of that field */
  int32_t n_seeds;
  int32_t width, height;
  int64_t tick;          /* TsCounters::step_count at the compute */
  uint64_t device_bytes; /* device memory held for walking: the hop plane (2 bytes a cell), the step-cost words of the
                            compute (4 bytes a cell) and the seeds by cell */
  /* the last trace, field for field a TsCfRouteBatch; all 0 without one */
  int32_t trace_n, trace_unreached;
  int64_t trace_steps, trace_longest, trace_tick;
  uint64_t trace_device_bytes;
  /* the last load, field for field a TsCfRouteLoadInfo; all 0 without one */
  int64_t load_routes, load_unreached;
  uint64_t load_steps;
  int64_t load_tick;
  uint64_t load_device_bytes;
} TsCfRouteInfo;

/* ts_costfield_compute, and the hop plane of the field it leaves. */
int ts_cfroute_compute(ts_handle h, const TsCostFieldQuery* q, TsCostFieldInfo* out);

/* Never TS_E_STATE. */
int ts_cfroute_info(ts_handle h, TsCfRouteInfo* out);

/* The routes of n starts ((x, y) pairs; start_heading NULL: none for all) become the batch, in place of the previous one.
 * `out` may be NULL. */
int ts_cfroute_trace(ts_handle h, int32_t n, const int32_t* start_xy, const int8_t* start_heading, TsCfRouteBatch* out);

/* Routes first .. first + count - 1 of the batch; every destination may be NULL.  off[count + 1] counts from the first
 * step of route `first` (off[0] = 0), dirs receives off[count] bytes, cost and owner count elements. */
int ts_cfroute_read(ts_handle h, int32_t first, int32_t count, int64_t* off, uint8_t* dirs, uint32_t* cost, int32_t* owner);

/* The same routes as cells: xy receives off[count] (x, y) pairs, every route without its first cell (TO: the start; FROM:
 * the seed's), like ts_astar_batch; expanded on the device.  Either destination may be NULL. */
int ts_cfroute_cells(ts_handle h, int32_t first, int32_t count, int64_t* off, int32_t* xy);

/* Device pointer of the hop plane (uint16_t) or of a part of the batch (int64_t off[n + 1], uint8_t dirs, uint32_t cost[n],
 * int32_t owner[n]), owned by the engine; valid until the next compute, trace or release.  Waits for the engine's stream. */
int ts_cfroute_device(ts_handle h, int32_t which, void** ptr);

/* All-or-nothing assignment: the load of the routes of n starts (weight NULL: 1 each) becomes the load held.  `out` may be
 * NULL. */
int ts_cfroute_load(ts_handle h, int32_t n, const int32_t* start_xy, const int8_t* start_heading, const uint32_t* weight,
                    TsCfRouteLoadInfo* out);

/* dst[height * width]: plane dir (0..3), or with dir -1 the four planes summed on the device. */
int ts_cfroute_load_download(ts_handle h, int32_t dir, uint32_t* dst);

/* Device pointer of plane dir (0..3; the four lie behind one another), valid until the next load or release. */
int ts_cfroute_load_device(ts_handle h, int32_t dir, void** ptr);

/* Free the hop plane, the batch and the load planes; the cost field stays.  TS_OK when there was nothing. */
int ts_cfroute_release(ts_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_CFROUTE_H */
