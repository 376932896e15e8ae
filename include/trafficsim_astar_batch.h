/*
 * trafficsim_astar_batch.h - the batched pathfinder operator: many A* queries in one launch, result as CSR.
 *
 * An engine-side extension of trafficsim.h, the batched twin of ts_astar (the reference's `astar_tensorflow_batch`
 * next to its single `astar`).  Implemented by libtrafficsim_hip.so only; the CPU oracle answers queries one by one.
 *
 * A query is 7 int32: sx, sy, gx, gy, soft_obstacles, ignore_flow, maximum_steps - the arguments of ts_astar in
 * ts_astar's order.  Every query is answered exactly as ts_astar would answer it on the engine's current maps
 * (astar_numba.py:243-281; field-of-view masking when the engine was created with respect_awareness); the batch only
 * changes how the searches are run: one wavefront per searcher slot takes queries off a device-side queue, and the
 * density planes and the map snapshot are built once for all of them.
 *
 * The result stays on the device as CSR in QUERY order: off[i] .. off[i + 1] are the cells of query i's path as
 * (x, y) pairs without the start cell; an empty range means "no path" (or start == goal).  Its bytes do not depend on
 * the order the searches were served or finished in.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - the result of the last batch can be fetched until the next batch or the next of exactly these calls: ts_step,
 *     ts_add_vehicles, ts_add_vehicles_dirs, ts_add_service_vehicle, ts_remove_vehicle, ts_upload_map,
 *     ts_debug_set_occupancy, ts_set_lights, ts_rain_spawn, ts_astar, ts_checkpoint_load (whether or not the call succeeds).
 *     After one of them ts_astar_batch_fetch and ts_astar_batch_device return TS_E_INVALID.  Every other entry - the
 *     read-backs (ts_counters, the ts_download_* family, ts_last_error), but also seeding, ts_set_traffic_generator,
 *     ts_set_replan_sharding, ts_group_links - leaves it fetchable: "valid" means "none of the listed calls happened",
 *     not "the maps are still what the batch saw".  The result buffers are the batch's own; nothing else writes them.
 *   - everything is validated before anything is launched; a refused batch computes nothing, moves no counter and
 *     leaves the previous result as it was.  ts_last_error names the index of the first offending query.
 *       TS_E_INVALID      n < 0, a null pointer, an endpoint out of bounds
 *       TS_E_UNSUPPORTED  a binding maximum_steps above 4094 and below width * height (the rule of ts_astar)
 *   - TS_E_CAPACITY: a search outgrew its heap or its path buffer (ts_last_error names the query); no result is kept.
 *     The failing search is not counted, but the searches of the batch that finished have moved the A* counters by then
 *     (a failing ts_astar counts nothing).
 *   - counters: every finished search adds to astar_calls / astar_expansions / astar_relaxations what the same ts_astar
 *     call adds.
 *   - like ts_astar, a batch drops the cached density planes and map snapshot afterwards: the next tick rebuilds them.
 *     With replan sharding set, a batch is answered by the rank it is called on, without an exchange.
 */
#ifndef TRAFFICSIM_ASTAR_BATCH_H
#define TRAFFICSIM_ASTAR_BATCH_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_ASTAR_QUERY_INTS 7

/* Run the n queries at `queries` (n x 7 int32, host memory); *total_cells = path cells of all of them together.
 * n == 0 is TS_OK with off = [0]. */
int ts_astar_batch(ts_handle h, int32_t n, const int32_t* queries, int64_t* total_cells);

/* Copy the last batch's result to host memory: off[n + 1], xy[total_cells][2].  xy may be null when total_cells is 0. */
int ts_astar_batch_fetch(ts_handle h, int64_t* off, int32_t* xy);

/* The last batch's result where it lies: device pointers to off[n + 1] and xy[total_cells][2], owned by the engine
 * (complete when the call returns).  Any of the four outputs may be null. */
int ts_astar_batch_device(ts_handle h, const int64_t** d_off, const int32_t** d_xy, int32_t* n, int64_t* total_cells);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_ASTAR_BATCH_H */
