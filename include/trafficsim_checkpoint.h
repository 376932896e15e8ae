/*
 * trafficsim_checkpoint.h - checkpoints of a running engine: save, restore and fork a simulation.
 *
 * An engine-side extension of trafficsim.h (the reference has no such entry: it is a plain Python object that
 * copy.deepcopy / pickle handle).  Implemented by libtrafficsim_hip.so only; the CPU oracle has no checkpoints.
 *
 * What a checkpoint is
 *   - an opaque byte blob holding ALL dynamic state of a handle between two ts_step calls: vehicles, their paths and
 *     aux paths, the cell records and the occupancy / stop / stuck / rain planes, the schedule and its keys, the light
 *     groups' state (ts_group_links' re-populated links included), both MT19937 stream positions, counters and cached
 *     stats, the traffic generator's trips and days, the rain manager and its clouds, city blocks, service vehicles
 *     and parked cells, and the spawn-time planner's path cache (city._path_cache).
 *   - it does NOT hold the static inputs.  The load target must be a handle built from the same world: the same
 *     ts_create world and TsParams, the same ts_set_lights tables and, if the source had a generator armed, the same
 *     ts_set_traffic_generator tables.  The blob's header carries fingerprints of those inputs and a load checks them.
 *   - environment switches (TS_QUAD*, TS_ASTAR_*, TS_DEBUG_*, ...) are not part of it: results do not depend on them.
 *   - identical states give byte-identical blobs: save -> load -> save reproduces the blob exactly.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - a save changes nothing the source computes afterwards.
 *   - TS_E_STATE: a save after a fatal error (a ts_step that returned the reference's exception), a save before
 *     both RNG streams are seeded, a load into a handle with replan sharding set (ts_set_replan_sharding, world > 1).
 *     Saving from a sharded rank is allowed: its state is the replicated whole.
 *   - TS_E_INVALID: a null argument, a blob with a wrong magic or format version, fingerprints that do not match
 *     the target, a short or truncated blob or a section whose size does not fit; ts_last_error says which check
 *     failed.  The target is then left exactly as it was: every check runs before anything in it is touched.
 */
#ifndef TRAFFICSIM_CHECKPOINT_H
#define TRAFFICSIM_CHECKPOINT_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exact size in bytes of a checkpoint of the handle's current state. */
int ts_checkpoint_size(ts_handle h, uint64_t* bytes);

/* Write the checkpoint to dst (cap bytes available); *written = its size.  TS_E_CAPACITY if cap is too small
 * (nothing is written then). */
int ts_checkpoint_save(ts_handle h, void* dst, uint64_t cap, uint64_t* written);

/* Replace every piece of dynamic state of h with the blob's (n bytes).  h may be a fresh handle built from the same
 * world or the source handle itself (rewind). */
int ts_checkpoint_load(ts_handle h, const void* src, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_CHECKPOINT_H */
