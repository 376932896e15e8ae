/*
 * trafficsim_observe.h - traffic observation: per-cell flow, presence and delay accumulated on the device.
 *
 * An engine-side extension of trafficsim.h (the reference keeps no such maps).  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no observation.
 *
 * A plane is uint32_t[height][width], row-major, indexed [y * width + x] like every map of trafficsim.h.  Planes only
 * ever grow (until ts_observe_reset); a sum wraps at 2^32.
 *
 *   TS_OBS_PRESENT    +1 at the cell of every live vehicle at the end of every tick.  A live vehicle is exactly a row
 *                     ts_download_vehicles would return after that tick: parked and servicing vehicles count, vehicles
 *                     removed in the tick do not.
 *   TS_OBS_WAITING    +1 for every such vehicle with stuck_ticks > 0 and without TS_F_PARKED: vehicle-ticks spent
 *                     standing in traffic.
 *   TS_OBS_SPEED      + current_speed of every such vehicle.  Mean speed of a cell is SPEED / PRESENT.
 *   TS_OBS_ENTER_N/_E/_S/_W
 *                     +1 at a cell every time a vehicle is moved into it, by the direction of that step (N 0, E 1, S 2,
 *                     W 3, the engine's codes: N is cell + width).  A move of k cells in one tick adds k increments, one
 *                     at every cell on the way.  Over any run the four planes together grow by exactly what the vehicles'
 *                     steps_traveled grow by.
 *
 * Observation never changes what a run computes: maps, vehicle rows, groups, counters and both RNG streams are bit for
 * bit the same with observation on, off, or started half-way.
 *
 * Observation and checkpoints (trafficsim_checkpoint.h)
 *   - observation is not simulation state and not part of a checkpoint: ts_checkpoint_save gives identical bytes with
 *     observation on or off.
 *   - ts_checkpoint_load leaves the mask, the planes and the tick count of the target as they are (rewinding a run does
 *     not rewind what was observed of it).
 *   - a handle built from a checkpoint starts with observation off, like every new handle.
 *
 * Sharded mode (ts_set_replan_sharding): the move phase is replicated, so every rank holds identical planes; nothing is
 * exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_STATE    observation has not been started, or a plane the call needs is not in the mask.
 *   - TS_E_INVALID  a null pointer, a plane index or mask out of range, factor < 1, n < 0.
 *   - TS_E_DEVICE   the planes could not be allocated.  The engine keeps running, with observation off.
 */
#ifndef TRAFFICSIM_OBSERVE_H
#define TRAFFICSIM_OBSERVE_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TS_OBS_PRESENT = 0,
  TS_OBS_WAITING = 1,
  TS_OBS_SPEED = 2,
  TS_OBS_ENTER_N = 3,
  TS_OBS_ENTER_E = 4,
  TS_OBS_ENTER_S = 5,
  TS_OBS_ENTER_W = 6,
  TS_OBS_NPLANES = 7
};
#define TS_OBS_ALL ((1u << TS_OBS_NPLANES) - 1u)

/* ts_observe_groups: one row per light group */
enum {
  TS_OG_NS_WAITING = 0, /* WAITING summed over the group's ns_in cells */
  TS_OG_NS_PRESENT = 1, /* PRESENT over the ns_in cells */
  TS_OG_EW_WAITING = 2, /* WAITING over the ew_in cells */
  TS_OG_EW_PRESENT = 3, /* PRESENT over the ew_in cells */
  TS_OG_ENTER_N = 4,    /* the four ENTER planes over the group's intersection_cells */
  TS_OG_ENTER_E = 5,
  TS_OG_ENTER_S = 6,
  TS_OG_ENTER_W = 7,
  TS_OG_NFIELDS = 8
};

typedef struct TsObserveInfo {
  uint32_t plane_mask; /* bit p set: plane p is held (0: observation is off) */
  int32_t width, height;
  int64_t ticks;        /* ticks observed since ts_observe_start / ts_observe_reset */
  uint64_t device_bytes; /* device memory held by the planes */
} TsObserveInfo;

/* Allocate and zero the planes of plane_mask (bit p = plane p, at least one) and observe from the next tick on.  A call
 * while observation is on frees the old planes first: the new ones start from zero, whatever the masks. */
int ts_observe_start(ts_handle h, uint32_t plane_mask);

/* Free the planes; observation is off afterwards.  TS_OK when it was off already. */
int ts_observe_stop(ts_handle h);

/* Zero the planes and the tick count; the mask stays. */
int ts_observe_reset(ts_handle h);

/* Never TS_E_STATE: with observation off the mask, ticks and bytes are 0. */
int ts_observe_info(ts_handle h, TsObserveInfo* out);

/* Copy one whole plane to host memory: dst[height * width]. */
int ts_observe_download(ts_handle h, int32_t plane, uint32_t* dst);

/* The plane summed over factor x factor blocks on the device: dst[ceil(height / factor)][ceil(width / factor)], row-major;
 * blocks at the right and top edge are partial. */
int ts_observe_pooled(ts_handle h, int32_t plane, int32_t factor, uint64_t* dst);

/* Sums over n rectangles: rects[n][4] = x0, y0, x1, y1, half-open, clipped to the map (an empty or inverted rectangle
 * sums to 0). */
int ts_observe_regions(ts_handle h, int32_t plane, int32_t n, const int32_t* rects, uint64_t* sums);

/* rows[ts_num_groups][TS_OG_NFIELDS].  Needs PRESENT, WAITING and the four ENTER planes in the mask. */
int ts_observe_groups(ts_handle h, int64_t* rows);

/* Device pointer of a plane (uint32_t[height * width]), owned by the engine; valid until the next ts_observe_start,
 * ts_observe_stop or ts_destroy.  The call waits for the engine's stream: the planes are complete when it returns. */
int ts_observe_device(ts_handle h, int32_t plane, void** ptr);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_OBSERVE_H */
