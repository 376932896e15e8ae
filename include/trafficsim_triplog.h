/*
 * trafficsim_triplog.h - the trip log: one record per vehicle that leaves the simulation, kept on the device, and
 * origin / destination (OD) sums over the log.
 *
 * An engine-side extension of trafficsim.h (the reference keeps no such log).  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no trip log.
 *
 * A record is written when a vehicle is removed: when it arrives (on_target_reached -> _despawn), when _despawn_check
 * gives it up, or when the host calls ts_remove_vehicle.  Vehicles that park and stay produce none; a service vehicle
 * produces one, when it finally leaves at its exit.
 *
 * Order.  Records appear in groups, in the order the groups happened: one group per tick that removed anything, one per
 * ts_remove_vehicle between ticks.  Inside a group the records are in ascending spawn_idx.  The order does not depend on
 * thread scheduling: two identical runs give byte-identical logs.
 *
 * Capacity.  A full log drops the newest records and counts them in `dropped`; a kept record is never overwritten, so
 * which records are kept is canonical too.
 *
 * Origin.  origin_x / origin_y / spawn_step are known for the vehicles the log saw being placed.  Vehicles already alive
 * at ts_triplog_start, and all vehicles alive when ts_checkpoint_load runs on the handle, carry -1.
 *
 * The log never changes what a run computes: maps, vehicle rows, groups, counters and both RNG streams are bit for bit
 * the same with the log on, off, or started half-way.
 *
 * The log and checkpoints (trafficsim_checkpoint.h)
 *   - the log is not simulation state and not part of a checkpoint: ts_checkpoint_save gives identical bytes with the log
 *     on or off.
 *   - ts_checkpoint_load leaves the kept records and the capacity of the target as they are.
 *   - a handle built from a checkpoint starts with the log off, like every new handle.
 *
 * Sharded mode (ts_set_replan_sharding): removals happen in replicated code, so every rank holds the identical log;
 * nothing is exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_STATE    the log has not been started, or (ts_triplog_od) no zone plane is set.
 *   - TS_E_INVALID  a null pointer, a range or count out of bounds, capacity < 1.
 *   - TS_E_DEVICE   the log could not be allocated.  The engine keeps running, with the log off.
 */
#ifndef TRAFFICSIM_TRIPLOG_H
#define TRAFFICSIM_TRIPLOG_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TS_TRIP_END_ARRIVED = 0,   /* on_target_reached -> _despawn (remove_on_arrival vehicles, service vehicles at their exit) */
  TS_TRIP_END_DESPAWNED = 1, /* _despawn_check: stuck too long (counts as errored_*) */
  TS_TRIP_END_REMOVED = 2    /* ts_remove_vehicle, by the host between ticks */
};
#define TS_TRIP_END_ALL 7u   /* reason mask of ts_triplog_od: bit r = TS_TRIP_END_* value r */
#define TS_TRIPLOG_MAX_ZONES 1024

typedef struct TsTripRecord { /* 72 bytes, no padding */
  int32_t spawn_idx;
  int32_t population;         /* the vehicle's own TS_POP_* */
  int32_t vehicle_type;       /* 0 plain, TS_TRIP_SERVICE_FOOD, TS_TRIP_SERVICE_WASTE */
  int32_t end_reason;         /* TS_TRIP_END_* */
  int32_t origin_x, origin_y; /* cell it was placed on; -1, -1 = unknown */
  int32_t dest_x, dest_y;     /* its target when it left */
  int32_t end_x, end_y;       /* the cell it left from */
  int32_t spawn_step, end_step; /* TsCounters::step_count (0-based tick index) during which it was placed / left; placed or
                                   removed by the host between ticks: the number of ticks completed so far; spawn_step -1 =
                                   unknown */
  int32_t distance;           /* steps_traveled when it left */
  int32_t stuck_ticks;        /* when it left */
  double depart_elapsed;      /* the `elapsed` it was placed at (0 with enable_traffic off) */
  double end_elapsed;         /* the `elapsed` its removal saw: for an ARRIVED vehicle end_elapsed - depart_elapsed is exactly
                                 what total_duration_* grew by */
} TsTripRecord;

typedef struct TsTripLogInfo {
  int64_t capacity;      /* records the log can hold (0: the log is off) */
  int64_t count;         /* records kept */
  int64_t dropped;       /* records that found the log full */
  int64_t groups;        /* groups sealed since ts_triplog_start / ts_triplog_clear (dropped ones included) */
  uint64_t device_bytes; /* device memory held by the log */
} TsTripLogInfo;

/* Allocate a log of capacity_records records and log from now on.  A call while the log is on frees the old log first:
 * the new one starts empty. */
int ts_triplog_start(ts_handle h, int64_t capacity_records);

/* Free the log; it is off afterwards.  TS_E_STATE when it was off already. */
int ts_triplog_stop(ts_handle h);

/* Empty the log (count, dropped and groups become 0); the capacity and the zone plane stay. */
int ts_triplog_clear(ts_handle h);

/* Never TS_E_STATE: with the log off every field is 0. */
int ts_triplog_info(ts_handle h, TsTripLogInfo* out);

/* Copy records [first, first + n) clipped to count; returns how many it copied. */
int64_t ts_triplog_read(ts_handle h, int64_t first, int64_t n, TsTripRecord* out);

/* Device pointer of the record array (TsTripRecord[capacity], the first *count valid), owned by the engine; valid until the
 * next ts_triplog_start, ts_triplog_stop or ts_destroy.  The call waits for the engine's stream. */
int ts_triplog_device(ts_handle h, void** ptr, int64_t* count);

/* Upload one int32[height * width] plane (row-major like every map): the zone of every cell, -1 = no zone, else
 * 0 .. n_zones - 1.  n_zones is 1 .. TS_TRIPLOG_MAX_ZONES; n_zones = 0 drops the plane (zone_of_cell may be NULL then). */
int ts_triplog_set_zones(ts_handle h, const int32_t* zone_of_cell, int32_t n_zones);

/* Three [n_zones][n_zones] matrices, indexed [zone(origin)][zone(dest)], over all records in the log whose end_reason is
 * in reason_mask (bit r = TS_TRIP_END_* value r): number of trips, sum of end_elapsed - depart_elapsed, sum of distance.
 * A record with unknown origin, or with either end outside every zone, adds 1 to *unzoned and nothing to the matrices.
 * Any of the three matrix pointers may be NULL.  The reduction runs on the device; only the matrices come down. */
int ts_triplog_od(ts_handle h, uint32_t reason_mask, uint64_t* count, double* duration, uint64_t* distance, uint64_t* unzoned);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_TRIPLOG_H */
