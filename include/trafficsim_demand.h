/*
 * trafficsim_demand.h - route demand: the planned load per cell and direction of every live vehicle's remaining route,
 * computed on the device.
 *
 * An engine-side extension of trafficsim.h (the reference keeps no such maps).  Implemented by libtrafficsim_hip.so
 * only; the CPU oracle has no route demand.
 *
 * A plane is uint32_t[height][width], row-major, indexed [y * width + x] like every map of trafficsim.h.  A result holds
 * n_bins * 4 planes, [bin][direction].
 *
 * What is counted
 *   - the vehicles are the rows of ts_download_vehicles at the time of the call (parked and servicing vehicles count),
 *     or those of them whose byte in the query's `select` array (indexed by spawn index) is not 0.
 *   - the cells of a vehicle are exactly what ts_download_path returns for it now: its remaining main path, without the
 *     cell it stands on, step k = 0 being its next cell.  Auxiliary overtake and detour paths do not count
 *     (ts_download_path does not return them either).
 *   - every planned step into cell c in direction d (N 0, E 1, S 2, W 3, as in the TS_OBS_ENTER planes: N is
 *     cell + width) adds 1 to plane [bin][d] at c.  A route that visits a cell twice counts twice.
 *   - for k < n_bins * bin_cells the bin is k / bin_cells.  A later step goes to the last bin when open_tail is set and
 *     is not counted otherwise.  n_bins = 1 with open_tail = 1 is the whole remaining path.
 *   - TsDemandInfo::steps and ::bin_steps are the sums of the planes (all of them / the four of a bin), formed while the
 *     planes are; ::vehicles is the number of vehicles counted (selected rows, whatever the length of their paths).
 *
 * The result is a snapshot of the state between two ts_step calls: ts_step neither updates nor clears it, and
 * TsDemandInfo::tick says which tick (TsCounters::step_count) it belongs to.  Computing it changes nothing a run
 * computes: maps, vehicle rows, groups, counters and both RNG streams are bit for bit the same with or without.
 *
 * Demand and checkpoints (trafficsim_checkpoint.h)
 *   - the result is not simulation state and not part of a checkpoint: ts_checkpoint_save gives identical bytes before
 *     and after a compute.
 *   - ts_checkpoint_load leaves the result of the target as it is.
 *   - a handle built from a checkpoint starts without a result, like every new handle.
 *
 * Sharded mode (ts_set_replan_sharding): vehicle state and paths are replicated, so every rank computes identical
 * planes; nothing is exchanged.
 *
 * Calls
 *   - only between ts_step calls, from the handle's caller thread (trafficsim.h conventions).
 *   - TS_E_STATE    a read (download, pooled, groups, device) before any compute, or after ts_demand_release.
 *   - TS_E_INVALID  a null pointer, a bin, direction or factor out of range, a query outside its limits, n_select other
 *                   than ts_num_spawned.
 *   - TS_E_DEVICE   the planes could not be allocated.
 *   A compute that is refused, for whatever reason, leaves the previous result readable and unchanged.  (A compute with
 *   the n_bins of the result held reuses its planes; one with another n_bins allocates the new planes before it frees
 *   the old.  Only a device failure under an accepted call - the TS_E_DEVICE of a broken device - can lose a result.)
 *
 * TS_DEBUG_DEMAND_CHUNK=n (read by ts_demand_compute) sets the number of path steps a team of lanes covers per
 * iteration (1..65536, rounded up to a multiple of the team), so that a small test walks the multi-iteration form.
 * Results do not depend on it.
 */
#ifndef TRAFFICSIM_DEMAND_H
#define TRAFFICSIM_DEMAND_H

#include "trafficsim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TS_DEMAND_MAX_BINS = 8 };

/* ts_demand_groups: one row per light group and bin, field for field beside TS_OG_* / the external light state */
enum {
  TS_DG_NS_IN = 0,   /* the direction-summed plane over the group's ns_in approach cells */
  TS_DG_EW_IN = 1,   /* ... over its ew_in approach cells */
  TS_DG_ENTER_N = 2, /* the four direction planes over the group's intersection_cells */
  TS_DG_ENTER_E = 3,
  TS_DG_ENTER_S = 4,
  TS_DG_ENTER_W = 5,
  TS_DG_NFIELDS = 6
};

typedef struct TsDemandQuery {
  int32_t n_bins;           /* 1..TS_DEMAND_MAX_BINS */
  int32_t bin_cells;        /* path steps per bin, at least 1 */
  int32_t open_tail;        /* 1: steps beyond the last bin count in the last bin; 0: they are not counted */
  int32_t n_select;         /* with select: its length, which must be ts_num_spawned; without: ignored */
  int32_t select_on_device; /* 1: select is device memory of the engine's device */
  int32_t reserved;         /* 0 */
  const uint8_t* select;    /* NULL: every vehicle; else one byte per spawn index, not 0 = counted */
} TsDemandQuery;

typedef struct TsDemandInfo {
  int32_t n_bins, bin_cells, open_tail; /* the query of the result held; all 0: there is none */
  int32_t selected;                     /* 1: it was computed with a select array */
  int32_t width, height;
  int64_t tick;     /* TsCounters::step_count at the compute */
  int64_t vehicles; /* vehicles counted */
  uint64_t steps;   /* sum of all planes */
  uint64_t bin_steps[8]; /* sum of the four planes of every bin */
  uint64_t device_bytes; /* device memory held by the planes */
} TsDemandInfo;

/* Compute the demand of the engine's current state and make it the result, in place of the previous one.  `out` may be
 * NULL; otherwise it receives what ts_demand_info would. */
int ts_demand_compute(ts_handle h, const TsDemandQuery* q, TsDemandInfo* out);

/* Never TS_E_STATE: without a result everything but width and height is 0. */
int ts_demand_info(ts_handle h, TsDemandInfo* out);

/* Copy one plane to host memory: dst[height * width].  dir 0..3, or -1: the sum of the four, added on the device. */
int ts_demand_download(ts_handle h, int32_t bin, int32_t dir, uint32_t* dst);

/* The plane (dir as above) summed over factor x factor blocks on the device:
 * dst[ceil(height / factor)][ceil(width / factor)], row-major; blocks at the right and top edge are partial. */
int ts_demand_pooled(ts_handle h, int32_t bin, int32_t dir, int32_t factor, uint64_t* dst);

/* rows[ts_num_groups][n_bins][TS_DG_NFIELDS], over the CSR tables ts_observe_groups and ts_lights_ext_observe use. */
int ts_demand_groups(ts_handle h, int64_t* rows);

/* Device pointer of a plane (uint32_t[height * width], dir 0..3), owned by the engine; valid until the next
 * ts_demand_compute, ts_demand_release or ts_destroy.  The call waits for the engine's stream. */
int ts_demand_device(ts_handle h, int32_t bin, int32_t dir, void** ptr);

/* Free the planes; there is no result afterwards.  TS_OK when there was none. */
int ts_demand_release(ts_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TRAFFICSIM_DEMAND_H */
