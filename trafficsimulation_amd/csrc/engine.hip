// engine.hip - MI355X-native per-timestep agent-update engine (gfx950), C-ABI of include/trafficsim.h.
//
// One tick = CityModel.step() (city_model.py:1831-1860):
//   decide  : k_decide_pre  -> host MT19937 scan (data-dependent sequential stream) -> k_decide_main
//   move    : host MT19937 shuffle (model.random) -> rank per scheduled agent ->
//             rounds of { k_move_claim (per-cell min-rank claims) ; k_move_resolve } until every agent
//             has stepped.  An agent executes in the round in which no lower-ranked unresolved agent
//             touches a cell it reads or writes, which reproduces the sequential shuffled order exactly.
//   compact : stable compaction of active_vehicle_agents / schedule after despawns.
//
// State lives in HBM as structure-of-arrays; maps are (H, W) byte planes.  All arithmetic is integer
// except the float32 density map.  See DESIGN.md for the layout and the per-kernel byte counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <chrono>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <unordered_map>
#include <vector>
#include <unistd.h>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>   // host_shuffle.h: the AVX-512 draw extraction (picked at run time)
#endif

#include <hipcub/hipcub.hpp>   // the radix sort that orders a tick's replanning queue in space (run_replans)

#include "../../include/trafficsim.h"
#include "mt19937.h"

// One translation unit; this file holds no function of its own.  The order is part of the code: device headers, the host state and
// its helpers, the host subsystems (each uses what stands above it), the entries of include/trafficsim.h, checkpoints, extensions.
#include "dev.h"
#include "astar_host.h"
#include "astar.h"
#include "decide.h"
#include "replan.h"
#include "astar_quad.h"
#include "astar_batch.h"
#include "observe.h"
#include "jams.h"
#include "demand.h"
#include "selectlink.h"
#include "triplog.h"
#include "kernels.h"
#include "lights_ext.h"
#include "lights_proto.h"
#include "render.h"
#include "costfield.h"
#include "cfroute.h"
#include "host_state.h"
#include "host_shuffle.h"
#include "host_agents.h"
#include "replan_host.h"
#include "exchange.h"
#include "rng_host.h"
#include "tick.h"
#include "core_api.h"

#include "checkpoint.h"
#include "astar_batch_api.h"
#include "observe_api.h"
#include "triplog_api.h"
#include "lights_ext_api.h"
#include "lights_proto_api.h"
#include "render_api.h"
#include "demand_api.h"
#include "costfield_api.h"
#include "cfroute_api.h"
#include "selectlink_api.h"
#include "jams_api.h"
