// astar_words.h - the words the A* searchers share, in one place: the snapshot word of a cell (Dev::amap), the tiled index it
// is stored under, k_replan's table record and the search penalties in half units (the direction deltas: path_words.h).  The three search
// loops (astar.h: the wave, astar_quad.h: the quads, astar_host.h: the host) stay three loops; this is the vocabulary they are
// written in.  Plain C++17 as well as HIP: tests/native/astar_words_check.cpp runs these functions on the host.
//
// In the search loops themselves (astar_loop, astar_wave, reach_strict_wave, quad_turn, k_replan_quad's set-up and walk) only the
// constants are used and every expression keeps its shape: a forced-inline accessor is not free there
// (profiles/device_code_diff.py shows what a change did to the kernels' code).  Cold kernels and host code use the functions.
#pragma once
#include <cstdint>
#include "arena_epochs.h"
#include "path_words.h"   // TS_WORDS_FN; the directions and their deltas (dir_dx, dir_dy)
#include "../../include/trafficsim.h"

// ---- the A* snapshot word: what a search reads about a cell, as of the last tick start (or the last ensure_amap) ------------------
// One 8-byte word per cell, in 8 x 8-tiled order (tix below: two rows of a tile are one 128-byte line, so the neighbours of a
// cell usually lie in its line or the one beside it), written by k_amap_build (and kept current by k_spawn's occupied bit).
//   low word:  bits 0-3  allowed directions (bit dd: the cell may be left in direction dd)
//              bit  4    is_road
//              bit  5    intersection
//              bits 6-7  road type        (bits 0-7: Cell::stat, the packed static byte - dev.h st_* read the same bits)
//              bit  8    occupied (occupancy_map == 1)
//              bit  9    red (stop_map == 1)
//              bits 10-31 the vehicle penalty of the cell in half units, for searches in half units (astar_half_units): the
//                        constant one, or with VEHICLE_DYNAMIC_PENALTIES the density-dependent one of this cell (density = the
//                        tick-start snapshot, so a rebuild inside the tick gives the same bits); 0 otherwise - those searches
//                        read the density map themselves
//   high word: the cell's search-node number, AM_NO_NODE = not a node.  Nodes are the cells a search can ever stand on (roads,
//              cells with flow bits, cells a flow bit points at), numbered in tiled order: k_replan's dist / came_from table has
//              one record per NODE, a quarter of one record per cell.
constexpr uint32_t AM_DIRS_MASK = 15u, AM_RT_MASK = 3u;
constexpr int AM_ROAD_BIT = 4, AM_INTER_BIT = 5, AM_RT_SHIFT = 6, AM_OCC_BIT = 8, AM_RED_BIT = 9;
constexpr uint32_t AM_BLOCKED = (1u << AM_OCC_BIT) | (1u << AM_RED_BIT);
constexpr int AM_PEN_SHIFT = 10, AM_PEN_BITS = 32 - AM_PEN_SHIFT;
constexpr uint32_t AM_NO_NODE = 0xFFFFFFFFu;
static_assert(AM_DIRS_MASK == (1u << AM_ROAD_BIT) - 1u && AM_INTER_BIT == AM_ROAD_BIT + 1 && AM_RT_SHIFT == AM_INTER_BIT + 1 &&
              ((AM_RT_MASK << AM_RT_SHIFT) | ((1u << AM_RT_SHIFT) - 1u)) == 0xFFu && AM_OCC_BIT == 8,
              "bits 0-7 of the snapshot word are Cell::stat as it is stored (dev.h st_*): the dynamic bits start at bit 8");

// the word from its low word (the ten flag bits | penalty << AM_PEN_SHIFT) and the node number; the fields of the low word
TS_WORDS_FN uint64_t am_word(uint32_t flags, uint32_t node) { return (uint64_t)flags | ((uint64_t)node << 32); }
TS_WORDS_FN uint32_t am_dirs(uint32_t a) { return a & AM_DIRS_MASK; }
TS_WORDS_FN bool am_road(uint32_t a) { return ((a >> AM_ROAD_BIT) & 1u) != 0u; }
TS_WORDS_FN bool am_inter(uint32_t a) { return ((a >> AM_INTER_BIT) & 1u) != 0u; }
TS_WORDS_FN uint32_t am_road_type(uint32_t a) { return (a >> AM_RT_SHIFT) & AM_RT_MASK; }
TS_WORDS_FN bool am_occ(uint32_t a) { return ((a >> AM_OCC_BIT) & 1u) != 0u; }
TS_WORDS_FN bool am_red(uint32_t a) { return ((a >> AM_RED_BIT) & 1u) != 0u; }
TS_WORDS_FN int am_pen2(uint32_t a) { return (int)(a >> AM_PEN_SHIFT); }
TS_WORDS_FN uint32_t am_node(uint64_t word) { return (uint32_t)(word >> 32); }

// position of cell (x, y) in the 8 x 8-tiled order of a map (or a table window) `tiles` tiles wide
TS_WORDS_FN uint32_t tix(int tiles, int x, int y) {
#ifdef __HIP_DEVICE_COMPILE__
  // (tile rows and tiles per row are far below 2^24: the full-rate 24-bit multiply)
  const uint32_t row = __umul24((uint32_t)(y >> 3), (uint32_t)tiles);
#else
  const uint32_t row = (uint32_t)(y >> 3) * (uint32_t)tiles;
#endif
  return (((row + (uint32_t)(x >> 3)) << 6) | (uint32_t)((y & 7) << 3) | (uint32_t)(x & 7));
}

// ---- k_replan's table record (astar.h TEnt; the host searcher keeps the same) -----------------------------------------------------
// 8 bytes per node: word 0 = dist, word 1 = meta = stamp << W_STAMP_SHIFT | steps << 2 | came-from direction.  The stamp is the
// epoch of the search that wrote the record (arena_epochs.h: its range, and why the quads' 4-byte records never look live here);
// a record of another epoch is stale: dist A_INF.  steps is only carried by searches with a binding step limit.
constexpr int A_INF = 0x3F3F3F3F;
constexpr uint32_t T_STEPS_SHIFT = 2, T_STEPS_MASK = 0xFFF, T_DIR_MASK = 3;
static_assert((T_DIR_MASK + 1u) == (1u << T_STEPS_SHIFT) && ((T_STEPS_MASK + 1u) << T_STEPS_SHIFT) == (1u << W_STAMP_SHIFT),
              "direction, steps and stamp fill the meta word without gaps");
TS_WORDS_FN uint64_t tent_word(int dist, uint32_t stamp, uint32_t steps, uint32_t dir) {
  return (uint64_t)(uint32_t)dist | ((uint64_t)((stamp << W_STAMP_SHIFT) | (steps << T_STEPS_SHIFT) | dir) << 32);
}
TS_WORDS_FN int tent_dist(uint64_t word, uint32_t epoch) { return wave_meta_live((uint32_t)(word >> 32), epoch) ? (int)(uint32_t)word : A_INF; }
TS_WORDS_FN int tent_steps(uint64_t word) { return (int)(((uint32_t)(word >> 32) >> T_STEPS_SHIFT) & T_STEPS_MASK); }
TS_WORDS_FN int tent_dir(uint64_t word) { return (int)((uint32_t)(word >> 32) & T_DIR_MASK); }

// ---- the search penalties in half units -----------------------------------------------------------------------------------------
// Half units carry the search costs exactly iff every penalty is a non-negative multiple of 0.5 of moderate size (the
// reference's defaults are).  Host (k_amap_build's penalty bits) and device (astar_wave) decide with the same function.
TS_WORDS_FN bool astar_half_units(const TsParams& P) {
  const double pp[7] = {(double)P.turn_penalty, (double)P.contraflow_penalty, (double)P.obstacle_penalty_vehicle,
                        (double)P.obstacle_penalty_stop, (double)P.road_type_penalty_r1, (double)P.road_type_penalty_r2,
                        (double)P.road_type_penalty_r3};
  bool half = true;
  for (int k = 0; k < 7; k++) half = half && pp[k] >= 0.0 && pp[k] < 1048576.0 && (double)(int)(pp[k] * 2.0) == pp[k] * 2.0;
  half = half && P.dynamic_penalty_scale >= 0.0 && P.dynamic_penalty_scale <= 64.0;   // (2 (g + 1) + penalties stays below 2^31 for every g < INF)
  // the per-cell vehicle penalty travels in 22 bits of the map snapshot (density <= 1)
  half = half && (double)P.obstacle_penalty_vehicle * (1.0 + (double)P.dynamic_penalty_scale) * 2.0 < 2097152.0;
  return half;
}
// TsParams' penalties in half units (exact where astar_half_units(P) holds): the one conversion
struct HalfCosts { int turn2, contra2, veh2, stop2, rt2_1, rt2_2, rt2_3; };
TS_WORDS_FN HalfCosts half_costs(const TsParams& P) {
  HalfCosts c;
  c.turn2 = (int)((double)P.turn_penalty * 2.0); c.contra2 = (int)((double)P.contraflow_penalty * 2.0);
  c.veh2 = (int)((double)P.obstacle_penalty_vehicle * 2.0); c.stop2 = (int)((double)P.obstacle_penalty_stop * 2.0);
  c.rt2_1 = (int)((double)P.road_type_penalty_r1 * 2.0); c.rt2_2 = (int)((double)P.road_type_penalty_r2 * 2.0);
  c.rt2_3 = (int)((double)P.road_type_penalty_r3 * 2.0);
  return c;
}
// the penalty of a road of type rt (0: none), for cold code
TS_WORDS_FN int rt2_of(const HalfCosts& c, uint32_t rt) { return rt == 1u ? c.rt2_1 : rt == 2u ? c.rt2_2 : rt == 3u ? c.rt2_3 : 0; }
