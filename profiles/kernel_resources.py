#!/usr/bin/env python3
"""Register / scratch / LDS budget of the replanning kernels as hipcc reports them (-Rpass-analysis=kernel-resource-usage,
device code only; no GPU needed):

    python profiles/kernel_resources.py > profiles/r03_kernel_resources.csv
"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trafficsimulation_amd", "csrc")
WANT = ["k_replan", "k_replan_quad", "quad_policy", "replan_turn", "k_astar_single", "k_astar_batch", "k_spawn_plan", "k_decide_main", "k_decide_pre",
        "k_move_claim", "k_move_resolve", "k_amap_build",
        # the kernels the trip log's hooks sit in, and its own (triplog.h)
        "k_decide_despawn", "k_remove_one", "k_spawn", "k_tl_mark", "k_tl_count", "k_tl_emit", "k_tl_finish", "k_triplog_od",
        # the external light control (lights_ext.h; k_le_sums: the last instance of the template the compiler reports)
        "k_le_sums", "k_le_static", "k_le_state", "k_le_commit", "k_le_check", "k_le_act", "k_le_request",
        # the A2C / GAT-DQN light protocols (lights_proto.h)
        "k_lp_a2c_state", "k_lp_gat_state", "k_lp_act", "k_lp_gat_next", "k_lp_greedy",
        # the renderer (render.h): the pre-pass and the two frame kernels
        "k_render_pend", "k_render_vehicles", "k_render_routes", "k_render_frame", "k_render_shrink",
        # route demand (demand.h; k_demand_walk: the last instance of the template the compiler reports)
        "k_demand_walk", "k_demand_sum4", "k_demand_groups",
        # cost fields (costfield.h; k_cf_seed / k_cf_tile / k_cf_finish: the last instance of each template the compiler reports)
        "k_cf_cells", "k_cf_seed", "k_cf_tile", "k_cf_finish", "k_cf_gather", "k_cf_bands",
        # routes along a cost field (cfroute.h; k_cfr_hops: the last instance of the template the compiler reports)
        "k_cfr_hops", "k_cfr_count", "k_cfr_write", "k_cfr_load", "k_cfr_cells",
        # the cold readers and movers of the path pool (path_words.h)
        "k_pool_gc", "k_replan_export", "k_replan_import", "k_ckpt_count_paths", "k_ckpt_pack_paths", "k_ckpt_unpack_paths", "k_rows", "k_path_cells",
        # select-link analysis (selectlink.h; k_selectlink_walk: the last instance of the template the compiler reports)
        "k_selectlink_walk", "k_selectlink_scatter", "k_selectlink_select", "k_selectlink_od",
        # jam detection (jams.h; k_jam_tile: the last instance of the template the compiler reports)
        "k_jam_mark_vehicles", "k_jam_mark_mask", "k_jam_init", "k_jam_tile", "k_jam_merge", "k_jam_flatten", "k_jam_number",
        "k_jam_record_cells", "k_jam_record_vehicles", "k_jam_finish", "k_jam_groups"]
r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-pthread", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                    "-o", "/dev/null", "engine.hip", "-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:], cwd=CSRC, capture_output=True, text=True)
cur, rows = None, {}
for line in r.stderr.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        # (mangled names of the anonymous namespace: _ZN12_GLOBAL__N_1<len><name>...)
        n = re.match(r"_ZN12_GLOBAL__N_1(\d+)", m.group(1))
        cur = m.group(1)[len(n.group(0)):len(n.group(0)) + int(n.group(1))] if n else m.group(1)
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = m.group(2)
print("function,VGPRs,AGPRs,SGPRs,scratch_bytes_per_lane,occupancy_waves_per_SIMD,LDS_bytes_per_block,SGPR_spills,VGPR_spills")
for k in WANT:
    if k in rows:
        v = rows[k]
        print(",".join([k, v.get("VGPRs", ""), v.get("AGPRs", ""), v.get("TotalSGPRs", ""), v.get("ScratchSize", ""), v.get("Occupancy", ""),
                        v.get("LDS Size", ""), v.get("SGPRs Spill", ""), v.get("VGPRs Spill", "")]))
