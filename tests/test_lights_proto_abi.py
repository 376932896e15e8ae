"""The A2C / GAT-DQN protocol entries (include/trafficsim_lights_proto.h) without a GPU: the header declares exactly them, the
three structs have the layout the Python binding declares, the protocol names stay out of LIGHT_ALGORITHMS, the HIP library
exports the entries, and the oracle-backed CApi - which shares the class and has no external control - refuses them."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.abi_util import ROOT, c_layout, declared, header, hip_lib, oracle_api
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi

ENTRIES = ["ts_lights_proto_act", "ts_lights_proto_act_q", "ts_lights_proto_config", "ts_lights_proto_device",
           "ts_lights_proto_download", "ts_lights_proto_info", "ts_lights_proto_observe"]


def test_header_declares_exactly_the_entries():
    assert sorted(declared("trafficsim_lights_proto.h")) == ENTRIES


def test_constants_and_names():
    src = header("trafficsim_lights_proto.h")
    for name, val in (("TS_LP_A2C", "1"), ("TS_LP_GAT", "2"), ("TS_LP_A2C_DIM", "13"), ("TS_LP_GAT_NODES", "5"),
                      ("TS_LP_GAT_FEATURES", "9"), ("TS_LP_DEFAULT_MIN_GREEN", "5"), ("TS_LP_DEFAULT_EPS_MIN", "0.1"),
                      ("TS_LP_DEFAULT_EPS_DECAY", "1e-5")):
        assert re.search(rf"#define\s+{name}\s+{re.escape(val)}\s", src), name
    assert capi.LIGHT_PROTOCOLS == {"RL_A2C_BATCHED": capi.LP_A2C, "GAT_DQN_BATCHED": capi.LP_GAT} and (capi.LP_A2C, capi.LP_GAT) == (1, 2)
    # the engine's light algorithms are untouched: the protocols belong to the extension
    assert sorted(set(capi.LIGHT_ALGORITHMS.values())) == list(range(7))
    for name in ("NEIGHBOR_RL", "RL_A2C_BATCHED", "GAT_DQN", "GAT_DQN_BATCHED"):
        assert name not in capi.LIGHT_ALGORITHMS
    for other in ("trafficsim.h", "trafficsim_lights_ext.h"):
        assert "lights_proto" not in header(other) and "TsLightsProto" not in header(other)


def test_struct_layouts(tmp_path):
    """sizeof and every offsetof of the three structs, as a C compiler sees the header."""
    structs = [("TsLightsProtoConfig", capi.TsLightsProtoConfig), ("TsLightsProtoInfo", capi.TsLightsProtoInfo),
               ("TsLightsProtoDevice", capi.TsLightsProtoDevice)]
    out = c_layout("trafficsim_lights_proto.h", [(cname, [f for f, _ in cls._fields_]) for cname, cls in structs], tmp_path)
    for (cname, cls), c in zip(structs, out):
        assert c[0] == ctypes.sizeof(cls), cname
        assert c[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    assert [ctypes.sizeof(c) for _, c in structs] == [24, 48, 56]


def test_hip_library_exports_the_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


@pytest.mark.parametrize("call", ["config", "info", "observe", "act", "act_q", "controller", "device"])
def test_oracle_protocols_are_unsupported(call):
    api = oracle_api()
    api.n_groups = 3
    z = np.zeros(3, np.int8)
    calls = {"config": lambda: api.lights_proto_config("GAT_DQN_BATCHED"), "info": api.lights_proto_info,
             "observe": api.lights_proto_observe, "act": lambda: api.lights_proto_act(z),
             "act_q": lambda: api.lights_proto_act_q(np.zeros((3, 2), np.float32)), "controller": api.lights_proto_controller,
             "device": api.lights_proto_device}
    refused(capi.TS_E_UNSUPPORTED, calls[call])


def test_params_still_refuse_the_names():
    """The translation to EXTERNAL plus a protocol is world.build_engine's; params_from_defaults knows light algorithms only."""
    api = oracle_api()
    for name in ("RL_A2C_BATCHED", "GAT_DQN_BATCHED", "GAT_DQN", "NEIGHBOR_RL"):
        refused(capi.TS_E_UNSUPPORTED, lambda: api.params_from_defaults({"TRAFFIC_LIGHT_AGENT_ALGORITHM": name}))


def test_recorded_kernel_resources_of_the_hot_kernels_equal_the_parents():
    """profiles/r09_kernel_resources.csv (this change) against r08 (its parent): every earlier kernel's line is unchanged - the
    budget of k_move_resolve, k_replan and k_replan_quad among them - and the k_lp_* kernels use neither scratch nor LDS."""
    def table(name):
        rows = [ln.split(",") for ln in open(os.path.join(ROOT, "profiles", name)).read().split()]
        return rows[0], {r[0]: r[1:] for r in rows[1:]}
    head, new = table("r09_kernel_resources.csv")
    _, old = table("r08_kernel_resources.csv")
    assert {"k_move_resolve", "k_replan", "k_replan_quad"} <= set(old)
    assert {k: v for k, v in new.items() if not k.startswith("k_lp_")} == old
    lp = {k: dict(zip(head[1:], v)) for k, v in new.items() if k.startswith("k_lp_")}
    assert sorted(lp) == ["k_lp_a2c_state", "k_lp_act", "k_lp_gat_next", "k_lp_gat_state", "k_lp_greedy"]
    for k, v in lp.items():
        assert v["scratch_bytes_per_lane"] == "0" and v["LDS_bytes_per_block"] == "0" and v["VGPR_spills"] == "0", k
