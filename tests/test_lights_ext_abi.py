"""The external-control entries (include/trafficsim_lights_ext.h) without a GPU: the header declares exactly them, the two
structs have the layout the Python binding declares, the algorithm names map to TS_LIGHTS_EXTERNAL, the HIP library exports
the entries, and the oracle-backed CApi - which shares the class and has no external control - refuses them cleanly."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi

ENTRIES = ["ts_lights_ext_act", "ts_lights_ext_config", "ts_lights_ext_device", "ts_lights_ext_download", "ts_lights_ext_info",
           "ts_lights_ext_observe", "ts_lights_ext_request", "ts_lights_ext_set_static"]


def test_header_declares_exactly_the_entries():
    assert sorted(declared("trafficsim_lights_ext.h")) == ENTRIES


def test_algorithm_names():
    src = header("trafficsim.h")
    assert re.search(r"\bTS_LIGHTS_EXTERNAL\s*=\s*6\b", src)
    assert capi.LIGHT_ALGORITHMS["EXTERNAL"] == capi.LIGHT_ALGORITHMS["NEIGHBOR_RL_BATCHED"] == 6
    assert sorted(set(capi.LIGHT_ALGORITHMS.values())) == list(range(7))
    for name in ("NEIGHBOR_RL", "RL_A2C_BATCHED", "GAT_DQN", "GAT_DQN_BATCHED"):      # the other RL names keep their refusal
        assert name not in capi.LIGHT_ALGORITHMS
    # nothing else of the extension leaks into the main header
    assert "lights_ext" not in src.replace("trafficsim_lights_ext.h", "") and "TsLightsExt" not in src
    ext = header("trafficsim_lights_ext.h")
    assert re.search(r"#define\s+TS_LIGHTS_EXT_DEFAULT_DIM\s+13\b", ext) and re.search(r"#define\s+TS_LIGHTS_EXT_DEFAULT_MIN_GREEN\s+5\b", ext)
    assert re.search(rf"#define\s+TS_LIGHTS_EXT_MAX_DIM\s+{max(capi.LIGHTS_EXT_DIMS)}\b", ext)


def test_params_accept_the_names_and_refuse_the_other_rl_variants():
    api = oracle_api()
    for name in ("EXTERNAL", "NEIGHBOR_RL_BATCHED"):
        assert api.params_from_defaults({"TRAFFIC_LIGHT_AGENT_ALGORITHM": name}).light_algorithm == 6
    refused(capi.TS_E_UNSUPPORTED, lambda: api.params_from_defaults({"TRAFFIC_LIGHT_AGENT_ALGORITHM": "GAT_DQN"}))


def test_struct_layouts(tmp_path):
    """sizeof and every offsetof of TsLightsExtInfo and TsLightsExtDevice, as a C compiler sees the header."""
    structs = [("TsLightsExtInfo", capi.TsLightsExtInfo), ("TsLightsExtDevice", capi.TsLightsExtDevice)]
    out = c_layout("trafficsim_lights_ext.h", [(cname, [f for f, _ in cls._fields_]) for cname, cls in structs], tmp_path)
    for (cname, cls), c in zip(structs, out):
        assert c[0] == ctypes.sizeof(cls), cname
        assert c[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    assert ctypes.sizeof(capi.TsLightsExtInfo) == 32 and ctypes.sizeof(capi.TsLightsExtDevice) == 40


def test_hip_library_exports_the_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_oracle_capi_has_no_external_control():
    assert oracle_api().has_lights_ext is False


@pytest.mark.parametrize("call", ["config", "set_static", "info", "observe", "act", "request", "controller", "device"])
def test_oracle_external_control_is_unsupported(call):
    api = oracle_api()
    api.n_groups = 3
    z = np.zeros(3, np.int8)
    calls = {"config": lambda: api.lights_config(13, 5), "set_static": lambda: api.lights_set_static(np.zeros(3), np.zeros(3)),
             "info": api.lights_info, "observe": api.lights_observe, "act": lambda: api.lights_act(z),
             "request": lambda: api.lights_request(z), "controller": api.lights_controller, "device": api.lights_device}
    refused(capi.TS_E_UNSUPPORTED, calls[call])


def test_approach_penalty_score_is_the_mean_of_the_penalties():
    got = capi.approach_penalty_score([[4, 2, 2, 0], [0, 0, 0, 0], [3, 0, 0, 3], [5, 1, 0, 0]], (0.5, 5, 50.0))
    assert np.array_equal(got, [2.75, 0.0, 50.0, 0.1])
