"""The observation entries (include/trafficsim_observe.h) without a GPU: the header declares exactly them, the HIP library
exports them, and the oracle-backed CApi - which shares the class and has no observation - still constructs and refuses
them cleanly."""
import re

import pytest

from tests.abi_util import declared, header, hip_lib, oracle_api
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi

ENTRIES = ["ts_observe_device", "ts_observe_download", "ts_observe_groups", "ts_observe_info", "ts_observe_pooled",
           "ts_observe_regions", "ts_observe_reset", "ts_observe_start", "ts_observe_stop"]


def test_header_declares_exactly_the_observe_entries():
    assert sorted(declared("trafficsim_observe.h")) == ENTRIES


def test_header_constants_match_the_python_names():
    src = header("trafficsim_observe.h")
    for k, name in enumerate(capi.OBS_PLANES):
        assert re.search(rf"\bTS_OBS_{name.upper()}\s*=\s*{k}\b", src), name
    assert re.search(rf"\bTS_OBS_NPLANES\s*=\s*{len(capi.OBS_PLANES)}\b", src)
    for k, name in enumerate(capi.OG_FIELDS):
        assert re.search(rf"\bTS_OG_{name.upper()}\s*=\s*{k}\b", src), name
    assert re.search(rf"\bTS_OG_NFIELDS\s*=\s*{len(capi.OG_FIELDS)}\b", src)


def test_observe_entries_stay_out_of_the_main_header():
    assert "observe" not in header("trafficsim.h") and "TS_OBS" not in header("trafficsim.h")


def test_hip_library_exports_the_observe_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_oracle_capi_constructs_and_has_no_observation():
    api = oracle_api()
    assert api.prefix == "tso_" and api.has_observe is False


@pytest.mark.parametrize("call", ["start", "stop", "reset", "info", "plane", "pooled", "regions", "groups", "device"])
def test_oracle_observation_is_unsupported(call):
    api = oracle_api()
    api.W = api.H = 4
    calls = {"start": api.observe_start, "stop": api.observe_stop, "reset": api.observe_reset, "info": api.observe_info,
             "plane": lambda: api.observe_plane("present"), "pooled": lambda: api.observe_pooled("present", 2),
             "regions": lambda: api.observe_regions("present", [(0, 0, 1, 1)]), "groups": api.observe_groups,
             "device": lambda: api.observe_device("present")}
    refused(capi.TS_E_UNSUPPORTED, calls[call])
