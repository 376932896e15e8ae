"""The observation entries (include/trafficsim_observe.h) without a GPU: the header declares exactly them, the HIP library
exports them, and the oracle-backed CApi - which shares the class and has no observation - still constructs and refuses
them cleanly."""
import ctypes
import os
import re

import pytest

from trafficsimulation_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ts_observe_device", "ts_observe_download", "ts_observe_groups", "ts_observe_info", "ts_observe_pooled",
           "ts_observe_regions", "ts_observe_reset", "ts_observe_start", "ts_observe_stop"]


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declares_exactly_the_observe_entries():
    assert sorted(set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", header("trafficsim_observe.h")))) == ENTRIES


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
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def oracle_api():
    from oracle import pyoracle
    return capi.CApi(ctypes.CDLL(pyoracle.build()), "tso_")


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
    with pytest.raises(capi.EngineError) as ex:
        calls[call]()
    assert ex.value.code == capi.TS_E_UNSUPPORTED
