"""The route-demand entries (include/trafficsim_demand.h) without a GPU: the header declares exactly them, its constants and
structs match the Python side, the HIP library exports them, the main header does not mention them, and the oracle-backed
CApi - which shares the class and has no route demand - refuses them cleanly."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import declared, header, hip_lib, oracle_api, struct_fields
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi

ENTRIES = ["ts_demand_compute", "ts_demand_device", "ts_demand_download", "ts_demand_groups", "ts_demand_info",
           "ts_demand_pooled", "ts_demand_release"]


def test_header_declares_exactly_the_demand_entries():
    assert sorted(declared("trafficsim_demand.h")) == ENTRIES


def test_header_constants_match_the_python_names():
    src = header("trafficsim_demand.h")
    for k, name in enumerate(capi.DG_FIELDS):
        assert re.search(rf"\bTS_DG_{name.upper()}\s*=\s*{k}\b", src), name
    assert re.search(rf"\bTS_DG_NFIELDS\s*=\s*{len(capi.DG_FIELDS)}\b", src)
    assert re.search(rf"\bTS_DEMAND_MAX_BINS\s*=\s*{capi.DEMAND_MAX_BINS}\b", src) and capi.DEMAND_MAX_BINS == 8
    # field for field beside the observed group rows: the ENTER fields keep their names and their order
    assert capi.DG_FIELDS[2:] == capi.OG_FIELDS[4:] == capi.OBS_ENTER


@pytest.mark.parametrize("struct,cls", [("TsDemandQuery", capi.TsDemandQuery), ("TsDemandInfo", capi.TsDemandInfo)])
def test_structs_match_field_for_field(struct, cls):
    want = struct_fields("trafficsim_demand.h", struct)
    got = list(cls._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, w) in zip(got, want):
        assert ctypes.sizeof(t) == ctypes.sizeof(w), n
    assert ctypes.sizeof(cls) == {"TsDemandQuery": 32, "TsDemandInfo": 120}[struct]


def test_demand_entries_stay_out_of_the_main_header():
    assert "demand" not in header("trafficsim.h") and "TS_DG_" not in header("trafficsim.h")


def test_hip_library_exports_the_demand_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_null_handles_are_refused_without_a_device():
    lib, arity = hip_lib(), declared("trafficsim_demand.h")
    for s in ENTRIES:
        fn = getattr(lib, s)
        fn.restype = ctypes.c_int
        assert fn(*([None] * arity[s])) == capi.TS_E_INVALID, s


def test_oracle_capi_constructs_and_has_no_demand():
    api = oracle_api()
    assert api.prefix == "tso_" and api.has_demand is False


@pytest.mark.parametrize("call", ["compute", "compute_select", "info", "plane", "pooled", "groups", "device", "release"])
def test_oracle_demand_is_unsupported(call):
    api = oracle_api()
    api.W = api.H = 4
    calls = {"compute": api.demand_compute, "compute_select": lambda: api.demand_compute(4, 16, False, np.ones(3, dtype=np.uint8)),
             "info": api.demand_info, "plane": lambda: api.demand_plane(0, "N"), "pooled": lambda: api.demand_pooled(2),
             "groups": api.demand_groups, "device": api.demand_device, "release": api.demand_release}
    refused(capi.TS_E_UNSUPPORTED, calls[call])
