"""The route-demand entries (include/trafficsim_demand.h) without a GPU: the header declares exactly them, its constants and
structs match the Python side, the HIP library exports them, the main header does not mention them, and the oracle-backed
CApi - which shares the class and has no route demand - refuses them cleanly."""
import ctypes
import os
import re

import numpy as np
import pytest

from trafficsimulation_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ts_demand_compute", "ts_demand_device", "ts_demand_download", "ts_demand_groups", "ts_demand_info",
           "ts_demand_pooled", "ts_demand_release"]


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declares_exactly_the_demand_entries():
    assert sorted(set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", header("trafficsim_demand.h")))) == ENTRIES


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
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header("trafficsim_demand.h"), flags=re.S).group(1)
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
    want = []
    for typ, names in re.findall(r"^\s*(?:const\s+)?(u?int(?:8|32|64)_t\s*\*?)\s*([^;]+);", body, flags=re.M):
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            t = ctypes.c_void_p if typ.endswith("*") else ctype[typ.strip()]
            want.append((m.group(1), t * int(m.group(2)) if m.group(2) else t))
    got = list(cls._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, w) in zip(got, want):
        assert ctypes.sizeof(t) == ctypes.sizeof(w), n
    assert ctypes.sizeof(cls) == {"TsDemandQuery": 32, "TsDemandInfo": 120}[struct]


def test_demand_entries_stay_out_of_the_main_header():
    assert "demand" not in header("trafficsim.h") and "TS_DG_" not in header("trafficsim.h")


def test_hip_library_exports_the_demand_entries():
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_null_handles_are_refused_without_a_device():
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in ENTRIES:
        fn = getattr(lib, s)
        fn.restype = ctypes.c_int
        assert fn(*([None] * {"ts_demand_compute": 3, "ts_demand_info": 2, "ts_demand_download": 4, "ts_demand_pooled": 5,
                              "ts_demand_groups": 2, "ts_demand_device": 4, "ts_demand_release": 1}[s])) == capi.TS_E_INVALID, s


def oracle_api():
    from oracle import pyoracle
    return capi.CApi(ctypes.CDLL(pyoracle.build()), "tso_")


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
    with pytest.raises(capi.EngineError) as ex:
        calls[call]()
    assert ex.value.code == capi.TS_E_UNSUPPORTED
