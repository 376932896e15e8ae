"""The trip-log entries (include/trafficsim_triplog.h) without a GPU: the header declares exactly them, the record's layout is
TRIP_DTYPE's, the enum values are the Python names', the HIP library exports the entries, and the oracle-backed CApi - which
shares the class and has no trip log - refuses them cleanly."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi

ENTRIES = ["ts_triplog_clear", "ts_triplog_device", "ts_triplog_info", "ts_triplog_od", "ts_triplog_read",
           "ts_triplog_set_zones", "ts_triplog_start", "ts_triplog_stop"]


def test_header_declares_exactly_the_triplog_entries():
    assert sorted(declared("trafficsim_triplog.h")) == ENTRIES


def test_enum_values_match_the_python_names():
    src = header("trafficsim_triplog.h")
    for name, k in capi.TRIP_END.items():
        assert re.search(rf"\bTS_TRIP_END_{name.upper()}\s*=\s*{k}\b", src), name
    assert sorted(capi.TRIP_END.values()) == [0, 1, 2]
    assert re.search(rf"#define\s+TS_TRIP_END_ALL\s+{sum(1 << k for k in capi.TRIP_END.values())}u", src)
    assert re.search(rf"#define\s+TS_TRIPLOG_MAX_ZONES\s+{capi.TRIPLOG_MAX_ZONES}\b", src)


def test_record_layout_is_the_dtype(tmp_path):
    """sizeof and every offsetof of TsTripRecord and TsTripLogInfo, as a C compiler sees the header."""
    fields = list(capi.TRIP_DTYPE.names)
    info = [n for n, _ in capi.TsTripLogInfo._fields_]
    rec, inf = c_layout("trafficsim_triplog.h", [("TsTripRecord", fields), ("TsTripLogInfo", info)], tmp_path)
    assert rec[0] == capi.TRIP_DTYPE.itemsize == 72
    assert rec[1:] == [capi.TRIP_DTYPE.fields[f][1] for f in fields]
    assert inf[0] == ctypes.sizeof(capi.TsTripLogInfo)
    assert inf[1:] == [getattr(capi.TsTripLogInfo, f).offset for f in info]
    # 14 int32 then 2 doubles, nothing between
    assert [capi.TRIP_DTYPE.fields[f][0] for f in fields] == [np.dtype(np.int32)] * 14 + [np.dtype(np.float64)] * 2


def test_triplog_stays_out_of_the_main_header():
    src = header("trafficsim.h")
    assert "triplog" not in src and "TS_TRIP_END" not in src and "TsTripRecord" not in src


def test_hip_library_exports_the_triplog_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_oracle_capi_has_no_trip_log():
    assert oracle_api().has_triplog is False


@pytest.mark.parametrize("call", ["start", "stop", "clear", "info", "trips", "device", "set_zones", "od"])
def test_oracle_trip_log_is_unsupported(call):
    api = oracle_api()
    api.W = api.H = 4
    calls = {"start": lambda: api.triplog_start(16), "stop": api.triplog_stop, "clear": api.triplog_clear, "info": api.triplog_info,
             "trips": api.trips, "device": api.triplog_device, "set_zones": lambda: api.triplog_set_zones(np.zeros((4, 4), np.int32), 1),
             "od": api.triplog_od}
    refused(capi.TS_E_UNSUPPORTED, calls[call])
