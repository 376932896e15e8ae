"""The trip-log entries (include/trafficsim_triplog.h) without a GPU: the header declares exactly them, the record's layout is
TRIP_DTYPE's, the enum values are the Python names', the HIP library exports the entries, and the oracle-backed CApi - which
shares the class and has no trip log - refuses them cleanly."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from trafficsimulation_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ts_triplog_clear", "ts_triplog_device", "ts_triplog_info", "ts_triplog_od", "ts_triplog_read",
           "ts_triplog_set_zones", "ts_triplog_start", "ts_triplog_stop"]


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declares_exactly_the_triplog_entries():
    assert sorted(set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", header("trafficsim_triplog.h")))) == ENTRIES


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
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "trafficsim_triplog.h"', 'int main(void) {',
            '  printf("%zu\\n", sizeof(TsTripRecord));']
    prog += [f'  printf("%zu\\n", offsetof(TsTripRecord, {f}));' for f in fields]
    prog += ['  printf("%zu\\n", sizeof(TsTripLogInfo));']
    prog += [f'  printf("%zu\\n", offsetof(TsTripLogInfo, {f}));' for f in info]
    prog += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == capi.TRIP_DTYPE.itemsize == 72
    assert out[1:1 + len(fields)] == [capi.TRIP_DTYPE.fields[f][1] for f in fields]
    k = 1 + len(fields)
    assert out[k] == ctypes.sizeof(capi.TsTripLogInfo)
    assert out[k + 1:] == [getattr(capi.TsTripLogInfo, f).offset for f in info]
    # 14 int32 then 2 doubles, nothing between
    assert [capi.TRIP_DTYPE.fields[f][0] for f in fields] == [np.dtype(np.int32)] * 14 + [np.dtype(np.float64)] * 2


def test_triplog_stays_out_of_the_main_header():
    src = header("trafficsim.h")
    assert "triplog" not in src and "TS_TRIP_END" not in src and "TsTripRecord" not in src


def test_hip_library_exports_the_triplog_entries():
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def oracle_api():
    from oracle import pyoracle
    return capi.CApi(ctypes.CDLL(pyoracle.build()), "tso_")


def test_oracle_capi_has_no_trip_log():
    assert oracle_api().has_triplog is False


@pytest.mark.parametrize("call", ["start", "stop", "clear", "info", "trips", "device", "set_zones", "od"])
def test_oracle_trip_log_is_unsupported(call):
    api = oracle_api()
    api.W = api.H = 4
    calls = {"start": lambda: api.triplog_start(16), "stop": api.triplog_stop, "clear": api.triplog_clear, "info": api.triplog_info,
             "trips": api.trips, "device": api.triplog_device, "set_zones": lambda: api.triplog_set_zones(np.zeros((4, 4), np.int32), 1),
             "od": api.triplog_od}
    with pytest.raises(capi.EngineError) as ex:
        calls[call]()
    assert ex.value.code == capi.TS_E_UNSUPPORTED
