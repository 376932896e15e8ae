"""The jam-detection entries (include/trafficsim_jams.h) without a GPU: the header declares exactly the entries of jams.ENTRIES
with their arities, the group stays out of _capi's table and of the main header, the HIP library exports the symbols, the three
structs lie as a C compiler lays them out and JAM_DTYPE is TsJamRecord, null handles are refused, and the oracle-backed CApi -
which shares the class and has no jam detection - refuses every call with the usual phrase."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api, struct_fields
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import jams as jm

HEADER = "trafficsim_jams.h"
ENTRIES = ["ts_jams_compute", "ts_jams_device", "ts_jams_download", "ts_jams_groups", "ts_jams_info", "ts_jams_records",
           "ts_jams_release", "ts_jams_vehicles"]


def test_header_declares_exactly_the_entries_of_the_python_table():
    want = declared(HEADER)
    phrase, entries = jm.ENTRIES
    assert phrase == "jam detection" and sorted(want) == ENTRIES == sorted("ts_" + n for n in entries)
    for n, argtypes in entries.items():
        assert len(argtypes) == want["ts_" + n], n


def test_the_group_is_a_table_of_its_own():
    assert not set(jm.ENTRIES[1]) & set(capi._GROUP_OF)
    assert "jams" not in capi.ENTRIES and not any("jams" in n for n in capi._GROUP_OF)
    assert "ts_jams" not in header("trafficsim.h") and "TS_JAM_" not in header("trafficsim.h")


def test_header_constants_match_the_python_names():
    src = header(HEADER)
    for name, v in (("TS_JAM_GRID", jm.LINK["grid"]), ("TS_JAM_FLOW", jm.LINK["flow"]), ("TS_JAM_VEHICLES", jm.SOURCE["vehicles"]),
                    ("TS_JAM_MASK", jm.SOURCE["mask"]), ("TS_JAM_PLANE_LABEL", jm.WHICH["label"]), ("TS_JAM_PLANE_COUNT", jm.WHICH["count"]),
                    ("TS_JAM_RECORDS", jm.WHICH["records"]), ("TS_JAM_VEHICLE_JAM", jm.WHICH["vehicles"]),
                    ("TS_JG_NFIELDS", len(jm.JG_FIELDS))):
        assert re.search(rf"\b{name}\s*=\s*{v}\b", src), name
    for k, n in enumerate(jm.JG_FIELDS):
        assert re.search(rf"\bTS_JG_{n.upper()}\s*=\s*{k}\b", src), n
    assert jm.JG_FIELDS.index("box_cells") == 11


STRUCTS = [("TsJamQuery", jm.TsJamQuery), ("TsJamRecord", jm.TsJamRecord), ("TsJamInfo", jm.TsJamInfo)]


@pytest.mark.parametrize("struct,cls", STRUCTS)
def test_structs_match_field_for_field(struct, cls):
    want = struct_fields(HEADER, struct)
    got = list(cls._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, w) in zip(got, want):
        assert ctypes.sizeof(t) == ctypes.sizeof(w), n


def test_struct_layouts_are_the_c_compilers(tmp_path):
    layouts = c_layout(HEADER, [(name, [n for n, _ in cls._fields_]) for name, cls in STRUCTS], tmp_path)
    for (name, cls), (size, *offsets) in zip(STRUCTS, layouts):
        assert ctypes.sizeof(cls) == size, name
        assert [getattr(cls, n).offset for n, _ in cls._fields_] == offsets, name
    assert [ctypes.sizeof(cls) for _, cls in STRUCTS] == [24, 56, 72]
    # explicit padding: no field starts behind a hole
    for _, cls in STRUCTS:
        end = 0
        for n, t in cls._fields_:
            assert getattr(cls, n).offset == end, n
            end += ctypes.sizeof(t)
        assert end == ctypes.sizeof(cls)


def test_the_record_dtype_is_the_struct():
    assert jm.JAM_DTYPE.itemsize == ctypes.sizeof(jm.TsJamRecord) == 56
    assert list(jm.JAM_DTYPE.names) == [n for n, _ in jm.TsJamRecord._fields_]
    for n, t in jm.TsJamRecord._fields_:
        assert jm.JAM_DTYPE.fields[n][1] == getattr(jm.TsJamRecord, n).offset and jm.JAM_DTYPE.fields[n][0].itemsize == ctypes.sizeof(t), n
    assert jm.JAM_DTYPE["vehicles"] == np.uint32 and jm.JAM_DTYPE["stuck_sum"] == np.int64


def test_hip_library_exports_the_entries():
    lib = hip_lib()
    for s in ENTRIES:
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_null_handles_are_refused_without_a_device():
    lib, arity = hip_lib(), declared(HEADER)
    for s in ENTRIES:
        fn = getattr(lib, s)
        fn.restype = ctypes.c_int
        assert fn(*([None] * arity[s])) == capi.TS_E_INVALID, s


def test_an_entry_is_bound_once_per_function_object():
    api = capi.CApi(hip_lib(), "ts_")
    fn = api.jams._ext("jams_records")
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == jm.ENTRIES[1]["jams_records"]
    mine = list(fn.argtypes)
    fn.argtypes = mine
    assert api.jams._ext("jams_records").argtypes is mine
    assert capi.CApi(api.lib, "ts_").jams._ext("jams_records").argtypes is mine
    assert api.jams.available


def test_names_are_checked_before_the_engine_is_asked():
    api = capi.CApi(hip_lib(), "ts_")
    api.W = api.H = 4
    for call in (lambda: api.jams.compute(link="diagonal"), lambda: api.jams.plane("records"), lambda: api.jams.device("nothing"),
                 lambda: api.jams.compute(mask=np.zeros((3, 4)))):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("call", ["compute", "info", "records", "vehicles", "plane", "groups", "device", "release"])
def test_oracle_has_no_jam_detection(call):
    api = oracle_api()
    api.W = api.H = 4
    j = api.jams
    assert not j.available
    entry = {"plane": "download"}.get(call, call)
    ex, = refused(capi.TS_E_UNSUPPORTED, getattr(j, call))
    assert str(ex).endswith(f"tso_jams_{entry}: this engine has no jam detection")


def test_the_oracle_refuses_before_it_looks_at_the_arguments():
    j = oracle_api().jams
    for call, entry in ((lambda: j.compute(link="nonsense", mask="x"), "compute"), (lambda: j.plane("nothing"), "download"),
                        (lambda: j.device("nothing"), "device"), (lambda: j.records(first="x"), "records")):
        with pytest.raises(capi.EngineError) as ex:
            call()
        assert str(ex.value).endswith(f"tso_jams_{entry}: this engine has no jam detection")
