"""The select-link entries (include/trafficsim_selectlink.h) without a GPU: the header declares exactly the entries of
selectlink.ENTRIES with their arities, the group stays out of _capi's table and of the main header, the HIP library exports
the symbols, the structs lie as a C compiler lays them out, null handles are refused, and the oracle-backed CApi - which
shares the class and has no select-link analysis - refuses every call with the usual phrase."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api, struct_fields
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import selectlink as sl

HEADER = "trafficsim_selectlink.h"
ENTRIES = ["ts_selectlink_compute", "ts_selectlink_device", "ts_selectlink_info", "ts_selectlink_od", "ts_selectlink_release",
           "ts_selectlink_select", "ts_selectlink_set_gates", "ts_selectlink_set_zones", "ts_selectlink_tables",
           "ts_selectlink_vehicles"]


def test_header_declares_exactly_the_entries_of_the_python_table():
    want = declared(HEADER)
    phrase, entries = sl.ENTRIES
    assert phrase == "select-link analysis" and sorted(want) == ENTRIES == sorted("ts_" + n for n in entries)
    for n, argtypes in entries.items():
        assert len(argtypes) == want["ts_" + n], n


def test_the_group_is_a_table_of_its_own():
    assert not set(sl.ENTRIES[1]) & set(capi._GROUP_OF)
    assert "selectlink" not in capi.ENTRIES and not any("selectlink" in n for n in capi._GROUP_OF)
    assert "selectlink" not in header("trafficsim.h") and "TS_SL_" not in header("trafficsim.h")


def test_header_constants_match_the_python_names():
    src = header(HEADER)
    for name, v in (("TS_SL_MAX_GATES", sl.SL_MAX_GATES), ("TS_SL_MAX_CELLS", sl.SL_MAX_CELLS), ("TS_SL_MAX_ZONES", sl.SL_MAX_ZONES),
                    ("TS_SL_DIR_N", sl.DIR_BITS["N"]), ("TS_SL_DIR_E", sl.DIR_BITS["E"]), ("TS_SL_DIR_S", sl.DIR_BITS["S"]),
                    ("TS_SL_DIR_W", sl.DIR_BITS["W"]), ("TS_SL_DIR_ALL", sl.SL_DIR_ALL), ("TS_SL_MASK", sl.WHICH["mask"]),
                    ("TS_SL_FIRST_STEP", sl.WHICH["first_step"]), ("TS_SL_FIRST_GATE", sl.WHICH["first_gate"]),
                    ("TS_SL_CROSSINGS", sl.WHICH["crossings"]), ("TS_SL_SELECT", sl.WHICH["select"]), ("TS_SL_GATES", sl.WHICH["gates"])):
        assert re.search(rf"\b{name}\s*=\s*{v}\b", src), name
    assert sl.SL_MAX_ZONES == capi.TRIPLOG_MAX_ZONES and sl.SL_MAX_CELLS == 2 ** 20


STRUCTS = [("TsSelectLinkQuery", sl.TsSelectLinkQuery), ("TsSelectLinkInfo", sl.TsSelectLinkInfo)]


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
    assert [ctypes.sizeof(cls) for _, cls in STRUCTS] == [16, 80]
    # explicit padding: no field starts behind a hole
    for _, cls in STRUCTS:
        end = 0
        for n, t in cls._fields_:
            assert getattr(cls, n).offset == end, n
            end += ctypes.sizeof(t)
        assert end == ctypes.sizeof(cls)


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
    fn = api.selectlink._ext("selectlink_vehicles")
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == sl.ENTRIES[1]["selectlink_vehicles"]
    mine = list(fn.argtypes)
    fn.argtypes = mine
    assert api.selectlink._ext("selectlink_vehicles").argtypes is mine
    assert capi.CApi(api.lib, "ts_").selectlink._ext("selectlink_vehicles").argtypes is mine
    assert api.selectlink.available


def test_gate_tables_from_python_gates():
    off, xy, dm = sl.gate_tables([[(1, 2), (3, 4, "n")], [(5, 6, "WE"), (7, 8, 4)]])
    assert off.tolist() == [0, 2, 4] and xy.tolist() == [[1, 2], [3, 4], [5, 6], [7, 8]] and dm.tolist() == [15, 1, 10, 4]
    assert off.dtype == xy.dtype == np.int32 and dm.dtype == np.uint8
    for bad in ("", "X", "NQ"):
        with pytest.raises(ValueError):
            sl.dir_mask(bad)
    with pytest.raises(ValueError):
        sl._u32(-1)
    assert sl._u32(1 << 31) == 0x80000000


@pytest.mark.parametrize("call", ["set_gates", "compute", "info", "tables", "vehicles", "select", "set_zones", "od", "device", "release"])
def test_oracle_has_no_select_link(call):
    api = oracle_api()
    api.W = api.H = 4
    s = api.selectlink
    assert not s.available
    calls = {"set_gates": lambda: s.set_gates([[(1, 1)]]), "compute": s.compute, "info": s.info, "tables": s.tables,
             "vehicles": s.vehicles, "select": lambda: s.select(any=1), "set_zones": lambda: s.set_zones(np.zeros((4, 4)), 1),
             "od": s.od, "device": s.device, "release": s.release}
    ex, = refused(capi.TS_E_UNSUPPORTED, calls[call])
    assert str(ex).endswith(f"tso_selectlink_{call}: this engine has no select-link analysis")


def test_the_oracle_refuses_before_it_looks_at_the_arguments():
    s = oracle_api().selectlink
    for call, entry in ((lambda: s.set_gates("nonsense"), "set_gates"), (lambda: s.select(any=-5), "select"),
                        (lambda: s.set_zones(np.zeros(3), 10 ** 12), "set_zones"), (lambda: s.device("nothing"), "device"),
                        (lambda: s.vehicles(first="x"), "vehicles")):
        with pytest.raises(capi.EngineError) as ex:
            call()
        assert str(ex.value).endswith(f"tso_selectlink_{entry}: this engine has no select-link analysis")
