"""The cost-field entries (include/trafficsim_costfield.h) without a GPU: the header declares exactly the entries of
costfield.ENTRIES with their arities, the group stays out of _capi's table and of the main header, the HIP library exports
the symbols, the structs lie as a C compiler lays them out, null handles are refused, and the oracle-backed CApi - which
shares the class and has no cost field - refuses every call with the usual phrase."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api, struct_fields
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import costfield as cf

HEADER = "trafficsim_costfield.h"
ENTRIES = ["ts_costfield_bands", "ts_costfield_compute", "ts_costfield_device", "ts_costfield_download", "ts_costfield_gather",
           "ts_costfield_info", "ts_costfield_release"]


def test_header_declares_exactly_the_entries_of_the_python_table():
    want = declared(HEADER)
    phrase, entries = cf.ENTRIES
    assert phrase == "cost field" and sorted(want) == ENTRIES == sorted("ts_" + n for n in entries)
    for n, argtypes in entries.items():
        assert len(argtypes) == want["ts_" + n], n


def test_the_group_is_a_table_of_its_own():
    assert not set(cf.ENTRIES[1]) & set(capi._GROUP_OF)
    assert "costfield" not in capi.ENTRIES and not any("costfield" in n for n in capi._GROUP_OF)
    assert "costfield" not in header("trafficsim.h") and "TS_CF_" not in header("trafficsim.h")


def test_header_constants_match_the_python_names():
    src = header(HEADER)
    for name, v in (("TS_CF_FROM", cf.CF_FROM), ("TS_CF_TO", cf.CF_TO), ("TS_CF_VALUE", cf.CF_VALUE), ("TS_CF_OWNER", cf.CF_OWNER),
                    ("TS_CF_MAX_SEEDS", cf.CF_MAX_SEEDS), ("TS_CF_MAX_BANDS", cf.CF_MAX_BANDS)):
        assert re.search(rf"\b{name}\s*=\s*{v}\b", src), name
    assert re.search(r"#define TS_CF_UNREACHABLE 0xFFFFFFFFu", src) and cf.CF_UNREACHABLE == 0xFFFFFFFF


STRUCTS = [("TsCostFieldQuery", cf.TsCostFieldQuery), ("TsCostFieldInfo", cf.TsCostFieldInfo)]


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
    assert [ctypes.sizeof(cls) for _, cls in STRUCTS] == [48, 80]


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
    fn = api.costfield._ext("costfield_gather")
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == cf.ENTRIES[1]["costfield_gather"]
    mine = list(fn.argtypes)
    fn.argtypes = mine
    assert api.costfield._ext("costfield_gather").argtypes is mine
    assert capi.CApi(api.lib, "ts_").costfield._ext("costfield_gather").argtypes is mine
    assert api.costfield.available


@pytest.mark.parametrize("call", ["compute", "info", "plane", "gather", "bands", "device", "release"])
def test_oracle_has_no_cost_field(call):
    api = oracle_api()
    api.W = api.H = 4
    c = api.costfield
    assert not c.available
    calls = {"compute": lambda: c.compute([(1, 1)]), "info": c.info, "plane": lambda: c.plane("owner"),
             "gather": lambda: c.gather("cost", [(0, 0)]), "bands": lambda: c.bands([1, 2]), "device": c.device, "release": c.release}
    entry = {"plane": "download"}.get(call, call)
    ex, = refused(capi.TS_E_UNSUPPORTED, calls[call])
    assert str(ex).endswith(f"tso_costfield_{entry}: this engine has no cost field")


def test_the_oracle_refuses_before_it_looks_at_the_arguments():
    with pytest.raises(capi.EngineError) as ex:
        oracle_api().costfield.compute(np.zeros((0, 2)))
    assert str(ex.value).endswith("tso_costfield_compute: this engine has no cost field")
