"""The cost-field route entries (include/trafficsim_cfroute.h) without a GPU: the header declares exactly the entries of
cfroute.ENTRIES with their arities, the group stays out of _capi's table, of the cost field's and of both their headers, the
HIP library exports the symbols, the structs lie as a C compiler lays them out, null handles are refused, and the
oracle-backed CApi - which shares the class and has no routes - refuses every call with the usual phrase."""
import ctypes
import re

import numpy as np
import pytest

from tests.abi_util import c_layout, declared, header, hip_lib, oracle_api, struct_fields
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi
from trafficsimulation_amd import cfroute as cr
from trafficsimulation_amd import costfield as cf

HEADER = "trafficsim_cfroute.h"
ENTRIES = ["ts_cfroute_cells", "ts_cfroute_compute", "ts_cfroute_device", "ts_cfroute_info", "ts_cfroute_load",
           "ts_cfroute_load_device", "ts_cfroute_load_download", "ts_cfroute_read", "ts_cfroute_release", "ts_cfroute_trace"]


def test_header_declares_exactly_the_entries_of_the_python_table():
    want = declared(HEADER)
    phrase, entries = cr.ENTRIES
    assert phrase == "cost-field routes" and sorted(want) == ENTRIES == sorted("ts_" + n for n in entries)
    for n, argtypes in entries.items():
        assert len(argtypes) == want["ts_" + n], n


def test_the_group_is_a_table_of_its_own():
    assert not set(cr.ENTRIES[1]) & set(capi._GROUP_OF) and not set(cr.ENTRIES[1]) & set(cf.ENTRIES[1])
    assert "cfroute" not in capi.ENTRIES and not any("cfroute" in n for n in capi._GROUP_OF)
    assert not any("cfroute" in n for n in cf.ENTRIES[1])
    for h in ("trafficsim.h", "trafficsim_costfield.h"):
        assert "cfroute" not in header(h) and "TS_CFR_" not in header(h), h
    assert not any(n.startswith("ts_cfroute") for n in declared("trafficsim_costfield.h"))


def test_header_constants_match_the_python_names():
    src = header(HEADER)
    for name, v in (("TS_CFR_STOP", cr.CFR_STOP), ("TS_CFR_NONE", cr.CFR_NONE), ("TS_CFR_HOPS", cr.CFR_HOPS), ("TS_CFR_OFF", cr.CFR_OFF),
                    ("TS_CFR_DIRS", cr.CFR_DIRS), ("TS_CFR_COST", cr.CFR_COST), ("TS_CFR_OWNER", cr.CFR_OWNER),
                    ("TS_CFR_MAX_STARTS", cr.CFR_MAX_STARTS)):
        assert re.search(rf"\b{name}\s*=\s*{v}\b", src), name
    assert cr.CFR_MAX_STARTS == 1 << 24


STRUCTS = [("TsCfRouteBatch", cr.TsCfRouteBatch), ("TsCfRouteLoadInfo", cr.TsCfRouteLoadInfo), ("TsCfRouteInfo", cr.TsCfRouteInfo)]


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
    assert [ctypes.sizeof(cls) for _, cls in STRUCTS] == [40, 40, 120]
    # the cost field's own structs are what they were
    assert [ctypes.sizeof(c) for c in (cf.TsCostFieldQuery, cf.TsCostFieldInfo)] == [48, 80]


def test_the_info_repeats_the_batch_and_load_structs():
    names = [n for n, _ in cr.TsCfRouteInfo._fields_]
    assert [n[6:] for n in names if n.startswith("trace_")] == [n for n, _ in cr.TsCfRouteBatch._fields_]
    assert [n[5:] for n in names if n.startswith("load_")] == [n for n, _ in cr.TsCfRouteLoadInfo._fields_]


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
    routes = api.costfield.routes
    assert isinstance(routes, cr.RouteField) and routes.available
    fn = routes._ext("cfroute_read")
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == cr.ENTRIES[1]["cfroute_read"]
    mine = list(fn.argtypes)
    fn.argtypes = mine
    assert api.costfield.routes._ext("cfroute_read").argtypes is mine
    assert capi.CApi(api.lib, "ts_").costfield.routes._ext("cfroute_read").argtypes is mine


CALLS = {"compute": lambda r: r.compute([(1, 1)]), "info": lambda r: r.info(), "trace": lambda r: r.trace([(1, 1)]),
         "read": lambda r: r.routes(0, 1), "cells": lambda r: r.cells(0, 1), "device": lambda r: r.device("hops"),
         "load": lambda r: r.load([(1, 1)]), "load_download": lambda r: r.load_plane(), "load_device": lambda r: r.device("load"),
         "release": lambda r: r.release()}


@pytest.mark.parametrize("call", sorted(CALLS))
def test_oracle_has_no_cost_field_routes(call):
    api = oracle_api()
    api.W = api.H = 4
    r = api.costfield.routes
    assert not r.available
    ex, = refused(capi.TS_E_UNSUPPORTED, lambda: CALLS[call](r))
    assert str(ex).endswith(f"tso_cfroute_{call}: this engine has no cost-field routes")


def test_every_entry_has_a_python_call():
    assert sorted("cfroute_" + c for c in CALLS) == sorted(cr.ENTRIES[1])


def test_the_oracle_refuses_before_it_looks_at_the_arguments():
    with pytest.raises(capi.EngineError) as ex:
        oracle_api().costfield.routes.trace(np.zeros((0, 2)))
    assert str(ex.value).endswith("tso_cfroute_trace: this engine has no cost-field routes")
