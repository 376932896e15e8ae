"""The checkpoint entries (include/trafficsim_checkpoint.h) without a GPU: the HIP library exports them, and the
oracle-backed CApi - which shares the class and has no checkpoints - still constructs and refuses them cleanly."""
import ctypes
import os
import re

import pytest

from trafficsimulation_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def checkpoint_symbols():
    src = open(os.path.join(ROOT, "include", "trafficsim_checkpoint.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_the_checkpoint_entries():
    assert checkpoint_symbols() == ["ts_checkpoint_load", "ts_checkpoint_save", "ts_checkpoint_size"]


def test_checkpoint_entries_stay_out_of_the_main_header():
    src = open(os.path.join(ROOT, "include", "trafficsim.h")).read()
    assert "checkpoint" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_hip_library_exports_the_checkpoint_entries():
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in checkpoint_symbols():
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def oracle_api():
    from oracle import pyoracle
    return capi.CApi(ctypes.CDLL(pyoracle.build()), "tso_")


def test_oracle_capi_still_constructs():
    api = oracle_api()
    assert api.prefix == "tso_"


@pytest.mark.parametrize("call", ["size", "save", "load"])
def test_oracle_checkpoints_are_unsupported(call):
    api = oracle_api()
    with pytest.raises(capi.EngineError) as ex:
        {"size": api.checkpoint_size, "save": api.checkpoint_save, "load": lambda: api.checkpoint_load(b"\0" * 64)}[call]()
    assert ex.value.code == capi.TS_E_UNSUPPORTED
