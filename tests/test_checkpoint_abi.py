"""The checkpoint entries (include/trafficsim_checkpoint.h) without a GPU: the HIP library exports them, and the
oracle-backed CApi - which shares the class and has no checkpoints - still constructs and refuses them cleanly."""
import pytest

from tests.abi_util import declared, header, hip_lib, oracle_api
from tests.engine_util import refused
from trafficsimulation_amd import _capi as capi


def checkpoint_symbols():
    return sorted(declared("trafficsim_checkpoint.h"))


def test_header_declares_the_checkpoint_entries():
    assert checkpoint_symbols() == ["ts_checkpoint_load", "ts_checkpoint_save", "ts_checkpoint_size"]


def test_checkpoint_entries_stay_out_of_the_main_header():
    assert "checkpoint" not in header("trafficsim.h")


def test_hip_library_exports_the_checkpoint_entries():
    lib = hip_lib()
    for s in checkpoint_symbols():
        assert hasattr(lib, s), f"{s} missing from libtrafficsim_hip.so"


def test_oracle_capi_still_constructs():
    api = oracle_api()
    assert api.prefix == "tso_"


@pytest.mark.parametrize("call", ["size", "save", "load"])
def test_oracle_checkpoints_are_unsupported(call):
    api = oracle_api()
    refused(capi.TS_E_UNSUPPORTED, {"size": api.checkpoint_size, "save": api.checkpoint_save, "load": lambda: api.checkpoint_load(b"\0" * 64)}[call])
