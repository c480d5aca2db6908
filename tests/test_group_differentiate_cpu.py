"""calipso_hip_group_differentiate at the drop-in boundary, without a GPU: the binding table names it, the library exports it, and it refuses a NULL group before it
touches a device (tests/test_abi_cpu.py ties the header, the exports and the binding table together as a whole)."""
from helpers import load_pkg

CALIPSO_ERR_ARGUMENT = -4      # include/calipso_hip.h


def test_group_differentiate_is_bound_exported_and_refuses_a_null_group():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    assert "calipso_hip_group_differentiate" in SYMBOLS
    L = lib()
    assert hasattr(L, "calipso_hip_group_differentiate"), "missing export"
    for tile in (0, 16, 64, 7):
        assert L.calipso_hip_group_differentiate(None, None, None, tile, None) == CALIPSO_ERR_ARGUMENT
