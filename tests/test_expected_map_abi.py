"""The C ABI of the expected contact map: the three entry points exist in the built library (no GPU needed: the symbols are looked
up, not called)."""
import ctypes as C
import os

import pytest


def test_the_three_symbols_exist_in_the_built_library():
    from instagraal_amd import hip_lib

    if not os.path.exists(hip_lib.LIB_PATH):
        pytest.fail("libinstagraal_hip.so is not built: run __graft_entry__.build()")
    lib = C.CDLL(hip_lib.LIB_PATH)
    for name in ("ig_expected_map", "ig_debug_expected_map_form", "ig_debug_expected_map_time"):
        assert hasattr(lib, name), name
    header = open(os.path.join(hip_lib.ROOT, "include", "instagraal_hip.h")).read()
    for name in ("int ig_expected_map(ig_ctx* ctx, int32_t max_side,", "int ig_debug_expected_map_form(ig_ctx* ctx, int32_t form);",
                 "int ig_debug_expected_map_time(ig_ctx* ctx, int32_t max_side, int32_t form, int32_t n, float* ms_n, int64_t* checksum);"):
        assert name in header, name
