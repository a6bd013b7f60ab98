"""The balancing's entry points (csrc/ig_host_bal.inc): declared in include/instagraal_hip.h, exported by the library, bound by
hip_lib.Context and reachable from the sampler.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_balance_build", "ig_balance_rows", "ig_balance_fetch", "ig_balance_run", "ig_balance_release", "ig_debug_balance_form",
                "ig_debug_balance_group", "ig_debug_lane_sums", "ig_debug_balance_time", "ig_debug_balance_build_time")


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    source = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_host_bal.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare


def test_the_python_layers_reach_them():
    from instagraal_amd import balance as bal, hip_lib
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("balance_build", "balance_fetch", "balance_run", "balance_release", "debug_balance_form", "debug_balance_group", "debug_lane_sums",
              "debug_balance_time", "debug_balance_build_time"):
        assert callable(getattr(hip_lib.Context, m)), m
    sig = inspect.signature(sampler.balance).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("level", "bin"), ("max_side", 2048)] + list(bal.DEFAULTS.items())
    assert bal.DEFAULTS == dict(ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200)
    for name in ("balanced_map", "display_balanced_matrix"):
        assert inspect.signature(getattr(sampler, name)).parameters["max_side"].default == 2048
    assert inspect.signature(sampler.assembly_contacts).parameters["balance"].default is False
    assert inspect.signature(sampler.write_assembly_contacts).parameters["balance"].default is False
    assert inspect.signature(run_instagraal).parameters["save_weights"].default is False
    assert inspect.signature(instagraal_class.full_em).parameters["save_weights"].default is False
    assert hip_lib.BALANCE_FORMS == ("default", "wave", "packed") and bal.LEVELS == ("sub", "bin", "map")
    for dep in ("ig_kernels_bal.cuh", "ig_host_bal.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)
