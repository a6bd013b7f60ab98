"""The gap support's entry points (csrc/ig_host_gap.inc): declared in include/instagraal_hip.h, exported by the library, bound by
hip_lib and reachable from the sampler and from a run.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_gap_support", "ig_model_values_host", "ig_debug_gap_support_time")


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_gap_support(") > header.index("ig_debug_balance_build_time(")  # behind the balancing's block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_gap.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_gap.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert '#include "ig_kernels_gap.cuh"' in unit and '#include "ig_host_gap.inc"' in unit


def test_the_python_layers_reach_them():
    from instagraal_amd import gap_support as gs, hip_lib
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("gap_support", "debug_gap_support_time"):
        assert callable(getattr(hip_lib.Context, m)), m
    assert callable(hip_lib.model_values_host)
    sig = inspect.signature(hip_lib.Context.gap_support).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("window", inspect.Parameter.empty), ("junctions", inspect.Parameter.empty),
                                                           ("gaps_kb", inspect.Parameter.empty), ("model", True)]
    sig = inspect.signature(sampler.gap_support).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("level", "block"), ("junctions", None), ("gaps_kb", None), ("window", None), ("window_kb", None),
                                                           ("model", True)]
    sig = inspect.signature(sampler.gapped_joins).parameters
    assert [(k, v.default) for k, v in sig.items()][1:4] == [("n", 20), ("min_observed", 0), ("result", None)]
    assert [(k, v.default) for k, v in inspect.signature(gs.gapped_joins).parameters.items()] == [("result", inspect.Parameter.empty), ("n", 20), ("min_observed", 0)]
    assert [(k, v.default) for k, v in inspect.signature(gs.write_gaps).parameters.items()][2:] == [("mode", "w"), ("title", None)]
    assert inspect.signature(run_instagraal).parameters["save_gaps"].default is False
    assert inspect.signature(instagraal_class.full_em).parameters["save_gaps"].default is False
    assert gs.DEFAULT_WINDOW == 64 and gs.MAX_WINDOW == 256 and (gs.MIN_GAPS, gs.MAX_GAPS, gs.DEFAULT_N_GAPS) == (2, 64, 32)
    assert gs.SCALARS == ("unplaced", "trans", "ring", "counted", "uncounted", "contributions", "n_judged", "n_placed")
    assert hip_lib.GAP_SUPPORT_PASSES == ("observed", "model", "model_wave", "model_workgroup")
    kernels = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_kernels_gap.cuh")).read()
    assert int(re.search(r"#define GAP_WAVE_TERMS (\d+)", kernels).group(1)) == hip_lib.GAP_SUPPORT_WAVE_TERMS
    assert int(re.search(r"#define GAP_MAX_WINDOW (\d+)", kernels).group(1)) == gs.MAX_WINDOW
    assert int(re.search(r"#define GAP_MAX_GAPS (\d+)", kernels).group(1)) == gs.MAX_GAPS
    for dep in ("ig_kernels_gap.cuh", "ig_host_gap.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)
