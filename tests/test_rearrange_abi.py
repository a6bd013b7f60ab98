"""The segment edits' entry points (csrc/ig_host_edit.inc): declared in include/instagraal_hip.h, exported by the library, bound by
hip_lib and reachable from the sampler and from a run.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_edit_score", "ig_edit_state", "ig_edit_apply", "ig_debug_edit_time")
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_edit_score(") > header.index("ig_debug_segment_placement_time(")  # behind the segment placement block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_edit.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_edit.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert '#include "ig_kernels_edit.cuh"' in unit and '#include "ig_host_edit.inc"' in unit
    assert unit.index('"ig_kernels_edit.cuh"') > unit.index('"ig_kernels_segplace.cuh"') and unit.index('"ig_host_edit.inc"') > unit.index('"ig_host_segplace.inc"')
    assert unit.index('"ig_host_edit.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_edit_buffers(") == 1
    assert "free_edit_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct EditBuf {") == 1 and "EditBuf edit;" in common
    # the kernels the feature is made of, and the device functions of the exact terms they call (no second definition of a term)
    kernels = open(os.path.join(csrc, "ig_kernels_edit.cuh")).read()
    for k in ("k_edit_plan", "k_edit_state", "k_edit_delta", "k_edit_zero_delta"):
        assert re.search(r"__global__ void (__launch_bounds__\(\w+\) )?%s\(" % k, kernels), k
    assert "eval_q(" in kernels and "zero_q(" in kernels and "k_fill_tables" in source and "launch_full_nz(" in source and "k_full_zero" in source
    assert "launch_recompute(c)" in source and "ig_acc_normalize" in source
    assert int(re.search(r"#define EDIT_CHUNK (\d+)", kernels).group(1)) == 64


def test_the_python_layers_reach_them():
    from instagraal_amd import hip_lib, rearrange as ra
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("edit_score", "edit_state", "edit_apply", "debug_edit_time"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(hip_lib.Context.edit_score)[1:] == [("edits", EMPTY), ("form", 0)]
    assert params(hip_lib.Context.edit_state)[1:] == [("edit", EMPTY)] and params(hip_lib.Context.edit_apply)[1:] == [("edit", EMPTY)]
    assert params(hip_lib.Context.debug_edit_time)[1:] == [("edits", EMPTY), ("form", 0), ("n", 1)]
    assert params(sampler.score_rearrangements)[1:] == [("edits", EMPTY), ("form", "delta")]
    assert params(sampler.apply_rearrangement)[1:] == [("edit", EMPTY)]
    assert params(sampler.propose_rearrangements)[1:] == [("n", 20), ("window", None), ("orientation_window", None)]
    assert params(sampler.polish)[1:4] == [("max_rounds", 10), ("n", 20), ("min_gain", 0.0)]
    assert params(ra.apply_host) == [("state", EMPTY), ("edit", EMPTY), ("next_cid", EMPTY)]
    assert params(ra.check) == [("state", EMPTY), ("edit", EMPTY)] and params(ra.touched_contigs) == [("state", EMPTY), ("edit", EMPTY)]
    assert params(ra.polish_round)[:2] == [("scores", EMPTY), ("edits", EMPTY)] and params(ra.write_polish_log) == [("path", EMPTY), ("log", EMPTY)]
    assert (ra.IN_PLACE, ra.NEW_CONTIG) == (-2, -1) and ra.FORMS == ("delta", "whole")
    assert inspect.signature(run_instagraal).parameters["polish"].default is False
    assert inspect.signature(instagraal_class.full_em).parameters["polish"].default is False
    assert hip_lib.EDIT_PASSES == ra.EDIT_PASSES == ("plan", "state", "tables", "delta", "zero", "whole")
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    host = open(os.path.join(csrc, "ig_host_edit.inc")).read()
    assert int(re.search(r"#define EDIT_PASSES (\d+)", host).group(1)) == len(hip_lib.EDIT_PASSES)
    for i, name in enumerate(hip_lib.EDIT_PASSES):
        assert int(re.search(r"#define EDIT_P_%s (\d+)" % name.upper(), host).group(1)) == i
    kernels = open(os.path.join(csrc, "ig_kernels_edit.cuh")).read()
    assert int(re.search(r"#define EDIT_IN_PLACE \((-?\d+)\)", kernels).group(1)) == ra.IN_PLACE
    assert int(re.search(r"#define EDIT_NEW_CONTIG \((-?\d+)\)", kernels).group(1)) == ra.NEW_CONTIG
    assert int(re.search(r"#define EDIT_ACC (\d+)", kernels).group(1)) == 5 == ra.SCORE_DTYPE["limbs"].shape[0]
    for dep in ("ig_kernels_edit.cuh", "ig_host_edit.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)
