"""The segment placement's entry points (csrc/ig_host_segplace.inc): declared in include/instagraal_hip.h, exported by the library, bound
by hip_lib and reachable from the sampler and from a run.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_segment_placement", "ig_debug_segment_placement_time")


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_segment_placement(") > header.index("ig_debug_zoom_time(")  # behind the zoom block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_segplace.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_segplace.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert '#include "ig_kernels_segplace.cuh"' in unit and '#include "ig_host_segplace.inc"' in unit
    assert unit.index('"ig_kernels_segplace.cuh"') > unit.index('"ig_kernels_zoom.cuh"') and unit.index('"ig_host_segplace.inc"') > unit.index('"ig_host_zoom.inc"')
    # one buffer struct on the handle, one free function: first thing and last thing of every call, and in ig_destroy
    assert source.count("static void free_segplace_buffers(") == 1 and source.count("free_segplace_buffers(c);") == 2
    assert "free_segplace_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    assert "SegPlaceBuf segplace;" in open(os.path.join(csrc, "ig_common.cuh")).read()


def test_the_python_layers_reach_them():
    from instagraal_amd import hip_lib, placement_support as ps, segment_placement as sp
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("segment_placement", "debug_segment_placement_time"):
        assert callable(getattr(hip_lib.Context, m)), m
    sig = inspect.signature(hip_lib.Context.segment_placement).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("window", inspect.Parameter.empty), ("first", inspect.Parameter.empty), ("last", inspect.Parameter.empty),
                                                           ("min_hosts", None)]
    sig = inspect.signature(sampler.segment_placement).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("level", "block"), ("segments", None), ("window", None), ("window_kb", None), ("min_hosts", None)]
    sig = inspect.signature(sampler.misplaced_segments).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("n", 20), ("min_ratio", 1.0), ("result", None), ("level", "block"), ("segments", None), ("window", None),
                                                           ("window_kb", None), ("min_hosts", None)]
    assert [(k, v.default) for k, v in inspect.signature(sp.misplaced_segments).parameters.items()] == [("result", inspect.Parameter.empty), ("n", 20), ("min_ratio", 1.0)]
    assert [(k, v.default) for k, v in inspect.signature(sp.write_segment_placements).parameters.items()][2:] == [("n", None), ("min_ratio", 1.0), ("mode", "w"),
                                                                                                                 ("title", None)]
    assert inspect.signature(run_instagraal).parameters["save_segment_placements"].default is False
    assert inspect.signature(instagraal_class.full_em).parameters["save_segment_placements"].default is False
    assert sp.INT_ARRAYS == ps.INT_ARRAYS + ("arm",) and sp.LONG_ARRAYS == ps.LONG_ARRAYS and len(sp.SCALARS) == 9
    assert hip_lib.SEGMENT_PLACEMENT_PASSES == ("records", "count", "rows", "scatter", "sort_short", "sort_lds", "sort_long", "reduce", "prefix", "scan", "quadrants")
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    host = open(os.path.join(csrc, "ig_host_segplace.inc")).read()
    assert int(re.search(r"#define SEGPLACE_PASSES (\d+)", host).group(1)) == len(hip_lib.SEGMENT_PLACEMENT_PASSES)
    assert int(re.search(r"#define SEGPLACE_SCALARS (\d+)", host).group(1)) == len(sp.SCALARS)
    kernels = open(os.path.join(csrc, "ig_kernels_segplace.cuh")).read()
    assert int(re.search(r"#define SEGPLACE_NS (\d+)", kernels).group(1)) == len(sp.SCALARS) - 3
    assert [int(re.search(r"#define SEGPLACE_%s (\d+)" % q, kernels).group(1)) for q in ("HL", "HR", "TL", "TR")] == [sp.HL, sp.HR, sp.TL, sp.TR]
    place = open(os.path.join(csrc, "ig_kernels_place.cuh")).read()
    assert int(re.search(r"#define PLACE_WAVE_ENTRIES (\d+)", place).group(1)) == sp.WAVE_ENTRIES
    for dep in ("ig_kernels_segplace.cuh", "ig_host_segplace.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)
