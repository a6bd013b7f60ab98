"""The entry points of the fixed-resolution maps (csrc/ig_host_zoom.inc): declared in include/instagraal_hip.h, exported by the
library, bound by hip_lib and reachable from the sampler and from a run.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_assembly_contacts_build_units", "ig_assembly_contacts_coarsen", "ig_balance_build_units", "ig_debug_zoom_coarsen", "ig_debug_zoom_fetch",
                "ig_debug_zoom_time")
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_assembly_contacts_build_units(") > header.index("ig_debug_gap_support_time(")  # behind the gap support's block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_zoom.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_zoom.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('#include "ig_kernels_zoom.cuh"') > unit.index('#include "ig_kernels_gap.cuh"')
    assert unit.index('#include "ig_host_zoom.inc"') > unit.index('#include "ig_host_gap.inc"')
    for dep in ("ig_kernels_zoom.cuh", "ig_host_zoom.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def _defaults(f, skip=1):
    return [(k, v.default) for k, v in inspect.signature(f).parameters.items()][skip:]


def test_the_python_layers_reach_them():
    from instagraal_amd import assembly_contacts as ac, balance as bal, hip_lib, zoom_levels as zl
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    assert _defaults(hip_lib.Context.assembly_contacts_units) == [("unit", EMPTY), ("n_units", EMPTY)]
    assert _defaults(hip_lib.Context.assembly_contacts_coarsen) == [("coarse_of_unit", EMPTY), ("n_coarse", EMPTY)]
    assert _defaults(hip_lib.Context.balance_build_units) == [("unit", EMPTY), ("n_units", EMPTY), ("ignore_diags", 2)]
    assert _defaults(hip_lib.Context.debug_zoom_coarsen) == [("rowptr", EMPTY), ("col", EMPTY), ("count", EMPTY), ("coarse_of_unit", EMPTY), ("n_coarse", EMPTY)]
    assert _defaults(hip_lib.Context.debug_zoom_time) == [("n", 1), ("coarse_of_unit", None), ("n_coarse", None)]
    assert hip_lib.ZOOM_PASSES == ("rowstart", "words", "sort_short", "sort_lds", "sort_long", "reduce")
    source = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_host_zoom.inc")).read()
    assert int(re.search(r"#define ZOOM_PASSES (\d+)", source).group(1)) == len(hip_lib.ZOOM_PASSES)
    assert _defaults(sampler.resolution_contacts) == [("binsize", None), ("units", None), ("diagonal", True), ("balance", False)]
    assert _defaults(sampler.scaffold_contacts) == [("diagonal", True)]
    assert _defaults(sampler.write_zoom_levels) == [("folder", EMPTY), ("resolutions", zl.DEFAULT_RESOLUTIONS), ("scaffolds", True), ("diagonal", True), ("balance", False),
                                                    ("block_rows", None)]
    assert zl.DEFAULT_RESOLUTIONS == (10_000, 20_000, 50_000, 100_000, 200_000, 500_000, 1_000_000)
    assert inspect.signature(run_instagraal).parameters["save_resolutions"].default is False
    assert inspect.signature(instagraal_class.full_em).parameters["save_resolutions"].default is False
    # the signatures and the level lists the feature had to leave alone
    assert _defaults(sampler.assembly_contacts) == [("level", "sub"), ("diagonal", True), ("balance", False)]
    assert _defaults(sampler.write_assembly_contacts) == [("folder", EMPTY), ("level", "sub"), ("diagonal", True), ("block_rows", None), ("balance", False)]
    assert ac.LEVELS == ("sub", "bin") and bal.LEVELS == ("sub", "bin", "map")
    for f in ("binnify", "units_of_positions", "scaffold_units", "lift_units_host", "coarsen_host", "coarse_map", "plan", "units_without_position", "write_level"):
        assert callable(getattr(zl, f)), f
    assert _defaults(zl.lift_units_host, 0) == [(k, EMPTY) for k in ("position", "row", "col", "cnt", "unit", "n_units")]
    assert _defaults(zl.coarsen_host, 0) == [(k, EMPTY) for k in ("rowptr", "col", "count", "coarse_of_unit", "n_coarse")]
