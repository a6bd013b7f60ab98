"""The entry points of the read pairs lifted onto the current genome (csrc/ig_host_pairs.inc): declared in include/instagraal_hip.h,
exported by the library, bound by hip_lib with the argument lists the header states, and reachable from the sampler and from a run; the
defaults leave every existing call as it was.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_pairs_begin", "ig_pairs_lift", "ig_pairs_pixels_build", "ig_pairs_law", "ig_pairs_clear", "ig_pairs_end", "ig_debug_pairs_time")
# the number of arguments of every entry point in the header, the handle included: what the ctypes calls of hip_lib pass
N_ARGS = dict(ig_pairs_begin=16, ig_pairs_lift=17, ig_pairs_pixels_build=6, ig_pairs_law=6, ig_pairs_clear=1, ig_pairs_end=1, ig_debug_pairs_time=14)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_pairs_begin(") > header.index("ig_zero_terms_host(")  # behind the cut and join scores' block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_pairs.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    binding = open(os.path.join(ROOT, "instagraal_amd", "hip_lib.py")).read()
    for name in ENTRY_POINTS:
        decl = _declaration(header, name)
        assert len(decl) == N_ARGS[name] and decl[0] == "ig_ctx* ctx", (name, decl)
        defn = re.search(r'extern "C" int %s\(([^)]*)\)' % name, source).group(1).replace("\n", " ").split(",")
        strip = lambda a: re.sub(r"\s+", " ", a.strip())  # noqa: E731
        assert [strip(a).replace("ig_ctx* c", "ig_ctx* ctx") for a in defn] == [strip(a) for a in decl], name  # the definition is the declaration
        _assert_bound_as_declared(header, binding, name)  # the live argtypes are the header's; one argument each, the handle first
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_pairs.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_pairs.cuh"') > unit.index('"ig_kernels_cutjoin.cuh"') and unit.index('"ig_host_cutjoin.inc"') < unit.index('"ig_host_pairs.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_pairs_buffers(") == 1
    assert "free_pairs_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct PairsBuf {") == 1 and "PairsBuf pairs;" in common
    # the kernels the feature is made of; the slots, the packing and the rows are the shared ones
    kernels = open(os.path.join(csrc, "ig_kernels_pairs.cuh")).read()
    for k in ("k_pairs_lift", "k_pairs_emit", "k_pairs_law"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) %s\(" % k, kernels), k
    for used in ("rows_slot<", "lift_pack(", "class_zero<", "class_flush<", "__ballot(", "__popcll("):
        assert used in kernels, used
    for used in ("rows_build(", "lift_release_snapshot(c)", "rows_free_temp(", "hipMemGetInfo"):
        assert used in source, used
    assert "asm" not in kernels and "__builtin_amdgcn" not in kernels  # plain C++: ordinary vector stores and atomics only
    assert int(re.search(r"#define PAIRS_MAX_EDGES (\d+)", kernels).group(1)) == __import__("instagraal_amd.pairs_lift", fromlist=["x"]).MAX_EDGES
    assert re.search(r"#define PAIRS_PASSES \(PAIRS_P_LAW \+ 1\)", source) and len(hip_lib.PAIRS_PASSES) == 1 + len(hip_lib.ASSEMBLY_CONTACTS_PASSES) + 1
    for dep in ("ig_kernels_pairs.cuh", "ig_host_pairs.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_the_python_layers_reach_them_and_the_defaults_stay():
    from instagraal_amd import hip_lib, pairs_lift as pl, zoom_levels as zl
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("pairs_begin", "pairs_lift", "pairs_pixels", "pairs_law", "pairs_clear", "pairs_end", "debug_pairs_time"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(sampler.lift_pairs)[1:] == [("contig", EMPTY), ("pos1", EMPTY), ("contig2", EMPTY), ("pos2", EMPTY), ("strands", None)]
    assert params(sampler.pairs_contacts)[1:] == [("pairs", EMPTY), ("binsize", None), ("units", None), ("balance", False)]
    assert params(sampler.write_pairs_zoom_levels)[1:5] == [("folder", EMPTY), ("pairs", EMPTY), ("resolutions", zl.DEFAULT_RESOLUTIONS), ("scaffolds", True)]
    assert params(sampler.pairs_distance_law)[1:] == [("pairs", EMPTY), ("edges_bp", None), ("flip_strands", True)]
    assert params(sampler.write_lifted_pairs)[1:3] == [("pairs_path", EMPTY), ("out_path", EMPTY)] and callable(sampler.display_pairs_distance_law)
    for f in (run_instagraal, instagraal_class.full_em):
        assert inspect.signature(f).parameters["pairs"].default is None and inspect.signature(f).parameters["save_lifted_pairs"].default is False
    assert pl.SCALARS[:6] == ("pairs_in", "pairs_kept", "end1_not_covered", "end2_not_covered", "unplaced", "pairs_stored")
    assert pl.UNIT_KINDS == ("sub", "bin", "binsize", "scaffold") and pl.STRAND_COMBOS == ("++", "+-", "-+", "--") and (pl.KEPT, pl.UNPLACED) == (0, 3)
    assert params(pl.law_host) == [("lifted", EMPTY), ("strands", EMPTY), ("edges_bp", EMPTY), ("flip_strands", True)]
