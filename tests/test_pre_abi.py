"""The entry points of the input folder from a FASTA and read pairs (csrc/ig_host_pre.inc): declared in include/instagraal_hip.h behind
the pairs block, exported by the library, defined nowhere else, bound by hip_lib with the argument lists the header states, and
reachable from ``pre.run_pre`` and ``simulation.run_from_pairs``; ``run_instagraal`` stays as it was.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_pre_begin", "ig_pre_digest", "ig_pre_fragments", "ig_pre_add_pairs", "ig_pre_pixels_build", "ig_pre_pixels_rows", "ig_pre_pixels_fetch", "ig_pre_clear",
                "ig_pre_end")
# the number of arguments of every entry point in the header, the handle included: what the ctypes calls of hip_lib pass
N_ARGS = dict(ig_pre_begin=6, ig_pre_digest=8, ig_pre_fragments=7, ig_pre_add_pairs=8, ig_pre_pixels_build=4, ig_pre_pixels_rows=3, ig_pre_pixels_fetch=5, ig_pre_clear=1,
              ig_pre_end=1)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import hip_lib, pre

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("int ig_pre_begin(") > header.index("int ig_debug_pairs_time(")  # behind the pairs block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_pre.inc")).read()
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
        if name != "ig_host_pre.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_pre.cuh"') > unit.index('"ig_kernels_pairs.cuh"') and unit.index('"ig_host_pairs.inc"') < unit.index('"ig_host_pre.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_pre_buffers(") == 1
    assert "free_pre_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct PreBuf {") == 1 and "PreBuf pre;" in common
    # the kernels the feature is made of; the scan, the slots, the packing and the rows are the shared ones
    kernels = open(os.path.join(csrc, "ig_kernels_pre.cuh")).read()
    for k in ("k_pre_sites", "k_pre_marks", "k_pre_popc", "k_pre_cuts", "k_pre_frags", "k_pre_assign", "k_pre_emit"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) %s\(" % k, kernels), k
    for used in ("rows_slot<", "lift_pack(", "class_zero<", "class_flush<", "__ballot(", "__popcll(", "atomicOr("):
        assert used in kernels, used
    for used in ("rows_build(", "scan64_enqueue(", "rows_free_temp(", "hipMemGetInfo", "scan_chunks("):
        assert used in source, used
    assert "asm" not in kernels and "__builtin_amdgcn" not in kernels  # plain C++: ordinary vector loads, stores and atomics only
    # the constants the rule and the device share
    assert int(re.search(r"#define PRE_MAX_SITE (\d+)", kernels).group(1)) == pre.MAX_SITE and int(re.search(r"#define PRE_MAX_ENZYMES (\d+)", kernels).group(1)) == pre.MAX_ENZYMES
    bits = {k: int(re.search(r"#define PRE_BIT_%s (\d+)" % k, kernels).group(1)) for k in ("A", "C", "G", "T", "VALID")}
    assert bits == dict(A=pre.BIT_A, C=pre.BIT_C, G=pre.BIT_G, T=pre.BIT_T, VALID=pre.BIT_VALID)
    letters = sum(1 << int(k) for k in re.findall(r"1u << (\d+)", re.search(r"#define PRE_LETTERS (.*)", kernels).group(1)))
    assert letters == sum(1 << (ord(ch) - ord("A")) for ch in pre.ALPHABET)
    assert int(re.search(r"#define PRE_NS (\d+)", kernels).group(1)) == len(pre.SCALARS) - 1
    assert re.search(r"#define PRE_DIGEST_PASSES 4", source) and len(hip_lib.PRE_DIGEST_PASSES) == 4
    for dep in ("ig_kernels_pre.cuh", "ig_host_pre.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_the_python_layers_reach_them_and_the_defaults_stay():
    from instagraal_amd import hip_lib, pre
    from instagraal_amd.simulation import run_from_pairs, run_instagraal

    for m in ("pre_begin", "pre_digest", "pre_add_pairs", "pre_pixels", "pre_clear", "pre_end"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(pre.run_pre) == [("fasta", EMPTY), ("pairs", EMPTY), ("enzymes", EMPTY), ("output_dir", EMPTY), ("device", True), ("plot", False),
                                   ("chunk_pairs", pre.DEFAULT_CHUNK_PAIRS)]
    assert [k for k, _ in params(run_from_pairs)] == ["fasta", "pairs", "enzymes", "output_folder", "run_kw"]
    assert params(pre.display_matrix) == [("rowptr", EMPTY), ("col", EMPTY), ("count", EMPTY), ("max_display_bins", 1000)]
    assert pre.SCALARS == ("pairs_in", "pairs_kept", "end1_without_fragment", "end2_without_fragment", "ends_beyond_record", "pixels")
    # run_instagraal's own signature and defaults: as the pairs feature left them
    want = ["hic_folder", "reference_fa", "output_folder", "level", "cycles", "coverage_std", "neighborhood", "device", "circular", "bomb", "pyramid_only", "save_pickle",
            "save_matrix", "simple", "save_law", "save_junctions", "save_contacts", "save_joins", "save_residuals", "save_placements", "save_orientations", "save_weights",
            "save_gaps", "save_resolutions", "save_segment_placements", "polish", "save_cut_join", "pairs", "save_lifted_pairs"]
    assert [k for k, _ in params(run_instagraal)] == want
    assert dict(params(run_instagraal))["level"] == 4 and dict(params(run_instagraal))["cycles"] == 100 and dict(params(run_instagraal))["pairs"] is None
    for name in ("DpnII", "MboI", "Sau3AI", "HinfI", "DdeI", "MseI", "NlaIII", "HindIII", "EcoRI", "NcoI", "BglII", "Csp6I"):
        assert name in pre.ENZYMES
    assert pre.ENZYME_SETS["Arima"] == ("DpnII", "HinfI")
