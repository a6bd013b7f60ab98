"""The entry points of the pyramid's contact levels (csrc/ig_host_pyr.inc): declared in include/instagraal_hip.h behind the seq block,
exported by the library, defined nowhere else, bound by hip_lib with the argument lists the header states, and reachable from
``pyramid_device`` and ``simulation.run_device_pyramid``; the pinned signatures stay as they were.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_pyr_begin", "ig_pyr_matrix", "ig_pyr_degrees", "ig_pyr_remap", "ig_pyr_rows", "ig_pyr_fetch", "ig_pyr_end", "ig_debug_pyr_piece")
# the number of arguments of every entry point in the header, the handle included: what the ctypes calls of hip_lib pass
N_ARGS = dict(ig_pyr_begin=7, ig_pyr_matrix=3, ig_pyr_degrees=2, ig_pyr_remap=8, ig_pyr_rows=3, ig_pyr_fetch=6, ig_pyr_end=1, ig_debug_pyr_piece=2)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import hip_lib, pyramid_levels

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("int ig_pyr_begin(") > header.index("int ig_seq_end(")  # behind the seq block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_pyr.inc")).read()
    defined = re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source)
    assert sorted(defined) == sorted(ENTRY_POINTS), sorted(set(defined) ^ set(ENTRY_POINTS))  # each once; nothing exported that the header does not declare
    binding = open(os.path.join(ROOT, "instagraal_amd", "hip_lib.py")).read()
    for name in ENTRY_POINTS:
        decl = _declaration(header, name)
        assert len(decl) == N_ARGS[name] and decl[0] == "ig_ctx* ctx", (name, decl)
        defn = re.search(r'extern "C" int %s\(([^)]*)\)' % name, source).group(1).replace("\n", " ").split(",")
        strip = lambda a: re.sub(r"\s+", " ", a.strip())  # noqa: E731
        assert [strip(a).replace("ig_ctx* c", "ig_ctx* ctx") for a in defn] == [strip(a) for a in decl], name  # the definition is the declaration
        assert binding.count("lib().%s(" % name) == 1, name
        _assert_bound_as_declared(header, binding, name)  # the live argtypes are the header's; one argument each, the handle first
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_pyr.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_pyr.cuh"') > unit.index('"ig_kernels_seq.cuh"') and unit.index('"ig_host_seq.inc"') < unit.index('"ig_host_pyr.inc"') < unit.index('"ig_host_batch.inc"')
    assert unit.index('"ig_host_rows.inc"') < unit.index('"ig_host_lift.inc"') < unit.index('"ig_host_pyr.inc"')  # rows_build and the LIFT_P_* passes it names
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_pyr_buffers(") == 1
    core = open(os.path.join(csrc, "ig_host_core.inc")).read()
    destroy = core[core.index('extern "C" void ig_destroy('):] if 'extern "C" void ig_destroy(' in core else core[core.index("ig_destroy("):]
    assert "free_pyr_buffers(c);" in destroy
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct PyrBuf {") == 1 and "PyrBuf pyr;" in common and "RowBuf rows[2];" in common
    # the kernels the feature is made of; the slots, the packing, the scalars and the rows are the shared ones
    kernels = open(os.path.join(csrc, "ig_kernels_pyr.cuh")).read()
    for k in ("k_pyr_canon", "k_pyr_emit", "k_pyr_largest", "k_pyr_degrees", "k_pyr_expand"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) %s\(" % k, kernels), k
    for used in ("rows_slot<", "lift_pack(", "class_zero<", "class_flush<", "wave_runs(", "wave_run_sum(", "raise_max(", "atomicAdd(", "atomicMin("):
        assert used in kernels, used
    for used in ("rows_build(", "rows_memory_guard(", "rows_free_temp(", "rows_free_result(", "LiftTimer timer(", "p.cur ^= 1"):
        assert used in source, used
    assert "lexsort" not in source and source.count("rows_build(") == 1  # one sort per level: the row builder's
    assert "asm" not in kernels and "__builtin" not in kernels  # plain C++: ordinary vector loads, stores and atomics only
    # the constants the rule and the device share
    assert int(re.search(r"#define PYR_LIMIT (0x[0-9a-f]+)ull", kernels).group(1), 16) == pyramid_levels.LIMIT == 1 << 31
    assert int(re.search(r"#define PYR_NS (\d+)", kernels).group(1)) == 4 and pyramid_levels.SCALARS[:4] == ("entries_in", "skipped", "dropped_by_lut", "entries_kept")
    assert [int(re.search(r"#define PYR_%s (\d+)" % k, kernels).group(1)) for k in ("IN", "SKIPPED", "DROPPED", "KEPT")] == [0, 1, 2, 3]
    assert pyramid_levels.SCALARS == ("entries_in", "skipped", "dropped_by_lut", "entries_kept", "pixels", "largest_sum")
    for dep in ("ig_kernels_pyr.cuh", "ig_host_pyr.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_the_python_layers_reach_them_and_the_pinned_signatures_stay():
    from instagraal_amd import hip_lib, pre, pyramid, pyramid_device
    from instagraal_amd.simulation import run_device_pyramid, run_from_pairs, run_instagraal

    for m in ("pyr_begin", "pyr_matrix", "pyr_degrees", "pyr_remap", "pyr_level", "pyr_end"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(pyramid_device.build_and_filter)[:7] == [("base_folder", EMPTY), ("size_pyramid", EMPTY), ("factor", EMPTY), ("thresh_factor", 1), ("output_folder", None),
                                                           ("device", True), ("level0", None)]
    assert params(pyramid_device.build)[:7] == [("base_folder", EMPTY), ("size_pyramid", EMPTY), ("factor", EMPTY), ("min_bin_per_contig", EMPTY), ("output_folder", None),
                                                ("device", True), ("level0", None)]
    assert [k for k, _ in params(run_device_pyramid)] == ["hic_folder", "reference_fa", "output_folder", "run_kw"] and dict(params(run_device_pyramid))["output_folder"] is None
    # the host path keeps its signatures; its two functions are a table part and a contact part now
    assert params(pyramid.build_and_filter) == [("base_folder", EMPTY), ("size_pyramid", EMPTY), ("factor", EMPTY), ("thresh_factor", 1), ("output_folder", None)]
    assert params(pyramid.build) == [("base_folder", EMPTY), ("size_pyramid", EMPTY), ("factor", EMPTY), ("min_bin_per_contig", EMPTY), ("output_folder", None)]
    assert [k for k, _ in params(pyramid.subsample_data_set)] == ["contig_info", "fragments_list", "fact_sub_sample", "abs_fragments_contacts", "new_abs_fragments_contacts_file",
                                                                 "min_bin_per_contig", "new_contig_list_file", "new_fragments_list_file", "old_2_new_file"]
    assert params(pyramid.remove_problematic_fragments) == [("contig_info", EMPTY), ("fragments_list", EMPTY), ("abs_fragments_contacts", EMPTY), ("new_contig_list_file", EMPTY),
                                                            ("new_fragments_list_file", EMPTY), ("new_abs_fragments_contacts_file", EMPTY), ("level0", EMPTY), ("thresh_factor", 1)]
    for f in ("subsample_tables", "subsample_contacts", "filter_tables", "filter_contacts"):
        assert callable(getattr(pyramid, f)), f
    # the signatures tests/test_pre_abi.py pins: as they were
    assert params(pre.run_pre) == [("fasta", EMPTY), ("pairs", EMPTY), ("enzymes", EMPTY), ("output_dir", EMPTY), ("device", True), ("plot", False),
                                   ("chunk_pairs", pre.DEFAULT_CHUNK_PAIRS)]
    assert [k for k, _ in params(run_from_pairs)] == ["fasta", "pairs", "enzymes", "output_folder", "run_kw"]
    want = ["hic_folder", "reference_fa", "output_folder", "level", "cycles", "coverage_std", "neighborhood", "device", "circular", "bomb", "pyramid_only", "save_pickle",
            "save_matrix", "simple", "save_law", "save_junctions", "save_contacts", "save_joins", "save_residuals", "save_placements", "save_orientations", "save_weights",
            "save_gaps", "save_resolutions", "save_segment_placements", "polish", "save_cut_join", "pairs", "save_lifted_pairs"]
    assert [k for k, _ in params(run_instagraal)] == want
    assert dict(params(run_instagraal))["level"] == 4 and dict(params(run_instagraal))["cycles"] == 100 and dict(params(run_instagraal))["coverage_std"] == 1
