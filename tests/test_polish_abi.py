"""The entry points of the polished FASTA of the polish step (csrc/ig_host_seq.inc): declared in include/instagraal_hip.h behind the
pre block, exported by the library, defined nowhere else, bound by hip_lib with the argument lists the header states, and reachable
from ``scaffold_polish.polish_assembly`` and ``simulation.run_and_polish``; ``run_instagraal`` stays as it was.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_seq_begin", "ig_seq_composition", "ig_seq_plan", "ig_seq_window", "ig_seq_out_composition", "ig_seq_end")
N_ARGS = dict(ig_seq_begin=6, ig_seq_composition=3, ig_seq_plan=16, ig_seq_window=5, ig_seq_out_composition=3, ig_seq_end=1)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import hip_lib, pre, scaffold_polish

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("int ig_seq_begin(") > header.index("int ig_pre_end(")  # behind the pre block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_seq.inc")).read()
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
        if name != "ig_host_seq.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_seq.cuh"') > unit.index('"ig_kernels_pre.cuh"') and unit.index('"ig_host_pre.inc"') < unit.index('"ig_host_seq.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_seq_buffers(") == 1
    assert "free_seq_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct SeqBuf {") == 1 and "SeqBuf seq;" in common
    # the two kernels the feature is made of; the layout check, the upload piece and the memory guard are the pre session's
    kernels = open(os.path.join(csrc, "ig_kernels_seq.cuh")).read()
    assert re.search(r"__global__ void __launch_bounds__\(\w+\) k_seq_composition\(", kernels) and re.search(r"__global__ void __launch_bounds__\(\w+\) k_seq_stitch\(", kernels)
    for used in ("wave_runs(", "wave_run_sum(", "atomicAdd(", "__shared__ unsigned char comp[256]", "(const uint4*)seq", "make_uint4("):
        assert used in kernels, used
    for used in ("records_layout_check(", "pre_memory_guard(", "PRE_UPLOAD_PIECE", "LiftTimer"):
        assert used in source, used
    pre_source = open(os.path.join(csrc, "ig_host_pre.inc")).read()
    assert pre_source.count("records_layout_check(") == 2  # defined once, called by ig_pre_begin: the two sessions refuse the same records
    assert "asm" not in kernels and "__builtin_amdgcn" not in kernels  # plain C++: ordinary vector loads, stores and atomics only
    # the constants the rule and the device share
    assert int(re.search(r"#define SEQ_NC (\d+)", kernels).group(1)) == len(scaffold_polish.CLASSES) == hip_lib.SEQ_CLASSES
    table = re.search(r'"([A-Z]{26})"\[i\]', kernels).group(1)
    for ch in pre.ALPHABET:
        assert table[ord(ch) - 65] == pre.COMPLEMENT[ch] == chr(scaffold_polish.COMPLEMENT[ord(ch)]), ch
    assert int(re.search(r"#define SEQ_THREADS (\d+)", kernels).group(1)) == 256  # the complement table in LDS is filled by one thread per byte
    for dep in ("ig_kernels_seq.cuh", "ig_host_seq.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_the_python_layers_reach_them_and_the_defaults_stay():
    from instagraal_amd import assembly_stats, hip_lib, scaffold_polish as sp
    from instagraal_amd.simulation import run_and_polish, run_instagraal

    for m in ("seq_begin", "seq_composition", "seq_plan", "seq_window", "seq_out_composition", "seq_end"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(sp.polish_assembly)[:11] == [("info_frags", EMPTY), ("fasta", None), ("output_dir", "out"), ("mode", "polishing"), ("criterion", None), ("min_scaffold_size", 0),
                                               ("min_scaffold_length", 0), ("junction", ""), ("lost", "reference"), ("device", True), ("width", 60)]
    assert params(sp.stitch_plan) == [("records", EMPTY), ("scaffolds", EMPTY), ("junction", ""), ("width", 60)]
    assert params(sp.integrate_lost_dna)[:3] == [("scaffolds", EMPTY), ("lost", EMPTY), ("mode", "reference")]
    assert sp.MODES == ("fasta", "singleton", "inversion", "inversion2", "rearrange", "reincorporation", "polishing")
    assert (sp.NEW_INFO_FRAGS_NAME, sp.POLISHED_GENOME_NAME) == ("new_info_frags.txt", "polished_genome.fa")
    assert sp.CLASSES == ("A", "C", "G", "T", "N", "other", "lower", "bases") and sp.DEFAULT_WINDOW == 1 << 28
    for f in ("compute_assembly_stats", "format_assembly_stats", "format_comparison_table"):
        assert callable(getattr(assembly_stats, f))
    # the polish behind a run is a function of its own: both of its switches default to off, and run_instagraal is as the pre feature left it
    d = dict(params(run_and_polish))
    assert d["post_polish"] is False and d["stats"] is False and d["lost"] == "reference"
    assert "post_polish" not in dict(params(run_instagraal)) and "stats" not in dict(params(run_instagraal))
    assert [k for k, _ in params(run_instagraal)][-2:] == ["pairs", "save_lifted_pairs"]
