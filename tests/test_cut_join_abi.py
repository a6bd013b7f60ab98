"""The cut and join scores' entry points (csrc/ig_host_cutjoin.inc): declared in include/instagraal_hip.h, exported by the library, bound
by hip_lib and reachable from the sampler and from a run; the defaults leave every existing call as it was.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRY_POINTS = ("ig_cut_scores", "ig_join_scores_build", "ig_join_scores_fetch", "ig_join_scores_release", "ig_debug_cut_join_form", "ig_debug_join_scores_forms",
                "ig_debug_cut_join_time", "ig_debug_contact_terms", "ig_contact_terms_host", "ig_zero_terms_host")
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_and_exported():
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("ig_cut_scores(") > header.index("ig_debug_edit_time(")  # behind the segment edits' block
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_cutjoin.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_cutjoin.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_cutjoin.cuh"') > unit.index('"ig_kernels_edit.cuh"') and unit.index('"ig_host_edit.inc"') < unit.index('"ig_host_cutjoin.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_cutjoin_buffers(") == 1
    assert "free_cutjoin_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct CutJoinBuf {") == 1 and "CutJoinBuf cutjoin;" in common
    # the kernels the feature is made of; the terms are the exact scorer's device functions, the scan and the rows the shared ones
    kernels = open(os.path.join(csrc, "ig_kernels_cutjoin.cuh")).read()
    for k in ("k_cut_span", "k_cut_zero", "k_cj_vk", "k_cj_pairs_emit", "k_cj_join", "k_cj_contig_zero", "k_cj_join_zero", "k_debug_contact_terms"):
        assert re.search(r"__global__ void (__launch_bounds__\(\w+\) )?%s\(" % k, kernels), k
    for used in ("eval_q(", "zero_q(", "wave_runs(", "wave_run_sum<", "rows_slot<", "lift_pack("):
        assert used in kernels, used
    for used in ("scan64_enqueue(", "rows_build(", "likelihood_of_limbs(", "flush_pending_sums(c)"):
        assert used in source, used
    assert int(re.search(r"#define CJ_LDS_PAIRS (\d+)", kernels).group(1)) == hip_lib.CUT_JOIN_LDS_PAIRS
    assert int(re.search(r"#define CJ_PASSES (\d+)", source).group(1)) == len(hip_lib.CUT_JOIN_PASSES)
    for i, name in enumerate(hip_lib.CUT_JOIN_PASSES):
        assert int(re.search(r"#define CJ_P_%s (\d+)" % name.upper(), source).group(1)) == i
    for dep in ("ig_kernels_cutjoin.cuh", "ig_host_cutjoin.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_the_python_layers_reach_them_and_the_defaults_stay():
    from instagraal_amd import cut_join as cj, hip_lib, rearrange as ra
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_instagraal

    for m in ("cut_scores", "join_scores", "debug_cut_join_form", "debug_join_scores_forms", "debug_cut_join_time", "debug_contact_terms"):
        assert callable(getattr(hip_lib.Context, m)), m
    assert callable(hip_lib.contact_terms_host) and callable(hip_lib.zero_terms_host)
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(hip_lib.contact_terms_host) == [(k, EMPTY) for k in ("params", "mean_kb", "s", "d", "trans", "count")]
    assert params(sampler.cut_scores)[1:] == [] and params(sampler.join_scores)[1:] == []
    assert params(sampler.weakest_cuts)[1:] == [("n", 20), ("cuts", None)] and params(sampler.strongest_joins)[1:] == [("n", 20), ("joins", None)]
    assert params(sampler.propose_cuts_joins)[1:] == [("n", 20), ("cuts", True), ("joins", True)]
    assert params(sampler.polish)[1:] == [("max_rounds", 10), ("n", 20), ("min_gain", 0.0), ("window", None), ("orientation_window", None), ("cuts", False), ("joins", False)]
    assert params(ra.propose_cuts_joins) == [("state", EMPTY), ("cuts", None), ("joins", None), ("n", 20)]
    assert params(cj.weakest_cuts) == [("state", EMPTY), ("cuts", EMPTY), ("n", 20)] and params(cj.strongest_joins) == [("joins", EMPTY), ("n", 20)]
    for f in (run_instagraal, instagraal_class.full_em):
        assert inspect.signature(f).parameters["save_cut_join"].default is False and inspect.signature(f).parameters["polish"].default is False
    assert (cj.HEAD, cj.TAIL) == (0, 1) and cj.CUT_DTYPE["edit"].shape == cj.LINK_DTYPE["edit"].shape == (5,)
    # the two host-only entries answer without a handle: a trans pair's term does not depend on s and d
    p8 = [50.0, 9.6, 1e-3, -1.5, 2.0, 250.0, 3.0e5, 5e-3]
    q = hip_lib.contact_terms_host(p8, 1.8, [1.0, 77.0, 1.0], [1, 40, 1], [1, 1, 0], [3, 3, 3])
    assert q[0] == q[1] != q[2] and q.dtype.name == "int64"
    z = hip_lib.zero_terms_host(p8, 1.8, [1, 2, 500], 600)
    assert (z < 0).all() and z[0] != z[1]
