"""The entry points of the balancing's rows from a built map (csrc/ig_host_balsnap.inc): declared in include/instagraal_hip.h in a block of
their own behind the pyramid's, exported by the library, defined nowhere else, bound by hip_lib with the argument lists the header
states, and reachable from the sampler and the run; the pinned names, defaults and signatures stay as they were.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_balance_build_snapshot", "ig_debug_balance_snapshot", "ig_debug_balance_snapshot_time")
# the number of arguments of every entry point in the header, the handle included: what the ctypes calls of hip_lib pass
N_ARGS = dict(ig_balance_build_snapshot=8, ig_debug_balance_snapshot=12, ig_debug_balance_snapshot_time=3)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import balance, hip_lib

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("int ig_balance_build_snapshot(") > header.index("int ig_debug_pyr_piece(")  # a block of its own behind the pyramid's
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_balsnap.inc")).read()
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
    for name in os.listdir(csrc):  # ... and defined nowhere else: the files whose exports other tests list stay as they were
        if name != "ig_host_balsnap.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    for used in ('"ig_kernels_wave.cuh"', '"ig_kernels_rows.cuh"', '"ig_kernels_zoom.cuh"', '"ig_kernels_pyr.cuh"'):  # wave_runs, rows_slot, zoom_row_of
        assert unit.index(used) < unit.index('"ig_kernels_balsnap.cuh"'), used
    for used in ('"ig_host_rows.inc"', '"ig_host_lift.inc"', '"ig_host_bal.inc"', '"ig_host_zoom.inc"', '"ig_host_pairs.inc"', '"ig_host_pyr.inc"'):
        assert unit.index(used) < unit.index('"ig_host_balsnap.inc"') < unit.index('"ig_host_batch.inc"'), used
    # a second BUILD, not a second balancer: the kernels are the two of the build, the iteration's are ig_kernels_bal.cuh's, the
    # buffers BalBuf's, freed by free_bal_buffers (which ig_destroy calls already)
    kernels = open(os.path.join(csrc, "ig_kernels_balsnap.cuh")).read()
    assert sorted(set(re.findall(r"\b(k_[a-z0-9_]+)\(", kernels))) == ["k_balsnap_emit", "k_balsnap_gather"]
    for used in ("template <bool SCATTER>", "rows_slot<SCATTER>(", "zoom_row_of(", "class_zero<BALSNAP_NS>(", "class_flush<BALSNAP_NS>(", "wave_runs(", "wave_run_sum<", "atomicAdd(&total["):
        assert used in kernels, used
    assert "asm" not in kernels and "__builtin" not in kernels and "lift_pack(" not in kernels  # plain C++; no 32-bit payload for a count
    assert source.count("c->nuis_in_flight || c->chain_busy") == 2 and "c->world != 1" in source  # both entry points refuse a handle that cannot answer
    for used in ("rows_build(", "free_bal_buffers(c)", "bal_free_build(c)", "bal_release_snapshot(c)", "LiftTimer timer(", "lift_release_snapshot(c)"):
        assert used in source, used
    assert source.count("rows_build(") == 1 and "lift_reduce_rows(" not in source and "k_bal_marginals" not in source and "struct " not in source
    assert re.search(r"const RowsSpec spec = \{p\.sc, BALSNAP_NS, BALSNAP_ENTRIES, \d+, [^;]*, false,", source)  # reduce = false, the memory guard on
    assert int(re.search(r"#define BALSNAP_NS (\d+)", kernels).group(1)) == int(re.search(r"#define BAL_NS (\d+)", open(os.path.join(csrc, "ig_kernels_bal.cuh")).read()).group(1)) == 5
    assert [int(re.search(r"#define BALSNAP_%s (\d+)" % k, kernels).group(1)) for k in ("WITHIN_OBS", "BAND_OBS", "OTHER_OBS", "KEPT_OBS", "ENTRIES")] == [0, 1, 2, 3, 4]
    assert balance.SNAPSHOT_SCALARS == ("within_observed", "band_observed", "other_observed", "kept_observed", "entries", "entries_in", "n_units", "entries_out")
    assert int(re.search(r"#define BALSNAP_PASSES (\d+)", source).group(1)) == len(hip_lib.BALANCE_SNAPSHOT_PASSES) == 7
    assert hip_lib.BALANCE_SNAPSHOT_PASSES == ("count", "rows", "scatter", "sort_short", "sort_lds", "sort_long", "gather")
    for dep in ("ig_kernels_balsnap.cuh", "ig_host_balsnap.inc"):  # a change of either rebuilds the library
        assert sum(d.endswith(dep) for d in hip_lib.DEPS) == 1
    assert all(os.path.exists(d) for d in hip_lib.DEPS)


def test_the_python_names_and_defaults():
    from instagraal_amd import balance, hip_lib
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import instagraal_class, run_balanced_pairs, run_instagraal

    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(hip_lib.Context.balance_build_snapshot) == [("self", EMPTY), ("ignore_diags", 2), ("mode", "all"), ("group", None)]
    assert params(hip_lib.Context.debug_balance_snapshot) == [("self", EMPTY), ("rowptr", EMPTY), ("col", EMPTY), ("count", EMPTY), ("ignore_diags", 2), ("mode", "all"),
                                                              ("group", None)]
    assert params(hip_lib.Context.debug_balance_snapshot_time) == [("self", EMPTY), ("n", 1)]
    assert params(balance.entries_of_rows) == [("rowptr", EMPTY), ("col", EMPTY), ("count", EMPTY), ("ignore_diags", 2), ("group", None), ("mode", "all")]
    assert params(balance.write_snapshot_weights) == [("path", EMPTY), ("table", EMPTY), ("result", EMPTY)] and params(balance.write_weights) == params(balance.write_snapshot_weights)
    assert params(balance.balance_rows_host) == [("rowptr", EMPTY), ("col", EMPTY), ("count", EMPTY), ("group", None), ("mode", "all")] + list(balance.DEFAULTS.items())
    assert params(sampler.pairs_balance) == [("self", EMPTY), ("pairs", EMPTY), ("binsize", None), ("units", None), ("mode", "all")] + list(balance.DEFAULTS.items())
    # what existing tests pin, as it was
    assert balance.LEVELS == ("sub", "bin", "map") and balance.DEFAULTS == dict(ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200)
    assert balance.SCALARS == ("unplaced_observed", "within_observed", "band_observed", "kept_observed", "entries", "n_placed", "n_units", "entries_out")
    assert params(sampler.pairs_contacts) == [("self", EMPTY), ("pairs", EMPTY), ("binsize", None), ("units", None), ("balance", False)]
    assert [k for k, _ in params(sampler.write_pairs_zoom_levels)] == ["self", "folder", "pairs", "resolutions", "scaffolds", "balance", "block_rows"]
    assert dict(params(sampler.write_pairs_zoom_levels))["balance"] is False
    assert [k for k, _ in params(sampler.write_zoom_levels)] == ["self", "folder", "resolutions", "scaffolds", "diagonal", "balance", "block_rows"]
    assert params(sampler.resolution_contacts) == [("self", EMPTY), ("binsize", None), ("units", None), ("diagonal", True), ("balance", False)]
    assert [k for k, _ in params(sampler.balance)] == ["self", "level", "max_side"] + list(balance.DEFAULTS)
    # the run: full_em takes the keyword; run_instagraal's signature is pinned by earlier tests, so the keyword's way in is a function of its own
    assert dict(params(instagraal_class.full_em))["balance_pairs"] is False and [k for k, _ in params(instagraal_class.full_em)][-1] == "balance_pairs"
    assert [k for k, _ in params(run_instagraal)][-2:] == ["pairs", "save_lifted_pairs"]
    from instagraal_amd.simulation import _run_instagraal

    forwarded = inspect.getsource(run_instagraal).split("return _run_instagraal(")[1]  # every parameter by name, nothing else
    assert [k for k, _ in params(_run_instagraal)] == [k for k, _ in params(run_instagraal)] + ["balance_pairs"]
    assert all(("%s=%s" % (k, k)) in forwarded for k, _ in params(run_instagraal)[2:]) and forwarded.startswith("hic_folder, reference_fa, ") and "locals()" not in forwarded
    assert params(run_balanced_pairs) == [("hic_folder", EMPTY), ("reference_fa", EMPTY), ("pairs", EMPTY), ("output_folder", None), ("balance_pairs", True),
                                          ("run_kw", EMPTY)]
    # the options of the writers' balance dict
    assert sampler._balance_options(True) == ("contacts", "all", {}) and sampler._balance_options(dict(tol=1e-3)) == ("contacts", "all", dict(tol=1e-3))
    assert sampler._balance_options(dict(source="snapshot", min_nnz=3)) == ("snapshot", "all", dict(min_nnz=3))
    assert sampler._balance_options(dict(mode="cis")) == ("snapshot", "cis", {}) and sampler._balance_options(dict(mode="trans", source="snapshot"))[0] == "snapshot"
    for bad, words in ((dict(source="pairs"), "source"), (dict(mode="cis", source="contacts"), "snapshot"), (dict(mode="both"), "mode")):
        try:
            sampler._balance_options(bad)
        except ValueError as e:
            assert words in str(e)
        else:
            raise AssertionError(bad)
