"""GPU tests of the balancing of the contact map of the current genome (ig_balance_build / _rows / _fetch / _run, sampler.balance)
against the rule's host statement (instagraal_amd.balance) on the order downloaded from the same handle.  Every comparison of device
arrays is equality of bytes (doubles through .view(np.uint64))."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FORMS = ("wave", "packed")
STATES = ("tiny_fresh", "matrix_tiny_plain", "matrix_tiny_bomb", "small_fresh", "small_moved")
UNITS = (("sub", 2048), ("bin", 2048), ("map", 64), ("map", 2048))
IGNORE_DIAGS = (1, 2, 3)
ROW_ARRAYS = ("rowptr", "col", "count", "nnz", "total")
RUN_ARRAYS = ("b", "marg_final", "variance")


def _sampler(cfg, seed=None):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    if seed is not None:
        np.random.seed(seed)
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return prob, s


def _state(name):
    if name in ("matrix_tiny_plain", "matrix_tiny_bomb"):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        prob, s = _sampler(str(g["config"]), seed=11)
        s.ctx.upload_state(g["state"])
        s.modify_gl_cuda_buffer()
        s.eval_likelihood_init()
        assert np.array_equal(s.ctx.contact_map_order(), g["full_order_high"])
        return prob, s
    prob, s = _sampler(name.split("_")[0], seed=12)
    if name.endswith("moved"):
        s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
        assert np.any(np.diff(s.ctx.contact_map_order().astype(np.int64)) < 0)
    return prob, s


@pytest.fixture(scope="module", params=STATES)
def state(request):
    prob, s = _state(request.param)
    yield request.param, prob, s, {}
    s.free_gpu()


def _host_inputs(ctx, prob):
    from instagraal_amd import assembly_contacts as ac

    order = ctx.contact_map_order().astype(np.int64)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    return ac.positions_of(order, prob.n_sub_frags), ac.units_along(parent[order])


def _rule_rows(cache, ctx, prob, level, max_side, d, contacts=None):
    """the rule's entries, once per (level, max_side, ignore_diags) of a state"""
    from instagraal_amd import balance as bal

    key = ("rows", level, max_side, d)
    if key not in cache:
        position, unit = _host_inputs(ctx, prob)
        k, U = bal.keys_of(position, level, unit, max_side)
        row, col, cnt = contacts if contacts is not None else (prob.coo_row, prob.coo_col, prob.coo_cnt)
        cache[key] = bal.entries_host(k, U, row, col, cnt, d)
    return cache[key]


def _device_rows(ctx, level, max_side, d):
    res = ctx.balance_build(level, max_side, d)
    res["col"], res["count"] = ctx.balance_fetch(0, res["entries_out"])
    return res


def _assert_rows(got, want, what):
    from instagraal_amd import balance as bal

    for k in ROW_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    for k in bal.SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def _assert_run(got, want, what):
    for k in RUN_ARRAYS:
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, k, int((a.view(np.uint64) != b.view(np.uint64)).sum()) if a.shape == b.shape else (a.shape, b.shape))
    assert got["n_iters"] == want["n_iters"] and got["converged"] == want["converged"], (what, got["n_iters"], want["n_iters"])


def test_rows_equal_the_rule(state):
    from instagraal_amd import balance as bal

    name, prob, s, cache = state
    total = int(prob.coo_cnt.astype(np.int64).sum())
    for level, max_side in UNITS:
        for d in IGNORE_DIAGS:
            want = _rule_rows(cache, s.ctx, prob, level, max_side, d)
            got = _device_rows(s.ctx, level, max_side, d)
            _assert_rows(got, want, (name, level, max_side, d))
            assert bal.observed_total(got) == total and got["entries"] % 2 == 0
            assert int(got["count"].sum()) == 2 * got["kept_observed"] == int(got["total"].sum())
            assert got["kept_observed"] > 0 and (d == 1) == (got["band_observed"] == 0)
    s.ctx.balance_release()


def _run_cases(nnz):
    """(the mask's min_nnz, tol, max_iters): the defaults, five iterations exactly, a mask at the median"""
    return ((10, 1e-5, 200), (10, 0.0, 5), (int(np.median(nnz)), 1e-5, 200))


def test_runs_equal_the_rule_in_every_form_and_group(state):
    from instagraal_amd import balance as bal

    name, prob, s, cache = state
    for level, max_side, d in (("bin", 2048, 2), ("sub", 2048, 1), ("map", 64, 2), ("map", 8, 1)):
        ent = _rule_rows(cache, s.ctx, prob, level, max_side, d)
        if level == "bin":  # rows on both sides of a wave's 64 lanes, and of the packed form's 16
            assert ent["nnz"].max() > 64 > ent["nnz"].min(), (name, ent["nnz"].min(), ent["nnz"].max())
        if max_side == 8:  # every row is short: the packed form serves four of them per wave
            assert 0 < ent["nnz"].max() <= 16
        got_ent = _device_rows(s.ctx, level, max_side, d)
        _assert_rows(got_ent, ent, (name, level))
        for ci, (min_nnz, tol, max_iters) in enumerate(_run_cases(ent["nnz"])):
            if level != "bin" and ci != 0:
                continue
            masked = bal.mask_units(ent["nnz"], ent["total"], 1 if max_side == 8 else min_nnz)  # (eight pixels have seven partners at the most)
            if ci == 2:
                assert masked.any() and not masked.all()
            b0 = np.where(masked, 0.0, 1.0)
            want = bal.iterate(ent["rowptr"], ent["col"], ent["count"], b0, tol, max_iters)
            assert want["n_iters"] == 5 if ci == 1 else want["converged"], (name, level, ci, want["n_iters"])
            group = 7 if want["n_iters"] % 7 else 6  # (a group size that does not divide the iterations: the done flag stops inside a group)
            assert want["n_iters"] % group != 0
            for form in FORMS + ("default",):
                for g in ((1, group) if form != "default" else (0,)):
                    s.ctx.debug_balance_form(form)
                    s.ctx.debug_balance_group(g)
                    got = s.ctx.balance_run(b0, tol, max_iters)
                    _assert_run(got, want, (name, level, ci, form, g))
                    assert np.all(got["b"][masked] == 0.0)
        s.ctx.debug_balance_form("default")
        s.ctx.debug_balance_group(0)
    s.ctx.balance_release()


def test_public_balance_equals_the_rule(state):
    from instagraal_amd import balance as bal

    name, prob, s, cache = state
    position, unit = _host_inputs(s.ctx, prob)
    for level, max_side, kw in (("bin", 2048, {}), ("sub", 2048, dict(ignore_diags=3, min_nnz=5)), ("map", 64, dict(ignore_diags=1, mad_max=3))):
        want = bal.balance_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, level, unit, max_side, **kw)
        got = s.balance(level=level, max_side=max_side, **kw)
        for k in ("weight", "b", "marg_final", "variance"):
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (name, level, k)
        for k in ("masked", "nnz", "total", "rowptr"):
            assert np.array_equal(got[k], want[k]), (name, level, k)
        for k in bal.SCALARS + ("n_iters", "converged", "ignore_diags", "min_nnz", "min_count", "mad_max", "tol", "max_iters", "level"):
            assert got[k] == want[k], (name, level, k)
        assert np.float64(got["scale"]).view(np.uint64) == np.float64(want["scale"]).view(np.uint64)
        assert got["converged"] and np.isfinite(got["weight"][~got["masked"]]).all()
        assert (got["bins"] is None) == (level == "map") and (level == "map" or got["bins"].size == got["weight"].size)
        if level == "bin" and name in ("tiny_fresh", "small_fresh"):
            assert not got["masked"].any()  # (the default min_nnz masks nothing there: the byte comparisons skip no unit)


def test_balanced_map_and_balanced_contacts(state):
    from instagraal_amd import assembly_contacts as ac, balance as bal

    name, prob, s, _ = state
    image, b = s.contact_map(64)
    w = s.balance(level="map", max_side=64)["weight"]
    got, b2 = s.balanced_map(64)
    assert b2 == b and got.dtype == np.float64 and np.array_equal(got.view(np.uint64), (image.astype(np.float64) * np.outer(w, w)).view(np.uint64))
    ok = ~np.isnan(w)
    rows = np.nansum(np.where(np.abs(np.subtract.outer(np.arange(w.size), np.arange(w.size))) >= 2, got, 0.0), axis=1)
    # balanced: the row sums off the ignored band are about one.  The last variance, the mean over at most 64 rows of (row sum / mean
    # - 1)^2, is below 1e-5, so no single row is further off than sqrt(64e-5) = 0.025
    assert ok.any() and np.allclose(rows[ok], 1.0, atol=0.03)
    for level in ("sub", "bin"):
        res = s.assembly_contacts(level, balance=True)
        want_w = s.balance(level=level)["weight"]
        assert np.array_equal(res["weight"].view(np.uint64), want_w.view(np.uint64))
        want = bal.balanced(res["count"], ac.rows_of(res["rowptr"]), res["col"], want_w)
        assert np.array_equal(res["balanced"].view(np.uint64), want.view(np.uint64)) and res["balanced"].size == res["count"].size
        plain = s.assembly_contacts(level)
        assert "weight" not in plain and "balanced" not in plain
        for k in ("rowptr", "col", "count"):
            assert np.array_equal(plain[k], res[k])


def test_write_assembly_contacts_with_and_without_weights(tmp_path):
    from instagraal_amd import assembly_contacts as ac, balance as bal

    prob, s = _sampler("tiny", seed=21)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    files = ("bins.bed", "chrom.sizes", "pixels.tsv")
    for level in ("sub", "bin"):
        plain, with_w, direct = (str(tmp_path / ("%s_%s" % (k, level))) for k in ("plain", "weights", "direct"))
        out_plain = s.write_assembly_contacts(plain, level=level)
        out_w = s.write_assembly_contacts(with_w, level=level, balance=True)
        assert out_plain == out_w and sorted(os.listdir(plain)) == sorted(files) and sorted(os.listdir(with_w)) == sorted(files + ("weights.tsv",))
        # the three files, byte for byte: with weights, without, and straight from the writer on the arrays of assembly_contacts()
        res = s.assembly_contacts(level, diagonal=False)
        frame = s._assembly_contacts_frame(level, True)
        s.ctx.assembly_contacts_release()
        ac.write_all(direct, res["bins"], res["rowptr"], lambda a, n: (res["col"][a:a + n], res["count"][a:a + n]), ac.DEFAULT_BLOCK_ROWS, frame[3])
        for f in files:
            blob = open(os.path.join(plain, f), "rb").read()
            assert blob == open(os.path.join(with_w, f), "rb").read() == open(os.path.join(direct, f), "rb").read() and blob, (level, f)
        unit, names, start, end, weight = bal.read_weights(os.path.join(with_w, "weights.tsv"))
        want = s.balance(level=level)
        assert np.array_equal(weight.view(np.uint64), want["weight"].view(np.uint64)) and np.array_equal(unit, np.arange(weight.size))
        bed = [ln.split("\t") for ln in open(os.path.join(with_w, "bins.bed")).read().splitlines()]
        assert [b[0] for b in bed] == names.tolist() and [int(b[1]) for b in bed] == start.tolist() and [int(b[2]) for b in bed] == end.tolist()
    s.free_gpu()


def test_no_contacts_and_every_unit_masked():
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, soa17_from_dict

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    none = np.zeros(0, np.int32)
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    for form in FORMS:
        bare.debug_balance_form(form)
        for level in ("sub", "bin", "map"):
            ent = bare.balance_build(level, 64, 2)
            U = ent["n_units"]
            assert U > 0 and ent["entries"] == 0 == ent["entries_out"] and not ent["rowptr"].any() and not ent["nnz"].any() and not ent["total"].any()
            got = bare.balance_run(np.ones(U), 1e-5, 200)
            assert got["n_iters"] == 0 and got["converged"] is False and got["variance"].size == 0
            assert np.all(got["b"] == 1.0) and not got["marg_final"].any()
    bare.close()
    prob, s = _sampler("tiny")
    for form in FORMS:
        s.ctx.debug_balance_form(form)
        ent = s.ctx.balance_build("bin", 2048, 2)
        got = s.ctx.balance_run(np.zeros(ent["n_units"]), 1e-5, 200)  # every unit masked
        assert got["n_iters"] == 0 and got["converged"] is False and not got["b"].any() and not got["marg_final"].any()
    res = s.balance(min_nnz=10 ** 6)
    assert res["masked"].all() and res["n_iters"] == 0 and not res["converged"] and np.isnan(res["weight"]).all() and np.isnan(res["scale"])
    s.free_gpu()


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES, problem_to_context

    prob, s = _sampler("tiny")
    ref = _device_rows(s.ctx, "bin", 2048, 2)
    b0 = np.ones(ref["n_units"])
    ref_run = s.ctx.balance_run(b0, 1e-5, 200)

    def ok():
        _assert_rows(_device_rows(s.ctx, "bin", 2048, 2), ref, "again")
        _assert_run(s.ctx.balance_run(b0, 1e-5, 200), ref_run, "again")

    for bad in (0, -1):
        with pytest.raises(hip_lib.HipError, match="ig_balance_build.*ignore_diags"):
            s.ctx.balance_build("bin", 2048, bad)
    with pytest.raises(hip_lib.HipError, match="nothing is built"):  # (a refused build leaves no rows behind)
        s.ctx.balance_run(b0, 1e-5, 200)
    with pytest.raises(hip_lib.HipError, match="level"):
        s.ctx.balance_build(3, 2048, 2)
    with pytest.raises(hip_lib.HipError, match="max_side"):
        s.ctx.balance_build("map", 0, 2)
    ok()
    with pytest.raises(hip_lib.HipError, match="tol"):
        s.ctx.balance_run(b0, -1e-9, 200)
    with pytest.raises(hip_lib.HipError, match="tol"):
        s.ctx.balance_run(b0, float("nan"), 200)
    with pytest.raises(hip_lib.HipError, match="max_iters"):
        s.ctx.balance_run(b0, 1e-5, 0)
    with pytest.raises(hip_lib.HipError, match="out of range"):
        s.ctx.balance_fetch(1, ref["entries_out"])
    ok()
    s.ctx.balance_release()
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        s.ctx.balance_fetch(0, 1)
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        s.ctx.debug_balance_time("marginals", 1)
    # between ig_nuis_begin and ig_nuis_end the build refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_balance_build.*in flight"):
        s.ctx.balance_build("bin", 2048, 2)
    s.ctx.nuis_end()
    for kw in (dict(ignore_diags=0), dict(ignore_diags=1.5), dict(tol=-1.0), dict(max_iters=0), dict(level="pixel")):
        with pytest.raises(ValueError):
            s.balance(**kw)
    s.free_gpu()
    shard = problem_to_context(prob)
    shard.set_shard(0, 2)
    with pytest.raises(hip_lib.HipError, match="balancing needs all contacts on one handle"):
        shard.balance_build("bin", 2048, 2)
    shard.set_shard(0, 1)
    _assert_rows(_device_rows(shard, "bin", 2048, 2), ref, "whole again")
    ms = shard.debug_balance_time("marginals", 3), shard.debug_balance_time("iteration", 3), shard.debug_balance_build_time("bin", 2048, 2, 2)
    assert ms[0].shape == (3,) and ms[1].shape == (3,) and ms[2].shape == (2, len(hip_lib.BALANCE_BUILD_PASSES)) and all((m >= 0).all() for m in ms) and ms[2].sum() > 0
    _assert_run(shard.balance_run(b0, 1e-5, 200), ref_run, "behind the timed calls")
    shard.close()


def test_run_instagraal_save_weights_writes_one_file(tmp_path):
    from instagraal_amd import balance as bal, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=1, bomb=True, save_weights=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    assert [f for f in os.listdir(folder) if f.startswith("weights")] == ["weights.txt"]
    unit, names, start, end, weight = bal.read_weights(os.path.join(folder, "weights.txt"))
    res = s.balance(level="bin")
    assert np.array_equal(weight.view(np.uint64), res["weight"].view(np.uint64)) and weight.size == res["n_units"] > 0 and np.isfinite(weight).any()
    assert np.array_equal(start, res["bins"]["start"]) and np.array_equal(end, res["bins"]["end"])
    fasta = set(ln[1:].split()[0] for ln in open(os.path.join(folder, "genome.fasta")) if ln.startswith(">"))
    assert set(names.tolist()) <= fasta
    lines = open(os.path.join(folder, "weights.txt")).read().splitlines()
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    upper = s.sparse_matrix.tocoo()
    total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
    assert lines[0][2:].split("\t") == list(bal.BALANCE_COLUMNS) and sum(int(sc[k]) for k in bal.OBSERVED_SCALARS) == total
    assert int(sc["n_iters"]) == res["n_iters"] and sc["level"] == "bin"
    p2.simulation.release()
