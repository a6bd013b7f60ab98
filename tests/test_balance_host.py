"""Host tests of the balancing rule (instagraal_amd.balance, pure numpy): the ordered sum against a plain loop, the rule against an
independent dense ICE, scaling invariance, the masks, the refusals and the weights file.  No GPU."""
import numpy as np
import pytest

ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)


def _problem(cfg):
    """(the problem, position, unit of every position) with the fresh genome's order: the sub-fragments in their own order"""
    from instagraal_amd import assembly_contacts as ac, synth

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    return prob, np.arange(prob.n_sub_frags, dtype=np.int64), ac.units_along(parent)


@pytest.fixture(scope="module")
def tiny():
    return _problem("tiny")


@pytest.fixture(scope="module")
def tiny_bin_entries(tiny):
    from instagraal_amd import balance as bal

    prob, position, unit = tiny
    key, U = bal.keys_of(position, "bin", unit)
    return {d: bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, d) for d in (1, 2)}


def _dense(ent):
    U = ent["n_units"]
    A = np.zeros((U, U), np.float64)
    A[np.repeat(np.arange(U), np.diff(ent["rowptr"])), ent["col"]] = ent["count"]
    return A


def test_lane_sum_vectorised_equals_the_loop():
    from instagraal_amd import balance as bal

    rng = np.random.default_rng(1)
    rowptr = np.concatenate([[0], np.cumsum(ROW_LENGTHS)]).astype(np.int64)
    for values in (rng.random(rowptr[-1]), np.where(rng.random(rowptr[-1]) < 0.05, 1e16, 1.0), rng.standard_normal(rowptr[-1]) * 1e8):
        a, b = bal.lane_sum(values, rowptr), bal.lane_sum_loop(values, rowptr)
        assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert a[0] == 0.0 and not np.signbit(a[0]) and a[1] == values[0]
    x = rng.random(1000)
    assert np.float64(bal.vec_sum(x)).view(np.uint64) == bal.lane_sum_loop(x, [0, 1000]).view(np.uint64)[0]
    assert bal.vec_sum(np.zeros(0)) == 0.0 and bal.lane_sum(np.zeros(0), np.zeros(1, np.int64)).size == 0


def test_the_order_of_the_additions_shows_in_the_bytes():
    """what makes the device's byte comparison meaningful: on {1e16, 1, 1, ...} another order gives another double"""
    from instagraal_amd import balance as bal

    for n in (129, 200, 1001):
        v = np.ones(n)
        v[0] = 1e16
        ordered = bal.vec_sum(v)
        # (lane 0 holds 1e16 and loses every 1.0 added to it one at a time; the other lanes add theirs exactly)
        assert ordered == bal.lane_sum_loop(v, [0, n])[0]
        assert ordered != np.sum(v) and ordered != bal.vec_sum(v[::-1]) and ordered != float(np.cumsum(v)[-1])


def test_entries_are_symmetric_sorted_and_add_up(tiny, tiny_bin_entries):
    from instagraal_amd import balance as bal

    prob, position, unit = tiny
    total = int(prob.coo_cnt.astype(np.int64).sum())
    for level, max_side in (("sub", 2048), ("bin", 2048), ("map", 64), ("map", 2048)):
        key, U = bal.keys_of(position, level, unit, max_side)
        for d in (1, 2, 3):
            ent = bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, d)
            A = _dense(ent)
            assert np.array_equal(A, A.T) and not np.diag(A).any() and bal.observed_total(ent) == total
            i, j = np.nonzero(A)
            assert np.all(np.abs(i - j) >= d) and np.array_equal(ent["col"], j) and ent["entries_out"] == i.size
            assert np.array_equal(ent["nnz"], (A != 0).sum(1)) and np.array_equal(ent["total"], A.sum(1).astype(np.int64))
            assert int(ent["count"].sum()) == 2 * ent["kept_observed"] and ent["n_units"] == U and (d == 1) == (ent["band_observed"] == 0)
    key, U = bal.keys_of(position, "sub")
    key[prob.coo_row[0]] = -1  # an unplaced sub-fragment: its contacts are counted apart
    ent = bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, 1)
    assert ent["unplaced_observed"] > 0 and bal.observed_total(ent) == total


# the rule against the dense reference below over 17, 41 and 98 iterations on tiny at bin level, ignore_diags 1 and 2: the largest
# relative difference of b measured on the CPU was 1.49e-15 (98 iterations, ignore_diags 1; the prototype's: 1.1e-15); times 10 for
# summation-order noise
DENSE_RTOL = 10 * 1.49e-15


def _dense_ice(A, b0, n_iters):
    """cooler's update with numpy's own sums"""
    b = b0.copy()
    for _ in range(n_iters):
        marg = b * (A @ b)
        nz = marg != 0
        m = np.where(nz, marg / np.mean(marg[nz]), 1.0)
        b = b / m
    return b, b * (A @ b)


@pytest.mark.parametrize("n_iters", (17, 41, 98))
def test_the_rule_against_a_dense_reference(tiny_bin_entries, n_iters):
    """measured here: max |b - b_dense| / b_dense = 5.9e-16 / 7.1e-16 (17 iterations, ignore_diags 1 / 2), 1.04e-15 / 1.17e-15 (41),
    1.49e-15 / 5.6e-16 (98); the bound is DENSE_RTOL = 10 times the largest"""
    from instagraal_amd import balance as bal

    for d, ent in tiny_bin_entries.items():
        masked = bal.mask_units(ent["nnz"], ent["total"])
        assert not masked.any()
        b0 = np.ones(ent["n_units"])
        got = bal.iterate(ent["rowptr"], ent["col"], ent["count"], b0, 0.0, n_iters)
        assert got["n_iters"] == n_iters and not got["converged"] and got["variance"].size == n_iters
        b, marg = _dense_ice(_dense(ent), b0, n_iters)
        err = np.max(np.abs(got["b"] - b) / b)
        print("dense reference: ignore_diags=%d n_iters=%d max relative difference %.3g" % (d, n_iters, err))
        assert err <= DENSE_RTOL
        assert np.allclose(got["marg_final"], marg, rtol=1e-12) and np.all(np.diff(got["variance"][:10]) < 0)


# the spread of w'_i beta_i / w_i over the units measured on the CPU on tiny at bin level: 4.46e-11 (the prototype's: 3.4e-10); times 10
SCALING_SPREAD = 10 * 4.46e-11


def test_scaling_invariance(tiny, tiny_bin_entries):
    """balancing A and diag(beta) A diag(beta), beta in {1, 2, 3}, gives weights with w'_i beta_i / w_i constant.  Measured here: a
    relative spread of 4.46e-11 at tol = 1e-20 (reached after 98 and 108 of at most 5000 iterations); the bound is SCALING_SPREAD"""
    from instagraal_amd import balance as bal

    ent = tiny_bin_entries[2]
    U = ent["n_units"]
    beta = np.random.default_rng(3).integers(1, 4, U)
    scaled = dict(ent)
    row = np.repeat(np.arange(U), np.diff(ent["rowptr"]))
    scaled["count"] = ent["count"] * beta[row] * beta[ent["col"]]
    scaled["total"] = np.bincount(row, scaled["count"], U).astype(np.int64)
    a = bal.balance_entries(ent, tol=1e-20, max_iters=5000)
    b = bal.balance_entries(scaled, tol=1e-20, max_iters=5000)
    assert a["converged"] and b["converged"] and a["n_iters"] < 5000 and b["n_iters"] < 5000
    ratio = b["weight"] * beta / a["weight"]
    spread = (ratio.max() - ratio.min()) / ratio.mean()
    print("scaling invariance: relative spread %.3g after %d / %d iterations" % (spread, a["n_iters"], b["n_iters"]))
    assert spread <= SCALING_SPREAD
    # and the balanced matrix has unit row sums, the same for both
    for r in (a, b):
        bm = bal.balanced(r["count"], row, r["col"], r["weight"])
        assert np.allclose(np.bincount(row, bm, U), 1.0, atol=1e-8)


def test_masks(tiny_bin_entries):
    from instagraal_amd import balance as bal

    ent = tiny_bin_entries[2]
    U = ent["n_units"]
    med = int(np.median(ent["nnz"]))
    res = bal.balance_entries(ent, min_nnz=med)
    m = res["masked"]
    assert m.any() and (~m).any() and np.array_equal(m, ent["nnz"] < med)
    assert np.all(res["b"][m] == 0.0) and np.isnan(res["weight"][m]).all() and np.isfinite(res["weight"][~m]).all() and res["converged"]
    # a unit whose partners are all masked: its marginal is zero, its weight nan, though it is not masked itself
    row = np.repeat(np.arange(U), np.diff(ent["rowptr"]))
    u = int(np.argmin(ent["nnz"]))
    partners = ent["col"][ent["rowptr"][u]:ent["rowptr"][u + 1]]
    b0 = np.ones(U)
    b0[partners] = 0.0
    run = bal.iterate(ent["rowptr"], ent["col"], ent["count"], b0)
    masked = b0 == 0.0
    w, scale = bal.finish(run["b"], run["marg_final"], masked)
    assert not masked[u] and run["marg_final"][u] == 0.0 and np.isnan(w[u]) and run["b"][u] == 1.0 and np.isfinite(scale)
    # min_count and cooler's MAD filter
    assert np.array_equal(bal.mask_units(ent["nnz"], ent["total"], 0, int(np.median(ent["total"]))), ent["total"] < int(np.median(ent["total"])))
    lg = np.log(ent["total"].astype(np.float64))
    cut = np.median(lg) - 1.0 * np.median(np.abs(lg - np.median(lg)))
    mad = bal.mask_units(ent["nnz"], ent["total"], 0, 0, 1.0)
    assert np.array_equal(mad, lg < cut) and mad.any() and not mad.all() and not bal.mask_units(ent["nnz"], ent["total"], 0, 0, 0).any()
    # every unit masked: no iteration, not converged, no weight
    res = bal.balance_entries(ent, min_nnz=10 ** 6)
    assert res["masked"].all() and res["n_iters"] == 0 and not res["converged"] and np.isnan(res["weight"]).all() and np.isnan(res["scale"])


@pytest.mark.parametrize("cfg", ("tiny", "small"))
def test_the_default_mask_keeps_every_bin(cfg):
    from instagraal_amd import balance as bal

    prob, position, unit = _problem(cfg)
    for d in (1, 2):
        res = bal.balance_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, "bin", unit, ignore_diags=d)
        assert not res["masked"].any() and res["converged"] and 10 <= res["n_iters"] <= 40 and res["nnz"].max() > 64
        assert np.isfinite(res["weight"]).all() and res["variance"][-1] < 1e-5 <= res["variance"][-2]


def test_refusals(tiny):
    from instagraal_amd import balance as bal

    prob, position, unit = tiny
    args = (position, prob.coo_row, prob.coo_col, prob.coo_cnt, "bin", unit)
    for kw in (dict(ignore_diags=0), dict(ignore_diags=-1), dict(ignore_diags=1.5), dict(tol=-1e-9), dict(tol=float("nan")), dict(max_iters=0), dict(max_iters=2.5)):
        with pytest.raises(ValueError):
            bal.balance_host(*args, **kw)
    with pytest.raises(ValueError):
        bal.balance_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, "pixel")
    key, U = bal.keys_of(position, "bin", unit)
    with pytest.raises(ValueError, match="2\\^53"):
        bal.entries_host(key, U, prob.coo_row, prob.coo_col, np.full(prob.coo_cnt.size, 1 << 50, np.int64), 1)


def test_write_weights_round_trips(tiny, tmp_path):
    from instagraal_amd import assembly_contacts as ac, balance as bal

    prob, position, unit = tiny
    res = bal.balance_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, "bin", unit, min_nnz=int(np.median(np.bincount(unit))) + 40)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    table = ac.bins_table(position, parent, prob.S_o_A_frags["id_c"], np.ones(prob.n_frags, np.int64), np.full(prob.n_sub_frags, 1000), "bin")
    path = str(tmp_path / "weights.tsv")
    assert bal.write_weights(path, table, res) == res["n_units"] == table.size
    u, names, start, end, w = bal.read_weights(path)
    assert np.array_equal(w.view(np.uint64), res["weight"].view(np.uint64)) and np.isnan(w).any() and np.isfinite(w).any()
    assert np.array_equal(u, np.arange(w.size)) and np.array_equal(start, table["start"]) and np.array_equal(end, table["end"])
    assert names.tolist() == ac.scaffold_names(table["contig"]).tolist()
    lines = open(path).read().splitlines()
    assert lines[0][2:].split("\t") == list(bal.BALANCE_COLUMNS) == ["unit", "scaffold", "start", "end", "weight"]
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert int(sc["n_iters"]) == res["n_iters"] and all(int(sc[k]) == res[k] for k in bal.SCALARS)
    with pytest.raises(ValueError):
        bal.write_weights(path, table[:-1], res)
    assert np.array_equal(bal.balanced([2, 3], [0, 1], [1, 0], [0.5, 4.0]), [4.0, 6.0])
