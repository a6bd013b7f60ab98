"""Host tests of the balancing's entries from a built map (instagraal_amd.balance.entries_of_rows / balance_rows_host, pure numpy):
against a dense construction in Python integers, against ``entries_host`` on the contacts the map was made from, against the dense
ICE of tests/test_balance_host.py, the modes, counts beyond 32 bits, the 2^53 refusal and every ValueError.  No GPU."""
import numpy as np
import pytest

ARRAYS = ("rowptr", "col", "count", "nnz", "total")


def _random_map(U, seed, density=0.2, big=False):
    """an upper-triangular CSR map with a diagonal -> (rowptr, col int32, count)"""
    rng = np.random.default_rng(seed)
    keep = np.triu(rng.random((U, U)) < density)
    cnt = np.where(keep, rng.integers(0, 40, (U, U)), -1)  # (a kept entry may count 0: it stays an entry)
    if big:
        cnt = np.where(keep & (rng.random((U, U)) < 0.1), rng.integers(1 << 33, 1 << 40, (U, U)), cnt)
    u, v = np.nonzero(cnt >= 0)
    rowptr = np.zeros(U + 1, np.int64)
    np.add.at(rowptr, u + 1, 1)
    return np.cumsum(rowptr), v.astype(np.int32), cnt[u, v].astype(np.int64)


def _dense_rule(rowptr, col, count, d, group, mode):
    """the rule by a dense construction in Python integers: the symmetric matrix of the pixels with the band and the blocks outside
    the mode zeroed (None: no entry) -> (matrix, the four observed sums)"""
    U = len(rowptr) - 1
    A = [[None] * U for _ in range(U)]
    sums = dict(within=0, band=0, other=0, kept=0)
    for u in range(U):
        for e in range(int(rowptr[u]), int(rowptr[u + 1])):
            v, c = int(col[e]), int(count[e])
            if u == v:
                sums["within"] += c
            elif v - u < d:
                sums["band"] += c
            elif mode != "all" and (group[u] == group[v]) != (mode == "cis"):
                sums["other"] += c
            else:
                sums["kept"] += c
                A[u][v] = A[v][u] = c
    return A, sums


def _assert_is_the_dense_rule(ent, A, sums, total_in):
    from instagraal_amd import balance as bal

    U = len(A)
    rows = [[(v, c) for v, c in enumerate(A[u]) if c is not None] for u in range(U)]
    assert ent["rowptr"].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    assert ent["col"].tolist() == [v for r in rows for v, _ in r] and ent["count"].tolist() == [c for r in rows for _, c in r]
    assert ent["nnz"].tolist() == [len(r) for r in rows] and ent["total"].tolist() == [sum(c for _, c in r) for r in rows]
    assert [ent[k + "_observed"] for k in ("within", "band", "other", "kept")] == [sums[k] for k in ("within", "band", "other", "kept")]
    assert ent["entries"] == ent["entries_out"] == 2 * sum(c is not None for u in range(U) for c in A[u][u:]) == ent["col"].size
    assert ent["n_units"] == U and bal.snapshot_observed_total(ent) == total_in  # the scalar identity
    assert ent["rowptr"].dtype == ent["count"].dtype == ent["nnz"].dtype == ent["total"].dtype == np.int64 and ent["col"].dtype == np.int32


@pytest.mark.parametrize("U,seed,big", ((1, 1, False), (2, 2, False), (13, 3, False), (40, 4, True), (71, 5, True)))
def test_entries_of_rows_against_the_dense_construction(U, seed, big):
    from instagraal_amd import balance as bal

    rowptr, col, count = _random_map(U, seed, big=big)
    rng = np.random.default_rng(seed + 100)
    group = np.sort(rng.integers(0, 4, U)) * 3 + 2
    for d in (1, 2, 5):
        for mode in bal.MODES:
            ent = bal.entries_of_rows(rowptr, col, count, d, group, mode)
            _assert_is_the_dense_rule(ent, *_dense_rule(rowptr, col, count, d, group, mode), sum(count.tolist()))
            assert ent["entries_in"] == col.size
    assert bal.entries_of_rows(rowptr, col, count)["col"].tobytes() == bal.entries_of_rows(rowptr, col, count, 2, None, "all")["col"].tobytes()
    assert bal.SNAPSHOT_SCALARS == ("within_observed", "band_observed", "other_observed", "kept_observed", "entries", "entries_in", "n_units", "entries_out")
    assert bal.MODES == ("all", "cis", "trans")


@pytest.fixture(scope="module")
def tiny():
    import test_balance_host as tb

    return tb._problem("tiny")


@pytest.mark.parametrize("what", ("bin", 2500, "scaffold-like"))
def test_the_two_routes_give_the_same_bytes(tiny, what):
    """a snapshot made from the contacts by zoom_levels.lift_units_host, then entries_of_rows, is entries_host on the same units"""
    from instagraal_amd import balance as bal, zoom_levels as zl

    prob, position, unit = tiny
    if what == 2500:  # units with gaps: every third unit holds no position
        unit = np.arange(position.size, dtype=np.int64) // 4 * 3 // 2
    elif what != "bin":
        unit = unit // 9
    U = int(unit[-1]) + 1
    snap = zl.lift_units_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, unit, U)
    key, U2 = bal.keys_of(position, "bin", unit)
    assert U2 == U
    for d in (1, 2, 4):
        want = bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, d)
        got = bal.entries_of_rows(snap["rowptr"], snap["col"], snap["count"], d)
        for k in ARRAYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, d, k)
        for k in ("within_observed", "band_observed", "kept_observed", "n_units", "entries_out"):
            assert got[k] == want[k], (what, d, k)
        # (entries counts what was emitted: twice the kept contacts there, twice the kept pixels -- already summed -- here)
        assert got["other_observed"] == 0 and want["unplaced_observed"] == 0 and got["entries"] == got["entries_out"] <= want["entries"]


@pytest.mark.parametrize("n_iters", (17, 41, 98))
def test_balance_rows_host_against_the_dense_ice(tiny, n_iters):
    """the rows are the bytes of entries_host (the test above), so the bound of tests/test_balance_host.py holds as it stands: DENSE_RTOL,
    10 times the largest relative difference measured there"""
    import test_balance_host as tb
    from instagraal_amd import balance as bal, zoom_levels as zl

    prob, position, unit = tiny
    U = int(unit[-1]) + 1
    snap = zl.lift_units_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, unit, U)
    for d in (1, 2):
        got = bal.balance_rows_host(snap["rowptr"], snap["col"], snap["count"], ignore_diags=d, tol=0.0, max_iters=n_iters)
        assert got["n_iters"] == n_iters and not got["converged"] and not got["masked"].any() and got["mode"] == "all" and got["ignore_diags"] == d
        b, marg = tb._dense_ice(tb._dense(got), np.ones(U), n_iters)
        err = np.max(np.abs(got["b"] - b) / b)
        print("dense reference: ignore_diags=%d n_iters=%d max relative difference %.3g" % (d, n_iters, err))
        assert err <= tb.DENSE_RTOL and np.allclose(got["marg_final"], marg, rtol=1e-12)
        # the chain is balance_host's
        key, _ = bal.keys_of(position, "bin", unit)
        want = bal.balance_entries(bal.entries_host(key, U, prob.coo_row, prob.coo_col, prob.coo_cnt, d), tol=0.0, max_iters=n_iters)
        assert got["weight"].tobytes() == want["weight"].tobytes() and got["variance"].tobytes() == want["variance"].tobytes() and got["scale"] == want["scale"]
    kw = dict(bal.DEFAULTS)
    assert bal.balance_rows_host(snap["rowptr"], snap["col"], snap["count"], None, "all", **kw)["weight"].tobytes() == \
        bal.balance_rows_host(snap["rowptr"], snap["col"], snap["count"])["weight"].tobytes()


def test_modes_that_keep_nothing_and_balanced_blocks():
    from instagraal_amd import balance as bal

    U = 30
    rowptr, col, count = _random_map(U, 9, density=0.6)
    off = sum(c for u in range(U) for v, c in zip(col[rowptr[u]:rowptr[u + 1]].tolist(), count[rowptr[u]:rowptr[u + 1]].tolist()) if v - u >= 1)
    cis = bal.entries_of_rows(rowptr, col, count, 1, np.arange(U), "cis")  # groups of one unit each
    assert cis["entries"] == 0 and cis["other_observed"] == off and not cis["rowptr"].any() and cis["col"].size == 0
    trans = bal.entries_of_rows(rowptr, col, count, 1, np.zeros(U, np.int64), "trans")  # one group
    assert trans["entries"] == 0 and trans["other_observed"] == off and trans["kept_observed"] == 0
    everything = bal.entries_of_rows(rowptr, col, count, 1)
    for group, mode in ((np.zeros(U, np.int64), "cis"), (np.arange(U), "trans")):
        got = bal.entries_of_rows(rowptr, col, count, 1, group, mode)
        assert all(got[k].tobytes() == everything[k].tobytes() for k in ARRAYS) and got["other_observed"] == 0
    # "cis" with two groups: no kept entry crosses them, and inside each group the weights balance its block -- the marginals of a
    # group's units are equal.  Nothing ties the two groups' scales together (the rule has ONE mean over all units), so their ratio
    # swaps from iteration to iteration and the variance does not fall below it: not converged, as documented
    group = np.repeat([0, 1], (12, 18))
    both = bal.balance_rows_host(rowptr, col, count, group, "cis", ignore_diags=1, min_nnz=1, tol=1e-12, max_iters=400)
    assert np.isfinite(both["weight"]).all() and both["n_iters"] == 400 and both["other_observed"] > 0
    assert not (group[np.repeat(np.arange(U), both["nnz"])] != group[both["col"]]).any()
    marg = bal.marginals(both["rowptr"], both["col"].astype(np.int64), both["count"].astype(np.float64), both["weight"])
    for g in (0, 1):
        assert np.ptp(marg[group == g]) <= 1e-9 * marg[group == g].mean()
    res = bal.balance_rows_host(rowptr, col, count, np.arange(U), "cis", ignore_diags=1)
    assert res["n_iters"] == 0 and np.isnan(res["weight"]).all() and res["masked"].all()


def test_counts_beyond_32_bits_and_the_2_53_refusal():
    from instagraal_amd import balance as bal

    ent = bal.entries_of_rows([0, 1, 2, 2, 2], [2, 3], [1 << 40, 3], 2)
    assert ent["count"].tolist() == [1 << 40, 3, 1 << 40, 3] and ent["total"].tolist() == [1 << 40, 3, 1 << 40, 3] and ent["kept_observed"] == (1 << 40) + 3
    top = (1 << 53) - 1
    ent = bal.entries_of_rows([0, 2, 3, 3, 3, 3], [2, 3, 4], [top - 5, 5, 1])
    assert ent["total"].tolist() == [top, 1, top - 5, 5, 1]
    with pytest.raises(ValueError, match="sum to 2\\^53 or more"):
        bal.entries_of_rows([0, 2, 3, 3, 3, 3], [2, 3, 4], [top - 5, 6, 1])
    with pytest.raises(ValueError, match="sum to 2\\^53 or more"):
        bal.entries_of_rows([0, 1, 1, 1], [2], [1 << 62])
    with pytest.raises(ValueError, match="sum to 2\\^53 or more"):  # sums that would wrap an int64
        bal.entries_of_rows([0, 3, 3, 3, 3], [1, 2, 3], [(1 << 62) + 7] * 3, 1)
    # inside the band, on the diagonal or outside the mode such a count is counted and dropped, exactly
    ent = bal.entries_of_rows([0, 2, 2, 2], [0, 1], [1 << 62, (1 << 62) + 1], 2)
    assert ent["within_observed"] == 1 << 62 and ent["band_observed"] == (1 << 62) + 1 and ent["entries"] == 0
    ent = bal.entries_of_rows([0, 1, 1, 1], [2], [1 << 60], 1, [0, 0, 1], "cis")
    assert ent["other_observed"] == 1 << 60 and ent["entries"] == 0


def test_every_value_error():
    from instagraal_amd import balance as bal

    good = ([0, 2, 3, 3], [1, 2, 2], [4, 5, 6])
    assert bal.entries_of_rows(*good, 1)["entries"] == 6
    for d in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ignore_diags"):
            bal.entries_of_rows(*good, d)
    with pytest.raises(ValueError, match="mode is one of"):
        bal.entries_of_rows(*good, 2, [0, 0, 1], "both")
    for mode in ("cis", "trans"):
        with pytest.raises(ValueError, match="needs the group"):
            bal.entries_of_rows(*good, 2, None, mode)
        with pytest.raises(ValueError, match="one entry per unit"):
            bal.entries_of_rows(*good, 2, [0, 1], mode)
        with pytest.raises(ValueError, match="negative group"):
            bal.entries_of_rows(*good, 2, [0, -1, 1], mode)
        with pytest.raises(ValueError, match="needs the group"):
            bal.balance_rows_host(*good, None, mode)
    assert bal.entries_of_rows(*good, 1, [0, -1], "all")["entries"] == 6  # mode "all" reads no group
    for rowptr, col, count, words in (([1, 2, 3, 3], [1, 2, 2], [4, 5, 6], "rowptr"), ([0, 3, 2, 3], [1, 2, 2], [4, 5, 6], "rowptr"), ([], [], [], "rowptr"),
                                      ([0, 2, 3, 3], [1, 2], [4, 5], "entries each"), ([0, 2, 3, 3], [1, 2, 2], [4, 5], "entries each"),
                                      ([0, 2, 3, 3], [1, 2, 0], [4, 5, 6], "upper triangular"), ([0, 2, 3, 3], [1, 3, 2], [4, 5, 6], "upper triangular"),
                                      ([0, 2, 3, 3], [2, 1, 2], [4, 5, 6], "ascend strictly"), ([0, 2, 3, 3], [1, 1, 2], [4, 5, 6], "ascend strictly"),
                                      ([0, 2, 3, 3], [1, 2, 2], [4, -5, 6], "negative count")):
        with pytest.raises(ValueError, match=words):
            bal.entries_of_rows(rowptr, col, count)
    with pytest.raises(ValueError, match="max_iters"):
        bal.balance_rows_host(*good, max_iters=0)
    with pytest.raises(ValueError, match="tol"):
        bal.balance_rows_host(*good, tol=-1.0)


def test_the_weights_file_names_the_mode(tmp_path):
    """write_snapshot_weights is write_weights, byte for byte, and one more comment line with the mode and the scalars only this route
    has; read_weights reads it back to the same doubles"""
    from instagraal_amd import balance as bal, zoom_levels as zl

    rowptr, col, count = _random_map(30, 9, density=0.6)
    table = np.zeros(30, zl.FIXED_BINS_DTYPE)
    table["contig"], table["end"] = np.repeat([4, 7], (12, 18)), 1000
    for mode in bal.MODES:
        res = bal.balance_rows_host(rowptr, col, count, table["contig"], mode, ignore_diags=1, min_nnz=1)
        one, two = str(tmp_path / "plain.tsv"), str(tmp_path / (mode + ".tsv"))
        assert bal.write_weights(one, table, res) == bal.write_snapshot_weights(two, table, res) == 30
        a, b = open(one).read(), open(two).read()
        assert b == a + "# source=snapshot mode=%s other_observed=%d entries_in=%d\n" % (mode, res["other_observed"], col.size)
        assert (res["other_observed"] > 0) == (mode != "all")
        got = bal.read_weights(two)
        assert got[4].tobytes() == res["weight"].tobytes() and got[0].tolist() == list(range(30))
