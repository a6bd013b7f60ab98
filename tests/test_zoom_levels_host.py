"""CPU tests of the rule of the fixed-resolution maps (instagraal_amd.zoom_levels): ``lift_units_host`` at fixed bins and at
scaffold level against brute force -- the dense symmetric matrix permuted by the genome order, its upper triangle, block-summed by
unit -- on ``tiny`` under several genomes; ``binnify`` against its three-line restatement; the identity coarsen(direct at B) =
direct at f B on ``tiny`` and ``small``; ``plan``; the writers.  Every comparison is exact."""
import os

import numpy as np
import pytest

# about half the median sub-fragment length, 2 x and 7 x that
BINSIZES = {"tiny": (882, 3528, 12348), "small": (889, 3556, 12446)}
FACTORS = (2, 3, 5)


@pytest.fixture(scope="module")
def probs():
    from instagraal_amd import synth

    return {k: synth.make_problem(*synth.CONFIGS[k]) for k in BINSIZES}


def _genome(prob, kind, seed=0):
    """state arrays (pos, id_c, activ, id_d, ori) of a genome over the bins of ``prob`` (as test_assembly_contacts_host.py)"""
    S = prob.S_o_A_frags
    N = prob.n_frags
    pos, id_c, ori = S["pos"].astype(np.int64).copy(), S["id_c"].astype(np.int64).copy(), np.ones(N, np.int64)
    activ, id_d = np.ones(N, np.int64), S["id_d"].astype(np.int64).copy()
    rng = np.random.RandomState(seed)
    if kind == "shuffled":
        perm = rng.permutation(N)
        cuts = np.sort(rng.choice(np.arange(1, N), 12, replace=False))
        starts = np.concatenate([[0], cuts])
        lens = np.diff(np.concatenate([starts, [N]]))
        id_c[perm] = np.repeat(rng.permutation(starts.size) + 1, lens)
        pos[perm] = np.arange(N) - np.repeat(starts, lens)
        ori = rng.choice([-1, 1], N)
    elif kind == "unplaced":
        ids, n = np.unique(id_c, return_counts=True)
        activ[np.nonzero(id_c == ids[np.argmax(n >= 3)])[0][1]] = 0
    elif kind == "nothing placed":
        activ[:] = 0
    return pos, id_c, activ, id_d, ori


def _frame(prob, kind="fresh"):
    """-> (order, position, the sub-fragment table, the contacts)"""
    from instagraal_amd import assembly_contacts as ac, contact_map as cmap

    genome = _genome(prob, kind)
    order = np.asarray(cmap.genome_order(*genome, prob.np_sub_frags_id)[2], np.int64)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    table = ac.bins_table(order, parent, genome[1], genome[4], prob.S_o_A_sub_frags["len_bp"], "sub")
    row, col, cnt = (np.asarray(a, np.int64) for a in (prob.coo_row, prob.coo_col, prob.coo_cnt))
    if kind == "no contacts":
        row, col, cnt = row[:0], col[:0], cnt[:0]
    return order, ac.positions_of(order, prob.n_sub_frags), table, (row, col, cnt)


def _brute(prob, order, row, col, cnt, unit, U):
    M = prob.n_sub_frags
    S = np.zeros((M, M), np.int64)
    S[row, col] = cnt
    S = S + S.T
    D = np.triu(S[order][:, order], k=1)
    P = np.zeros((order.size, U), np.int64)
    P[np.arange(order.size), unit] = 1
    D = P.T @ D @ P
    assert not np.tril(D, k=-1).any()
    i, j = np.nonzero(D)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=U))]).astype(np.int64)
    return rowptr, j.astype(np.int32), D[i, j]


@pytest.mark.parametrize("kind", ["fresh", "shuffled", "unplaced", "nothing placed", "no contacts"])
def test_the_rule_equals_brute_force_on_tiny(probs, kind):
    from instagraal_amd import zoom_levels as zl

    prob = probs["tiny"]
    order, position, table, (row, col, cnt) = _frame(prob, kind)
    T = order.size
    assert (T == 0) == (kind == "nothing placed")
    tables = [zl.units_of_positions(table, B) for B in BINSIZES["tiny"][1:]] + [zl.scaffold_units(table)]
    for unit, U in tables:
        assert unit.dtype == np.int64 and unit.size == T and (T == 0 or (np.all(np.diff(unit) >= 0) and 0 <= unit.min() and unit.max() < U))
        got = zl.lift_units_host(position, row, col, cnt, unit, U)
        rowptr, c, v = _brute(prob, order, row, col, cnt, unit, U)
        assert got["rowptr"].dtype == np.int64 and got["col"].dtype == np.int32 and got["count"].dtype == np.int64
        assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["col"], c) and np.array_equal(got["count"], v), kind
        assert got["contacts_kept"] + got["contacts_unplaced"] == int(cnt.sum()) and int(got["count"].sum()) == got["contacts_kept"]
        assert got["entries_kept"] + got["entries_unplaced"] == got["entries_in"] == row.size
        assert got["entries_out"] == got["col"].size == got["rowptr"][-1] and got["n_placed"] == T and got["n_units"] == U
        assert (got["entries_unplaced"] > 0) == (kind in ("unplaced", "nothing placed"))
        r = np.repeat(np.arange(U), np.diff(got["rowptr"]))
        assert np.all(r <= got["col"]) and np.all(np.diff(got["col"].astype(np.int64))[r[1:] == r[:-1]] > 0)
    if T:  # the scaffold units are the ranks of the scaffolds, and a scaffold is one run of the order
        unit, U = tables[-1]
        assert U == np.unique(table["contig"]).size and np.array_equal(np.unique(table["contig"], return_index=True)[1], np.nonzero(np.diff(unit, prepend=-1))[0])


def test_with_the_bin_table_of_level_bin_the_rule_is_lift_host(probs):
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    prob = probs["tiny"]
    order, position, table, (row, col, cnt) = _frame(prob, "shuffled")
    unit = ac.units_along(prob.np_sub_frags_2_frags["x"].astype(np.int64)[order])
    a, b = ac.lift_host(position, row, col, cnt, unit), zl.lift_units_host(position, row, col, cnt, unit, int(unit[-1]) + 1)
    assert all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


def _restated(ids, sizes, B):
    return [(c, s, min(s + B, n)) for c, n in zip(ids, sizes) for s in (range(0, n, B) if n else [0])]


@pytest.mark.parametrize("sizes, B", [([10, 3, 25], 4), ([10, 3, 25], 100), ([5, 2], 1), ([12, 8, 4], 4), ([1], 1), ([7, 0, 9], 3)])
def test_binnify(sizes, B):
    from instagraal_amd import zoom_levels as zl

    ids = [7 + 2 * k for k in range(len(sizes))]
    t = zl.binnify((ids, sizes), B)
    assert [tuple(int(x) for x in r) for r in t.tolist()] == _restated(ids, sizes, B)
    nb, off = zl.bins_per_scaffold((ids, sizes), B)
    assert nb.tolist() == [max(1, -(-n // B)) for n in sizes] and off.tolist() == np.concatenate([[0], np.cumsum(nb)]).tolist() and t.size == off[-1]
    if B == 100:
        assert t.size == len(sizes)  # larger than every scaffold: one bin each, cut at its end
    if B == 1:
        assert t.size == sum(sizes)
    if sizes == [12, 8, 4]:
        assert np.all(t["end"] - t["start"] == B)  # exact multiples: no short last bin, no empty one behind it
    with pytest.raises(ValueError):
        zl.binnify((ids, sizes), 0)


def test_binnify_on_the_genome_and_units_of_positions(probs):
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    prob = probs["tiny"]
    order, position, table, _ = _frame(prob, "shuffled")
    for B in BINSIZES["tiny"]:
        ids, sizes = ac.chrom_sizes(table)
        bins = zl.binnify((ids, sizes), B)
        assert [tuple(r) for r in bins.tolist()] == _restated(ids.tolist(), sizes.tolist(), B)
        unit, U = zl.units_of_positions(table, B)
        assert U == bins.size
        mid = (table["start"] + table["end"]) // 2
        assert np.array_equal(bins["contig"][unit], table["contig"])  # the midpoint lies in its bin, of its scaffold
        inside = (bins["start"][unit] <= mid) & (mid < bins["end"][unit])
        assert np.all(inside | (table["end"] == table["start"]))  # (only a sub-fragment of 0 bp at its scaffold's end needs the min)
        assert ac.chrom_sizes(bins)[1].tolist() == sizes.tolist()


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_coarsening_a_level_is_building_the_coarser_level(probs, cfg):
    """the identity: 18 cases, and the chain x2 then x5 against x10"""
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    prob = probs[cfg]
    order, position, table, (row, col, cnt) = _frame(prob)
    sizes = ac.chrom_sizes(table)
    for B in BINSIZES[cfg]:
        unit, U = zl.units_of_positions(table, B)
        fine = zl.lift_units_host(position, row, col, cnt, unit, U)
        for f in FACTORS + (10,):
            m, C = zl.coarse_map(sizes, B, f)
            unit_c, U_c = zl.units_of_positions(table, f * B)
            assert C == U_c and np.array_equal(m[unit], unit_c)
            want = zl.lift_units_host(position, row, col, cnt, unit_c, U_c)
            got = zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], m, C)
            for g, k in zip(got, ("rowptr", "col", "count")):
                assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), (cfg, B, f, k)
        m2, C2 = zl.coarse_map(sizes, B, 2)
        m5, C5 = zl.coarse_map(sizes, 2 * B, 5)
        m10, C10 = zl.coarse_map(sizes, B, 10)
        assert C5 == C10 and np.array_equal(m5[m2], m10)
        chain = zl.coarsen_host(*zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], m2, C2), m5, C5)
        once = zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], m10, C10)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(chain, once))
        # down to the scaffolds
        ms, K = zl.scaffold_map(sizes, B)
        us, Ks = zl.scaffold_units(table)
        want = zl.lift_units_host(position, row, col, cnt, us, Ks)
        got = zl.coarsen_host(fine["rowptr"], fine["col"], fine["count"], ms, K)
        assert K == Ks and all(g.tobytes() == want[k].tobytes() for g, k in zip(got, ("rowptr", "col", "count")))


def test_units_without_position(probs):
    """below what the fragments carry a resolution has units no midpoint falls into; well above it has none"""
    from instagraal_amd import zoom_levels as zl

    seen = []
    for cfg in ("tiny", "small"):
        _, _, table, _ = _frame(probs[cfg])
        for B in BINSIZES[cfg]:
            unit, U = zl.units_of_positions(table, B)
            n = zl.units_without_position(unit, U)
            assert n == U - np.unique(unit).size == int((np.bincount(unit, minlength=U) == 0).sum())
            seen.append((cfg, B, n))
    by = {(c, b): n for c, b, n in seen}
    assert by[("tiny", 882)] > 0 and by[("small", 889)] > 0 and by[("small", 12446)] == 0, seen


def test_plan():
    from instagraal_amd import zoom_levels as zl

    assert zl.DEFAULT_RESOLUTIONS == (10_000, 20_000, 50_000, 100_000, 200_000, 500_000, 1_000_000)
    assert zl.plan(zl.DEFAULT_RESOLUTIONS) == [("direct",), ("coarsen", 2), ("direct",), ("coarsen", 2), ("coarsen", 2), ("direct",), ("coarsen", 2)]
    assert zl.plan((3556, 7112, 35560)) == [("direct",), ("coarsen", 2), ("coarsen", 5)]
    assert zl.plan([3, 5, 7]) == [("direct",)] * 3
    assert zl.plan([1000]) == [("direct",)]
    # 4 is a multiple of 2 but 6 is not one of 4: only the level built immediately before is resident
    assert zl.plan([2, 4, 6]) == [("direct",), ("coarsen", 2), ("direct",)]
    for bad in ([10, 10], [20, 10], [], [0, 5], [2.5]):
        with pytest.raises(ValueError):
            zl.plan(bad)


def test_arguments_are_checked():
    from instagraal_amd import zoom_levels as zl

    ok = zl.lift_units_host([0, 1, 2], [0], [2], [5], [0, 3, 3], 6)  # gaps are fine
    assert ok["rowptr"].tolist() == [0, 1, 1, 1, 1, 1, 1] and ok["col"].tolist() == [3] and ok["count"].tolist() == [5]
    with pytest.raises(ValueError, match="non-decreasing"):
        zl.lift_units_host([0, 1, 2], [0], [2], [5], [0, 2, 1], 6)
    with pytest.raises(ValueError, match="non-decreasing"):
        zl.lift_units_host([0, 1, 2], [0], [2], [5], [0, 2, 6], 6)
    with pytest.raises(ValueError, match="positions"):
        zl.lift_units_host([0, 1, 2], [0], [2], [5], [0, 2], 6)
    with pytest.raises(ValueError, match="2\\^31"):
        zl.check_units([0], 1 << 31)
    with pytest.raises(ValueError, match="coarse map"):
        zl.coarsen_host([0, 1, 1], [1], [1], [1, 0], 2)
    with pytest.raises(ValueError, match="coarse map"):
        zl.coarsen_host([0, 1, 1], [1], [1], [0], 2)
    r, c, v = zl.coarsen_host([0, 2, 3], [0, 1, 1], [1 << 40, 1 << 41, 5], [0, 0], 1)
    assert r.tolist() == [0, 1] and c.tolist() == [0] and v.tolist() == [(1 << 40) + (1 << 41) + 5]


def test_the_writers(tmp_path, probs):
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    prob = probs["tiny"]
    order, position, table, (row, col, cnt) = _frame(prob, "shuffled")
    sizes = ac.chrom_sizes(table)
    folder = str(tmp_path / "zoom")
    diag_sub = np.arange(order.size, dtype=np.int64) % 3  # self-contacts per position
    totals, texts = [], []
    levels = [(B, zl.units_of_positions(table, B), zl.binnify(sizes, B), zl.level_folder(folder, B)) for B in BINSIZES["tiny"][1:]]
    levels.append((None, zl.scaffold_units(table), zl.scaffold_table(table), zl.scaffold_folder(folder)))
    for B, (unit, U), bins, where in levels:
        res = zl.lift_units_host(position, row, col, cnt, unit, U)
        diag = np.zeros(U, np.int64)
        np.add.at(diag, unit, diag_sub)
        n = zl.write_level(where, bins, res["rowptr"], zl.fetch_of(res["col"], res["count"]), block_rows=7, diag=diag)
        assert sorted(os.listdir(where)) == ["bins.bed", "chrom.sizes", "pixels.tsv"]
        b1, b2, c = zl.read_pixels(os.path.join(where, "pixels.tsv"))
        rp, cc, vv = ac.merge_diagonal(0, res["rowptr"], res["col"], res["count"], diag)
        assert n == b1.size == cc.size and np.array_equal(b1, ac.rows_of(rp)) and np.array_equal(b2, cc) and np.array_equal(c, vv)
        assert int(c.sum()) == res["contacts_kept"] + int(diag_sub.sum())
        back = zl.read_bins_bed(os.path.join(where, "bins.bed"))
        assert back.tobytes() == bins.tobytes() and back.size == U
        totals.append(int(c.sum()))
        texts.append(open(os.path.join(where, "chrom.sizes")).read())
    assert len(set(totals)) == 1 and len(set(texts)) == 1 and texts[0].count("\n") == sizes[0].size
    assert os.path.isdir(os.path.join(folder, "resolutions", str(BINSIZES["tiny"][1]))) and os.path.isdir(os.path.join(folder, "scaffolds"))


# ---- the crafted CSR data the device's coarsening is run over (tests/test_hip_zoom_levels.py)

SEGMENTS = (0, 1, 2, 63, 64, 65, 1024, 1025, 3000)  # raw entries per coarse row (before equal columns are summed)


def crafted():
    """A fine level of U rows under a map to C coarse rows.  Coarse row k < len(SEGMENTS) takes SEGMENTS[k] raw entries, spread
    over three fine rows of which the middle one is empty; behind them: a coarse row whose fine rows are all empty, a coarse unit
    no fine unit maps to, a coarse row whose entries all lie on one mapped column, one with three entries of 2^31 - 1 on one pixel
    and one with a pixel summing to just under 2^62.  The columns of a row are strictly ascending and at or behind the row."""
    per = 3
    n_seg = len(SEGMENTS)
    # fine rows: per coarse row three; the coarse unit without a fine unit gets none
    coarse_rows = n_seg + 5  # ... all-empty, (no fine unit), one column, 3 x (2^31 - 1), just under 2^62
    m = []
    for R in range(coarse_rows):
        if R == n_seg + 1:
            continue
        m += [R] * per
    # a wide last coarse unit, so that long rows have enough columns at or behind them
    tail_R = coarse_rows
    U = len(m) + 3200
    m += [tail_R] * 3200
    m = np.array(m, np.int64)
    C_ = tail_R + 1
    rows = [[] for _ in range(U)]
    first_of = {int(R): int(np.argmax(m == R)) for R in np.unique(m)}
    tail0 = first_of[tail_R]
    for k, n in enumerate(SEGMENTS):
        u0 = first_of[k]
        a = n // 2
        # the first fine row ends on the mapped column that opens the third: columns tail0 .. tail0 + a - 1, then tail0 + a - 1 + ...
        rows[u0] = [(tail0 + j, 1 + (j * 7) % 50) for j in range(a)]
        rows[u0 + 2] = [(tail0 + j, 3 + (j * 11) % 40) for j in range(n - a)]
    one_col = first_of[n_seg + 2]
    rows[one_col] = [(one_col + j, 5) for j in range(3)]  # three fine columns of one coarse unit
    rows[one_col + 1] = [(one_col + 1 + j, 9) for j in range(2)]
    big = first_of[n_seg + 3]
    rows[big] = [(big + j, 2 ** 31 - 1) for j in range(3)]
    huge = first_of[n_seg + 4]
    rows[huge] = [(huge, 2 ** 61), (huge + 1, 2 ** 60), (huge + 2, 2 ** 60 - 1)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], np.int32)
    count = np.array([v for r in rows for _, v in r], np.int64)
    return rowptr, col, count, m, C_, dict(n_seg=n_seg, first_of=first_of, one_col=n_seg + 2, big=n_seg + 3, huge=n_seg + 4, empty=n_seg, nobody=n_seg + 1, tail=tail_R)


def test_the_crafted_inputs_hold_each_case():
    """the host half of tests/test_hip_zoom_levels.py's crafted cases: a wrong input fails here and not as a device mismatch"""
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    rowptr, col, count, m, C_, info = crafted()
    r = ac.rows_of(rowptr)
    assert np.all(col >= r) and np.all(np.diff(col.astype(np.int64))[r[1:] == r[:-1]] > 0) and col.max() < m.size
    seg = np.bincount(m[r], minlength=C_)
    assert tuple(seg[:info["n_seg"]].tolist()) == SEGMENTS
    assert seg[info["empty"]] == 0 and (m == info["empty"]).sum() == 3 and not (m == info["nobody"]).any() and info["nobody"] < C_
    out_rowptr, out_col, out_count = zl.coarsen_host(rowptr, col, count, m, C_)
    w = np.diff(out_rowptr)
    assert w[info["empty"]] == 0 and w[info["nobody"]] == 0
    k = SEGMENTS.index(3000)  # a mapped column that ends one fine row and opens the next: both fine rows reach the same coarse column
    u0 = info["first_of"][k]
    assert m[col[rowptr[u0 + 1] - 1]] == m[col[rowptr[u0 + 2]]] == info["tail"] and rowptr[u0 + 1] == rowptr[u0 + 2]
    assert all(w[k2] == (1 if n else 0) for k2, n in enumerate(SEGMENTS))  # all entries of these segments lie on one mapped column ...
    assert w[info["one_col"]] == 1 and seg[info["one_col"]] == 5  # ... and so do those of the diagonal case
    assert out_count[out_rowptr[info["big"]]] == 3 * (2 ** 31 - 1) > 2 ** 32 and w[info["big"]] == 1
    assert out_count[out_rowptr[info["huge"]]] == 2 ** 62 - 1 and w[info["huge"]] == 1
    assert int(out_count.sum()) == sum(count.tolist())


def crafted_spread():
    """a second fine level whose segments keep many distinct mapped columns: every fine row u of 600 holds the columns u, u + 1, ...
    up to its length (1, 2, 63, 64, 65, 1000 in turn), mapped three fine units to a coarse one"""
    U = 1800
    lens = [1, 2, 63, 64, 65, 1000]
    rows = [list(range(u, u + lens[u % len(lens)])) if u < 600 else [] for u in range(U)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], np.int32)
    count = (1 + (np.arange(col.size, dtype=np.int64) * 7919) % 1000) << 24  # sums leave 32 bits
    return rowptr, col, count, np.arange(U, dtype=np.int64) // 3, (U + 2) // 3


def test_the_spread_inputs_hold_their_case():
    import test_rows_rule_host as rule
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl

    rowptr, col, count, m, C_ = crafted_spread()
    r = ac.rows_of(rowptr)
    assert np.all(col >= r) and col.max() < m.size and np.all(np.diff(m) >= 0) and m.max() == C_ - 1
    lengths = np.bincount(m[r], minlength=C_)
    out = zl.coarsen_host(rowptr, col, count, m, C_)
    assert lengths.max() > rule.LDS_CAP and np.diff(out[0]).max() > 64 and int(out[2].max()) > 2 ** 32 and out[1].size < col.size
