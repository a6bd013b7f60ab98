"""CPU tests of the rule of the contacts in genome coordinates (instagraal_amd.assembly_contacts): ``lift_host`` against brute force
-- the dense symmetric matrix permuted by the genome order, its upper triangle, block-summed by unit for level "bin" -- on ``tiny``
under several genomes; the identities between the scalars; the bins table; the writers.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def tiny():
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS["tiny"])


def _genome(prob, kind, seed=0):
    """state arrays (pos, id_c, activ, id_d, ori) of a genome over the bins of ``prob``"""
    S = prob.S_o_A_frags
    N = prob.n_frags
    pos, id_c, ori = S["pos"].astype(np.int64).copy(), S["id_c"].astype(np.int64).copy(), np.ones(N, np.int64)
    activ, id_d = np.ones(N, np.int64), S["id_d"].astype(np.int64).copy()
    rng = np.random.RandomState(seed)
    if kind == "shuffled":  # a random permutation of the bins cut into contigs of random lengths, random orientations
        perm = rng.permutation(N)
        cuts = np.sort(rng.choice(np.arange(1, N), 12, replace=False))
        starts = np.concatenate([[0], cuts])
        lens = np.diff(np.concatenate([starts, [N]]))
        id_c[perm] = np.repeat(rng.permutation(starts.size) + 1, lens)
        pos[perm] = np.arange(N) - np.repeat(starts, lens)
        ori = rng.choice([-1, 1], N)
    elif kind == "unplaced":  # one bin of a contig of several is not active: the whole contig is left out
        ids, n = np.unique(id_c, return_counts=True)
        activ[np.nonzero(id_c == ids[np.argmax(n >= 3)])[0][1]] = 0
    elif kind == "nothing placed":
        activ[:] = 0
    return pos, id_c, activ, id_d, ori


def _order(prob, genome):
    from instagraal_amd import contact_map as cmap

    return np.asarray(cmap.genome_order(*genome, prob.np_sub_frags_id)[2], np.int64)


def _brute(prob, order, row, col, cnt, unit):
    """the dense matrix permuted by the order, its upper triangle, block-summed by unit -> (rowptr, col, count)"""
    M = prob.n_sub_frags
    S = np.zeros((M, M), np.int64)
    S[row, col] = cnt
    S = S + S.T
    D = np.triu(S[order][:, order], k=1)
    if unit is not None:
        U = int(unit[-1]) + 1 if unit.size else 0
        P = np.zeros((order.size, U), np.int64)
        P[np.arange(order.size), unit] = 1
        D = P.T @ D @ P
        assert not np.tril(D, k=-1).any()
    i, j = np.nonzero(D)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=D.shape[0]))]).astype(np.int64)
    return rowptr, j.astype(np.int32), D[i, j]


@pytest.mark.parametrize("kind", ["fresh", "shuffled", "unplaced", "nothing placed", "no contacts"])
def test_the_rule_equals_brute_force_on_tiny(tiny, kind):
    from instagraal_amd import assembly_contacts as ac

    prob = tiny
    genome = _genome(prob, kind)
    order = _order(prob, genome)
    row, col, cnt = (np.asarray(a, np.int64) for a in (prob.coo_row, prob.coo_col, prob.coo_cnt))
    assert cnt.min() >= 1
    if kind == "no contacts":
        row, col, cnt = row[:0], col[:0], cnt[:0]
    position = ac.positions_of(order, prob.n_sub_frags)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    T = order.size
    assert (T == 0) == (kind == "nothing placed") and (T < prob.n_sub_frags) == (kind in ("unplaced", "nothing placed"))
    for level in ac.LEVELS:
        unit = None if level == "sub" else ac.units_along(parent[order])
        got = ac.lift_host(position, row, col, cnt, unit)
        rowptr, c, v = _brute(prob, order, row, col, cnt, unit)
        assert got["rowptr"].dtype == np.int64 and got["col"].dtype == np.int32 and got["count"].dtype == np.int64
        assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["col"], c) and np.array_equal(got["count"], v), (kind, level)
        # the identities
        assert got["contacts_kept"] + got["contacts_unplaced"] == int(cnt.sum())
        assert int(got["count"].sum()) == got["contacts_kept"]
        assert got["entries_kept"] + got["entries_unplaced"] == got["entries_in"] == row.size
        assert got["entries_out"] == got["col"].size == got["rowptr"][-1] and got["n_placed"] == T
        assert got["n_units"] == got["rowptr"].size - 1 == (T if level == "sub" else np.unique(parent[order]).size)
        if level == "sub":
            assert got["entries_out"] == got["entries_kept"]
        else:
            assert got["entries_out"] <= got["entries_kept"]
        r = ac.rows_of(got["rowptr"])
        assert np.all(r <= got["col"]) and (level == "bin" or np.all(r < got["col"]))
        same_row = r[1:] == r[:-1]
        assert np.all(np.diff(got["col"].astype(np.int64))[same_row] > 0)  # strictly ascending inside a row
        assert (got["entries_unplaced"] > 0) == (kind in ("unplaced", "nothing placed"))
        if level == "bin" and T:  # the unit list is the reference's full_order
            from instagraal_amd import contact_map as cmap

            assert parent[order][np.concatenate([[True], np.diff(unit) > 0])].tolist() == cmap.genome_order(*genome, prob.np_sub_frags_id)[0]


def test_arguments_are_checked(tiny):
    from instagraal_amd import assembly_contacts as ac

    position = ac.positions_of(np.arange(5)[::-1], 7)
    assert position.tolist() == [4, 3, 2, 1, 0, -1, -1]
    with pytest.raises(ValueError, match="each once"):
        ac.lift_host([0, 0, 1], [0], [1], [1])
    with pytest.raises(ValueError, match="upper triangle"):
        ac.lift_host([0, 1, 2], [1], [1], [1])
    with pytest.raises(ValueError, match="unit"):
        ac.lift_host([0, 1, 2], [0], [1], [1], unit=[0, 2, 2])
    with pytest.raises(ValueError, match="twice"):
        ac.lift_host([0, 1, 2], [0, 0], [1, 1], [1, 1])
    with pytest.raises(ValueError, match="level"):
        ac.check_level("frag")
    assert ac.check_level("sub") == 0 and ac.check_level("bin") == 1
    got = ac.lift_host([2, -1, 0, 1], [0, 0, 2], [1, 2, 3], [5, 7, 11], unit=[0, 0, 1])
    assert got["rowptr"].tolist() == [0, 2, 2] and got["col"].tolist() == [0, 1] and got["count"].tolist() == [11, 7]
    assert got["contacts_unplaced"] == 5 and got["entries_unplaced"] == 1


def _table(prob, genome, level):
    from instagraal_amd import assembly_contacts as ac

    order = _order(prob, genome)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    return order, ac.bins_table(order, parent, genome[1], genome[4], prob.S_o_A_sub_frags["len_bp"], level)


@pytest.mark.parametrize("kind", ["fresh", "shuffled", "unplaced", "nothing placed"])
def test_bins_table(tiny, kind):
    from instagraal_amd import assembly_contacts as ac

    prob = tiny
    genome = _genome(prob, kind, seed=3)
    order, sub = _table(prob, genome, "sub")
    _, per_bin = _table(prob, genome, "bin")
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    len_bp = prob.S_o_A_sub_frags["len_bp"].astype(np.int64)
    assert sub.size == order.size and np.array_equal(sub["bin"], parent[order]) and np.array_equal(sub["end"] - sub["start"], len_bp[order])
    for t in (sub, per_bin):
        if t.size == 0:
            assert kind == "nothing placed"
            continue
        head = np.concatenate([[True], t["contig"][1:] != t["contig"][:-1]])
        assert np.all(t["start"][head] == 0) and np.all(t["end"][:-1][~head[1:]] == t["start"][1:][~head[1:]])
        assert np.all(np.diff(t["contig"][head]) > 0)  # contigs in ascending id, each one run
        assert np.array_equal(t["contig"], genome[1][t["bin"]]) and np.array_equal(t["ori"], genome[4][t["bin"]])
        ids, sizes = ac.chrom_sizes(t)
        assert np.array_equal(ids, t["contig"][head])
        placed = order
        want = {int(c): int(len_bp[placed][genome[1][parent[placed]] == c].sum()) for c in ids}
        assert dict(zip(ids.tolist(), sizes.tolist())) == want
    if sub.size:  # the level-"bin" table is the level-"sub" table merged by unit
        unit = ac.units_along(parent[order])
        first = np.concatenate([[True], np.diff(unit) > 0])
        last = np.concatenate([first[1:], [True]])
        assert per_bin.size == unit[-1] + 1 and np.array_equal(per_bin["start"], sub["start"][first]) and np.array_equal(per_bin["end"], sub["end"][last])
        assert np.array_equal(per_bin["bin"], sub["bin"][first]) and np.array_equal(per_bin["contig"], sub["contig"][first])
        assert ac.scaffold_names(sub["contig"][:1])[0] == "3C-assembly-contig_%d" % sub["contig"][0]
    unplaced_contigs = np.setdiff1d(genome[1], sub["contig"])
    assert (unplaced_contigs.size > 0) == (kind in ("unplaced", "nothing placed"))


@pytest.mark.parametrize("level", ["sub", "bin"])
def test_the_writers_round_trip_whatever_the_block_size(tiny, level, tmp_path):
    from instagraal_amd import assembly_contacts as ac

    prob = tiny
    genome = _genome(prob, "shuffled", seed=5)
    order, table = _table(prob, genome, level)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    unit = None if level == "sub" else ac.units_along(parent[order])
    res = ac.lift_host(ac.positions_of(order, prob.n_sub_frags), prob.coo_row, prob.coo_col, prob.coo_cnt, unit)
    U = res["n_units"]
    calls = []

    def fetch(first, n):
        calls.append(n)
        return res["col"][first:first + n], res["count"][first:first + n]

    diag = np.zeros(U, np.int64)
    diag[::3] = np.arange(1, U + 1)[::3]
    files = {}
    for with_diag in (False, True):
        for block in (1, 7, U):
            folder = str(tmp_path / ("%s_%d_%d" % (level, block, with_diag)))
            del calls[:]
            n = ac.write_all(folder, table, res["rowptr"], fetch, block, diag if with_diag else None)
            assert len(calls) == -(-U // block) and sum(calls) == res["entries_out"]  # (a fetch per block of rows, every entry once)
            files[(with_diag, block)] = {k: open(os.path.join(folder, k)).read() for k in ("bins.bed", "pixels.tsv", "chrom.sizes")}
            assert n == files[(with_diag, block)]["pixels.tsv"].count("\n")
        assert files[(with_diag, 1)] == files[(with_diag, 7)] == files[(with_diag, U)]
        folder = str(tmp_path / ("%s_%d_%d" % (level, U, with_diag)))
        px = np.loadtxt(os.path.join(folder, "pixels.tsv"), dtype=np.int64, ndmin=2)
        b1, b2, v = px.T
        assert np.all(b1 <= b2) and b2.max() < U and b1.min() >= 0
        key = b1 * U + b2
        assert np.all(np.diff(key) > 0)  # sorted by (bin1, bin2), no key twice
        want_rows = ac.rows_of(res["rowptr"])
        if not with_diag:
            assert np.array_equal(b1, want_rows) and np.array_equal(b2, res["col"]) and np.array_equal(v, res["count"])
        else:
            D = np.zeros((U, U), np.int64)
            D[want_rows, res["col"]] = res["count"]
            D[np.arange(U), np.arange(U)] += diag
            i, j = np.nonzero(D)
            assert np.array_equal(b1, i) and np.array_equal(b2, j) and np.array_equal(v, D[i, j])
            ptr, c2, v2 = ac.merge_diagonal(0, res["rowptr"], res["col"], res["count"], diag)
            assert np.array_equal(ac.rows_of(ptr), i) and np.array_equal(c2, j) and np.array_equal(v2, D[i, j]) and c2.dtype == np.int32
        bed = np.loadtxt(os.path.join(folder, "bins.bed"), dtype=str, ndmin=2)
        assert bed.shape == (U, 3) and np.array_equal(bed[:, 1].astype(np.int64), table["start"]) and np.array_equal(bed[:, 2].astype(np.int64), table["end"])
        assert bed[:, 0].tolist() == ac.scaffold_names(table["contig"]).tolist()
        sizes = np.loadtxt(os.path.join(folder, "chrom.sizes"), dtype=str, ndmin=2)
        ids, want = ac.chrom_sizes(table)
        assert sizes[:, 0].tolist() == ac.scaffold_names(ids).tolist() and np.array_equal(sizes[:, 1].astype(np.int64), want)


def test_import_needs_neither_scipy_nor_the_library():
    code = ("import sys; import numpy as np\n"
            "import instagraal_amd.assembly_contacts as a, instagraal_amd.hip_lib as h\n"
            "r = a.lift_host([1, 0, 2], [0, 0], [1, 2], [3, 5])\n"
            "assert r['rowptr'].tolist() == [0, 1, 2, 2] and r['col'].tolist() == [1, 2] and r['count'].tolist() == [3, 5]\n"
            "assert h._lib is None, 'the shared library was loaded'\n"
            "sys.exit(1 if 'scipy' in sys.modules else 0)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
