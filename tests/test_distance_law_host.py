"""CPU tests of the distance law's rule (instagraal_amd.distance_law): the numerator against the matrix the reference's own
``display_current_matrix`` produced on the two ``tiny`` trajectories (tests/golden/matrix_tiny_*.npz), with the coordinates of the
fixture's state from the oracle's tables; the two conservation identities; the edges; the import."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")


def fill_tables(state, sub):
    """numpy restatement of k_fill_tables (KA:3763-3822) -> dist f32, stot f32, contig, rank, len, placed (bool: every bin of the
    contig active)"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    f = sub["x"].astype(np.int64)
    ori = col["ori"][f]
    dfi = np.where(ori == 1, sub["y"], sub["z"]).astype(np.float32)
    dist = (col["start_bp"][f].astype(np.float32) / np.float32(1000.0) + dfi).astype(np.float32)
    stot_i = ((col["circ"][f] == 1).astype(np.float32) * col["l_cont_bp"][f].astype(np.float32) / np.float32(1000.0)).astype(np.int32)
    w = sub["w"].astype(np.int64)
    rank = np.where(ori == 1, col["sub_pos"][f] + w, col["sub_pos"][f] + (col["sub_len"][f] - 1) - w)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][f], bad)
    return dist, stot_i.astype(np.float32), col["id_c"][f].astype(np.int64), rank.astype(np.int64), col["sub_l_cont"][f], placed


def _fixture(name):
    from instagraal_amd import synth

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob = synth.make_problem(*synth.CONFIGS[str(g["config"])])
    return g, prob


def _edge_sets(longest, mean_kb):
    from instagraal_amd import distance_law as dlaw

    return {
        "linear": np.arange(0, 60.0 + 1.0, 1.0, dtype=np.float32),  # the reference's estimate shape: separations beyond fall out
        "geometric": dlaw.default_edges(mean_kb, longest),
        "both_ends_out": np.linspace(5.0, 40.0, 12).astype(np.float32),
        "one_bin": np.array([2.0, 30.0], np.float32),
        "fine": np.linspace(0.0, longest * 1.01, 4097).astype(np.float32),
    }


@pytest.mark.parametrize("name", FIXTURES)
def test_observed_is_the_reference_matrix_grouped_by_contig_and_separation(name, oracle_lib):
    from instagraal_amd import distance_law as dlaw
    from oracle.sampler_oracle import OracleSampler

    g, prob = _fixture(name)
    state = g["state"]
    # the coordinates of the fixture's state from the oracle's own table kernel ...
    s = OracleSampler(**prob.sampler_kwargs(), mode=oracle_lib.MODE_DET)
    s.gpu_vect_frags.assign(oracle_lib.FragStruct(prob.n_frags, {k: state[i] for i, k in enumerate(oracle_lib.FRAG_FIELDS)}))
    s.fill_dist_single()
    dist, stot, contig = s.vect_dist.copy(), s.vect_s_tot.copy(), s.vect_id_c.astype(np.int64)
    # ... which the restatement the other tests of this file use agrees with, bit for bit
    d2, st2, c2, rank2, len2, placed = fill_tables(state, prob.np_sub_frags_2_frags)
    assert np.array_equal(dist.view(np.uint32), d2.view(np.uint32)) and np.array_equal(stot, st2) and np.array_equal(contig, c2)
    assert np.array_equal(s.vect_pos, rank2) and np.array_equal(s.vect_len, len2)
    assert placed.all() and not stot.any()
    order = g["full_order_high"].astype(np.int64)
    matrix = g["matrix"].astype(np.int64)  # (m + m.T)[order][:, order], from the reference
    assert np.array_equal(np.sort(order), np.arange(prob.n_sub_frags))
    iu, ju = np.triu_indices(order.size, k=1)
    si, sj = order[iu], order[ju]
    sep = np.abs(dist[si] - dist[sj])
    cis = contig[si] == contig[sj]
    total = int(matrix[iu, ju].sum())
    assert total == int(prob.coo_cnt.astype(np.int64).sum())
    for label, edges in _edge_sets(float(dist.max()), float(s.mean_kb())).items():
        law = dlaw.law_host(dist, stot, contig, placed, prob.coo_row, prob.coo_col, prob.coo_cnt, edges)
        nb = edges.size - 1
        want_obs, want_pairs = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
        inside = np.zeros(sep.size, bool)
        for b in range(nb):  # the definition, bin by bin
            sel = cis & (sep >= edges[b]) & (sep < edges[b + 1])
            inside |= sel
            want_obs[b] = matrix[iu[sel], ju[sel]].sum()
            want_pairs[b] = sel.sum()
        assert np.array_equal(law["observed"], want_obs), label
        assert np.array_equal(law["pairs"], want_pairs), label
        assert law["out_of_range_observed"] == int(matrix[iu, ju][cis & ~inside].sum()), label
        assert law["out_of_range_pairs"] == int((cis & ~inside).sum()), label
        assert law["trans_observed"] == int(matrix[iu, ju][~cis].sum()) and law["trans_pairs"] == int((~cis).sum()), label
        assert law["ring_observed"] == law["ring_pairs"] == law["unplaced_observed"] == 0
        assert law["placed_pairs"] == int(cis.sum())
        assert dlaw.observed_total(law) == total and dlaw.pairs_total(law) == law["placed_pairs"], label
        if label == "both_ends_out":  # (nothing is out of range unless a pair is: below the first edge always, beyond the last in the plain
            # trajectory -- the bombed one has no contig that long)
            assert law["out_of_range_observed"] > 0 and (cis & (sep < edges[0])).any()
            assert (cis & (sep >= edges[-1])).any() == (name == "matrix_tiny_plain")


def _hand_made(seed=0):
    """tables made by hand: five contigs -- a ring, one not placed, one whose dist is NOT monotone in the rank, two plain -- and
    contacts between everything"""
    rng = np.random.RandomState(seed)
    lens = [40, 25, 30, 1, 60]
    contig = np.repeat(np.arange(5) * 7 + 3, lens)  # (ids with gaps)
    M = contig.size
    dist = np.concatenate([np.cumsum(rng.uniform(0.2, 3.0, n)) for n in lens]).astype(np.float32)
    dist[lens[0] + lens[1]:lens[0] + lens[1] + lens[2]] = rng.permutation(dist[lens[0] + lens[1]:lens[0] + lens[1] + lens[2]])
    stot = np.where(contig == 3, np.float32(77.0), np.float32(0.0)).astype(np.float32)  # contig 3 (the first) is a ring
    placed = contig != 10  # the second is not placed
    perm = rng.permutation(M)  # the table is not in genome order
    dist, stot, contig, placed = dist[perm], stot[perm], contig[perm], placed[perm]
    iu, ju = np.triu_indices(M, k=1)
    keep = rng.rand(iu.size) < 0.3
    row, col = iu[keep], ju[keep]
    cnt = rng.randint(1, 50, row.size)
    return dist, stot, contig, placed, row, col, cnt


@pytest.mark.parametrize("label", ["linear", "geometric", "both_ends_out", "one_bin", "fine"])
def test_conservation_identities_with_a_ring_and_an_unplaced_contig(label):
    from instagraal_amd import distance_law as dlaw

    dist, stot, contig, placed, row, col, cnt = _hand_made()
    edges = _edge_sets(float(dist.max()), 1.6)[label]
    law = dlaw.law_host(dist, stot, contig, placed, row, col, cnt, edges)
    assert law["observed"].dtype == law["pairs"].dtype == np.int64 and law["observed"].size == edges.size - 1
    assert dlaw.observed_total(law) == int(cnt.sum())
    n_c = np.array([np.sum((contig == c) & placed) for c in np.unique(contig)])
    assert law["placed_pairs"] == int((n_c * (n_c - 1) // 2).sum()) == dlaw.pairs_total(law)
    T = int(placed.sum())
    assert law["trans_pairs"] == T * (T - 1) // 2 - law["placed_pairs"]
    assert law["ring_pairs"] == 40 * 39 // 2 and law["ring_observed"] > 0 and law["unplaced_observed"] > 0 and law["trans_observed"] > 0
    # the ring's and the unplaced contig's contacts are nowhere in the law: the same law without them
    keep = placed[row] & placed[col] & ~((stot[row] != 0) & (contig[row] == contig[col]))
    law2 = dlaw.law_host(dist, stot, contig, placed, row[keep], col[keep], cnt[keep], edges)
    assert np.array_equal(law2["observed"], law["observed"]) and law2["ring_observed"] == law2["unplaced_observed"] == 0
    # a brute-force double loop over one contig whose dist is not monotone in the rank
    members = np.nonzero(contig == 17)[0]
    want = np.zeros(edges.size - 1, np.int64)
    for a in range(members.size):
        for b in range(a + 1, members.size):
            s = np.abs(dist[members[a]] - dist[members[b]])
            k = int(np.searchsorted(edges, s, side="right")) - 1
            if 0 <= k < edges.size - 1:
                want[k] += 1
    only = dlaw.law_host(dist, stot, contig, contig == 17, row, col, cnt, edges)
    assert np.array_equal(only["pairs"], want)
    # pairs=False leaves the pair counts out and the observed part alone
    lean = dlaw.law_host(dist, stot, contig, placed, row, col, cnt, edges, pairs=False)
    assert lean["pairs"] is None and lean["placed_pairs"] == -1 and np.array_equal(lean["observed"], law["observed"])


def test_edges_are_checked():
    from instagraal_amd import distance_law as dlaw

    for bad in ([1.0], [], [1.0, 3.0, 2.0], [0.0, np.nan], [0.0, np.inf], np.arange(4098)):
        with pytest.raises(ValueError):
            dlaw.check_edges(bad)
    e = dlaw.check_edges([0, 1, 1, 2])
    assert e.dtype == np.float32 and e.size == 4
    assert dlaw.check_edges(np.arange(4097)).size == dlaw.MAX_EDGES


@pytest.mark.parametrize("mean_kb, longest", [(1.6, 90.0), (0.3, 250_000.0), (2.0, 1.0), (1e-3, 1e9)])
def test_default_edges(mean_kb, longest):
    from instagraal_amd import distance_law as dlaw

    e = dlaw.default_edges(mean_kb, longest)
    assert e.dtype == np.float32 and np.all(np.diff(e) > 0) and 2 <= e.size <= dlaw.MAX_EDGES
    assert e[0] == np.float32(mean_kb / 2) and e[-1] > np.float32(longest)  # covers the longest contig
    assert np.array_equal(dlaw.check_edges(e), e)
    fine = dlaw.default_edges(mean_kb, longest, per_octave=100_000)
    assert fine.size <= dlaw.MAX_EDGES and fine[-1] > np.float32(longest)
    with pytest.raises(ValueError):
        dlaw.default_edges(0.0, 10.0)


def test_mean_per_pair_and_centres():
    from instagraal_amd import distance_law as dlaw

    law = dict(observed=np.array([10, 0, 5, 0], np.int64), pairs=np.array([4, 2, 0, 0], np.int64))
    m = dlaw.mean_per_pair(law)
    assert m.dtype == np.float64 and m[0] == 2.5 and m[1] == 0.0 and np.isnan(m[2]) and np.isnan(m[3])
    c = dlaw.bin_centres(np.array([0.0, 1.0, 4.0], np.float32))
    assert c[0] == 0.5 and c[1] == 2.0


def test_write_law_round_trips(tmp_path):
    from instagraal_amd import distance_law as dlaw

    dist, stot, contig, placed, row, col, cnt = _hand_made(1)
    law = dlaw.law_host(dist, stot, contig, placed, row, col, cnt, np.arange(0, 50, 2.5, dtype=np.float32))
    path = str(tmp_path / "law.txt")
    dlaw.write_law(path, law)
    t = np.loadtxt(path)
    assert np.array_equal(t[:, 0].astype(np.float32), law["edges"][:-1]) and np.array_equal(t[:, 1].astype(np.float32), law["edges"][1:])
    assert np.array_equal(t[:, 2].astype(np.int64), law["observed"]) and np.array_equal(t[:, 3].astype(np.int64), law["pairs"])


def test_import_needs_neither_matplotlib_nor_the_library():
    code = ("import sys; import numpy as np\n"
            "import instagraal_amd.distance_law as d, instagraal_amd.sampler, instagraal_amd.simulation, instagraal_amd.hip_lib as h\n"
            "law = d.law_host(np.arange(4, dtype=np.float32), np.zeros(4), np.zeros(4), np.ones(4, bool), [0], [1], [3], [0.0, 2.0])\n"
            "assert law['observed'][0] == 3 and law['pairs'][0] == 3 and law['out_of_range_pairs'] == 3\n"
            "assert h._lib is None, 'the shared library was loaded'\n"
            "sys.exit(1 if any(m == 'matplotlib' or m.startswith('matplotlib.') for m in sys.modules) else 0)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]


def test_estimate_parameters_rippe_without_a_matrix_names_the_alternative():
    from instagraal_amd.sampler import sampler

    class bare(sampler):
        def __init__(self):
            self.sparse_matrix = None

    with pytest.raises(ValueError, match="estimate_parameters_from_genome"):
        bare().estimate_parameters_rippe(60.0, 1.0)
