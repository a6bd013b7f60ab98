"""CPU tests of the expected contact map's rule (instagraal_amd.expected_map): ``expected_host`` against a dense statement over all
pairs of positions on the tables of ``tiny`` (from the oracle) in six states, the block-sum relation, the identities, ``compose``,
``residuals``, the ranking and the file on hand-made tables, and the preconditions of the GPU tests (tests/test_hip_expected_map.py)
that can be stated without a device.  Every comparison is exact unless it says otherwise."""
import numpy as np
import pytest

STATES = ("fresh", "permuted", "ring", "unplaced", "single", "nothing")


def _toy_model_q(s):
    """a stand-in for the quantised model: any deterministic s -> int64 will do for the rule (negative beyond 40 kb: signed sums)"""
    s = np.asarray(s, np.float64)
    return (np.rint(1000.0 / (1.0 + s) * 2.0 ** 32) * np.where(s > 40.0, -1, 1)).astype(np.int64)


def _max_sides(T):
    """descending: one position per pixel first"""
    return sorted({T + 5, T, -(-T // 2), -(-T // 3), -(-T // 7), 64, 1} - {0}, reverse=True)


def _oracle_tables(cfg, oracle_lib):
    """dist, s_tot and contig of every sub-fragment of the fresh genome, and the sub-fragments in genome order"""
    from instagraal_amd import synth
    from oracle.sampler_oracle import OracleSampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    s = OracleSampler(**prob.sampler_kwargs(), mode=oracle_lib.MODE_DET)
    s.fill_dist_single()
    ds, stot, contig, rank = s.vect_dist.astype(np.float32), s.vect_s_tot.astype(np.float32), s.vect_id_c.astype(np.int64), s.vect_pos.astype(np.int64)
    order = np.lexsort((rank, contig))
    assert not stot.any()
    return prob, ds, stot, contig, order


@pytest.fixture(scope="module")
def tiny(oracle_lib):
    return _oracle_tables("tiny", oracle_lib)


def _state(tiny, kind):
    """-> ds, stot, contig, position ([M] each) of the state ``kind`` made from the fresh tables"""
    _, ds, stot, contig, order = tiny
    ds, stot, contig = ds.copy(), stot.copy(), contig.copy()
    M = ds.size
    position = np.empty(M, np.int64)
    position[order] = np.arange(M)
    ids = np.unique(contig)
    rng = np.random.RandomState(5)
    if kind == "permuted":  # the contigs in another order, half of them turned round (dist counts from the new head)
        pos = 0
        for c in rng.permutation(ids):
            m = order[contig[order] == c]
            if rng.rand() < 0.5:
                m = m[::-1]
                ds[m] = ds[m[0]] - ds[m]
                assert np.all(np.diff(ds[m]) >= 0)
            position[m] = pos + np.arange(m.size)
            pos += m.size
    elif kind == "ring":
        stot[contig == ids[1]] = np.float32(ds[contig == ids[1]].max() + 1.0)
    elif kind == "unplaced":
        position[contig == ids[2]] = -1
        placed = position >= 0
        position[placed] = np.argsort(np.argsort(position[placed]))
    elif kind == "single":  # the head of a contig becomes a contig of its own
        head = order[contig[order] == ids[3]][0]
        contig[head] = contig.max() + 7
    elif kind == "nothing":
        position[:] = -1
    return ds, stot, contig, position


def _dense(ds, stot, contig, position, max_side, model_q):
    """the definition over ALL pairs of positions, classified one by one"""
    from instagraal_amd.contact_map import binning

    members = np.nonzero(position >= 0)[0]
    members = members[np.argsort(position[members])]
    T = members.size
    b, side = binning(T, max_side)
    d, c, ring = ds[members], contig[members], stot[members] != 0
    i, k = np.triu_indices(T, k=1)
    same = c[i] == c[k]
    lin, rg = same & ~ring[i], same & ring[i]
    q = model_q(np.abs(d[i] - d[k]))
    out = {}
    for name, sel, val in (("cis_q", lin, q), ("cis_pairs", lin, np.ones(i.size, np.int64)), ("ring_pairs", rg, np.ones(i.size, np.int64))):
        img = np.zeros((side, side), np.int64)
        np.add.at(img, (i[sel] // b, k[sel] // b), val[sel])
        np.add.at(img, (k[sel] // b, i[sel] // b), val[sel])
        out[name] = img
    out.update(side=side, bin=b, n_placed=T, linear_cis_pairs=int(lin.sum()), ring_pairs_total=int(rg.sum()), max_q=int(np.abs(q[lin]).max()) if lin.any() else 0)
    return out


@pytest.mark.parametrize("kind", STATES)
def test_expected_host_equals_the_dense_statement(tiny, kind):
    from instagraal_amd import expected_map as em

    ds, stot, contig, position = _state(tiny, kind)
    T = int((position >= 0).sum())
    assert (T == 0) == (kind == "nothing")
    one = None
    partial = 0
    for max_side in _max_sides(T):
        got = em.expected_host(ds, stot, contig, position, max_side, _toy_model_q)
        want = _dense(ds, stot, contig, position, max_side, _toy_model_q)
        for k in em.IMAGES:
            assert got[k].dtype == np.int64 and got[k].shape == (want["side"], want["side"]) and np.array_equal(got[k], want[k]), (kind, max_side, k)
            assert np.array_equal(got[k], got[k].T)
        for k in ("side", "bin", "n_placed", "linear_cis_pairs", "ring_pairs_total", "max_q"):
            assert got[k] == want[k], (kind, max_side, k)
        assert got["tiles_evaluated"] == got["tiles_constant"] == 0
        # the identities
        assert int(got["cis_pairs"].sum()) == 2 * got["linear_cis_pairs"] and int(got["ring_pairs"].sum()) == 2 * got["ring_pairs_total"]
        full = em.compose(dict(got), 12345)
        assert int(full["total"].sum()) == T * (T - 1)
        assert np.array_equal(full["trans_pairs"] + got["cis_pairs"] + got["ring_pairs"], full["total"]) and (full["trans_pairs"] >= 0).all()
        partial += T % got["bin"] != 0 if got["bin"] > 1 else 0
        if got["bin"] == 1:
            one = got
            assert all(not np.diagonal(got[k]).any() for k in em.IMAGES)
        else:  # the block sums of the image at one position per pixel
            assert one is not None or T == 0
            for k in em.IMAGES:
                assert np.array_equal(em.block_sum(one[k], got["bin"], got["side"]), got[k]), (kind, max_side, k)
    assert partial > 0 or T == 0  # (a partial last pixel was among them)
    if kind == "ring":
        assert one["ring_pairs_total"] > 0
    if kind == "single":
        lengths = np.unique(contig[position >= 0], return_counts=True)[1]
        assert (lengths == 1).any()


@pytest.mark.parametrize("kind", ("fresh", "ring", "unplaced"))
def test_the_identities_with_the_law_and_the_junction_profile(tiny, kind):
    from instagraal_amd import distance_law as dlaw, expected_map as em, junction_profile as jp

    ds, stot, contig, position = _state(tiny, kind)
    placed = position >= 0
    T = int(placed.sum())
    none = np.zeros(0, np.int64)
    got = em.expected_host(ds, stot, contig, position, T, _toy_model_q)
    law = dlaw.law_host(ds, stot, contig, placed, none, none, none, np.array([0.0, 1e9], np.float32))
    assert got["linear_cis_pairs"] + got["ring_pairs_total"] == law["placed_pairs"] and got["ring_pairs_total"] == law["ring_pairs"]
    i, k = np.triu_indices(T, k=1)
    j = np.arange(1, T)
    for w in (1, 64):
        prof = jp.profile_host(ds, stot, contig, placed, position, none, none, none, w, model_q=_toy_model_q)
        S = np.zeros((T, T), np.int64)
        near = k - i <= w
        S[i[near], k[near]] = got["cis_q"][i[near], k[near]]
        R = S.cumsum(0).cumsum(1)
        want = np.zeros(T, np.int64)
        want[1:] = R[j - 1, T - 1] - R[j - 1, j - 1]  # rows i < j, columns k >= j
        assert np.array_equal(prof["expected_q"], want) and want.any(), (kind, w)


def test_compose_with_hand_made_images():
    from instagraal_amd import expected_map as em

    # T = 7 positions, 3 per pixel: pixels of 3, 3 and 1 positions
    cis_pairs = np.array([[6, 2, 0], [2, 2, 0], [0, 0, 0]], np.int64)
    ring_pairs = np.array([[0, 0, 0], [0, 2, 1], [0, 1, 0]], np.int64)
    cis_q = np.array([[600, 20, 0], [20, -7, 0], [0, 0, 0]], np.int64)
    r = em.compose(dict(side=3, bin=3, n_placed=7, cis_q=cis_q, cis_pairs=cis_pairs, ring_pairs=ring_pairs, max_q=100), 10)
    assert np.array_equal(em.pixel_sizes(7, 3, 3), [3, 3, 1])
    assert np.array_equal(r["total"], [[6, 9, 3], [9, 6, 3], [3, 3, 0]]) and int(r["total"].sum()) == 7 * 6
    assert np.array_equal(r["trans_pairs"], [[0, 7, 3], [7, 2, 2], [3, 2, 0]])
    assert np.array_equal(r["expected_q"], [[600, 90, 30], [90, 13, 20], [30, 20, 0]]) and r["expected_q"].dtype == np.int64
    assert np.array_equal(r["expected"], r["expected_q"] / 2.0 ** 32) and r["expected"].dtype == np.float64
    with pytest.raises(ValueError, match="more cis and ring pairs"):
        em.compose(dict(side=1, bin=3, n_placed=3, cis_q=np.zeros((1, 1), np.int64), cis_pairs=np.full((1, 1), 7), ring_pairs=np.zeros((1, 1), np.int64), max_q=0), 1)
    with pytest.raises(ValueError, match="too large for this pixel size"):
        em.compose(dict(side=1, bin=1 << 20, n_placed=1 << 20, cis_q=np.zeros((1, 1), np.int64), cis_pairs=np.zeros((1, 1), np.int64),
                        ring_pairs=np.zeros((1, 1), np.int64), max_q=1 << 21), 1)
    assert em.quantize(np.float32(0.5)) == 1 << 31 and em.quantize(float("nan")) == 0 and em.quantize(1e9) == 1 << 52 and em.quantize(-1e9) == -(1 << 52)
    empty = em.compose(dict(side=0, bin=1, n_placed=0, cis_q=np.zeros((0, 0), np.int64), cis_pairs=np.zeros((0, 0), np.int64),
                            ring_pairs=np.zeros((0, 0), np.int64), max_q=0), 5)
    assert empty["expected"].shape == (0, 0)


def _hand_made_residuals():
    from instagraal_amd import expected_map as em

    side, b, T = 4, 2, 7
    zero = np.zeros((side, side), np.int64)
    ring = zero.copy()
    ring[0, 1] = ring[1, 0] = 1
    cis_q = zero.copy()
    cis_q[0, 0] = 8 << 32
    result = em.compose(dict(side=side, bin=b, n_placed=T, cis_q=cis_q, cis_pairs=zero.copy(), ring_pairs=ring, max_q=8 << 32), 1 << 31)  # trans level 0.5
    observed = np.array([[16, 9, 8, 0], [9, 3, 2, 5], [8, 2, 0, 1], [0, 5, 1, 0]], np.int64)
    return em, result, observed


def test_residuals_mask_ranking_and_file(tmp_path):
    em, result, observed = _hand_made_residuals()
    res = em.residuals(observed, result)
    E = result["expected"]
    assert E[0, 0] == 8 + 0.5 * 2 and E[0, 2] == 2.0 and E[3, 3] == 0.0 and E[2, 3] == 1.0
    mask = np.zeros((4, 4), bool)
    mask[0, 1] = mask[1, 0] = True  # a ring pair
    mask[3, 3] = True  # E == 0: one position, no pair
    assert np.array_equal(res["mask"], mask)
    assert np.array_equal(np.isnan(res["log2_ratio"]), mask) and np.array_equal(np.isnan(res["z"]), mask)
    assert res["log2_ratio"][0, 2] == 2.0 and res["z"][0, 2] == (8 - 2) / np.sqrt(2.0)
    assert res["log2_ratio"][0, 3] == -np.inf and res["z"][0, 3] == -1.0  # (nothing observed where 1 was expected)
    with pytest.raises(ValueError, match="observed image"):
        em.residuals(observed[:3, :3], result)
    # the ranking: pixels a < b, total >= min_pairs, z descending, stable
    assert em.default_min_pairs(2) == 2 and em.default_min_pairs(3) == 5
    contig_of_position = np.array([4, 4, 4, 9, 9, 9, 2])
    t = em.strongest(res, 10, None, contig_of_position)
    z = res["z"]
    want = sorted(((a, c) for a in range(4) for c in range(a + 1, 4) if not mask[a, c] and result["total"][a, c] >= 2), key=lambda p: -z[p])
    assert [(int(r["pixel_a"]), int(r["pixel_b"])) for r in t] == want == [(0, 2), (1, 3), (1, 2), (2, 3), (0, 3)]
    top = t[1]
    assert (top["first_a"], top["last_a"], top["first_b"], top["last_b"]) == (2, 3, 6, 6) and (top["contig_a"], top["contig_b"]) == (4, 2)
    assert top["pairs"] == 2 and top["observed"] == 5 and top["expected"] == 1.0 and top["z"] == 4.0
    assert em.strongest(res, 2).size == 2 and em.strongest(res, 0).size == 0 and np.all(em.strongest(res, 2)["contig_a"] == -1)
    assert [(int(r["pixel_a"]), int(r["pixel_b"])) for r in em.strongest(res, 10, 4)] == [(0, 2), (1, 2)]  # (the last pixel holds one position)
    tie = dict(res)
    tie["z"] = np.where(np.isnan(z), np.nan, 1.0)
    assert [(int(r["pixel_a"]), int(r["pixel_b"])) for r in em.strongest(tie, 10)] == [(0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]  # stable: row-major
    # the file
    full = dict(res)
    full.update(linear_cis_pairs=0, ring_pairs_total=1, max_q=8 << 32, tiles_evaluated=0, tiles_constant=0)
    path = str(tmp_path / "residuals.txt")
    em.write_residuals(path, t, full)
    lines = open(path).read().splitlines()
    assert lines[0][2:].split() == list(em.STRONGEST_COLUMNS) and len(lines) == 2 + t.size
    assert lines[1].split() == ["0", "2", "0", "1", "4", "5", "4", "9", "4", "8", "2", "%.9g" % (6 / np.sqrt(2.0))]
    assert lines[2].split() == ["1", "3", "2", "3", "6", "6", "4", "2", "2", "5", "1", "4"]
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert sc == dict(side="4", bin="2", n_placed="7", linear_cis_pairs="0", ring_pairs_total="1", max_q=str(8 << 32), tiles_evaluated="0", tiles_constant="0")


def test_tile_census_on_hand_made_contigs():
    """three linear contigs of 5, 2 and 9 positions at 4 per pixel: pixels {0: c0}, {1: c0 c1 c2}, {2: c2}, {3: c2}"""
    from instagraal_amd import expected_map as em

    lens = [5, 2, 9]
    contig = np.repeat([3, 1, 8], lens)
    ds = np.concatenate([np.arange(n, dtype=np.float32) for n in lens])
    stot = np.zeros(16, np.float32)
    got = em.tile_census(ds, stot, contig, np.arange(16), 4, 6.0)
    # listed: (0,0) (0,1) | (1,1) (1,2) (1,3) | (2,2) (2,3) | (3,3); (1,3): ds[12] - ds[7] = 5 - 0 = 5 < 6; with d_max = 5 it is constant
    assert got == dict(listed=8, diagonal=4, constant=0, evaluated=8, ring=0, below=2, straddling=2, max_contigs_per_pixel=3)
    low = em.tile_census(ds, stot, contig, np.arange(16), 4, 5.0)
    assert low["constant"] == 1 and low["evaluated"] == 7 and low["listed"] == 8
    stot[contig == 8] = 9.0
    assert em.tile_census(ds, stot, contig, np.arange(16), 4, 5.0)["ring"] == 3


def gpu_bigctg_d_max(ds):
    """the lowered d_max of the GPU tests on ``bigctg``: a third of the longest contig's span (dist counts from a contig's head)"""
    return np.float32(ds.max() / 3.0)


def test_preconditions_of_the_gpu_tests(oracle_lib):
    """what tests/test_hip_expected_map.py leans on, on the fresh genomes (the states behind moves keep the contigs or merge them):
    ``small`` has pixels that straddle two and three contigs; ``bigctg`` under the lowered d_max has constant tiles, tiles that
    straddle d_max and tiles entirely below it, at both image sizes"""
    from instagraal_amd import expected_map as em

    _, ds, stot, contig, order = _oracle_tables("small", oracle_lib)
    position = np.empty(ds.size, np.int64)
    position[order] = np.arange(ds.size)
    T = ds.size
    most = [em.tile_census(ds, stot, contig, position, m, 1e9)["max_contigs_per_pixel"] for m in _max_sides(T)]
    assert 2 in most and max(most) >= 3, most
    _, ds, stot, contig, order = _oracle_tables("bigctg", oracle_lib)
    position = np.empty(ds.size, np.int64)
    position[order] = np.arange(ds.size)
    low = gpu_bigctg_d_max(ds)
    for max_side in (64, 512):
        c = em.tile_census(ds, stot, contig, position, max_side, low)
        assert c["constant"] > 0 and c["straddling"] > 0 and c["below"] > 0 and c["evaluated"] + c["constant"] == c["listed"], (max_side, c)
