"""CPU tests of the gap support's rule (instagraal_amd.gap_support): hand-made tables with two linear contigs, a ring, an unplaced
contig and a contig of one position against the definition with python loops; gap 0 against the junction profile; a planted gap, a
planted misjoin and a true adjacency told apart; the grid, the junction builders on the three state situations of ``tiny``, the
file; and the host-only model values (``hip_lib.model_values_host``) against the oracle in DET mode.  Integer comparisons are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
# the parameters of the synthetic problems (synth.make_problem), in the order of ig_params
P8 = np.array([50.0, 9.6, 5.039808092988096e-05, -1.5, 2.0, 453.5715779621543, 958351.3076670185, 0.005], np.float32)


def _toy_model(s):
    """a stand-in for the two quantised model values: any deterministic s -> (int64, int64) will do for the rule"""
    s = np.asarray(s, np.float64)
    e = np.where(np.isfinite(s), 1000.0 / (1.0 + np.where(np.isfinite(s), s, 0.0)), 0.25)
    return np.rint(e * 2.0 ** 20).astype(np.int64), np.rint(np.log10(e) * 2.0 ** 20).astype(np.int64)


def _hand_made(seed=0):
    """tables made by hand, in genome order: a linear contig of 40 positions, a ring of 25, a contig that is not placed, a contig of
    one position, a linear one of 60; contacts between everything; the table itself is shuffled.  Positions: the 40 at 0 .. 39, the
    ring at 40 .. 64, the one at 65, the 60 at 66 .. 125"""
    rng = np.random.RandomState(seed)
    lens = [40, 25, 30, 1, 60]
    contig = np.repeat(np.arange(5) * 7 + 3, lens)
    M = contig.size
    dist = np.concatenate([np.cumsum(rng.uniform(0.2, 3.0, n)) for n in lens]).astype(np.float32)
    stot = np.where(contig == 10, np.float32(77.0), np.float32(0.0)).astype(np.float32)  # the second is a ring
    placed = contig != 17  # the third is not placed
    position = np.where(placed, np.cumsum(placed) - 1, -1)
    perm = rng.permutation(M)
    dist, stot, contig, placed, position = dist[perm], stot[perm], contig[perm], placed[perm], position[perm]
    iu, ju = np.triu_indices(M, k=1)
    keep = rng.rand(iu.size) < 0.3
    row, col = iu[keep], ju[keep]
    cnt = rng.randint(1, 50, row.size)
    return dist, stot, contig, placed, position, row, col, cnt


# junctions on the hand-made tables: the first and the last of the 40, neighbours (5, 6), one deep inside, two on the ring, the first
# of the 60, neighbours deep inside it, its last -- with junctions that are not listed in between
HAND_JUNCTIONS = np.array([1, 5, 6, 20, 39, 45, 50, 67, 90, 91, 125])
HAND_RING = np.array([0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0], bool)
HAND_GAPS = np.array([0.0, 1.5, 40.0], np.float32)


def _brute(dist, stot, contig, placed, position, row, col, cnt, junc, gaps, w, model):
    """the definition, contact by contact and pair by pair, with python loops"""
    T = int(placed.sum())
    where = np.full(T, -1, np.int64)
    where[position[placed]] = np.nonzero(placed)[0]
    start, end = np.zeros(T, np.int64), np.zeros(T, np.int64)
    r = 0
    while r < T:
        e = r
        while e < T and contig[where[e]] == contig[where[r]]:
            e += 1
        start[r:e], end[r:e] = r, e
        r = e
    K = gaps.size
    one = lambda s, k: model(np.array([np.float32(s) + gaps[k]], np.float32))  # noqa: E731
    obs, prs = np.zeros(junc.size, np.int64), np.zeros(junc.size, np.int64)
    lq, eq = np.zeros((junc.size, K), np.int64), np.zeros((junc.size, K), np.int64)
    sc = dict(unplaced=0, trans=0, ring=0, counted=0, uncounted=0, contributions=0)
    for a, b, v in zip(row.tolist(), col.tolist(), cnt.tolist()):
        if not (placed[a] and placed[b]):
            sc["unplaced"] += v
        elif contig[a] != contig[b]:
            sc["trans"] += v
        elif stot[a] != 0:
            sc["ring"] += v
        else:
            pa, pb = sorted((int(position[a]), int(position[b])))
            hit = [n for n, j in enumerate(junc.tolist()) if pa < j <= pb] if pb - pa <= w else []
            sc["counted" if hit else "uncounted"] += v
            sc["contributions"] += len(hit)
            s = np.abs(dist[a:a + 1] - dist[b:b + 1])[0]
            for n in hit:
                obs[n] += v
                for k in range(K):
                    lq[n, k] += v * int(one(s, k)[1][0])
    for n, j in enumerate(junc.tolist()):
        if stot[where[j]] != 0:
            continue
        for i in range(int(start[j]), j):
            for m in range(j, int(end[j])):
                if m - i <= w:
                    prs[n] += 1
                    s = np.abs(dist[where[i]:where[i] + 1] - dist[where[m]:where[m] + 1])[0]
                    for k in range(K):
                        eq[n, k] += int(one(s, k)[0][0])
    return obs, prs, lq, eq, sc, start, end


@pytest.mark.parametrize("w", [1, 2, 7, 20, 64, 256])
def test_hand_made_tables_with_a_ring_an_unplaced_contig_and_a_contig_of_one(w):
    from instagraal_amd import gap_support as gs, junction_profile as jp

    t = _hand_made()
    dist, stot, contig, placed, position, row, col, cnt = t
    got = gs.support_host(*t, HAND_JUNCTIONS, HAND_GAPS, w, _toy_model)
    assert got["n_placed"] == 126 and got["n_junctions"] == 11 and got["window"] == w and np.array_equal(got["junction"], HAND_JUNCTIONS)
    assert got["status"].dtype == np.int32 and got["geometry"].dtype == np.int32 and got["geometry"].shape == (11, 4)
    assert got["observed"].dtype == got["pairs"].dtype == got["log_q"].dtype == got["expected_q"].dtype == np.int64 and got["log_q"].shape == (11, 3)
    assert np.array_equal(got["status"], np.where(HAND_RING, 2, 0)) and got["n_judged"] == 9
    obs, prs, lq, eq, sc, start, end = _brute(*t, HAND_JUNCTIONS, HAND_GAPS, w, _toy_model)
    j = HAND_JUNCTIONS
    assert np.array_equal(got["geometry"][:, 1], np.where(HAND_RING, 0, np.minimum(w, j - start[j])))
    assert np.array_equal(got["geometry"][:, 2], np.where(HAND_RING, 0, np.minimum(w, end[j] - j))) and not got["geometry"][:, 3].any()
    assert got["geometry"][:, 0].tolist() == [3] * 5 + [10] * 2 + [31] * 4  # (without canonical ids: the caller's labels)
    assert np.array_equal(got["observed"], obs) and np.array_equal(got["pairs"], prs)
    assert np.array_equal(got["log_q"], lq) and np.array_equal(got["expected_q"], eq)
    assert all(got[k] == sc[k] for k in sc), (sc, {k: got[k] for k in sc})
    # the class identity; the rows of the ring are zero, the judged rows hold something
    assert gs.observed_total(got) == int(cnt.sum()) and all(got[k] > 0 for k in gs.CLASS_SCALARS)
    for k in ("observed", "pairs", "log_q", "expected_q"):
        assert not got[k][HAND_RING].any() and got[k][~HAND_RING].any(), k
    assert got["pairs"][~HAND_RING].all() and got["expected_q"][~HAND_RING].all() and (w < 7 or got["observed"][~HAND_RING].all())
    assert got["contributions"] >= 1 and int(got["observed"].sum()) >= got["counted"]
    # gap 0 is the junction profile at the listed junctions
    prof = jp.profile_host(*t, w, model_q=lambda s: _toy_model(s)[0])
    for k, mine in (("observed", got["observed"]), ("pairs", got["pairs"]), ("expected_q", got["expected_q"][:, 0])):
        assert np.array_equal(prof[k][j], mine), k
    # canonical ids are reported where the caller gives them; without the model half the rest is the same
    lean = gs.support_host(*t, HAND_JUNCTIONS, HAND_GAPS, w, _toy_model, want_expected=False, canonical=contig // 7)
    assert lean["expected_q"] is None and np.array_equal(lean["log_q"], lq) and lean["geometry"][:, 0].tolist() == [0] * 5 + [1] * 2 + [4] * 4
    with pytest.raises(ValueError, match="expected_q"):
        gs.derived(lean)


def test_arguments_are_checked():
    from instagraal_amd import gap_support as gs

    t = _hand_made()
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match="window"):
            gs.support_host(*t, HAND_JUNCTIONS, HAND_GAPS, bad, _toy_model)
    for junc, what in (([5, 5], "ascending"), ([9, 4], "ascending"), ([40], "boundary"), ([65], "boundary"), ([66], "boundary"), ([0], "range"), ([126], "range"),
                       ([-3], "range"), ([], "at least one"), ([1.0], "integer")):
        with pytest.raises(ValueError, match=what):
            gs.support_host(*t, np.array(junc), HAND_GAPS, 8, _toy_model)
    for gaps in ([0.0], [1.0, 2.0], [0.0, 2.0, 2.0], [0.0, 3.0, 1.0], [0.0, np.inf], [0.0, np.nan], np.arange(65.0)):
        with pytest.raises(ValueError, match="gaps"):
            gs.support_host(*t, HAND_JUNCTIONS, np.array(gaps), 8, _toy_model)
    assert gs.DEFAULT_WINDOW == 64 and gs.MAX_WINDOW == 256 and gs.check_window(256) == 256 and (gs.MIN_GAPS, gs.MAX_GAPS) == (2, 64)


def test_default_gaps():
    from instagraal_amd import gap_support as gs

    for mean_kb, d_max in ((2.1, 453.57), (0.004, 10.0), (50.0, 13.0), (2.0, 1e6)):
        g = gs.default_gaps(mean_kb, d_max)
        assert g.dtype == np.float32 and g.size == 32 and g[0] == 0 and np.all(np.diff(g) > 0) and np.all(np.isfinite(g))
        assert g[1] == np.float32(mean_kb / 4) and np.isclose(g[-1], d_max, rtol=1e-6)
        ratio = g[2:].astype(np.float64) / g[1:-1]
        assert np.allclose(ratio, ratio[0], rtol=1e-5)  # geometric
        assert np.array_equal(gs.check_gaps(g), g)
    for mean_kb, d_max in ((2.0, 0.5), (2.0, 0.4), (0.0, 5.0), (np.nan, 5.0), (2.0, np.inf)):
        with pytest.raises(ValueError):
            gs.default_gaps(mean_kb, d_max)


def _scaled_model(scale):
    """the product's host model with the amplitude (fact and v_inter) times ``scale``: counts of tens, not of 0 and 1"""
    from instagraal_amd import hip_lib

    hip_lib.build_lib()
    p = P8.copy()
    p[6] *= np.float32(scale)
    p[7] *= np.float32(scale)
    return p, (lambda s: hip_lib.model_values_host(p, s))


def test_a_planted_gap_a_planted_misjoin_and_a_true_adjacency_are_told_apart(tmp_path):
    """one linear contig of 160 positions; the counts of the pairs across junction 80 are the model's own expectation, rounded, at a
    shifted separation (a gap), at the trans level (a misjoin), at the separation as it is (adjacent).  The scale sits in the MODEL
    (counts of round(E) under a model whose amplitude is 600 times the synthetic problems'), so the counts are the maximum of the
    likelihood the rule writes down"""
    from instagraal_amd import gap_support as gs

    rng = np.random.RandomState(5)
    T, j, w = 160, 80, 30
    dist = np.cumsum(rng.uniform(1.0, 3.2, T)).astype(np.float32)
    stot, contig, placed, position = np.zeros(T, np.float32), np.full(T, 2), np.ones(T, bool), np.arange(T)
    p, model = _scaled_model(600.0)
    gaps = gs.default_gaps(2.1, float(p[5]))
    k_star = 19
    g_star = gaps[k_star]
    assert 20.0 < g_star < 60.0
    iu, ju = np.triu_indices(T, k=1)
    near = ju - iu <= w
    iu, ju = iu[near], ju[near]
    sep = np.abs(dist[iu] - dist[ju])
    across = (iu < j) & (ju >= j)
    e_inf = model(np.array([np.inf], np.float32))[0][0] / 2.0 ** 32
    assert round(e_inf) == 3  # 600 * v_inter

    def counts(shift_across):
        s = np.where(across, shift_across(sep), sep).astype(np.float32)
        return np.rint(model(s)[0] / 2.0 ** 32).astype(np.int64)

    results = {}
    for what, shift in (("gap", lambda s: s + g_star), ("apart", lambda s: np.full_like(s, np.inf)), ("adjacent", lambda s: s)):
        cnt = counts(shift)
        assert cnt[across].max() > 1 and cnt[across].min() >= 1 and cnt[across].sum() > 1000
        res = gs.support_host(dist, stot, contig, placed, position, iu, ju, cnt, np.array([40, j, 120]), gaps, w, model)
        assert res["observed"][1] == cnt[across].sum() and res["pairs"][1] == w * (w + 1) // 2 == across.sum()
        d = gs.derived(res)
        results[what] = dict(res, **d)
        assert d["verdict"].tolist() == ["adjacent", what, "adjacent"], (what, d["verdict"], d["best"], d["llr_gap"], d["llr_apart"])
        assert d["best"][0] == d["best"][2] == 0 and d["gap_kb"][0] == 0 and d["gap_lo"][0] == 0 and d["llr_gap"][0] == 0
        assert np.all(d["gap_lo"] <= d["gap_kb"]) and np.all(d["gap_kb"] <= d["gap_hi"]) and np.all(d["llr_gap"] >= 0)
        assert np.array_equal(d["ll"][np.arange(3), d["best"]], d["ll"].max(axis=1))
    d = results["gap"]
    assert d["best"][1] == k_star and d["gap_kb"][1] == g_star and d["gap_lo"][1] <= g_star <= d["gap_hi"][1] and d["llr_gap"][1] > gs.HALF_CHI2_95
    assert d["llr_apart"][1] < 0 and d["gap_hi"][1] < gaps[-1] and d["gap_lo"][1] > 0
    d = results["apart"]
    assert d["llr_apart"][1] == 0 and d["best"][1] > k_star and d["gap_hi"][1] == gaps[-1]  # the plateau beyond d_max IS the apart hypothesis
    d = results["adjacent"]
    assert d["best"][1] == 0 and d["llr_gap"][1] == 0 and d["llr_apart"][1] < 0
    # the ranking: the misjoin and the gap, never the adjacency; by how much better than "adjacent" they read
    for what in ("gap", "apart"):
        top = gs.gapped_joins(results[what])
        assert top.size == 1 and top["index"][0] == 1 and top["junction"][0] == j and top["verdict"][0] == what and top["score"][0] > gs.HALF_CHI2_95
        assert top["observed"][0] == results[what]["observed"][1] and top["left_bin"][0] == -1
        assert gs.gapped_joins(results[what], min_observed=10 ** 9).size == 0 and gs.gapped_joins(results[what], n=0).size == 0
    assert gs.gapped_joins(results["adjacent"]).size == 0
    # the file, and back
    res = dict(results["gap"], scaffold=np.array([7, 7, 7]), left_bin=np.array([3, 5, 8]), right_bin=np.array([4, 6, 9]))
    path = str(tmp_path / "gaps.txt")
    gs.write_gaps(path, res, title="level=block")
    lines = open(path).read().splitlines()
    assert lines[0] == "# level=block" and lines[1][2:].split() == list(gs.COLUMNS)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert len(rows) == 3 and all(len(r) == len(gs.COLUMNS) for r in rows)
    for i, r in enumerate(rows):
        assert [int(x) for x in r[:5]] == [7, res["left_bin"][i], res["right_bin"][i], res["observed"][i], res["pairs"][i]] and r[10] == res["verdict"][i]
        for c, k in enumerate(("gap_kb", "gap_lo", "gap_hi", "llr_gap", "llr_apart")):
            assert np.isclose(float(r[5 + c]), res[k][i], rtol=1e-8, atol=0), (i, k)
    tail = dict(kv.split("=") for kv in lines[-1][2:].split())
    assert int(tail["window"]) == w and int(tail["n_gaps"]) == 32 and int(tail["n_junctions"]) == 3 and int(tail["n_judged"]) == 3
    assert sum(int(tail[k]) for k in gs.CLASS_SCALARS) == gs.observed_total(res)
    gs.write_gaps(path, res, mode="a", title="level=bin")
    assert len(open(path).read().splitlines()) == 2 * len(lines)


def _loop_junctions(order, parent, id_c, ori, id_d, init_c, init_p):
    """the two junction lists with a python loop over the positions"""
    bins, blocks = [], []
    for j in range(1, order.size):
        a, b = int(parent[order[j - 1]]), int(parent[order[j]])
        if a == b or id_c[a] != id_c[b]:
            continue
        bins.append(j)
        step = int(init_p[id_d[b]]) - int(init_p[id_d[a]])
        colinear = init_c[id_d[a]] == init_c[id_d[b]] and ((step == 1 and ori[a] == 1 and ori[b] == 1) or (step == -1 and ori[a] == -1 and ori[b] == -1))
        if not colinear:
            blocks.append(j)
    return np.array(bins, np.int64), np.array(blocks, np.int64)


def test_the_junction_builders_on_the_three_state_situations():
    from instagraal_amd import gap_support as gs, synth
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    S0 = prob.S_o_A_frags
    init_c, init_p = S0["id_c"].astype(np.int64), S0["pos"].astype(np.int64)
    N, M = prob.n_frags, parent.size
    # fresh: the order is the table's; a block is its contig, so there is no block junction; a bin junction per bin but the contigs' first
    order = np.arange(M)
    ones, ids = np.ones(N, np.int64), S0["id_d"].astype(np.int64)
    b = gs.bin_junctions(order, parent, init_c)
    k = gs.block_junctions(order, parent, init_c, ones, ids, init_c, init_p)
    assert k["junction"].size == 0 and b["junction"].size == N - np.unique(init_c).size
    want_bins, want_blocks = _loop_junctions(order, parent, init_c, ones, ids, init_c, init_p)
    assert np.array_equal(b["junction"], want_bins) and want_blocks.size == 0
    assert np.array_equal(b["left_bin"], parent[b["junction"] - 1]) and np.array_equal(b["right_bin"], parent[b["junction"]])
    assert np.array_equal(b["scaffold"], init_c[b["right_bin"]])
    # behind moves, and behind the bomb and moves: the two trajectories of the fixtures
    seen = 0
    for name in FIXTURES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        col = {f: g["state"][i].astype(np.int64) for i, f in enumerate(FRAG_FIELDS)}
        order = g["full_order_high"].astype(np.int64)
        b = gs.bin_junctions(order, parent, col["id_c"])
        k = gs.block_junctions(order, parent, col["id_c"], col["ori"], col["id_d"], init_c, init_p)
        want_bins, want_blocks = _loop_junctions(order, parent, col["id_c"], col["ori"], col["id_d"], init_c, init_p)
        assert np.array_equal(b["junction"], want_bins) and np.array_equal(k["junction"], want_blocks), name
        assert np.isin(k["junction"], b["junction"]).all() and k["junction"].size < b["junction"].size
        for t in (b, k):
            assert np.array_equal(t["left_bin"], parent[order[t["junction"] - 1]]) and np.array_equal(t["right_bin"], parent[order[t["junction"]]])
            assert np.array_equal(t["scaffold"], col["id_c"][t["left_bin"]]) and np.array_equal(t["scaffold"], col["id_c"][t["right_bin"]])
        seen += k["junction"].size
    assert seen > 0  # (the moves made joins the input assembly does not vouch for)
    empty = gs.block_junctions(np.zeros(0, np.int64), parent, init_c, ones, ids, init_c, init_p)
    assert all(empty[f].size == 0 for f in ("junction", "left_bin", "right_bin", "scaffold"))


def test_model_values_host_against_the_oracle(oracle_lib):
    """e_q bit for bit; l_q within half a quantum of log10 of the oracle's value plus the stated error of ig_log2_pos
    (include/ig_detmath.h, "absolute error below 1e-15", the comment above ig_log2_pos; test_contract_precision_host.py holds the
    function to it) with slack for the final multiply and add"""
    from instagraal_amd import hip_lib
    from oracle.oracle_lib import PARAM_DTYPE

    hip_lib.build_lib()
    d_max = float(P8[5])
    rng = np.random.RandomState(9)
    s = np.concatenate([[0.0, 1e-45, 1e-40, 1.1754942e-38, 1e-30, 1e-6, d_max, np.nextafter(np.float32(d_max), np.float32(0)), np.nextafter(np.float32(d_max), np.float32(1e9)),
                         2 * d_max], rng.uniform(0.0, 2 * d_max, 8990), np.exp(rng.uniform(np.log(1e-3), np.log(2 * d_max), 1000))]).astype(np.float32)
    assert s.size == 10000 and s[1] > 0 and s[1] < 1.1754944e-38 and s[6] == np.float32(d_max)
    p = np.zeros(1, PARAM_DTYPE)
    for k, v in zip(PARAM_DTYPE.names, P8):
        p[k] = v
    before = oracle_lib.lib().igo_get_mode()
    oracle_lib.set_mode(oracle_lib.MODE_DET)
    try:
        ex = oracle_lib.eval_terms(s, np.zeros(s.size, np.float32), np.zeros(s.size, np.int32), p)[0]
    finally:
        oracle_lib.set_mode(before)
    e_q, l_q = hip_lib.model_values_host(P8, s)
    assert e_q.dtype == l_q.dtype == np.int64 and e_q.shape == l_q.shape == s.shape
    clipped = np.minimum(ex.astype(np.float64), 2.0 ** 20)  # (ig_quantize clamps a term at 2^20: the power law near s = 0)
    assert np.array_equal(e_q, np.rint(clipped * 2.0 ** 32).astype(np.int64))
    assert (ex > 2.0 ** 20).sum() < 50 and (ex == np.float32(P8[7])).sum() > 4000  # beyond d_max, and at 0: v_inter
    with np.errstate(invalid="ignore"):  # (ig_quantize clamps at +-2^20: only the infinite values of denormal separations get there)
        err = np.abs(l_q * 2.0 ** -32 - np.clip(np.log10(ex.astype(np.float64)), -2.0 ** 20, 2.0 ** 20))
    assert np.isinf(ex).sum() < 5 and np.all(np.abs(np.log10(ex[np.isfinite(ex)].astype(np.float64))) < 40)
    assert err.max() <= 2.0 ** -33 + 1e-12, err.max()
    # shapes, the empty call, the infinite separation, a wrong number of parameters
    e2, l2 = hip_lib.model_values_host(P8, s.reshape(100, 100))
    assert e2.shape == (100, 100) and np.array_equal(e2.ravel(), e_q) and np.array_equal(l2.ravel(), l_q)
    e0, l0 = hip_lib.model_values_host(P8, np.zeros(0, np.float32))
    assert e0.size == 0 and l0.size == 0
    e_inf, l_inf = hip_lib.model_values_host(P8, np.array([np.inf], np.float32))
    assert e_inf[0] == np.rint(np.float64(P8[7]) * 2.0 ** 32) and abs(l_inf[0] * 2.0 ** -32 - np.log10(np.float64(P8[7]))) <= 2.0 ** -33 + 1e-12
    with pytest.raises(hip_lib.HipError, match="eight"):
        hip_lib.model_values_host(P8[:7], s)


def test_support_host_with_the_products_model_and_with_the_oracles_agree_on_expected_q(oracle_lib):
    """the e_q half of the callable built from the oracle gives the same expected_q as the product's host entry"""
    from instagraal_amd import gap_support as gs, hip_lib
    from oracle.oracle_lib import PARAM_DTYPE

    hip_lib.build_lib()
    p = np.zeros(1, PARAM_DTYPE)
    for k, v in zip(PARAM_DTYPE.names, P8):
        p[k] = v

    def from_oracle(s):
        s = np.ascontiguousarray(s, np.float32)
        before = oracle_lib.lib().igo_get_mode()
        oracle_lib.set_mode(oracle_lib.MODE_DET)
        try:
            ex = oracle_lib.eval_terms(s, np.zeros(s.size, np.float32), np.zeros(s.size, np.int32), p)[0]
        finally:
            oracle_lib.set_mode(before)
        return np.rint(np.minimum(ex.astype(np.float64), 2.0 ** 20) * 2.0 ** 32).astype(np.int64), np.zeros(s.size, np.int64)

    t = _hand_made()
    gaps = gs.default_gaps(2.1, float(P8[5]))
    a = gs.support_host(*t, HAND_JUNCTIONS, gaps, 20, lambda s: hip_lib.model_values_host(P8, s))
    b = gs.support_host(*t, HAND_JUNCTIONS, gaps, 20, from_oracle)
    assert np.array_equal(a["expected_q"], b["expected_q"]) and a["expected_q"][~HAND_RING].all() and a["apart_q"][0] == b["apart_q"][0]
    assert np.array_equal(a["observed"], b["observed"]) and a["log_q"].any() and not b["log_q"].any()
    # expected_q falls with the gap and flattens at the trans level: pairs * v_inter beyond d_max
    assert np.all(np.diff(a["expected_q"][~HAND_RING], axis=1) <= 0)
    assert np.array_equal(a["expected_q"][:, -1], a["pairs"] * a["apart_q"][0])


def test_import_needs_neither_matplotlib_nor_the_library():
    code = ("import sys; sys.modules['matplotlib'] = None; sys.modules['ctypes'] = None\n"
            "from instagraal_amd import gap_support as g; print(g.DEFAULT_WINDOW, len(g.SCALARS))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["64", "8"], out.stderr
