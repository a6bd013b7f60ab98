"""GPU tests of the distance law of the current genome (ig_distance_law, sampler.distance_law, estimate_parameters_from_genome)
against the rule's host statement (instagraal_amd.distance_law.law_host: brute force, no monotonicity assumption) on the tables and
the state downloaded from the same handle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
ALL = ("observed", "pairs")


def _sampler(cfg, seed=None, coo=False):
    from instagraal_amd import synth
    from instagraal_amd.sampler import sampler as hip_sampler

    prob = synth.make_problem(*synth.CONFIGS[cfg])
    if seed is not None:
        np.random.seed(seed)
    extra = dict(coo=(prob.coo_row, prob.coo_col, prob.coo_cnt)) if coo else {}
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0, **extra)
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return prob, s


def _host_inputs(s, prob):
    """what law_host takes, from ig_debug_tables and download_state of the handle (the tables are pinned bit for bit against the
    oracle in tests/test_hip_parity.py)"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, rank, ln = s.ctx.debug_tables()
    state = s.ctx.download_state()
    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][parent], bad)
    return dist, stot, contig, placed


def _edge_sets(s, dist):
    from instagraal_amd import distance_law as dlaw

    longest = float(dist.max())
    return {
        "linear": np.arange(0, 60.0 + 1.0, 1.0, dtype=np.float32),  # the reference's estimate shape
        "geometric": dlaw.default_edges(s.mean_kb(), longest),
        "one_bin": np.array([2.0, 30.0], np.float32),
        "4096_bins": np.linspace(0.0, longest * 1.01 + 1.0, 4097).astype(np.float32),
    }


def _assert_law_equals_host(s, prob, what, want_ring=False):
    from instagraal_amd import distance_law as dlaw

    dist, stot, contig, placed = _host_inputs(s, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    for label, edges in _edge_sets(s, dist).items():
        want = dlaw.law_host(dist, stot, contig, placed, prob.coo_row, prob.coo_col, prob.coo_cnt, edges)
        got = s.ctx.distance_law(edges)
        for k in ALL:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, label, k)
        for k in dlaw.SCALARS:
            assert got[k] == want[k], (what, label, k, got[k], want[k])
        assert dlaw.observed_total(got) == total and dlaw.pairs_total(got) == got["placed_pairs"], (what, label)
        if want_ring:
            assert got["ring_observed"] > 0 and got["ring_pairs"] > 0
        lean = s.ctx.distance_law(edges, pairs=False)  # the pairs pass skipped: the observed half is the same
        assert lean["pairs"] is None and np.array_equal(lean["observed"], want["observed"])
        assert [lean[k] for k in dlaw.OBSERVED_SCALARS] == [want[k] for k in dlaw.OBSERVED_SCALARS]
        assert lean["out_of_range_pairs"] == lean["trans_pairs"] == lean["ring_pairs"] == lean["placed_pairs"] == -1
    # dist does not decrease with the rank inside a contig: what the run form of the pairs pass rests on (law_host does not)
    _, _, _, rank, _ = s.ctx.debug_tables()
    by = np.lexsort((rank, contig))
    same = contig[by][1:] == contig[by][:-1]
    assert np.all(np.diff(dist[by])[same] >= 0), what


def _moves_then_bomb(s, prob, what, n_moves=300):
    _assert_law_equals_host(s, prob, what + " fresh")
    frags = np.random.permutation(prob.n_frags)[:n_moves]
    s.step_sampler_batch(frags, 5)
    _assert_law_equals_host(s, prob, what + " after batch moves")
    s.bomb_the_genome()
    _assert_law_equals_host(s, prob, what + " after the bomb")


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_host_on_the_fixture_states(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    _moves_then_bomb(s, prob, name)
    s.free_gpu()


@pytest.mark.parametrize("cfg", ["small", "bigctg"])
def test_device_equals_host(cfg):
    prob, s = _sampler(cfg, seed=12)
    _moves_then_bomb(s, prob, cfg)
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


@pytest.mark.parametrize("cfg", ["small", "bigctg"])
def test_a_state_with_a_ring(cfg):
    """operator 10 (split at A upstream, split at B downstream, paste) forced on the first and the last bin of one contig closes
    it on itself (paste_contigs KA:3367-3693)"""
    prob, s = _sampler(cfg, seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    _assert_law_equals_host(s, prob, cfg + " with a ring", want_ring=True)
    s.free_gpu()


def test_both_forms_of_the_observed_pass_agree():
    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    for label, edges in _edge_sets(s, s.ctx.debug_tables()[0]).items():
        ms_a, ms_p, ck_a = s.ctx.debug_distance_law_time(edges, privatised=True, n=1)
        ms_b, none, ck_b = s.ctx.debug_distance_law_time(edges, privatised=False, n=1, pairs=False)
        law = s.ctx.distance_law(edges)
        want = int((law["observed"] * np.arange(1, edges.size)).sum()) + sum(law[k] * (4096 + 1 + i) for i, k in enumerate(
            ("out_of_range_observed", None, "trans_observed", None, "ring_observed", None, "unplaced_observed")) if k)
        assert ck_a == ck_b == want, label
        assert ms_a.size == 1 and ms_a[0] > 0 and ms_p[0] > 0 and ms_b[0] > 0 and none is None
    s.free_gpu()


def test_the_shards_add_up():
    from instagraal_amd import distance_law as dlaw, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    edges = dlaw.default_edges(1.6, float(whole.debug_tables()[0].max()))
    want = whole.distance_law(edges)
    parts = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        parts.append(ctx.distance_law(edges))
        ctx.close()
    assert all(p["observed"].sum() > 0 for p in parts)
    assert np.array_equal(parts[0]["observed"] + parts[1]["observed"], want["observed"])
    for k in dlaw.OBSERVED_SCALARS:
        assert parts[0][k] + parts[1][k] == want[k], k
    for p in parts:  # the pairs whole on every rank
        assert np.array_equal(p["pairs"], want["pairs"])
        assert all(p[k] == want[k] for k in ("out_of_range_pairs", "trans_pairs", "ring_pairs", "placed_pairs"))
    whole.close()


def test_the_pass_disturbs_nothing(tmp_path):
    outs = []
    for with_law in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_law:
            law = s.distance_law()
            assert law["observed"].sum() > 0 and law["pairs"].sum() > 0 and law["model"].shape == law["observed"].shape
            s.ctx.distance_law(np.arange(0, 61, dtype=np.float32), pairs=False)
            s.display_distance_law(str(tmp_path / "law.png"))
            s.ctx.debug_distance_law_time(law["edges"], privatised=False, n=2)
        res.append(s.step_sampler_batch(frags[100:], 5))
        sums, ints = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
        outs.append((np.concatenate(res).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(),
                     np.random.get_state()[1].copy(), np.random.get_state()[2], [int(x) for x in s.ctx.valid_insert()]))
        s.free_gpu()
    a, b = outs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5] == b[5] and a[6] == b[6]
    assert open(str(tmp_path / "law.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_sampler_distance_law_returns_the_law_and_the_model():
    from instagraal_amd import distance_law as dlaw
    from instagraal_amd import optim_rippe_curve_update as opti

    prob, s = _sampler("small", seed=5)
    law = s.distance_law()
    dist = s.ctx.debug_tables()[0]
    assert np.array_equal(law["edges"], dlaw.default_edges(s.mean_kb(), float(dist.max())))
    m = law["mean_per_pair"]
    ok = law["pairs"] > 0
    assert np.array_equal(m[ok], law["observed"][ok] / law["pairs"][ok]) and np.all(np.isnan(m[~ok]))
    kuhn, lm, c1, slope, d, d_max, fact, d_nuc = s.param_simu[0]
    y = np.asarray(opti.peval(law["centres_kb"], [kuhn, lm, slope, d, fact]), np.float64)
    assert np.array_equal(law["model"], np.where(law["centres_kb"] < d_max, y, np.float64(d_nuc)))
    assert law["mean_value_trans_observed"] == law["trans_observed"] / law["trans_pairs"]
    # the synthetic contacts were drawn from a law that falls with the separation: so does what the device counted
    dense = ok & (law["pairs"] > 1000)
    assert m[dense][0] > 5 * m[dense][-1] > 0
    custom = s.distance_law(np.array([1.0, 10.0, 100.0]))
    assert custom["observed"].size == 2 and custom["edges"].dtype == np.float32
    s.free_gpu()


def test_estimate_parameters_from_genome_on_a_coo_sampler():
    from instagraal_amd import distance_law as dlaw
    from instagraal_amd import optim_rippe_curve_update as opti
    from instagraal_amd.sampler import PARAM_NAMES, fit_law

    prob, s = _sampler("small", seed=6, coo=True)
    assert s.sparse_matrix is None
    with pytest.raises(ValueError, match="estimate_parameters_from_genome"):
        s.estimate_parameters_rippe(60.0, 1.0)
    mvt0 = s.mean_value_trans
    s.estimate_parameters_from_genome(60.0, 1.0)
    got = [s.param_simu[k][0] for k in PARAM_NAMES]
    assert np.all(np.isfinite(got)) and s.param_simu["d_max"][0] > 0
    assert np.array_equal(s.param_simu, s.param_simu_test) and np.isfinite(s.likelihood_t).all()
    # the same functions on the host-computed law: the same bits
    edges = np.arange(0, 61.0, 1.0).astype(np.float32)
    dist, stot, contig, placed = _host_inputs(s, prob)
    host = dlaw.law_host(dist, stot, contig, placed, prob.coo_row, prob.coo_col, prob.coo_cnt, edges)
    with opti.quiet_runs():
        bins_upd, mean_upd, p, y, mvt, d_max = fit_law(host, mvt0)
    assert mvt == mvt0 / 10.0 == s.mean_value_trans
    mean = host["observed"] / np.maximum(host["pairs"], 1)
    good = (host["pairs"] > 0) & (host["observed"] > 0)
    assert np.array_equal(bins_upd, edges[1:][good].astype(np.float64)) and np.array_equal(mean_upd, (mean[good] + mvt0).astype(np.float32))
    p2, _ = opti.estimate_param_rippe(mean_upd, bins_upd)
    assert np.array_equal(np.asarray(p), np.asarray(p2)) and d_max == opti.estimate_max_dist_intra(p2, mvt)
    want = s.setup_rippe_parameters(p, d_max)
    assert want.tobytes() == s.param_simu.tobytes()
    s.free_gpu()


def test_estimate_parameters_rippe_with_a_matrix_is_what_it_was():
    """the reference-shaped estimate on a sampler that has its matrix: the host function's result, parameter for parameter"""
    from instagraal_amd.sampler import estimate_rippe_host

    prob, s = _sampler("small", seed=7)
    mvt0 = s.mean_value_trans
    want = estimate_rippe_host(s.sparse_matrix, s.np_sub_frags_2_frags, s.S_o_A_frags, s.n_frags, mvt0, 60.0, 1.0)
    s.estimate_parameters_rippe(60.0, 1.0)
    assert s.param_simu.tobytes() == s.setup_rippe_parameters(want[2], want[5]).tobytes() and s.mean_value_trans == want[4]
    s.free_gpu()


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny")
    good = np.arange(0, 61, dtype=np.float32)
    ref = s.ctx.distance_law(good)
    too_many = np.arange(4098, dtype=np.float32)
    for bad, word in (([0.0, 2.0, 1.0], "sorted"), ([0.0, np.nan, 3.0], "finite"), ([0.0, np.inf], "finite"), (too_many, "n_edges"),
                      ([1.0], "n_edges")):
        with pytest.raises(hip_lib.HipError, match=word):
            s.ctx.distance_law(np.array(bad, np.float32))
        assert np.array_equal(s.ctx.distance_law(good)["observed"], ref["observed"])
    lib = hip_lib.lib()
    obs, prs, sc = np.full(60, -7, np.int64), np.full(60, -7, np.int64), np.full(8, -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for args in ((C.c_void_p(0), C.c_int32(61), p(obs), p(prs), p(sc)), (p(good), C.c_int32(61), C.c_void_p(0), p(prs), p(sc)),
                 (p(good), C.c_int32(61), p(obs), p(prs), C.c_void_p(0))):
        assert lib.ig_distance_law(s.ctx._h, *args) != 0 and b"NULL" in lib.ig_last_error()
        assert np.all(obs == -7) and np.all(prs == -7) and np.all(sc == -7)  # nothing written
    assert lib.ig_distance_law(s.ctx._h, p(good), C.c_int32(61), p(obs), C.c_void_p(0), p(sc)) == 0  # (pairs may be NULL)
    assert np.array_equal(obs, ref["observed"])
    # no contacts uploaded
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.distance_law(good)
    bare.close()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.distance_law(good)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_distance_law_time(good)
    s.ctx.nuis_end()
    assert s.ctx.distance_law(good)["observed"].size == 60
    s.free_gpu()


def test_run_instagraal_save_law_writes_one_file_per_cycle(tmp_path):
    from instagraal_amd import synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=2, bomb=True, save_law=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    upper = s.sparse_matrix.tocoo()
    total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
    for j in range(2):
        path = os.path.join(folder, "distance_law_cycle_%d.txt" % j)
        lines = open(path).read().splitlines()
        rows = [ln.split() for ln in lines if not ln.startswith("#")]
        assert rows and all(len(r) == 4 for r in rows)
        lo, hi = [float(r[0]) for r in rows], [float(r[1]) for r in rows]
        obs, prs = [int(r[2]) for r in rows], [int(r[3]) for r in rows]  # (integers that parse)
        assert lo[1:] == hi[:-1] and all(a < b for a, b in zip(lo, hi)) and min(obs) >= 0 and min(prs) >= 0
        sc = dict(kv.split("=") for kv in lines[-1][2:].split())
        assert sum(obs) + sum(int(sc[k]) for k in ("out_of_range_observed", "trans_observed", "ring_observed", "unplaced_observed")) == total
        assert sum(prs) + int(sc["out_of_range_pairs"]) + int(sc["ring_pairs"]) == int(sc["placed_pairs"])
    assert not os.path.exists(os.path.join(folder, "distance_law_cycle_2.txt"))
    p2.simulation.release()
    data2 = str(tmp_path / "data2")  # (a folder of its own: the first run left its pyramid in the other)
    synth.write_text_dataset(data2, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p3 = run_instagraal(data2, os.path.join(data2, "genome.fa"), output_folder=str(tmp_path / "out2"), level=2, cycles=1, bomb=True)
    assert not [f for f in os.listdir(p3.simulation.output_folder) if f.startswith("distance_law")]
    p3.simulation.release()


def _host_observed(dist, stot, contig, placed, prob, edges):
    """the observed part as a vectorised numpy histogram (M-length tables, every contact once)"""
    row, col, cnt = prob.coo_row, prob.coo_col, prob.coo_cnt.astype(np.int64)
    both = placed[row] & placed[col]
    cis = both & (contig[row] == contig[col])
    lin = cis & (stot[row] == 0)
    sep = np.abs(dist[row[lin]] - dist[col[lin]])
    b = np.searchsorted(edges, sep, side="right") - 1
    inside = (b >= 0) & (b < edges.size - 1)
    w = np.bincount(b[inside], weights=cnt[lin][inside].astype(np.float64), minlength=edges.size - 1)
    assert w.max() < 2.0 ** 52
    return (w.astype(np.int64), int(cnt[lin][~inside].sum()), int(cnt[both & ~cis].sum()), int(cnt[cis & ~lin].sum()), int(cnt[~both].sum()))


@pytest.mark.slow
def test_headline_shape():
    """cfg3 (50 k bins, 149 k sub-fragments, 50 M contacts) from coo=, after 2 000 batch moves: both identities, and the observed
    part against a vectorised numpy histogram.  The pairs at this size are held to their identity only (brute force is out of reach
    here: the entry-for-entry check runs at small and bigctg)."""
    from instagraal_amd import distance_law as dlaw

    prob, s = _sampler("cfg3", coo=True)
    np.random.seed(4)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:2000].astype(np.int32), 5)
    dist, stot, contig, placed = _host_inputs(s, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    for edges in (dlaw.default_edges(s.mean_kb(), float(dist.max())), np.arange(0, 61, dtype=np.float32)):
        law = s.ctx.distance_law(edges)
        obs, oor, trans, ring, unplaced = _host_observed(dist, stot, contig, placed, prob, edges)
        assert np.array_equal(law["observed"], obs)
        assert (law["out_of_range_observed"], law["trans_observed"], law["ring_observed"], law["unplaced_observed"]) == (oor, trans, ring, unplaced)
        assert dlaw.observed_total(law) == total
        n_c = np.bincount(contig[placed])
        assert law["placed_pairs"] == int((n_c * (n_c - 1) // 2).sum()) == dlaw.pairs_total(law)
        T = int(placed.sum())
        assert law["trans_pairs"] == T * (T - 1) // 2 - law["placed_pairs"]
        again = s.ctx.distance_law(edges)
        assert all(np.array_equal(again[k], law[k]) for k in ALL)  # the same from run to run
        ms_a, ms_p, ck_a = s.ctx.debug_distance_law_time(edges, privatised=True, n=3)
        ms_b, _, ck_b = s.ctx.debug_distance_law_time(edges, privatised=False, n=3, pairs=False)
        print("distance law at cfg3, %d bins: observed pass %.1f us privatised, %.1f us one atomic per contact; pairs pass %.1f us"
              % (edges.size - 1, 1e3 * ms_a.min(), 1e3 * ms_b.min(), 1e3 * ms_p.min()))
        assert ck_a == ck_b
    s.free_gpu()
