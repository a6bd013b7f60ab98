"""GPU tests of the junction support profile of the current genome (ig_junction_profile, sampler.junction_profile) against the
rule's host statement (instagraal_amd.junction_profile.profile_host: every contact expanded, every pair enumerated) on the tables,
the state and the genome order downloaded from the same handle, with the model's quantised values from the oracle in DET mode.
Every comparison is exact integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
ALL = ("observed", "pairs", "expected_q")
WINDOWS = (1, 63, 64, 65, 1024)  # (beyond 64 positions the model pass takes a wave per position instead of a thread)


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
    """what profile_host takes, from ig_debug_tables, download_state and contact_map_order of the handle"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, rank, ln = s.ctx.debug_tables()
    state = s.ctx.download_state()
    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][parent], bad)
    order = s.ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return dist, stot, contig, placed, position


def _model_q(oracle_lib, s):
    """s (f32) -> the quantised model value under the sampler's parameter set 0: the oracle's ``ex`` in DET mode is ig_rippe bit
    for bit"""
    from oracle.oracle_lib import PARAM_DTYPE

    p = np.zeros(1, PARAM_DTYPE)
    for k in PARAM_DTYPE.names:
        p[k] = s.param_simu[k][0]

    def q(sep):
        sep = np.ascontiguousarray(sep, np.float32)
        before = oracle_lib.lib().igo_get_mode()
        oracle_lib.set_mode(oracle_lib.MODE_DET)
        try:
            ex = oracle_lib.eval_terms(sep, np.zeros(sep.size, np.float32), np.zeros(sep.size, np.int32), p)[0]
        finally:
            oracle_lib.set_mode(before)
        return np.rint(ex.astype(np.float64) * 2.0 ** 32).astype(np.int64)

    return q


def _assert_profile_equals_host(s, prob, oracle_lib, what, windows=WINDOWS, want_ring=False):
    from instagraal_amd import junction_profile as jp

    dist, stot, contig, placed, position = _host_inputs(s, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    q = _model_q(oracle_lib, s)
    kind = jp.junction_kinds(stot, contig, position)
    lengths = np.bincount(contig[placed & (stot == 0)])
    for w in windows:
        want = jp.profile_host(dist, stot, contig, placed, position, prob.coo_row, prob.coo_col, prob.coo_cnt, w, model_q=q)
        got = s.ctx.junction_profile(w)
        assert got["n_placed"] == want["n_placed"] == int(placed.sum()) and got["window"] == w
        for k in ALL:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, w, k)
        for k in jp.SCALARS:
            assert got[k] == want[k], (what, w, k, got[k], want[k])
        assert jp.observed_total(got) == total and got["spanned_observed"] == int(got["observed"].sum()), (what, w)
        assert int(got["pairs"].sum()) == jp.pairs_total_closed_form(lengths[lengths > 0], w), (what, w)
        assert all(not got[k][kind != jp.KIND_INTERNAL].any() for k in ALL), (what, w)
        assert got["internal_junctions"] == int((kind == jp.KIND_INTERNAL).sum())
        if want_ring:
            assert got["ring_observed"] > 0 and (kind == jp.KIND_RING).sum() >= 2
        lean = s.ctx.junction_profile(w, model=False)  # the model pass skipped: the observed part is the same
        assert lean["pairs"] is None and lean["expected_q"] is None and np.array_equal(lean["observed"], want["observed"])
        assert [lean[k] for k in jp.SCALARS] == [want[k] for k in jp.SCALARS]


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_host_on_the_fixture_states(name, oracle_lib):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    _assert_profile_equals_host(s, prob, oracle_lib, name)
    s.free_gpu()


def test_device_equals_host_on_small_fresh_after_moves_and_after_the_bomb(oracle_lib):
    prob, s = _sampler("small", seed=12)
    _assert_profile_equals_host(s, prob, oracle_lib, "small fresh")
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    _assert_profile_equals_host(s, prob, oracle_lib, "small after batch moves")
    s.bomb_the_genome()  # contigs of one bin: every window is longer than every contig
    _assert_profile_equals_host(s, prob, oracle_lib, "small after the bomb")
    s.free_gpu()


def test_device_equals_host_with_full_windows_of_1024(oracle_lib):
    prob, s = _sampler("bigctg", seed=12)
    _assert_profile_equals_host(s, prob, oracle_lib, "bigctg", windows=(64, 1024))
    full = s.ctx.junction_profile(1024)
    assert full["pairs"].max() == 1024 * 1025 // 2  # (contigs of about 3 000 sub-fragments: a window of 1 024 is full in their middle)
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring(oracle_lib):
    """operator 10 forced on the first and the last bin of one contig closes it on itself (paste_contigs KA:3367-3693)"""
    from instagraal_amd import junction_profile as jp

    prob, s = _sampler("small", seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    _assert_profile_equals_host(s, prob, oracle_lib, "small with a ring", windows=(1, 64, 1024), want_ring=True)
    prof = s.junction_profile(8)
    ring = prof["kind"] == jp.KIND_RING
    assert ring.any() and not any(prof[k][ring].any() for k in ALL) and prof["ring_observed"] > 0
    assert not np.isin(prof["bins"]["position"], np.nonzero(ring)[0]).any()
    s.free_gpu()


def test_observed_equals_the_contact_map_summed_across_every_junction():
    """an independent device path: the image of ig_contact_map at one position per pixel"""
    prob, s = _sampler("tiny", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    order = s.ctx.contact_map_order().astype(np.int64)
    T = order.size
    image, b = s.ctx.contact_map(max(T, 1))
    assert b == 1 and image.shape == (T, T)
    _, contig, stot, _, _ = s.ctx.debug_tables()
    c_pos, ring = contig[order], stot[order] != 0  # (a move may have closed a contig on itself: rings are left out)
    a, k = np.triu_indices(T, k=1)
    j = np.arange(1, T)
    for w in (1, 5, 64, 1024):
        keep = (c_pos[a] == c_pos[k]) & ~ring[a] & (k - a <= w)
        S = np.zeros((T, T), np.int64)
        S[a[keep], k[keep]] = image[a[keep], k[keep]]
        R = S.cumsum(0).cumsum(1)
        want = np.zeros(T, np.int64)
        want[1:] = R[j - 1, T - 1] - R[j - 1, j - 1]  # rows < j, columns >= j
        got = s.ctx.junction_profile(w, model=False)
        assert np.array_equal(got["observed"], want) and want.any(), w
    s.free_gpu()


def _checksum(prof):
    from instagraal_amd import junction_profile as jp

    T = prof["n_placed"]
    tot = sum(int(v) * (j + 1) for j, v in enumerate(prof["observed"].tolist())) + sum(prof[k] * (T + 1 + i) for i, k in enumerate(jp.OBSERVED_SCALARS))
    tot %= 1 << 64
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def test_both_forms_of_the_observed_pass_agree():
    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    for w in (1, 64, 1024):
        ms_a, ms_m, ms_s, ck_a = s.ctx.debug_junction_profile_time(w, combine=True, n=1)
        ms_b, none, none2, ck_b = s.ctx.debug_junction_profile_time(w, combine=False, n=1, model=False, scan=False)
        assert ck_a == ck_b == _checksum(s.ctx.junction_profile(w)), w
        assert ms_a.size == 1 and ms_a[0] > 0 and ms_m[0] > 0 and ms_s[0] > 0 and ms_b[0] > 0 and none is None and none2 is None
    s.free_gpu()


def test_the_shards_add_up():
    from instagraal_amd import junction_profile as jp, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    want = whole.junction_profile(64)
    parts = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        parts.append(ctx.junction_profile(64))
        ctx.close()
    assert all(p["observed"].sum() > 0 for p in parts)
    assert np.array_equal(parts[0]["observed"] + parts[1]["observed"], want["observed"])
    for k in jp.OBSERVED_SCALARS + ("spanned_observed",):
        assert parts[0][k] + parts[1][k] == want[k], k
    for p in parts:  # the model part whole on every rank
        assert np.array_equal(p["pairs"], want["pairs"]) and np.array_equal(p["expected_q"], want["expected_q"])
        assert p["internal_junctions"] == want["internal_junctions"]
    whole.close()


def test_the_pass_disturbs_nothing(tmp_path):
    outs = []
    for with_profile in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_profile:
            prof = s.junction_profile()
            assert prof["window"] == 64 and prof["observed"].sum() > 0 and prof["pairs"].sum() > 0 and prof["bins"].size > 0
            s.ctx.junction_profile(1024, model=False)
            s.display_junction_profile(str(tmp_path / "junctions.png"), window_kb=20.0)
            s.ctx.debug_junction_profile_time(64, combine=False, n=2)
            s.ctx.debug_junction_profile_time(200, combine=True, n=2)
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
    assert open(str(tmp_path / "junctions.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_parameters_matter(oracle_lib):
    from instagraal_amd import junction_profile as jp

    prob, s = _sampler("small", seed=5)
    before = s.ctx.junction_profile(64)
    p = dict(prob.params)
    p["slope"] = np.float32(p["slope"]) * np.float32(1.25)
    s.set_param_simu(p)
    after = s.ctx.junction_profile(64)
    assert np.array_equal(after["observed"], before["observed"]) and np.array_equal(after["pairs"], before["pairs"])
    assert not np.array_equal(after["expected_q"], before["expected_q"])
    dist, stot, contig, placed, position = _host_inputs(s, prob)
    want = jp.profile_host(dist, stot, contig, placed, position, prob.coo_row, prob.coo_col, prob.coo_cnt, 64, model_q=_model_q(oracle_lib, s))
    assert np.array_equal(after["expected_q"], want["expected_q"])
    s.free_gpu()


def test_sampler_junction_profile_table_and_weakest():
    from instagraal_amd import junction_profile as jp

    prob, s = _sampler("small", seed=6)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    prof = s.junction_profile()
    raw = s.ctx.junction_profile(jp.DEFAULT_WINDOW)
    assert prof["window"] == 64 and all(np.array_equal(prof[k], raw[k]) for k in ALL)
    assert np.array_equal(prof["expected"], raw["expected_q"] / 2.0 ** 32)
    ok = raw["expected_q"] != 0
    assert np.array_equal(prof["ratio"][ok], raw["observed"][ok] / prof["expected"][ok]) and np.all(np.isnan(prof["ratio"][~ok]))
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)[prof["order"]]
    t = prof["bins"]
    j = t["position"]
    want_j = np.nonzero((prof["kind"][1:] == jp.KIND_INTERNAL) & (parent[1:] != parent[:-1]))[0] + 1
    assert np.array_equal(j, want_j) and j.size > 0
    assert np.array_equal(t["left_frag"], parent[j - 1]) and np.array_equal(t["right_frag"], parent[j])
    g = s.gpu_vect_frags.copy_from_gpu()
    assert np.array_equal(t["contig"], g.id_c[parent[j]]) and np.array_equal(g.id_c[t["left_frag"]], g.id_c[t["right_frag"]])
    assert np.array_equal(t["observed"], raw["observed"][j]) and np.array_equal(t["pairs"], raw["pairs"][j])
    kb = s.junction_profile(window_kb=16.0)
    assert kb["window"] == jp.window_from_kb(16.0, s.mean_kb())
    with pytest.raises(ValueError):
        s.junction_profile(window=8, window_kb=16.0)
    weak = s.weakest_junctions(5, window=8)
    assert 0 < weak.size <= 5 and np.all(np.diff(weak["ratio"]) >= 0) and np.all(weak["pairs"] >= jp.default_min_pairs(8))
    assert s.weakest_junctions(3, min_pairs=10 ** 9, window=8).size == 0
    s.free_gpu()


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny")
    ref = s.ctx.junction_profile(64)
    T = ref["n_placed"]
    for bad in (0, 1025, -1):
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.junction_profile(bad)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_junction_profile_time(bad)
        assert np.array_equal(s.ctx.junction_profile(64)["observed"], ref["observed"])
    lib = hip_lib.lib()
    obs, prs, exq, sc = (np.full(T, -7, np.int64) for _ in range(4))
    sc = sc[:8].copy()
    n = C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    null = C.c_void_p(0)
    for args in ((null, p(prs), p(exq), C.c_int64(T), C.byref(n), p(sc)), (p(obs), p(prs), p(exq), C.c_int64(T), null, p(sc)),
                 (p(obs), p(prs), p(exq), C.c_int64(T), C.byref(n), null), (p(obs), null, p(exq), C.c_int64(T), C.byref(n), p(sc)),
                 (p(obs), p(prs), null, C.c_int64(T), C.byref(n), p(sc))):
        assert lib.ig_junction_profile(s.ctx._h, C.c_int32(64), *args) != 0 and b"NULL" in lib.ig_last_error()
        assert all(np.all(x == -7) for x in (obs, prs, exq, sc)) and n.value == -7  # nothing written
    # a short capacity: the size is reported, nothing else is written
    assert lib.ig_junction_profile(s.ctx._h, C.c_int32(64), p(obs), p(prs), p(exq), C.c_int64(T - 1), C.byref(n), p(sc)) != 0
    assert b"capacity" in lib.ig_last_error() and n.value == T and all(np.all(x == -7) for x in (obs, prs, exq, sc))
    assert lib.ig_junction_profile(s.ctx._h, C.c_int32(64), p(obs), null, null, C.c_int64(T), C.byref(n), p(sc)) == 0  # (both may be NULL)
    assert np.array_equal(obs, ref["observed"]) and np.all(prs == -7)
    # a parameter set whose values times the pairs of a window could overflow the 64-bit sum: refused, not wrapped
    vals = [np.float32(s.param_simu[k][0]) for k in PARAM_NAMES]
    huge = list(vals)
    huge[PARAM_NAMES.index("fact")] = np.float32(vals[PARAM_NAMES.index("fact")] * 1e12)
    s.ctx.set_params(huge, s.mean_kb(), 0)
    with pytest.raises(hip_lib.HipError, match="model value too large for this window"):
        s.ctx.junction_profile(1024)
    assert s.ctx.junction_profile(1024, model=False)["pairs"] is None  # (without the model pass there is nothing to guard)
    assert s.ctx.junction_profile(1)["expected_q"].max() > 0  # (one pair per junction: no sum to overflow)
    s.ctx.set_params(vals, s.mean_kb(), 0)
    again = s.ctx.junction_profile(64)
    assert all(np.array_equal(again[k], ref[k]) for k in ALL)
    # no contacts uploaded
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.junction_profile(64)
    bare.close()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.junction_profile(64)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_junction_profile_time(64)
    s.ctx.nuis_end()
    assert s.ctx.junction_profile(64)["observed"].size == T
    s.free_gpu()


def test_run_instagraal_save_junctions_writes_one_file_per_cycle(tmp_path):
    from instagraal_amd import junction_profile as jp, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=2, bomb=True, save_junctions=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    upper = s.sparse_matrix.tocoo()
    total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
    for j in range(2):
        lines = open(os.path.join(folder, "junctions_cycle_%d.txt" % j)).read().splitlines()
        assert lines[0][2:].split() == list(jp.BIN_COLUMNS)
        rows = [ln.split() for ln in lines if not ln.startswith("#")]
        assert all(len(r) == 8 for r in rows)
        ints = [[int(x) for x in r[:6]] for r in rows]  # (integers that parse)
        assert all(min(r) >= 0 for r in ints) and all(float(r[6]) >= 0 for r in rows)
        sc = dict(kv.split("=") for kv in lines[-1][2:].split())
        assert int(sc["window"]) == 64 and sum(int(sc[k]) for k in jp.OBSERVED_SCALARS) == total
        assert len(rows) <= int(sc["internal_junctions"]) < int(sc["n_placed"])
    assert len([ln for ln in open(os.path.join(folder, "junctions_cycle_1.txt")) if not ln.startswith("#")]) > 0  # (joins were made)
    assert not os.path.exists(os.path.join(folder, "junctions_cycle_2.txt"))
    p2.simulation.release()
    data2 = str(tmp_path / "data2")  # (a folder of its own: the first run left its pyramid in the other)
    synth.write_text_dataset(data2, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p3 = run_instagraal(data2, os.path.join(data2, "genome.fa"), output_folder=str(tmp_path / "out2"), level=2, cycles=1, bomb=True)
    assert not [f for f in os.listdir(p3.simulation.output_folder) if f.startswith("junctions")]
    p3.simulation.release()


@pytest.mark.slow
def test_headline_shape():
    """cfg3 (50 k bins, 149 k sub-fragments, 50 M contacts) from coo=, after 2 000 batch moves, w = 64: observed against a numpy
    restatement by difference arrays, the identities, and the weakest junctions"""
    from instagraal_amd import junction_profile as jp

    prob, s = _sampler("cfg3", coo=True)
    np.random.seed(4)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:2000].astype(np.int32), 5)
    dist, stot, contig, placed, position = _host_inputs(s, prob)
    row, col, cnt = prob.coo_row, prob.coo_col, prob.coo_cnt.astype(np.int64)
    w = 64
    prof = s.junction_profile(w)
    T = prof["n_placed"]
    both = placed[row] & placed[col]
    cis = both & (contig[row] == contig[col])
    lin = cis & (stot[row] == 0)
    pa, pb = np.minimum(position[row[lin]], position[col[lin]]), np.maximum(position[row[lin]], position[col[lin]])
    near = pb - pa <= w
    c = cnt[lin]
    diff = np.bincount(pa[near] + 1, weights=c[near].astype(np.float64), minlength=T + 1) - np.bincount(pb[near] + 1, weights=c[near].astype(np.float64), minlength=T + 1)
    assert np.abs(diff).max() < 2.0 ** 52
    want = np.cumsum(diff.astype(np.int64))[:T]
    assert np.array_equal(prof["observed"], want)
    assert (prof["in_window_observed"], prof["beyond_window_observed"], prof["trans_observed"], prof["ring_observed"], prof["unplaced_observed"]) == (
        int(c[near].sum()), int(c[~near].sum()), int(cnt[both & ~cis].sum()), int(cnt[cis & ~lin].sum()), int(cnt[~both].sum()))
    assert jp.observed_total(prof) == int(cnt.sum())
    assert prof["spanned_observed"] == int(want.sum()) == int((c * (pb - pa))[near].sum())
    lengths = np.bincount(contig[placed & (stot == 0)])
    assert int(prof["pairs"].sum()) == jp.pairs_total_closed_form(lengths[lengths > 0], w)
    kind = prof["kind"]
    assert prof["internal_junctions"] == int((kind == jp.KIND_INTERNAL).sum()) and not prof["expected_q"][kind != jp.KIND_INTERNAL].any()
    assert (prof["expected_q"][kind == jp.KIND_INTERNAL] > 0).all()
    again = s.ctx.junction_profile(w)
    assert all(np.array_equal(again[k], prof[k]) for k in ALL)  # the same from run to run
    weak = s.weakest_junctions(20, profile=prof)
    assert weak.size > 0 and np.all(weak["pairs"] >= jp.default_min_pairs(w)) and np.all(np.diff(weak["ratio"]) >= 0)
    ms_a, ms_m, ms_s, ck_a = s.ctx.debug_junction_profile_time(w, combine=True, n=3)
    ms_b, _, _, ck_b = s.ctx.debug_junction_profile_time(w, combine=False, n=3, model=False, scan=False)
    print("junction profile at cfg3, w = %d: observed pass %.1f us combined, %.1f us one atomic per end; model pass %.1f us; scan %.1f us"
          % (w, 1e3 * ms_a.min(), 1e3 * ms_b.min(), 1e3 * ms_m.min(), 1e3 * ms_s.min()))
    assert ck_a == ck_b == _checksum(prof)
    s.free_gpu()
