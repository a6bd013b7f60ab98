"""GPU tests of the expected contact map of the current genome (ig_expected_map, sampler.expected_map / residual_map) against the
rule's host statement (instagraal_amd.expected_map.expected_host: every pair of every contig enumerated) on the tables, the state and
the genome order downloaded from the same handle, with the model's quantised values from the oracle in DET mode.  Every comparison
of the device with the rule is exact integer equality; the row form, the tile form and the tile form without its constant shortcut
must return the same bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
FORM_ROWS, FORM_TILES, FORM_PLAIN = 1, 2, 3
FORMS = (FORM_ROWS, FORM_TILES, FORM_PLAIN)
COMPARED = ("n_placed", "linear_cis_pairs", "ring_pairs_total", "max_q")


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


def _host_inputs(ctx):
    """what expected_host takes, from ig_debug_tables and contact_map_order of the handle (the order holds the placed
    sub-fragments only: the contigs with every bin active)"""
    dist, contig, stot, _, _ = ctx.debug_tables()
    order = ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return dist, stot, contig.astype(np.int64), position


def _model_q(oracle_lib, params):
    """s (f32) -> the quantised model value under ``params`` (a PARAM_DTYPE record or a dict): the oracle's ``ex`` in DET mode is
    ig_rippe bit for bit"""
    from oracle.oracle_lib import PARAM_DTYPE

    p = np.zeros(1, PARAM_DTYPE)
    for k in PARAM_DTYPE.names:
        p[k] = np.float32(params[k][0] if isinstance(params, np.ndarray) else params[k])

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


def _max_sides(T):
    """descending: one position per pixel first; T / 2, T / 3 and T / 7 leave pixels of 2, 3 and 7 positions (a partial last one
    unless they divide T), 64 pixels of tens, 1 a single pixel"""
    return sorted({T + 5, T, -(-T // 2), -(-T // 3), -(-T // 7), 64, 1} - {0}, reverse=True)


def _checksum(got):
    from instagraal_amd import expected_map as em

    words = np.concatenate([got[k].ravel() for k in em.IMAGES]).astype(np.uint64)
    with np.errstate(over="ignore"):
        tot = int((words * np.arange(1, words.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    tot += sum(got[k] * (words.size + 1 + i) for i, k in enumerate(COMPARED[1:]))
    tot %= 1 << 64
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def _assert_device_equals_rule(ctx, oracle_lib, params, what, max_sides=None, direct=False, forms=FORMS):
    """every form of the device pass against the rule at every max_side.  The rule is enumerated once, at one position per pixel;
    the other sizes are its block sums (tests/test_expected_map_host.py holds that relation against the dense statement) --
    ``direct``: enumerated at every size instead (states too long for an image of T x T).  -> the last device result"""
    from instagraal_amd import expected_map as em

    ds, stot, contig, position = _host_inputs(ctx)
    T = int((position >= 0).sum())
    q = _model_q(oracle_lib, params)
    d_max = np.float32(params["d_max"][0] if isinstance(params, np.ndarray) else params["d_max"])
    one = None if direct else em.expected_host(ds, stot, contig, position, max(T, 1), q)
    got, refused = None, []
    for max_side in (_max_sides(T) if max_sides is None else max_sides):
        if direct:
            want = em.expected_host(ds, stot, contig, position, max_side, q)
        else:
            from instagraal_amd.contact_map import binning

            b, side = binning(T, max_side)
            want = dict(one, bin=b, side=side)
            want.update((k, em.block_sum(one[k], b, side)) for k in em.IMAGES)
        # the overflow guard is part of the entry point: where the rule's own numbers say 2 bin^2 max(max_q, q_trans) >= 2^62 (one pixel
        # over the whole of ``small``: 1.8 10^7 pairs of up to 150 contacts each) the device must refuse under every form, not return bytes
        q_trans = abs(em.quantize(np.float32(params["v_inter"][0] if isinstance(params, np.ndarray) else params["v_inter"])))
        if 2 * want["bin"] ** 2 * max(want["max_q"], q_trans) >= 1 << 62:
            from instagraal_amd import hip_lib

            assert want["bin"] > 1000, (what, max_side)  # (only a pixel of thousands of positions can get there)
            for form in forms:
                ctx.debug_expected_map_form(form)
                with pytest.raises(hip_lib.HipError, match="model value too large for this pixel size"):
                    ctx.expected_map(max_side)
                with pytest.raises(hip_lib.HipError, match="model value too large for this pixel size"):
                    ctx.debug_expected_map_time(max_side, form, 1)
            ctx.debug_expected_map_form(0)
            refused.append(max_side)
            continue
        census = em.tile_census(ds, stot, contig, position, max_side, d_max) if want["bin"] > 1 else None  # (one position per pixel: the row form)
        sums = set()
        for form in (forms if want["bin"] > 1 else forms[:2]):  # (one position per pixel: every form is the rows; that the setting is ignored is seen once)
            ctx.debug_expected_map_form(form)
            got = ctx.expected_map(max_side)
            assert got["side"] == want["side"] and got["bin"] == want["bin"], (what, max_side, form)
            for k in em.IMAGES:
                assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, max_side, form, k)
            for k in COMPARED:
                assert got[k] == want[k], (what, max_side, form, k, got[k], want[k])
            tiles = (got["tiles_evaluated"], got["tiles_constant"])
            if form == FORM_ROWS or got["bin"] == 1:
                assert tiles == (0, 0), (what, max_side, form)
            elif form == FORM_TILES:
                assert tiles == (census["evaluated"], census["constant"]), (what, max_side, tiles, census)
            else:
                assert tiles == (census["listed"], 0), (what, max_side, tiles, census)
            ms, ck = ctx.debug_expected_map_time(max_side, form, 1)
            assert ms.size == 1 and ms[0] > 0 and ck == _checksum(got), (what, max_side, form)
            sums.add(ck)
        assert len(sums) == 1
        ctx.debug_expected_map_form(0)
        assert int(got["cis_pairs"].sum()) == 2 * got["linear_cis_pairs"] and int(got["ring_pairs"].sum()) == 2 * got["ring_pairs_total"]
    assert got is not None and refused in ([], [1])  # (nothing but the single pixel is ever refused)
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_rule_on_the_fixture_states(name, oracle_lib):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, name)
    s.free_gpu()


def test_device_equals_the_rule_on_small_fresh(oracle_lib):
    from instagraal_amd import expected_map as em

    prob, s = _sampler("small", seed=12)
    _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "small fresh")
    ds, stot, contig, position = _host_inputs(s.ctx)
    most = [em.tile_census(ds, stot, contig, position, m, 1e9)["max_contigs_per_pixel"] for m in _max_sides(ds.size)]
    assert 2 in most and max(most) >= 3  # (pixels that straddle two and three contigs were among them)
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_moves(oracle_lib):
    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "small after batch moves")
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_the_bomb(oracle_lib):
    prob, s = _sampler("small", seed=12)
    s.bomb_the_genome()  # contigs of one bin: up to three positions each
    got = _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "small after the bomb")
    assert got["linear_cis_pairs"] < 3 * prob.n_frags
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring(oracle_lib):
    """operator 10 forced on the first and the last bin of one contig closes it on itself (paste_contigs KA:3367-3693)"""
    prob, s = _sampler("small", seed=13)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    got = _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "small with a ring")
    assert got["ring_pairs_total"] > 0
    res = s.residual_map(64)
    assert res["mask"].any() and np.array_equal(res["mask"], (s.expected_map(64)["ring_pairs"] != 0) | (res["expected"] == 0))
    s.free_gpu()


def test_a_state_with_an_unplaced_contig(oracle_lib):
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    before = s.ctx.expected_map(64)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    members = np.nonzero(id_c == ids[np.argmax(n >= 3)])[0]
    s.ctx.debug_set_bin_active(members[1], False)
    got = _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "small with an unplaced contig")
    assert got["n_placed"] < before["n_placed"]
    s.ctx.debug_set_bin_active(members[1], True)
    again = s.ctx.expected_map(64)
    assert all(np.array_equal(again[k], before[k]) for k in ("cis_q", "cis_pairs", "ring_pairs")) and again["n_placed"] == before["n_placed"]
    s.free_gpu()


@pytest.mark.parametrize("lowered", (False, True))
def test_long_contigs_and_constant_tiles(lowered, oracle_lib):
    """``bigctg``: contigs of thousands of positions, pixels of 188 and 24 -- a wave per row of a tile; once under the synthetic
    parameters and once with d_max at a third of the longest contig's span"""
    prob, s = _sampler("bigctg", seed=12)
    p = dict(prob.params)
    if lowered:
        p["d_max"] = np.float32(s.ctx.debug_tables()[0].max() / 3.0)
        s.set_param_simu(p)
    for max_side in (64, 512):
        got = _assert_device_equals_rule(s.ctx, oracle_lib, p, "bigctg lowered=%r" % lowered, max_sides=(max_side,), direct=True, forms=(FORM_ROWS, FORM_TILES, FORM_PLAIN))
        s.ctx.debug_expected_map_form(FORM_TILES)
        tiles = s.ctx.expected_map(max_side)
        s.ctx.debug_expected_map_form(0)
        assert tiles["tiles_constant"] > 0 and tiles["tiles_evaluated"] > 0, (max_side, tiles["tiles_constant"], tiles["tiles_evaluated"])
        assert all(np.array_equal(tiles[k], got[k]) for k in ("cis_q", "cis_pairs", "ring_pairs"))
    s.free_gpu()


def test_cross_checks_with_the_junction_profile_and_the_distance_law():
    """two other device paths on the same handle: expected_q of ig_junction_profile is the band of cis_q at one position per pixel
    summed across every junction; placed_pairs of ig_distance_law is the two pair counts"""
    prob, s = _sampler("tiny", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    T = s.ctx.contact_map_order().size
    got = s.ctx.expected_map(max(T, 1))
    assert got["bin"] == 1 and got["side"] == T
    i, k = np.triu_indices(T, k=1)
    j = np.arange(1, T)
    for w in (1, 64):
        near = k - i <= w
        S = np.zeros((T, T), np.int64)
        S[i[near], k[near]] = got["cis_q"][i[near], k[near]]
        R = S.cumsum(0).cumsum(1)
        want = np.zeros(T, np.int64)
        want[1:] = R[j - 1, T - 1] - R[j - 1, j - 1]  # rows i < j, columns k >= j
        prof = s.ctx.junction_profile(w)
        assert np.array_equal(prof["expected_q"], want) and want.any(), w
    law = s.ctx.distance_law(np.array([0.0, 1e9], np.float32))
    assert got["linear_cis_pairs"] + got["ring_pairs_total"] == law["placed_pairs"] and got["ring_pairs_total"] == law["ring_pairs"]
    s.free_gpu()


def test_a_sharded_handle_returns_the_same_bytes():
    from instagraal_amd import synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    shard = problem_to_context(prob)
    shard.set_shard(1, 2)
    for max_side in (prob.n_sub_frags, 64):
        for form in (FORM_ROWS, FORM_TILES):
            whole.debug_expected_map_form(form)
            shard.debug_expected_map_form(form)
            a, b = whole.expected_map(max_side), shard.expected_map(max_side)
            assert all(np.array_equal(a[k], b[k]) for k in ("cis_q", "cis_pairs", "ring_pairs")) and a["cis_q"].any()
            assert all(a[k] == b[k] for k in a if np.isscalar(a[k]))
    whole.close()
    shard.close()


def test_two_calls_with_moves_in_between(oracle_lib):
    prob, s = _sampler("small", seed=15)
    frags = np.random.permutation(prob.n_frags)
    s.step_sampler_batch(frags[:100], 5)
    first = s.ctx.expected_map(64)
    s.step_sampler_batch(frags[100:150], 5)
    second = _assert_device_equals_rule(s.ctx, oracle_lib, s.param_simu, "behind 50 more moves", max_sides=(s.ctx.contact_map_order().size, 64), forms=(FORM_ROWS, FORM_TILES))
    assert not np.array_equal(first["cis_q"], second["cis_q"])
    s.free_gpu()


def test_the_pass_disturbs_nothing(tmp_path):
    outs = []
    for with_map in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_map:
            for form in (0,) + FORMS:
                s.ctx.debug_expected_map_form(form)
                assert s.ctx.expected_map(64)["cis_q"].any()
            s.ctx.debug_expected_map_form(0)
            s.ctx.debug_expected_map_time(32, FORM_TILES, 2)
            s.display_residual_matrix(str(tmp_path / "residuals.png"), max_side=128)
            assert s.strongest_residuals(5, max_side=128).size == 5
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
    assert open(str(tmp_path / "residuals.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, soa17_from_dict

    prob, s = _sampler("tiny")
    ref = s.ctx.expected_map(64)
    side = ref["side"]
    lib = hip_lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    img = [np.full(side * side, -7, np.int64) for _ in range(3)]
    sc = np.full(8, -7, np.int64)
    n, b = C.c_int32(-7), C.c_int32(-7)
    call = lambda max_side, cap: lib.ig_expected_map(s.ctx._h, C.c_int32(max_side), p(img[0]), p(img[1]), p(img[2]), C.c_int64(cap), C.byref(n), C.byref(b), p(sc))  # noqa: E731
    for bad in (0, -3):
        assert call(bad, side * side) != 0 and b"max_side" in lib.ig_last_error()
        with pytest.raises(hip_lib.HipError, match="max_side"):
            s.ctx.expected_map(bad)
        with pytest.raises(hip_lib.HipError, match="max_side"):
            s.ctx.debug_expected_map_time(bad)
    assert all(np.all(x == -7) for x in img + [sc]) and n.value == -7  # nothing written
    # a short capacity: the size is reported, nothing else is written
    assert call(64, side * side - 1) != 0 and b"hold" in lib.ig_last_error()
    assert n.value == side and b.value == ref["bin"] and all(np.all(x == -7) for x in img + [sc])
    assert call(64, side * side) == 0 and all(np.array_equal(x.reshape(side, side), ref[k]) for x, k in zip(img, ("cis_q", "cis_pairs", "ring_pairs")))
    with pytest.raises(hip_lib.HipError, match="form"):
        s.ctx.debug_expected_map_form(4)
    # a parameter set whose values times the pairs of a pixel could overflow the 64-bit sum: refused, not wrapped
    vals = [np.float32(s.param_simu[k][0]) for k in PARAM_NAMES]
    huge = list(vals)
    huge[PARAM_NAMES.index("fact")] = np.float32(vals[PARAM_NAMES.index("fact")] * 1e12)
    s.ctx.set_params(huge, s.mean_kb(), 0)
    for form in (FORM_ROWS, FORM_TILES):
        s.ctx.debug_expected_map_form(form)
        with pytest.raises(hip_lib.HipError, match="model value too large for this pixel size"):
            s.ctx.expected_map(1)
    s.ctx.debug_expected_map_form(0)
    assert s.ctx.expected_map(10 ** 6)["cis_q"].max() > 0  # (one pair per pixel: no sum to overflow)
    s.ctx.set_params(vals, s.mean_kb(), 0)
    again = s.ctx.expected_map(64)
    assert all(np.array_equal(again[k], ref[k]) for k in ("cis_q", "cis_pairs", "ring_pairs"))
    # parameters never set (no contact is needed: none is read)
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="state"):
        bare.expected_map(64)
    none = np.zeros(0, np.int32)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    with pytest.raises(hip_lib.HipError, match="parameters"):
        bare.expected_map(64)
    with pytest.raises(hip_lib.HipError, match="parameters"):
        bare.debug_expected_map_time(64)
    bare.set_params(vals, s.mean_kb(), 0)
    assert all(np.array_equal(bare.expected_map(64)[k], ref[k]) for k in ("cis_q", "cis_pairs", "ring_pairs"))
    bare.close()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.expected_map(64)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_expected_map_time(64)
    s.ctx.nuis_end()
    assert s.ctx.expected_map(64)["side"] == side
    s.free_gpu()


def test_nothing_placed_and_one_position():
    """T == 0: side = 0 and success; T == 1: one pixel, no pair"""
    from instagraal_amd import hip_lib

    prob, s = _sampler("tiny", seed=2)
    s.bomb_the_genome()  # every bin a contig of its own
    lonely = int(np.nonzero(prob.np_sub_frags_id["w"] == 1)[0][0])  # a bin of one sub-fragment
    for f in range(prob.n_frags):
        s.ctx.debug_set_bin_active(f, False)
    for form in (FORM_ROWS, FORM_TILES):
        s.ctx.debug_expected_map_form(form)
        got = s.ctx.expected_map(64)
        assert got["side"] == 0 and got["bin"] == 1 and all(got[k].shape == (0, 0) for k in ("cis_q", "cis_pairs", "ring_pairs"))
        assert all(got[k] == 0 for k in COMPARED + ("tiles_evaluated", "tiles_constant"))
    with pytest.raises(hip_lib.HipError, match="no sub-fragment is placed"):
        s.ctx.debug_expected_map_time(64)
    s.ctx.debug_set_bin_active(lonely, True)
    for form in (FORM_ROWS, FORM_TILES):
        s.ctx.debug_expected_map_form(form)
        for max_side in (1, 64):
            got = s.ctx.expected_map(max_side)
            assert got["side"] == 1 and got["bin"] == 1 and got["n_placed"] == 1 and all(got[k].tolist() == [[0]] for k in ("cis_q", "cis_pairs", "ring_pairs"))
            assert got["linear_cis_pairs"] == got["ring_pairs_total"] == got["max_q"] == 0
    s.ctx.debug_expected_map_form(0)
    full = s.expected_map(64)
    assert full["total"].tolist() == [[0]] and full["expected"].tolist() == [[0.0]]
    s.free_gpu()


def test_the_sampler_layer(oracle_lib):
    from instagraal_amd import expected_map as em

    prob, s = _sampler("small", seed=6)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    ds, stot, contig, position = _host_inputs(s.ctx)
    T = int((position >= 0).sum())
    for max_side in (2048, 100):
        full = s.expected_map(max_side)
        raw = s.ctx.expected_map(max_side)
        assert all(np.array_equal(full[k], raw[k]) for k in em.IMAGES) and all(full[k] == raw[k] for k in em.SCALARS)
        q_trans = em.quantize(np.float32(s.param_simu["v_inter"][0]))
        assert full["q_trans"] == q_trans == int(_model_q(oracle_lib, s.param_simu)(np.array([1e9], np.float32))[0])  # (beyond d_max the model IS the trans level)
        assert int(full["total"].sum()) == T * (T - 1)
        assert np.array_equal(full["trans_pairs"], full["total"] - raw["cis_pairs"] - raw["ring_pairs"])
        assert np.array_equal(full["expected_q"], raw["cis_q"] + full["trans_pairs"] * q_trans)
        # the f64 sum of the rule: every pair's own value, cis from the enumeration, trans at the trans level
        want = em.compose(em.expected_host(ds, stot, contig, position, max_side, _model_q(oracle_lib, s.param_simu)), q_trans)
        rule_sum = float(np.sum(want["expected_q"].astype(np.float64) / 2.0 ** 32))
        assert abs(float(full["expected"].sum()) - rule_sum) <= 1e-9 * abs(rule_sum) and rule_sum > 0
        res = s.residual_map(max_side)
        observed, b = s.ctx.contact_map(max_side)
        assert b == full["bin"] and np.array_equal(res["observed"], observed) and np.array_equal(res["expected"], full["expected"])
        mask = (full["expected"] == 0) | (full["ring_pairs"] != 0)
        assert np.array_equal(np.isnan(res["log2_ratio"]), mask) and np.array_equal(np.isnan(res["z"]), mask) and np.array_equal(res["mask"], mask)
        ok = ~mask
        assert np.array_equal(res["z"][ok], (observed[ok] - full["expected"][ok]) / np.sqrt(full["expected"][ok]))
        with np.errstate(divide="ignore"):
            assert np.array_equal(res["log2_ratio"][ok], np.log2(observed[ok] / full["expected"][ok]))
        order = s.ctx.contact_map_order().astype(np.int64)
        parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
        contig_of_position = s.gpu_vect_frags.copy_from_gpu().id_c.astype(np.int64)[parent][order]
        top = s.strongest_residuals(7, max_side=max_side)
        assert np.array_equal(top, em.strongest(res, 7, None, contig_of_position)) and top.size == 7
        assert np.all(np.diff(top["z"]) <= 0) and np.all(top["pixel_a"] < top["pixel_b"]) and np.all(top["pairs"] >= em.default_min_pairs(full["bin"]))
        assert s.strongest_residuals(3, min_pairs=10 ** 12, max_side=max_side).size == 0
    s.free_gpu()


def test_run_instagraal_save_residuals_writes_two_files_per_cycle(tmp_path):
    from instagraal_amd import expected_map as em, synth
    from instagraal_amd.contact_map import binning
    from instagraal_amd.simulation import run_instagraal

    folders = []
    for k, flag in enumerate((True, False)):
        data = str(tmp_path / ("run%d" % k) / "data")  # (a folder of its own: a run leaves its pyramid in it; the same name: the outputs carry it)
        os.makedirs(os.path.dirname(data))
        synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        np.random.seed(17)
        p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / ("out%d" % k)), level=2, cycles=2, bomb=True, save_residuals=flag)
        folders.append(p2.simulation.output_folder)
        if flag:
            s = p2.simulation.sampler
            T = s.ctx.contact_map_order().size
        p2.simulation.release()
    with_flag, without = folders
    for j in range(2):
        assert open(os.path.join(with_flag, "residuals_cycle_%d.png" % j), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
        lines = open(os.path.join(with_flag, "residuals_cycle_%d.txt" % j)).read().splitlines()
        assert lines[0][2:].split() == list(em.STRONGEST_COLUMNS)
        rows = [ln.split() for ln in lines if not ln.startswith("#")]
        assert 0 < len(rows) <= 20 and all(len(r) == len(em.STRONGEST_COLUMNS) for r in rows)
        assert all(int(r[0]) < int(r[1]) for r in rows) and [float(r[-1]) for r in rows] == sorted((float(r[-1]) for r in rows), reverse=True)
        sc = dict(kv.split("=") for kv in lines[-1][2:].split())
        assert int(sc["n_placed"]) == T and (int(sc["bin"]), int(sc["side"])) == binning(T, 2048) and int(sc["linear_cis_pairs"]) >= 0
    assert not os.path.exists(os.path.join(with_flag, "residuals_cycle_2.txt"))
    extra = sorted(f for f in os.listdir(with_flag) if f.startswith("residuals"))
    assert extra == ["residuals_cycle_0.png", "residuals_cycle_0.txt", "residuals_cycle_1.png", "residuals_cycle_1.txt"]
    rest = sorted(f for f in os.listdir(with_flag) if f not in extra)
    assert rest == sorted(os.listdir(without))  # every other output byte for byte
    for f in rest:
        pa, pb = os.path.join(with_flag, f), os.path.join(without, f)
        if os.path.isfile(pa):
            assert open(pa, "rb").read() == open(pb, "rb").read(), f
