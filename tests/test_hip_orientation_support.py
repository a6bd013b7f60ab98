"""GPU tests of the orientation support (ig_orientation_support, sampler.orientation_support) against the rule's host statement
(instagraal_amd.orientation_support.support_host: contact by contact, pair by pair) on the tables, the state and the genome order
downloaded from the same handle, with the model's quantised values from the oracle in DET mode.  Every comparison is exact integer
equality."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
ALL = ("geometry", "observed", "expected_q")


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


def _host_inputs(s, prob):
    """what support_host takes, from ig_debug_tables, download_state and contact_map_order of the handle; and the state's columns"""
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
    return (dist, stot, contig, placed, position), order, parent, col


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


def _levels(s, prob):
    """the two segment lists of the state of the moment, built here from the downloaded state -> {level: (first, last)}"""
    from instagraal_amd import orientation_support as osup

    _, order, parent, col = _host_inputs(s, prob)
    S0 = prob.S_o_A_frags
    b = osup.bin_segments(order, parent)
    k = osup.block_segments(order, parent, col["id_c"], col["ori"], col["id_d"], S0["id_c"], S0["pos"])
    return dict(bin=b, block=k)


def _assert_equals_host(s, prob, oracle_lib, what, windows, levels=("bin", "block"), segments=None, lean=True):
    """the device's arrays and scalars against support_host, for every window and list; -> the last result"""
    from instagraal_amd import orientation_support as osup

    tables, order, parent, col = _host_inputs(s, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    q = _model_q(oracle_lib, s)
    lists = _levels(s, prob)
    got = None
    for level in (levels if segments is None else ("custom",)):
        for w in windows:
            if segments is None:
                got = s.orientation_support(level=level, window=w)
                assert np.array_equal(got["first"], lists[level]["first"]) and np.array_equal(got["last"], lists[level]["last"]), (what, level)
                assert np.array_equal(got["first_bin"], lists[level]["first_bin"]) and np.array_equal(got["last_bin"], lists[level]["last_bin"])
            else:
                got = s.orientation_support(segments=segments, window=w)
            want = osup.support_host(*tables, prob.coo_row, prob.coo_col, prob.coo_cnt, got["first"], got["last"], w, model_q=q)
            assert got["n_placed"] == want["n_placed"] == int(tables[3].sum()) and got["window"] == w and got["level"] == level
            assert got["geometry"].dtype == np.int32 and got["observed"].dtype == np.int64 and got["expected_q"].dtype == np.int64
            for k in ALL:
                assert np.array_equal(got[k], want[k]), (what, level, w, k)
            for k in osup.SCALARS:
                assert got[k] == want[k], (what, level, w, k, got[k], want[k])
            assert osup.observed_total(got) == total and got["counted"] <= got["entries_observed"] <= 2 * got["counted"], (what, level, w)
            assert got["entries_observed"] == int(got["observed"].sum()) and got["n_judged"] == int((got["status"] == 0).sum())
            idle = got["status"] != 0
            assert not got["observed"][idle].any() and not got["expected_q"][idle].any() and (got["expected_q"][~idle] > 0).all()
            assert np.array_equal(got["scaffold"], col["id_c"][got["first_bin"]]) and np.array_equal(got["order"], order)
            if lean:  # the model pass skipped: the observed part is the same
                raw = s.ctx.orientation_support(w, got["first"], got["last"], model=False)
                assert raw["expected_q"] is None and np.array_equal(raw["observed"], want["observed"]) and np.array_equal(raw["geometry"], want["geometry"])
                assert [raw[k] for k in osup.SCALARS] == [want[k] for k in osup.SCALARS]
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_host_on_the_fixture_states(name, oracle_lib):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    _assert_equals_host(s, prob, oracle_lib, name, windows=(1, 2, 8, 64))
    s.free_gpu()


def _gappy_segments(T, starts_of_contigs, lengths):
    """custom segments that leave gaps, with segments of 1, 2 and 3 positions, each inside one contig"""
    first, last = [], []
    for st, n in zip(starts_of_contigs.tolist(), lengths.tolist()):
        r = st + 1
        for size in (1, 2, 3, 7, 2, 30):
            if r + size + 2 > st + n:
                break
            first.append(r)
            last.append(r + size - 1)
            r += size + (0 if size == 7 else 2)  # (a segment right behind another, and gaps)
    return np.array(first, np.int64), np.array(last, np.int64)


def test_device_equals_host_on_small_fresh_after_moves_and_after_the_bomb(oracle_lib):
    from instagraal_amd import junction_profile as jp

    prob, s = _sampler("small", seed=12)
    windows = (1, 8, 63, 64, 65, 1024)
    got = _assert_equals_host(s, prob, oracle_lib, "small fresh", windows)
    assert got["level"] == "block" and set(got["status"].tolist()) <= {1, 3} and got["n_judged"] == 0  # fresh: a block is its contig
    fresh_bins = s.orientation_support(level="bin")
    assert fresh_bins["window"] == 8 and fresh_bins["n_judged"] > 900 and (fresh_bins["keep"] > fresh_bins["flip"]).sum() > 0.95 * fresh_bins["n_judged"]
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    got = _assert_equals_host(s, prob, oracle_lib, "small after batch moves", windows)
    assert got["n_judged"] > 0
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    first, last = _gappy_segments(order.size, start, length)
    assert {1, 2, 3} <= set((last - first + 1).tolist()) and first.size > 20
    got = _assert_equals_host(s, prob, oracle_lib, "small, custom segments", (1, 8, 64, 1024), segments=(first, last))
    assert got["uncounted"] > 0 and got["within_segment"] > 0 and got["counted"] > 0 and {0, 1} <= set(got["status"].tolist())
    s.bomb_the_genome()  # contigs of one bin: no segment has a flank
    got = _assert_equals_host(s, prob, oracle_lib, "small after the bomb", windows)
    for level in ("bin", "block"):
        res = s.orientation_support(level=level, window=64)
        assert set(res["status"].tolist()) <= {1, 3} and res["n_judged"] == 0 and res["counted"] == 0 and res["n_seg"] == prob.n_frags
        assert res["unplaced"] + res["trans"] + res["ring"] + res["within_segment"] + res["uncounted"] == int(prob.coo_cnt.astype(np.int64).sum())
    s.free_gpu()


def test_arms_of_1024_and_segments_across_the_wave_threshold(oracle_lib):
    from instagraal_amd import hip_lib, junction_profile as jp

    prob, s = _sampler("bigctg", seed=12)
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    k = int(np.argmax(length))  # the long contig: two segments of 2 000+ positions fit in it, flanks and all
    assert length[k] >= 6600
    first = start[k] + np.array([300, 3500])
    last = first + np.array([2099, 2047])
    got = _assert_equals_host(s, prob, oracle_lib, "bigctg, segments of 2 000+ positions", (1024,), segments=(first, last), lean=False)
    assert got["geometry"][:, 1].tolist() == [1024, 1024] and got["geometry"][:, 2].tolist() == [300, 1024] and (got["pairs"] > 10 ** 6).all()
    # 2 * pairs just under, at and just over ORIENT_WAVE_PAIRS: arms of 15, 16 and 17 positions with both flanks full at w = 64
    W = hip_lib.ORIENTATION_SUPPORT_WAVE_PAIRS
    f3 = start[k] + np.array([200, 400, 600])
    l3 = f3 + np.array([29, 31, 33])
    got = _assert_equals_host(s, prob, oracle_lib, "bigctg, the threshold", (64,), segments=(f3, l3), lean=False)
    assert (2 * got["pairs"]).tolist() == [W - 256, W, W + 256]
    # every form of the model pass returns the same bytes
    cks = [s.ctx.debug_orientation_support_time(64, f3, l3, which="model", form=form)[1] for form in ("default", "wave", "workgroup")]
    both = np.concatenate([f3, first[1:]]), np.concatenate([l3, last[1:]])
    cks2 = [s.ctx.debug_orientation_support_time(1024, *both, which="model", form=form)[1] for form in ("default", "wave", "workgroup")]
    want = sum(int(v) * (i + 1) for i, v in enumerate(got["expected_q"].ravel().tolist())) % (1 << 64)
    assert cks[0] == cks[1] == cks[2] == (want - (1 << 64) if want >= 1 << 63 else want) and cks2[0] == cks2[1] == cks2[2]
    s.free_gpu()


def test_a_planted_inversion_is_found(oracle_lib):
    from instagraal_amd import orientation_support as osup

    prob, s = _sampler("small", seed=13)
    tables, order, parent, col = _host_inputs(s, prob)
    seg = osup.bin_segments(order, parent)
    before = osup.support_host(*tables, prob.coo_row, prob.coo_col, prob.coo_cnt, seg["first"], seg["last"], 8)
    d = osup.derived(before)
    interior = (before["geometry"][:, 0] == 0) & (before["geometry"][:, 2] == 8) & (before["geometry"][:, 3] == 8)
    score = np.where(interior & (d["keep"] + d["flip"] > 0), (d["keep"] - d["flip"]) / np.sqrt(np.maximum(d["keep"] + d["flip"], 1)), -np.inf)
    k = int(np.argmax(score))
    focal = int(seg["first_bin"][k])
    assert np.isfinite(score[k]) and before["observed"][k].sum() > 0
    s.test_copy_struct(focal, int(seg["first_bin"][k + 1]), 1)  # operator 1: the focal bin turned round where it lies
    s.modify_gl_cuda_buffer()
    assert s.gpu_vect_frags.copy_from_gpu().ori[focal] == -1
    tables, order, parent, col = _host_inputs(s, prob)
    q = _model_q(oracle_lib, s)
    after = osup.support_host(*tables, prob.coo_row, prob.coo_col, prob.coo_cnt, seg["first"], seg["last"], 8, model_q=q)
    assert np.array_equal(after["observed"][k], before["observed"][k][[osup.RL, osup.RR, osup.LL, osup.LR]])  # the swap, exactly
    da = osup.derived(after)
    assert da["flip"][k] > da["keep"][k]
    for res in (after, dict(after, expected_q=None)):
        assert osup.inverted_segments(res, 1)["segment"].tolist() == [k]
    got = _assert_equals_host(s, prob, oracle_lib, "small with a planted inversion", (8,), levels=("bin",))
    assert np.array_equal(got["observed"], after["observed"]) and np.array_equal(got["expected_q"], after["expected_q"])
    top = s.inverted_segments(1)
    assert top.size == 1 and top["segment"][0] == k and top["first_bin"][0] == top["last_bin"][0] == focal and top["flip"][0] > top["keep"][0]
    assert top["scaffold"][0] == col["id_c"][focal] and np.isfinite(top["llr"][0]) and top["llr"][0] > 0
    # at block level the bin is a block of its own between two blocks
    blocks = _assert_equals_host(s, prob, oracle_lib, "... at block level", (8,), levels=("block",))
    j = int(np.nonzero(blocks["first_bin"] == focal)[0][0])
    assert blocks["last_bin"][j] == focal and blocks["first"][j] == seg["first"][k] and blocks["last"][j] == seg["last"][k]
    assert blocks["scaffold"][j - 1] == blocks["scaffold"][j] == blocks["scaffold"][j + 1] and blocks["status"][j] == 0
    assert blocks["last"][j - 1] + 1 == blocks["first"][j] and blocks["last"][j] + 1 == blocks["first"][j + 1]
    assert s.inverted_segments(1, level="block")["first_bin"][0] == focal
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
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    got = _assert_equals_host(s, prob, oracle_lib, "small with a ring", (1, 8, 1024), levels=("bin",))
    on_ring = g.circ[got["first_bin"]] == 1
    assert on_ring.sum() >= 3 and got["ring"] > 0
    long_enough = got["last"] > got["first"]
    assert set(got["status"][on_ring & long_enough].tolist()) == {2} and not got["geometry"][on_ring & long_enough, 1:].any()
    assert not got["observed"][on_ring].any() and not got["expected_q"][on_ring].any() and 2 not in got["status"][~on_ring]
    s.free_gpu()


def _checksum(res):
    from instagraal_amd import orientation_support as osup

    words = res["observed"].ravel().tolist() + [res[k] for k in osup.SCALARS[:7]]
    tot = sum(int(v) * (j + 1) for j, v in enumerate(words)) % (1 << 64)
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def test_both_forms_of_the_observed_pass_agree():
    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    lists = _levels(s, prob)
    for level in ("bin", "block"):
        f, l = lists[level]["first"], lists[level]["last"]
        for w in (1, 8, 1024):
            ms_a, ck_a = s.ctx.debug_orientation_support_time(w, f, l, which="observed", form="combined", n=2)
            ms_b, ck_b = s.ctx.debug_orientation_support_time(w, f, l, which="observed", form="atomic", n=1)
            assert ck_a == ck_b == _checksum(s.ctx.orientation_support(w, f, l, model=False)), (level, w)
            assert ms_a.size == 2 and (ms_a > 0).all() and ms_b.size == 1 and ms_b[0] > 0
    s.free_gpu()


def test_the_shards_add_up():
    from instagraal_amd import orientation_support as osup, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    seg = osup.bin_segments(whole.contact_map_order().astype(np.int64), parent)
    want = whole.orientation_support(8, seg["first"], seg["last"])
    assert want["n_judged"] > 0 and want["counted"] > 0
    parts = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        parts.append(ctx.orientation_support(8, seg["first"], seg["last"]))
        ctx.close()
    assert all(p["observed"].sum() > 0 for p in parts)
    assert np.array_equal(parts[0]["observed"] + parts[1]["observed"], want["observed"])
    for k in osup.SCALARS[:7]:
        assert parts[0][k] + parts[1][k] == want[k], k
    for p in parts:  # the model part and the geometry whole on every rank
        assert np.array_equal(p["expected_q"], want["expected_q"]) and np.array_equal(p["geometry"], want["geometry"]) and p["n_judged"] == want["n_judged"]
    whole.close()


def test_refusals_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib, junction_profile as jp, orientation_support as osup
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny")
    lists = _levels(s, prob)
    f, l = lists["bin"]["first"], lists["bin"]["last"]
    ref = s.ctx.orientation_support(8, f, l)
    T, n_seg = ref["n_placed"], ref["n_seg"]

    def ok():
        again = s.ctx.orientation_support(8, f, l)
        assert all(np.array_equal(again[k], ref[k]) for k in ALL) and [again[k] for k in osup.SCALARS] == [ref[k] for k in osup.SCALARS]

    for bad in (0, 1025, -1):
        with pytest.raises(hip_lib.HipError, match="ig_orientation_support.*window"):
            s.ctx.orientation_support(bad, f, l)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_orientation_support_time(bad, f, l)
        with pytest.raises(ValueError, match="window"):
            s.orientation_support(window=bad)
        ok()
    # malformed lists: overlapping, unsorted, across two contigs, out of range
    tables, order, parent, col = _host_inputs(s, prob)
    _, start, length = jp.contig_runs(tables[2], tables[4])
    assert start.size >= 2 and length[0] >= 8
    edge = int(start[1])
    for first, last, what in (([2, 4], [4, 6], "not ascending and disjoint"), ([6, 1], [7, 3], "not ascending and disjoint"),
                              ([edge - 2], [edge + 1], "spans two contigs"), ([0], [T], "out of range"), ([-1], [2], "out of range"),
                              ([5], [4], "out of range"), ([T - 1, T + 5], [T - 1, T + 9], "out of range")):
        with pytest.raises(hip_lib.HipError, match="ig_orientation_support: segment list.*" + what):
            s.ctx.orientation_support(8, np.array(first), np.array(last))
        with pytest.raises(hip_lib.HipError, match="segment list"):
            s.ctx.debug_orientation_support_time(8, np.array(first), np.array(last))
        ok()
    with pytest.raises(hip_lib.HipError, match="segment list"):
        s.ctx.orientation_support(8, np.arange(T + 1), np.arange(T + 1))  # more segments than positions
    with pytest.raises(hip_lib.HipError, match="segment list"):
        s.ctx.orientation_support(8, [1, 2], [3])
    ok()
    empty = s.ctx.orientation_support(8, np.zeros(0, np.int64), np.zeros(0, np.int64))  # no segment is no error
    assert empty["n_seg"] == 0 and empty["observed"].shape == (0, 4) and empty["counted"] == empty["within_segment"] == 0
    assert osup.observed_total(empty) == osup.observed_total(ref) and empty["uncounted"] == ref["uncounted"] + ref["counted"] + ref["within_segment"]
    # NULL outputs: nothing is written
    lib = hip_lib.lib()
    f32, l32 = f.astype(np.int32), l.astype(np.int32)
    geo = np.full((n_seg, 4), -7, np.int32)
    obs, exq, sc = np.full((n_seg, 4), -7, np.int64), np.full((n_seg, 2), -7, np.int64), np.full(8, -7, np.int64)
    n = C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    null = C.c_void_p(0)
    head = (s.ctx._h, C.c_int32(8), C.c_int32(1), C.c_int32(n_seg))
    for args in ((p(f32), p(l32), null, p(obs), p(exq), p(sc), C.byref(n)), (p(f32), p(l32), p(geo), null, p(exq), p(sc), C.byref(n)),
                 (p(f32), p(l32), p(geo), p(obs), null, p(sc), C.byref(n)), (p(f32), p(l32), p(geo), p(obs), p(exq), null, C.byref(n)),
                 (p(f32), p(l32), p(geo), p(obs), p(exq), p(sc), null), (null, p(l32), p(geo), p(obs), p(exq), p(sc), C.byref(n)),
                 (p(f32), null, p(geo), p(obs), p(exq), p(sc), C.byref(n))):
        assert lib.ig_orientation_support(*head, *args) != 0 and b"NULL" in lib.ig_last_error()
        assert all(np.all(x == -7) for x in (geo, obs, exq, sc)) and n.value == -7
    # model == 0: expected_q may be NULL
    assert lib.ig_orientation_support(s.ctx._h, C.c_int32(8), C.c_int32(0), C.c_int32(n_seg), p(f32), p(l32), p(geo), p(obs), null, p(sc), C.byref(n)) == 0
    assert np.array_equal(obs, ref["observed"]) and np.array_equal(geo, ref["geometry"]) and n.value == T and np.all(exq == -7)
    # a parameter set whose values times the pairs of a window could overflow the 64-bit sum: refused, not wrapped
    vals = [np.float32(s.param_simu[k][0]) for k in PARAM_NAMES]
    huge = list(vals)
    huge[PARAM_NAMES.index("fact")] = np.float32(vals[PARAM_NAMES.index("fact")] * 1e12)
    s.ctx.set_params(huge, s.mean_kb(), 0)
    with pytest.raises(hip_lib.HipError, match="model value too large for this window"):
        s.ctx.orientation_support(1024, f, l)
    assert s.ctx.orientation_support(1024, f, l, model=False)["expected_q"] is None  # (without the model pass there is nothing to guard)
    s.ctx.set_params(vals, s.mean_kb(), 0)
    ok()
    # no contacts uploaded
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="ig_orientation_support.*contacts"):
        bare.orientation_support(8, f, l)
    bare.close()
    # between ig_nuis_begin and ig_nuis_end the call refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_orientation_support.*in flight"):
        s.ctx.orientation_support(8, f, l)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_orientation_support_time(8, f, l)
    s.ctx.nuis_end()
    assert s.ctx.orientation_support(8, *[_levels(s, prob)["bin"][k] for k in ("first", "last")])["n_placed"] == T
    s.free_gpu()


def test_a_chain_in_flight_refuses():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny", seed=21)
    lists = _levels(s, prob)
    f, l = lists["bin"]["first"], lists["bin"]["last"]
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    frags = np.arange(8, dtype=np.int32)
    cands = np.array([[(x + 7 + 3 * q) % prob.n_frags for q in range(3)] for x in frags], np.int32)
    mean_kb = s.mean_kb()
    s.ctx.nuis_run_begin(frags, cands)
    s.ctx.nuis_step_begin(0, p8, mean_kb)
    s.ctx.nuis_step_next(1e6, float("inf"), None, None, mean_kb, True)  # (rejected: no finite ratio reaches u = inf)
    s.ctx.nuis_chain_begin(1, np.tile(p8, (2, 1)), np.full(2, np.inf), np.full(2, 1e6), mean_kb)
    with pytest.raises(hip_lib.HipError, match="ig_orientation_support: a chain is in flight"):
        s.ctx.orientation_support(8, f, l)
    with pytest.raises(hip_lib.HipError, match="a chain is in flight"):
        s.ctx.debug_orientation_support_time(8, f, l)
    s.ctx.nuis_chain_end()
    lists = _levels(s, prob)
    assert s.ctx.orientation_support(8, lists["bin"]["first"], lists["bin"]["last"])["n_seg"] == lists["bin"]["first"].size
    s.free_gpu()


def test_the_report_disturbs_nothing():
    outs = []
    for with_report in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_report:
            bins = s.orientation_support()
            blocks = s.orientation_support(level="block", window=64)
            assert bins["window"] == 8 and bins["n_judged"] > 0 and bins["observed"].sum() > 0 and blocks["n_seg"] < bins["n_seg"]
            s.orientation_support(level="bin", window_kb=20.0, model=False)
            s.inverted_segments(5)
            for which, forms in (("observed", ("atomic", "combined")), ("model", ("default", "wave", "workgroup"))):
                for form in forms:
                    s.ctx.debug_orientation_support_time(64, blocks["first"], blocks["last"], which=which, form=form, n=2)
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


def test_run_instagraal_save_orientations_writes_one_file_and_changes_nothing_else(tmp_path):
    from instagraal_amd import orientation_support as osup, synth
    from instagraal_amd.simulation import run_instagraal

    outs = []
    for k, flag in enumerate((True, False)):
        data = str(tmp_path / ("data%d" % k))  # (a folder of its own: a run leaves its pyramid in it)
        synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
        np.random.seed(17)
        p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / ("out%d" % k)), level=2, cycles=1, bomb=True, save_orientations=flag)
        folder = p2.simulation.output_folder
        s = p2.simulation.sampler
        sums, ints = s.ctx.debug_globals()
        outs.append((s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(), np.random.get_state()[1].copy(), np.random.get_state()[2],
                     [int(x) for x in s.ctx.valid_insert()], open(os.path.join(folder, "save_simu_step_0.txt")).read()))
        names = [x for x in os.listdir(folder) if x.startswith("orientations")]
        if flag:
            assert names == ["orientations.txt"]
            upper = s.sparse_matrix.tocoo()
            total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
            lines = open(os.path.join(folder, "orientations.txt")).read().splitlines()
            titles = [ln for ln in lines if ln.startswith("# level=")]
            assert titles == ["# level=block", "# level=bin"] and lines[0] == titles[0] and lines[1][2:].split() == list(osup.COLUMNS)
            tails = [dict(kv.split("=") for kv in ln[2:].split()) for ln in lines if ln.startswith("# window=")]
            assert len(tails) == 2 and lines[-1].startswith("# window=8 ")
            blocks, bins = (s.orientation_support(level=lv) for lv in ("block", "bin"))
            for tail, res in zip(tails, (blocks, bins)):
                assert sum(int(tail[c]) for c in osup.CLASS_SCALARS) == total and int(tail["n_seg"]) == res["n_seg"] and int(tail["n_judged"]) == res["n_judged"]
            rows = [ln.split() for ln in lines if not ln.startswith("#")]
            assert len(rows) == blocks["n_judged"] + bins["n_judged"] > 0 and all(len(r) == len(osup.COLUMNS) for r in rows)
            for r, k_seg in zip(rows[:blocks["n_judged"]], np.nonzero(blocks["status"] == 0)[0].tolist()):
                assert int(r[0]) == k_seg and [int(x) for x in r[10:14]] == blocks["observed"][k_seg].tolist() and int(r[3]) == blocks["first_bin"][k_seg]
        else:
            assert names == []
        p2.simulation.release()
    a, b = outs
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[5] == b[5] and a[6] == b[6]
