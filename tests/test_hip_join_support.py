"""GPU tests of the join support (ig_join_support_build, sampler.join_support) against the rule's host statement
(instagraal_amd.join_support.support_host: every contact tried against the four pairs of ends, every pair of every link laid out) on
the tables, the state and the genome order downloaded from the same handle, with the model's quantised values from the oracle in
DET mode.  Every comparison is exact integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("matrix_tiny_plain", "matrix_tiny_bomb")
ARRAYS = ("rowptr", "col", "observed", "pairs", "expected_q")
# 64 +- 1 as the junction profile's tests; 10, 11, 12: a full window of 11 positions has JOIN_WAVE_PAIRS = 66 pairs, the last link a
# thread sums in the model pass; the full window of 12 (78 pairs) is the first a wave does (tests/test_join_support_host.py checks that
# the fresh `small` has links of exactly 55, 66 and 78 pairs and none in between)
WINDOWS = (1, 10, 11, 12, 63, 64, 65, 1024)
WAVE_PAIRS = 66


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


def _host_inputs(ctx, prob):
    """what support_host takes, from ig_debug_tables, download_state and contact_map_order of the handle"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, rank, ln = ctx.debug_tables()
    state = ctx.download_state()
    col = {k: state[i] for i, k in enumerate(FRAG_FIELDS)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bad = np.unique(col["id_c"][col["activ"] != 1])
    placed = ~np.isin(col["id_c"][parent], bad)
    order = ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return dist, stot, contig, placed, position, col["l_cont_bp"].astype(np.int64)[parent]


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


def _device(ctx, window, model=True, release=True):
    """build + fetch (+ release) -> the result as the rule's dict"""
    res = ctx.join_support(window, model=model)
    res["col"], res["observed"], res["pairs"], res["expected_q"] = ctx.join_support_fetch(0, res["n_links"], model=model)
    if release:
        ctx.join_support_release()
    return res


def _assert_equal(got, want, what, arrays=ARRAYS):
    from instagraal_amd import join_support as js

    for k in arrays + ("first_position", "n_positions"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    for k in js.SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def _assert_device_equals_rule(s, prob, oracle_lib, what, windows=WINDOWS, want=()):
    from instagraal_amd import join_support as js

    t = _host_inputs(s.ctx, prob)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    q = _model_q(oracle_lib, s)
    forms = set()
    for w in windows:
        rule = js.support_host(*t, prob.coo_row, prob.coo_col, prob.coo_cnt, w, model_q=q)
        got = _device(s.ctx, w)
        _assert_equal(got, rule, (what, w))
        assert js.observed_total(got) == total and int(got["observed"].sum()) == got["contributions"], (what, w)
        assert got["n_links"] == got["col"].size and got["rowptr"].size == 2 * got["n_contigs"] + 1
        if got["n_links"]:
            assert got["expected_q"].min() > 0 and got["pairs"].min() >= 1 and got["pairs"].max() <= w * (w + 1) // 2
            forms |= {"thread"} if got["pairs"].min() <= WAVE_PAIRS else set()
            forms |= {"wave"} if got["pairs"].max() > WAVE_PAIRS else set()
        lean = _device(s.ctx, w, model=False)  # the model pass skipped: the observed part is the same
        assert lean["pairs"] is None and lean["expected_q"] is None
        _assert_equal(lean, rule, (what, w, "no model"), arrays=ARRAYS[:3])
        for k in want:  # (a window of one position links two end sub-fragments only: whether a moved state has such a contact is left open)
            assert got[k] > 0 or (w == 1 and k == "in_reach_observed"), (what, w, k)
    return forms


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_rule_on_the_fixture_states(name, oracle_lib):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, s = _sampler(str(g["config"]), seed=11)
    s.ctx.upload_state(g["state"])
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    forms = _assert_device_equals_rule(s, prob, oracle_lib, name, want=("in_reach_observed",))
    assert "thread" in forms and (name.endswith("bomb") or "wave" in forms)
    s.free_gpu()


def test_device_equals_the_rule_on_small_fresh(oracle_lib):
    prob, s = _sampler("small", seed=12)
    assert _assert_device_equals_rule(s, prob, oracle_lib, "small fresh", want=("in_reach_observed", "cis_observed")) == {"thread", "wave"}
    got = _device(s.ctx, 11)
    assert got["pairs"].max() == WAVE_PAIRS and _device(s.ctx, 12)["pairs"].max() == 78  # the threshold of the model's forms, from both sides
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_moves(oracle_lib):
    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    assert _assert_device_equals_rule(s, prob, oracle_lib, "small after batch moves", want=("in_reach_observed",)) == {"thread", "wave"}
    s.free_gpu()


def test_device_equals_the_rule_on_small_after_the_bomb(oracle_lib):
    """contigs of one bin: every window beyond a few positions is longer than every pair of contigs"""
    prob, s = _sampler("small", seed=12)
    s.bomb_the_genome()
    _assert_device_equals_rule(s, prob, oracle_lib, "small after the bomb", want=("in_reach_observed",))
    got = _device(s.ctx, 1024)
    assert got["n_contigs"] == prob.n_frags and got["out_of_reach_observed"] == 0 and got["contributions"] == 4 * got["in_reach_observed"]
    assert got["cis_observed"] > 0 and got["pairs"].max() <= WAVE_PAIRS
    s.free_gpu()


def _first_and_last_of_a_contig(prob, min_frags=3):
    S = prob.S_o_A_frags
    ids, cnt = np.unique(S["id_c"], return_counts=True)
    c = ids[np.argmax(cnt >= min_frags)]
    fr = np.nonzero(S["id_c"] == c)[0]
    return int(fr[np.argmin(S["pos"][fr])]), int(fr[np.argmax(S["pos"][fr])])


def test_a_state_with_a_ring(oracle_lib):
    """operator 10 forced on the first and the last bin of one contig closes it on itself: its contacts are ``ring``, it has no ends"""
    prob, s = _sampler("small", seed=13)
    fresh = _device(s.ctx, 64)
    first, last = _first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3 and s.ctx.debug_tables()[2].any()
    _assert_device_equals_rule(s, prob, oracle_lib, "small with a ring", windows=(1, 64, 1024), want=("ring_observed", "in_reach_observed"))
    assert _device(s.ctx, 64)["n_contigs"] == fresh["n_contigs"] - 1
    s.free_gpu()


def test_a_state_with_an_unplaced_contig(oracle_lib):
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("small", seed=14)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:100], 5)
    before = _device(s.ctx, 64)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    members = np.nonzero(id_c == ids[np.argmax(n >= 3)])[0]
    s.ctx.debug_set_bin_active(members[1], False)
    _assert_device_equals_rule(s, prob, oracle_lib, "small with an unplaced contig", windows=(1, 64, 1024), want=("unplaced_observed", "in_reach_observed"))
    assert _device(s.ctx, 64)["n_contigs"] == before["n_contigs"] - 1
    s.ctx.debug_set_bin_active(members[1], True)
    _assert_equal(_device(s.ctx, 64), before, "the contig placed again")
    s.free_gpu()


def test_with_full_windows_of_1024(oracle_lib):
    """contigs of thousands of sub-fragments: a link of 1024 * 1025 / 2 pairs, a wave per link"""
    prob, s = _sampler("bigctg", seed=12)
    _assert_device_equals_rule(s, prob, oracle_lib, "bigctg", windows=(1024,), want=("in_reach_observed", "out_of_reach_observed"))
    assert _device(s.ctx, 1024)["pairs"].max() == 1024 * 1025 // 2
    s.free_gpu()


def _checksum(res):
    words = res["rowptr"].tolist()
    for c, o in zip(res["col"].tolist(), res["observed"].tolist()):
        words += [c, o]
    tot = sum(int(v) * (k + 1) for k, v in enumerate(words)) % (1 << 64)
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def test_both_emit_forms_agree():
    from instagraal_amd import hip_lib

    prob, s = _sampler("small", seed=15)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200], 5)
    for w in (1, 64, 1024):
        want = _device(s.ctx, w)
        sums = []
        for combine in (True, False, None):
            s.ctx.debug_join_support_combine(combine)
            ms, ck = s.ctx.debug_join_support_time(w, n=1)
            assert ms.shape == (1, len(hip_lib.JOIN_SUPPORT_PASSES)) and (ms[0, :4] > 0).all() and ms[0, 7] > 0 and ms[0, 8] > 0
            sums.append(ck)
            _assert_equal(_device(s.ctx, w), want, (w, combine))
        assert sums[0] == sums[1] == sums[2] == _checksum(want), w
    s.free_gpu()


def test_every_sort_form_and_the_reduction_are_reached(oracle_lib):
    """the limits of ig_debug_assembly_contacts_limits reach this feature's sorts: a tiny problem goes through all three forms, and
    the rows each form took are the ones the rule's entries per row say"""
    from instagraal_amd import join_support as js

    prob, s = _sampler("tiny", seed=16)
    s.bomb_the_genome()  # 600 ends: rows of a few entries up to a few hundred
    t = _host_inputs(s.ctx, prob)
    q = _model_q(oracle_lib, s)
    used = {k: 0 for k in ("short", "lds", "long")}
    for w in (1, 64):
        want = js.support_host(*t, prob.coo_row, prob.coo_col, prob.coo_cnt, w, model_q=q)
        n = want["row_entries"]
        assert int(n.sum()) == want["entries"] and (want["entries"] > want["n_links"]) == (w == 64)  # at 64 the reduction has equal columns to sum
        for limits in ((0, 0), (2, 4), (1, 1)):
            short_max, lds_max = limits if limits != (0, 0) else (64, 1024)
            s.ctx.debug_assembly_contacts_limits(*limits)
            for combine in (False, True):
                s.ctx.debug_join_support_combine(combine)
                _assert_equal(_device(s.ctx, w, release=False), want, (w, limits, combine))
                forms = s.ctx.debug_join_support_forms()
                rows = dict(short=(n >= 2) & (n <= short_max), lds=(n >= 2) & (n > short_max) & (n <= lds_max), long=(n >= 2) & (n > short_max) & (n > lds_max))
                for k in used:
                    assert forms[k] == (int(rows[k].sum()), int(n[rows[k]].sum())), (w, limits, k, forms)
                    used[k] += forms[k][0]
                assert forms["longest"] == (int(n[rows["long"]].max()) if rows["long"].any() else 0)
                if limits == (1, 1):
                    assert forms["short"][0] == forms["lds"][0] == 0 and forms["long"][0] > 0 and forms["runs"] == 0
                if limits == (2, 4):
                    assert forms["long"][0] > 0 and forms["runs"] == int(((n[rows["long"]] + 3) // 4).sum()) > forms["long"][0]
                if limits == (0, 0) and w == 64:
                    assert forms["short"][0] > 0 and forms["lds"][0] > 0 and forms["long"][0] == 0
                if limits == (2, 4) and w == 1:
                    assert forms["short"][0] > 0 and forms["lds"][0] > 0
    assert all(v > 0 for v in used.values()), used
    s.ctx.debug_assembly_contacts_limits(0, 0)
    s.ctx.debug_join_support_combine(None)
    lifted = s.ctx.assembly_contacts("bin")  # the lift still sorts under its own name
    assert lifted["entries_out"] > 0 and sum(s.ctx.debug_assembly_contacts_forms()[k][0] for k in used) > 0
    s.ctx.assembly_contacts_release()
    s.free_gpu()


def test_observed_against_the_lift_as_an_independent_device_path():
    """``observed`` recomputed on the host from the contacts in genome coordinates (ig_assembly_contacts_build, level "sub") of the
    same handle: positions instead of sub-fragments, nothing shared with the emit pass but the contacts"""
    from instagraal_amd import assembly_contacts as ac, join_support as js

    prob, s = _sampler("small", seed=17)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    lift = s.ctx.assembly_contacts("sub")
    pb, cnt = s.ctx.assembly_contacts_fetch(0, lift["n_entries"])
    s.ctx.assembly_contacts_release()
    pa, pb = ac.rows_of(lift["rowptr"]), pb.astype(np.int64)
    for w in (1, 64, 1024):
        got = _device(s.ctx, w)
        start, n = got["first_position"].astype(np.int64), got["n_positions"].astype(np.int64)
        K = start.size

        def run_of(p):
            k = np.searchsorted(start, p, side="right") - 1
            return np.where((k >= 0) & (p < start[np.maximum(k, 0)] + n[np.maximum(k, 0)]), k, -1)

        ka, kb = run_of(pa), run_of(pb)
        trans = (ka >= 0) & (kb >= 0) & (ka != kb)
        a, b, ca, cb, c = pa[trans], pb[trans], ka[trans], kb[trans], cnt[trans]
        sums = {}
        for sa in (0, 1):
            for sb in (0, 1):
                da = a - start[ca] if sa == 0 else start[ca] + n[ca] - 1 - a
                db = b - start[cb] if sb == 0 else start[cb] + n[cb] - 1 - b
                ok = da + db + 1 <= w
                ea, eb = 2 * ca[ok] + sa, 2 * cb[ok] + sb
                for key, v in zip((np.minimum(ea, eb) * 2 * K + np.maximum(ea, eb)).tolist(), c[ok].tolist()):
                    sums[key] = sums.get(key, 0) + v
        keys = (js.rows_of(got["rowptr"]) * 2 * K + got["col"]).tolist()
        assert keys == sorted(sums) and got["observed"].tolist() == [sums[k] for k in keys] and len(keys) > 0, w
    s.free_gpu()


def test_two_builds_agree_fetches_in_pieces_and_the_snapshot():
    from instagraal_amd import hip_lib

    prob, s = _sampler("small", seed=18)
    s.bomb_the_genome()  # (more than 997 links)
    a = _device(s.ctx, 64)
    b = _device(s.ctx, 64, release=False)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ARRAYS) and a["n_links"] > 2000
    n = a["n_links"]
    for step in (997, 1):
        span = range(0, n, step) if step > 1 else list(range(0, 300)) + list(range(n - 300, n))  # (one by one: the first and the last 300)
        parts = [s.ctx.join_support_fetch(o, min(step, n - o)) for o in span]
        want = a if step > 1 else {k: np.concatenate([a[k][:300], a[k][n - 300:]]) for k in ARRAYS[1:]}
        for i, k in enumerate(ARRAYS[1:]):
            assert np.array_equal(np.concatenate([p[i] for p in parts]), want[k]), (step, k)
    assert s.ctx.join_support_fetch(n, 0)[0].size == 0
    before = s.ctx.contact_map_order()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:50], 5)
    assert not np.array_equal(s.ctx.contact_map_order(), before)  # the genome moved on, the snapshot did not
    got = s.ctx.join_support_fetch(0, n)
    assert all(np.array_equal(got[i], a[k]) for i, k in enumerate(ARRAYS[1:]))
    rows = np.zeros(a["rowptr"].size, np.int64)
    assert hip_lib.lib().ig_join_support_rows(s.ctx._h, C.c_void_p(rows.ctypes.data), C.c_int64(rows.size)) == 0 and np.array_equal(rows, a["rowptr"])
    s.ctx.join_support_release()
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        s.ctx.join_support_fetch(0, 1)
    s.ctx.join_support_release()  # (twice is fine)
    assert _device(s.ctx, 64)["n_contigs"] < a["n_contigs"]  # (the moves joined bins)
    s.free_gpu()


def test_the_shards_merge_to_the_whole():
    from instagraal_amd import join_support as js, synth
    from instagraal_amd.sampler import problem_to_context

    prob = synth.make_problem(*synth.CONFIGS["small"])
    whole = problem_to_context(prob)
    shards = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        shards.append(ctx)
    for w in (1, 64):
        want = _device(whole, w)
        parts = [_device(ctx, w) for ctx in shards]
        assert all(p["n_links"] > 0 for p in parts)
        merged = js.merge_shards(parts)
        _assert_equal(merged, want, ("merged", w))
        for k in js.SUMMED_SCALARS:
            assert parts[0][k] + parts[1][k] == want[k], (w, k)
    for ctx in shards + [whole]:
        ctx.close()


def test_the_builds_disturb_nothing():
    outs = []
    for with_build in (False, True):
        prob, s = _sampler("small", seed=3)
        frags = np.random.permutation(prob.n_frags)[:200]
        res = [s.step_sampler_batch(frags[:100], 5)]
        if with_build:
            assert _device(s.ctx, 64, release=False)["n_links"] > 0  # (the snapshot stays on the device through the moves below)
            ms, _ = s.ctx.debug_join_support_time(1024, n=2)
            assert ms.shape == (2, 9)
            assert s.join_support(window_kb=20.0)["observed"].sum() > 0 and s.best_joins(5).size > 0
            _device(s.ctx, 8, model=False, release=False)
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


def test_errors_are_loud_and_leave_the_context_usable():
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, soa17_from_dict

    prob, s = _sampler("tiny")
    with pytest.raises(hip_lib.HipError, match="nothing is built"):  # a fetch before any build
        s.ctx.join_support_fetch(0, 1)
    ref = _device(s.ctx, 64)

    def ok():
        _assert_equal(_device(s.ctx, 64, release=False), ref, "again")

    ok()
    for bad in (0, 1025, -1):
        with pytest.raises(hip_lib.HipError, match="ig_join_support_build.*window"):
            s.ctx.join_support(bad)
        with pytest.raises(hip_lib.HipError, match="nothing is built"):  # (a failed build leaves no stale result)
            s.ctx.join_support_fetch(0, 1)
        with pytest.raises(hip_lib.HipError, match="window"):
            s.ctx.debug_join_support_time(bad)
        ok()
    n = ref["n_links"]
    for first, count in ((n, 1), (-1, 1), (0, n + 1), (0, -1), (n + 1, 0)):
        with pytest.raises(hip_lib.HipError, match="out of range"):
            s.ctx.join_support_fetch(first, count)
    lib = hip_lib.lib()
    K = ref["n_contigs"]
    rows, first, npos = np.full(2 * K + 1, -7, np.int64), np.full(K, -7, np.int32), np.full(K, -7, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.ig_join_support_rows(s.ctx._h, p(rows), C.c_int64(2 * K)) != 0 and b"capacity" in lib.ig_last_error() and np.all(rows == -7)
    assert lib.ig_join_support_ends(s.ctx._h, p(first), p(npos), C.c_int64(K - 1)) != 0 and b"capacity" in lib.ig_last_error()
    assert np.all(first == -7) and np.all(npos == -7)
    assert lib.ig_join_support_rows(s.ctx._h, C.c_void_p(0), C.c_int64(2 * K + 1)) != 0 and b"NULL" in lib.ig_last_error()
    assert lib.ig_join_support_rows(s.ctx._h, p(rows), C.c_int64(2 * K + 1)) == 0 and np.array_equal(rows, ref["rowptr"])
    assert lib.ig_join_support_ends(s.ctx._h, p(first), p(npos), C.c_int64(K)) == 0 and np.array_equal(first, ref["first_position"])
    sc = np.full(8, -7, np.int64)
    ne = C.c_int64(-7)
    assert lib.ig_join_support_build(s.ctx._h, C.c_int32(64), C.c_int32(1), C.byref(ne), C.c_void_p(0), p(sc)) != 0 and b"NULL" in lib.ig_last_error()
    assert np.all(sc == -7) and ne.value == -7
    ok()
    # a result built without the model has no model part to fetch
    s.ctx.join_support(64, model=False)
    with pytest.raises(hip_lib.HipError, match="model = 0"):
        s.ctx.join_support_fetch(0, 1, model=True)
    assert np.array_equal(s.ctx.join_support_fetch(0, n, model=False)[1], ref["observed"])
    # a parameter set whose values times the pairs of a window could overflow the 64-bit sum: refused, not wrapped
    vals = [np.float32(s.param_simu[k][0]) for k in PARAM_NAMES]
    huge = list(vals)
    huge[PARAM_NAMES.index("fact")] = np.float32(vals[PARAM_NAMES.index("fact")] * 1e12)
    s.ctx.set_params(huge, s.mean_kb(), 0)
    with pytest.raises(hip_lib.HipError, match="model value too large for this window"):
        s.ctx.join_support(1024)
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        s.ctx.join_support_fetch(0, 1)
    assert s.ctx.join_support(1024, model=False)["n_links"] > 0  # (without the model pass there is nothing to guard)
    s.ctx.set_params(vals, s.mean_kb(), 0)
    ok()
    # between ig_nuis_begin and ig_nuis_end the build refuses, and the step ends as if nothing had happened
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    with pytest.raises(hip_lib.HipError, match="ig_join_support_build.*in flight"):
        s.ctx.join_support(64)
    with pytest.raises(hip_lib.HipError, match="in flight"):
        s.ctx.debug_join_support_time(64)
    s.ctx.nuis_end()
    ok()
    s.free_gpu()
    # before the contacts are uploaded, before a state; a new upload releases the result
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    with pytest.raises(hip_lib.HipError, match="contacts"):
        bare.join_support(64)
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    with pytest.raises(hip_lib.HipError, match="state"):
        bare.join_support(64)
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    with pytest.raises(hip_lib.HipError, match="parameters"):
        bare.join_support(64)
    _assert_equal(_device(bare, 64, model=False, release=False), ref, "bare", arrays=ARRAYS[:3])
    bare.upload_contacts(prob.coo_row, prob.coo_col, prob.coo_cnt, prob.n_sub_frags)
    with pytest.raises(hip_lib.HipError, match="nothing is built"):
        bare.join_support_fetch(0, 1, model=False)
    bare.close()


def test_nothing_placed_no_contacts_and_one_contig():
    """T == 0, Z == 0 and K < 2: an all-zero rowptr and success"""
    from instagraal_amd import hip_lib, join_support as js, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, problem_to_context, soa17_from_dict

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    ctx = problem_to_context(prob)
    for f in range(prob.n_frags):  # nothing placed: a bin of every contig is inactive
        ctx.debug_set_bin_active(f, False)
    got = _device(ctx, 64)
    assert got["n_contigs"] == 0 and got["rowptr"].tolist() == [0] and got["n_links"] == 0 and got["unplaced_observed"] == int(prob.coo_cnt.astype(np.int64).sum())
    S = prob.S_o_A_frags
    keep = np.unique(S["id_c"])[0]
    for f in np.nonzero(S["id_c"] == keep)[0]:  # one contig placed: it has two ends and nothing to link them to
        ctx.debug_set_bin_active(int(f), True)
    got = _device(ctx, 1024)
    assert got["n_contigs"] == 1 and got["rowptr"].tolist() == [0, 0, 0] and got["n_links"] == 0 and got["cis_observed"] > 0
    ctx.close()
    shard = problem_to_context(prob)  # an empty shard: no row i with i % world == rank
    shard.set_shard(prob.n_sub_frags + 6, prob.n_sub_frags + 7)
    got = _device(shard, 64)
    assert got["n_contigs"] == 6 and not got["rowptr"].any() and got["rowptr"].size == 13 and got["n_links"] == 0 and all(got[k] == 0 for k in js.SUMMED_SCALARS)
    shard.close()
    none = np.zeros(0, np.int32)  # no contacts at all
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    got = _device(bare, 64, model=False)
    assert got["n_contigs"] == 6 and not got["rowptr"].any() and got["n_links"] == 0 and all(got[k] == 0 for k in js.SUMMED_SCALARS)
    bare.close()


def test_sampler_join_support_and_best_joins():
    from instagraal_amd import join_support as js

    prob, s = _sampler("small", seed=6)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    res = s.join_support()
    raw = _device(s.ctx, js.DEFAULT_WINDOW)
    assert res["window"] == 64
    _assert_equal(res, raw, "sampler")
    assert np.array_equal(res["expected"], raw["expected_q"] / 2.0 ** 32) and np.array_equal(res["ratio"], raw["observed"] / res["expected"])
    ends, order = res["ends"], res["order"]
    K = res["n_contigs"]
    assert ends.size == 2 * K and np.array_equal(order, s.ctx.contact_map_order())
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    g = s.gpu_vect_frags.copy_from_gpu()
    assert np.array_equal(ends["sub_frag"][0::2], order[res["first_position"]]) and np.array_equal(ends["sub_frag"][1::2], order[res["first_position"] + res["n_positions"] - 1])
    assert np.array_equal(ends["bin"], parent[ends["sub_frag"]]) and np.array_equal(ends["scaffold"], g.id_c[ends["bin"]])
    assert np.array_equal(ends["scaffold"][0::2], ends["scaffold"][1::2]) and np.unique(ends["scaffold"]).size == K
    assert np.array_equal(ends["length_bp"], g.l_cont_bp[ends["bin"]]) and np.array_equal(ends["n_positions"], np.repeat(res["n_positions"], 2))
    kb = s.join_support(window_kb=16.0)
    assert kb["window"] == js.window_from_kb(16.0, s.mean_kb())
    with pytest.raises(ValueError):
        s.join_support(window=8, window_kb=16.0)
    best = s.best_joins(5, window=8)
    assert 0 < best.size <= 5 and np.all(np.diff(best["ratio"]) <= 0) and np.all(best["pairs"] >= js.default_min_pairs(8))
    assert np.array_equal(best, js.best_joins(s.join_support(8), 5))
    assert s.best_joins(3, min_pairs=10 ** 9, window=8).size == 0
    s.free_gpu()


def test_run_instagraal_save_joins_writes_one_file(tmp_path):
    from instagraal_amd import join_support as js, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=2, bomb=True, save_joins=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    assert [f for f in os.listdir(folder) if f.startswith("joins")] == ["joins.txt"]
    lines = open(os.path.join(folder, "joins.txt")).read().splitlines()
    assert lines[0][2:].split() == list(js.JOIN_COLUMNS)
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    sc = dict(kv.split("=") for kv in lines[-1][2:].split())
    res = s.join_support()
    assert len(rows) == int(sc["n_links"]) == res["n_links"] > 0 and int(sc["window"]) == 64
    upper = s.sparse_matrix.tocoo()
    total = int(upper.data[upper.row < upper.col].astype(np.int64).sum())  # what the device holds: the strict upper triangle
    assert sum(int(sc[k]) for k in js.OBSERVED_SCALARS) == total and sum(int(r[4]) for r in rows) == int(sc["contributions"])
    names = set(r[0] for r in rows) | set(r[2] for r in rows)
    fasta = set(ln[1:].split()[0] for ln in open(os.path.join(folder, "genome.fasta")) if ln.startswith(">"))
    assert names <= fasta and all(r[1] in js.SIDE_NAMES and r[3] in js.SIDE_NAMES for r in rows)
    p2.simulation.release()
    data2 = str(tmp_path / "data2")  # (a folder of its own: the first run left its pyramid in the other)
    synth.write_text_dataset(data2, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p3 = run_instagraal(data2, os.path.join(data2, "genome.fa"), output_folder=str(tmp_path / "out2"), level=2, cycles=1, bomb=True)
    assert not [f for f in os.listdir(p3.simulation.output_folder) if f.startswith("joins")]
    p3.simulation.release()
