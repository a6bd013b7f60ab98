"""GPU tests of the reports on the current genome and of the scorer at contact counts up to 2^31 - 1 (the problems of
tests/_large_counts.py; tests/test_large_counts_host.py proves on the host that they fill whole waves with one destination and holds
every rule against Python integers).

* the contact map, the junction profile and the orientation support pick the `int` or the `long long` form of their segmented wave
  scan by the largest count of the upload (2^25): every family of counts through both sides of that threshold, against the rules,
  in both forms of the pass, sharded, and behind batch moves;
* the other reports (distance law, join support, placement support, assembly contacts, balance) with every sum beyond 2^32, through
  the harness of their own test files;
* gap support: the second guard refuses `int_max` and writes nothing; the largest counts it admits are held to the rule;
* the scorer across 2^24, where the slice entries change from the packed 8-byte form (24-bit counts) to the 12-byte one.

Every comparison is exact integer (or byte) equality."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import _large_counts as lc
from conftest import ROOT

pytestmark = pytest.mark.gpu

W_RUN = 256  # the window at which a dense row's 192 contacts are all in window
SCAN_FAMILIES = ("base", "narrow_max", "wide_min", "int_max", "one_wide")


@functools.lru_cache(maxsize=None)
def _prob(family):
    cfg = lc.smallest_config()
    assert lc.longest_contig(lc._synth(cfg))[1] >= 200 + 8
    return lc.make(cfg, family)


def _sampler_of(prob, seed=None):
    from instagraal_amd.sampler import sampler as hip_sampler

    if seed is not None:
        np.random.seed(seed)
    s = hip_sampler(**prob.sampler_kwargs(), device_id=0, coo=(prob.coo_row, prob.coo_col, prob.coo_cnt))
    s.set_param_simu(dict(prob.params))
    s.bins = np.arange(1.0, 60.0, 1.0)
    s.eval_likelihood_init()
    return s


def _total(prob):
    return sum(prob.coo_cnt.tolist())  # a Python int


def _position(ctx, prob):
    from instagraal_amd import assembly_contacts as ac

    return ac.positions_of(ctx.contact_map_order().astype(np.int64), prob.n_sub_frags)


def _py_sum(a):
    return sum(np.asarray(a).ravel().tolist())


def _signed64(x):
    x %= 1 << 64
    return x - (1 << 64) if x >= 1 << 63 else x


# ---- the three passes with a segmented wave scan


def _assert_map(s, prob, what, fresh=True):
    position = _position(s.ctx, prob)
    T = int((position >= 0).sum())
    placed_total = sum(prob.coo_cnt[(position[prob.coo_row] >= 0) & (position[prob.coo_col] >= 0)].tolist())  # a Python int
    if fresh:
        assert T == prob.n_sub_frags and placed_total == _total(prob)
    for max_side in (1, 2, 37, T):
        want, b = lc.map_host(position, prob.coo_row, prob.coo_col, prob.coo_cnt, max_side)
        got, gb = s.ctx.contact_map(max_side)
        assert gb == b and got.dtype == np.int64 and np.array_equal(got, want), (what, max_side)
        assert _py_sum(got) == 2 * placed_total, (what, max_side)  # every placed contact, once for each of its ends
        _, sum_a = s.ctx.debug_contact_map_time(max_side, combine=True, n=1)
        _, sum_b = s.ctx.debug_contact_map_time(max_side, combine=False, n=1)
        assert sum_a == sum_b == _signed64(_py_sum(want)), (what, max_side)


def _assert_junctions(s, prob, oracle_lib, what, windows=(1, 64, W_RUN, 1024)):
    import test_hip_junction_profile as tj

    tj._assert_profile_equals_host(s, prob, oracle_lib, what, windows=windows)  # arrays, scalars, the identities, model=False
    for w in windows:
        prof = s.ctx.junction_profile(w)
        assert sum(prof[k] for k in ("in_window_observed", "beyond_window_observed", "trans_observed", "ring_observed", "unplaced_observed")) == _total(prob)
        _, _, _, ck_a = s.ctx.debug_junction_profile_time(w, combine=True, n=1)
        _, _, _, ck_b = s.ctx.debug_junction_profile_time(w, combine=False, n=1, model=False, scan=False)
        assert ck_a == ck_b == tj._checksum(prof), (what, w)


def _segment_lists(s, prob, fresh):
    import test_hip_orientation_support as to

    lists = dict(to._levels(s, prob))
    lists = {k: (v["first"], v["last"]) for k, v in lists.items()}
    if fresh:
        lists["custom"] = lc.dense_segments(prob)
    return lists


def _assert_orientations(s, prob, oracle_lib, what, fresh=True, windows=(8, W_RUN)):
    import test_hip_orientation_support as to
    from instagraal_amd import orientation_support as osup

    to._assert_equals_host(s, prob, oracle_lib, what, windows)  # bin and block: arrays, scalars, the identities, model=False
    lists = _segment_lists(s, prob, fresh)
    if fresh:
        got = to._assert_equals_host(s, prob, oracle_lib, what + ", the dense rows' segments", (8, lc.DENSE_LEN - 1, lc.DENSE_LEN, W_RUN), segments=lists["custom"])
        assert got["window"] == W_RUN and (got["status"] == 0).all()
        rows = lc.dense_rows(prob)
        dense = np.isin(prob.coo_row, rows) & (prob.coo_col - prob.coo_row <= lc.DENSE_LEN)
        if int(dense.sum()) == lc.N_DENSE * lc.DENSE_LEN:  # at a window that holds the whole row the 192 counts of a dense row are its segment's RR
            assert np.all(got["observed"][:, osup.RR] >= lc.DENSE_LEN * int(prob.coo_cnt[dense].min()))
    for name, (first, last) in lists.items():
        for w in windows:
            raw = s.ctx.orientation_support(w, first, last, model=False)
            assert sum(raw[k] for k in osup.CLASS_SCALARS) == _total(prob), (what, name, w)
            _, ck_a = s.ctx.debug_orientation_support_time(w, first, last, which="observed", form="combined", n=1)
            _, ck_b = s.ctx.debug_orientation_support_time(w, first, last, which="observed", form="atomic", n=1)
            assert ck_a == ck_b == to._checksum(raw), (what, name, w)


@pytest.mark.parametrize("family", SCAN_FAMILIES)
def test_map_junctions_and_orientations_on_the_fresh_genome(family, oracle_lib):
    prob = _prob(family)
    s = _sampler_of(prob, seed=21)
    assert np.array_equal(s.ctx.contact_map_order(), lc.fresh_order(prob))  # what the host's wave statistics assume
    _assert_map(s, prob, family)
    _assert_junctions(s, prob, oracle_lib, family)
    _assert_orientations(s, prob, oracle_lib, family)  # (`one_wide` has no dense rows: their segments are a custom list like any other)
    s.free_gpu()


@pytest.mark.parametrize("family", SCAN_FAMILIES)
def test_two_shards_add_up_to_the_whole(family):
    from instagraal_amd import junction_profile as jp, orientation_support as osup
    from instagraal_amd.sampler import problem_to_context

    prob = _prob(family)
    first, last = lc.dense_segments(_prob("base"))
    T = prob.n_sub_frags

    def reports(ctx):
        return ([ctx.contact_map(m)[0] for m in (1, 2, 37, T)], ctx.junction_profile(W_RUN, model=False), ctx.orientation_support(W_RUN, first, last, model=False))

    whole = problem_to_context(prob)
    want = reports(whole)
    whole.close()
    parts = []
    for rank in range(2):
        ctx = problem_to_context(prob)
        ctx.set_shard(rank, 2)
        parts.append(reports(ctx))
        ctx.close()
    for a, b, w in zip(parts[0][0], parts[1][0], want[0]):
        assert a.any() and b.any() and np.array_equal(a + b, w)
    assert np.array_equal(parts[0][1]["observed"] + parts[1][1]["observed"], want[1]["observed"])
    for k in jp.OBSERVED_SCALARS + ("spanned_observed",):
        assert parts[0][1][k] + parts[1][1][k] == want[1][k], k
    assert np.array_equal(parts[0][2]["observed"] + parts[1][2]["observed"], want[2]["observed"])
    for k in osup.SCALARS[:7]:
        assert parts[0][2][k] + parts[1][2][k] == want[2][k], k
    assert jp.observed_total(want[1]) == osup.observed_total(want[2]) == _total(prob)


def test_int_max_behind_200_batch_moves(oracle_lib):
    """the same three reports on a genome the sampler has worked on (no claim about the runs of equal destinations there)"""
    prob = _prob("int_max")
    s = _sampler_of(prob, seed=22)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:200].astype(np.int32), 5)
    assert np.any(np.diff(s.ctx.contact_map_order().astype(np.int64)) < 0)
    sums, _ = s.ctx.debug_globals()
    _, _, limbs = s.ctx.full_likelihood(0)
    assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]
    _assert_map(s, prob, "int_max moved", fresh=False)
    _assert_junctions(s, prob, oracle_lib, "int_max moved", windows=(64, W_RUN))
    _assert_orientations(s, prob, oracle_lib, "int_max moved", fresh=False)
    s.free_gpu()


# ---- the other reports


@pytest.fixture(scope="module", params=("narrow_max", "int_max"))
def big(request):
    prob = _prob(request.param)
    s = _sampler_of(prob, seed=23)
    yield request.param, prob, s
    s.free_gpu()


def test_distance_law(big):
    import test_hip_distance_law as tl

    family, prob, s = big
    tl._assert_law_equals_host(s, prob, family)
    for label, edges in tl._edge_sets(s, s.ctx.debug_tables()[0]).items():
        _, _, ck_a = s.ctx.debug_distance_law_time(edges, privatised=True, n=1)
        _, _, ck_b = s.ctx.debug_distance_law_time(edges, privatised=False, n=1, pairs=False)
        law = s.ctx.distance_law(edges)
        want = sum(v * (i + 1) for i, v in enumerate(law["observed"].tolist())) + sum(law[k] * (4096 + 1 + i) for i, k in enumerate(
            ("out_of_range_observed", None, "trans_observed", None, "ring_observed", None, "unplaced_observed")) if k)
        assert ck_a == ck_b == _signed64(want), (family, label)
        assert _py_sum(law["observed"]) + sum(law[k] for k in ("out_of_range_observed", "trans_observed", "ring_observed", "unplaced_observed")) == _total(prob)


def test_join_support(big, oracle_lib):
    import test_hip_join_support as tjs

    family, prob, s = big
    tjs._assert_device_equals_rule(s, prob, oracle_lib, family, windows=(1, 64, 1024), want=("in_reach_observed",))
    for combine in (False, True, None):
        s.ctx.debug_join_support_combine(combine)
        got = tjs._device(s.ctx, 1024)
        assert _py_sum(got["observed"]) == got["contributions"] and sum(got[k] for k in ("in_reach_observed", "out_of_reach_observed", "cis_observed", "ring_observed",
                                                                                         "unplaced_observed")) == _total(prob)
        if combine is False:
            first = got
        assert all(np.array_equal(got[k], first[k]) for k in tjs.ARRAYS)
    if family == "int_max":
        assert got["observed"].max() > 2 ** 32


def test_placement_support(big):
    import test_hip_placement_support as tp

    family, prob, s = big
    out = tp._assert_device_equals_rule(s, prob, family, windows=(64, 1024), forms=tp.FORMS, min_hosts=lambda w: (w,))
    if family == "int_max":
        assert max(int(v["best_left"].max()) + int(v["best_right"].max()) for v in out.values()) > 2 ** 32


def test_assembly_contacts(big):
    import test_hip_assembly_contacts as ta

    family, prob, s = big
    ta._assert_device_equals_rule(s, prob, family)
    if family == "int_max":
        got = ta._device(s.ctx, "bin")
        assert got["count"].max() > 2 ** 32 and _py_sum(got["count"]) == _total(prob)
        s.ctx.assembly_contacts_release()


def test_balance(big):
    import test_hip_balance as tb
    from instagraal_amd import balance as bal

    family, prob, s = big
    cache = {}
    for level, max_side in tb.UNITS:
        for d in (1, 2):
            want = tb._rule_rows(cache, s.ctx, prob, level, max_side, d)
            got = tb._device_rows(s.ctx, level, max_side, d)
            tb._assert_rows(got, want, (family, level, max_side, d))
            assert bal.observed_total(got) == _total(prob) and _py_sum(got["count"]) == 2 * got["kept_observed"] == _py_sum(got["total"])
    for level, max_side, d in (("bin", 2048, 2), ("map", 64, 2)):
        ent = tb._rule_rows(cache, s.ctx, prob, level, max_side, d)
        tb._assert_rows(tb._device_rows(s.ctx, level, max_side, d), ent, (family, level))
        if family == "int_max":
            assert ent["total"].max() > 2 ** 32
        b0 = np.where(bal.mask_units(ent["nnz"], ent["total"], 10), 0.0, 1.0)
        want = bal.iterate(ent["rowptr"], ent["col"], ent["count"], b0, 0.0, 5)
        assert want["n_iters"] == 5
        for form in tb.FORMS + ("default",):
            s.ctx.debug_balance_form(form)
            tb._assert_run(s.ctx.balance_run(b0, 0.0, 5), want, (family, level, form))
        s.ctx.debug_balance_form("default")
    s.ctx.balance_release()


# ---- gap support: the second guard


GAPS = np.array([0.0, 0.5, 3.0, 40.0, 1000.0], np.float32)


def _gap_inputs(s, prob):
    """what the rule takes in front of the contacts, downloaded once per state (it does not depend on the counts)"""
    import test_hip_gap_support as tg

    tables, order, parent, col = tg._host_inputs(s, prob)
    return tables, col["id_c"].astype(np.int64)[parent], tg._model(s)


def _gap_rule(inputs, prob, junctions, window, check=False):
    from instagraal_amd import gap_support as gs

    tables, canonical, model = inputs
    return gs.support_host(*tables, prob.coo_row, prob.coo_col, prob.coo_cnt, junctions, GAPS, window, model, want_expected=False, canonical=canonical,
                           check=check)


def test_gap_support_refuses_int_max_and_writes_nothing():
    import test_hip_gap_support as tg
    from instagraal_amd import gap_support as gs, hip_lib

    prob = _prob("int_max")
    s = _sampler_of(prob, seed=24)
    junc = np.asarray(tg._levels(s, prob)["bin"]["junction"], np.int64)
    inputs = _gap_inputs(s, prob)
    rule = _gap_rule(inputs, prob, junc, W_RUN)
    product = int(rule["observed"].max()) * rule["max_abs_log_q"]
    assert product >= 1 << 62 and not gs.log_sum_fits(int(rule["observed"].max()), rule["max_abs_log_q"])
    assert lc.INT_MAX * rule["max_abs_log_q"] >= 1 << 62  # (one such contact across a judged junction is enough)
    msg = "too many contacts across one junction for this model"
    with pytest.raises(hip_lib.HipError, match=msg):
        s.ctx.gap_support(W_RUN, junc, GAPS)
    with pytest.raises(hip_lib.HipError, match=msg):
        s.ctx.gap_support(W_RUN, junc, GAPS, model=False)
    with pytest.raises(hip_lib.HipError, match=msg):
        s.ctx.debug_gap_support_time(W_RUN, junc, GAPS, which="observed")
    with pytest.raises(ValueError, match=msg):
        _gap_rule(inputs, prob, junc, W_RUN, check=True)
    # the C entry: nothing is written
    j32 = np.ascontiguousarray(junc, np.int32)
    n_j, K = j32.size, GAPS.size
    status, geo = np.full(n_j, -7, np.int32), np.full((n_j, 4), -7, np.int32)
    obs, prs, lgq, exq, sc = (np.full(n, -7, np.int64) for n in (n_j, n_j, n_j * K, n_j * K, 8))
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = hip_lib.lib().ig_gap_support(s.ctx._h, C.c_int32(W_RUN), C.c_int32(1), C.c_int32(n_j), p(j32), C.c_int32(K), p(GAPS), p(status), p(geo), p(obs), p(prs), p(lgq),
                                      p(exq), p(sc))
    assert rc != 0 and msg.encode() in hip_lib.lib().ig_last_error()
    assert all(np.all(a == -7) for a in (status, geo, obs, prs, lgq, exq, sc))
    # the context still answers: at a window of one position, the junctions whose one contact is small
    one = _gap_rule(inputs, prob, junc, 1)
    quiet = junc[one["observed"] < 1000]
    assert 50 < quiet.size < junc.size
    want = _gap_rule(inputs, prob, quiet, 1, check=True)
    got = s.ctx.gap_support(1, quiet, GAPS)
    for k in ("status", "geometry", "observed", "pairs", "log_q"):
        assert np.array_equal(got[k], want[k]), k
    assert all(got[k] == want[k] for k in gs.SCALARS) and gs.observed_total(got) == _total(prob) and got["observed"].any()
    # ... and, behind an upload of the `base` counts on the same handle, the call it refused
    base = _prob("base")
    assert np.array_equal(base.coo_row, prob.coo_row) and np.array_equal(base.coo_col, prob.coo_col)
    s.ctx.upload_contacts(base.coo_row, base.coo_col, base.coo_cnt, base.n_sub_frags)
    want = _gap_rule(inputs, base, junc, W_RUN, check=True)
    for model in (True, False):
        got = s.ctx.gap_support(W_RUN, junc, GAPS, model=model)
        for k in ("status", "geometry", "observed", "pairs", "log_q"):
            assert np.array_equal(got[k], want[k]), (k, model)
        assert all(got[k] == want[k] for k in gs.SCALARS) and gs.observed_total(got) == _total(base) and got["observed"].max() > 100
    _, ck = s.ctx.debug_gap_support_time(W_RUN, junc, GAPS, which="observed")
    assert ck == tg._checksum(got)
    s.free_gpu()


def test_gap_support_at_the_largest_counts_the_guard_admits():
    """family `gap_max`: the dense rows at the largest power of two for which max_j observed[j] * max |l_q|, from the rule, stays
    below 2^62 -- found by halving from 2^25"""
    import test_hip_gap_support as tg
    from instagraal_amd import gap_support as gs

    base = _prob("base")
    s0 = _sampler_of(base, seed=25)
    junc = np.asarray(tg._levels(s0, base)["bin"]["junction"], np.int64)
    inputs = _gap_inputs(s0, base)
    s0.free_gpu()
    count, prob, rule = 2 ** 25, None, None
    while count >= 1:
        prob = lc.with_dense_count(base, count)
        rule = _gap_rule(inputs, prob, junc, W_RUN)
        if gs.log_sum_fits(int(rule["observed"].max()), rule["max_abs_log_q"]):
            break
        count //= 2
    print("gap_max: dense rows at 2^%d, max observed %d, max |l_q| %d" % (count.bit_length() - 1, int(rule["observed"].max()), rule["max_abs_log_q"]))
    assert count >= 2 ** 12 and int(np.abs(rule["log_q"]).max()) > 2 ** 56
    twice = _gap_rule(inputs, lc.with_dense_count(base, 2 * count), junc, W_RUN)
    assert not gs.log_sum_fits(int(twice["observed"].max()), twice["max_abs_log_q"])  # (the largest)
    s = _sampler_of(prob, seed=25)
    got = tg._assert_equals_host(s, prob, "gap_max", windows=(W_RUN,), n_gaps=(5,), levels=("bin",))  # all arrays, scalars, model=False
    assert np.array_equal(got["junction"], junc) and int(np.abs(got["log_q"]).max()) > 2 ** 56
    got = tg._assert_equals_host(s, prob, "gap_max, a custom list", windows=(64, W_RUN), n_gaps=(2, 64), junctions=junc[::3])
    assert int(np.abs(got["log_q"]).max()) > 2 ** 56
    s.free_gpu()


# ---- the scorer across 2^24


SCORER_FAMILIES = {"packed_max": (53, 2 ** 24 - 1), "wide_min": (53, 2 ** 24), "int_max": (97, 2 ** 31 - 1)}


@functools.lru_cache(maxsize=None)
def _scorer_prob(family):
    step, value = SCORER_FAMILIES[family]
    prob = lc._synth("tiny")
    cnt = prob.coo_cnt.astype(np.int64)
    cnt[::step] = value
    return lc._rebuild(prob, prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64), cnt)


def _long_oracle():
    spec = importlib.util.spec_from_file_location("long_oracle", os.path.join(ROOT, "tools", "long_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("family", list(SCORER_FAMILIES))
def test_scorer_against_the_oracle(family, oracle_lib, monkeypatch):
    from instagraal_amd.sampler import sampler as hip_sampler
    from oracle.sampler_oracle import OracleSampler

    ol = oracle_lib
    for k in ("IG_SCREEN", "IG_SCREEN_VERIFY", "IG_WIDE_LISTS", "IG_POOL_ENTRIES"):
        monkeypatch.delenv(k, raising=False)
    prob = _scorer_prob(family)
    assert int(prob.coo_cnt.max()) == SCORER_FAMILIES[family][1] and np.array_equal(prob.coo_row, lc._synth("tiny").coo_row)
    kw = prob.sampler_kwargs()
    np.random.seed(31)
    s = hip_sampler(**kw, device_id=0)
    o = OracleSampler(**kw, mode=ol.MODE_DET)
    for x in (s, o):
        x.set_param_simu(prob.params)
        x.bins = np.arange(1.0, 60.0, 1.0)
        x.eval_likelihood_init()
    # the from-scratch pass: both limbs
    hi, lo = ol.last_limbs()
    nz, z, limbs = s.ctx.full_likelihood()
    assert nz == float(o.gpu_curr_likelihood_nz[0]) == float(s.curr_likelihood_on_nz[0])
    assert (int(limbs[0]), int(limbs[1])) == (int(hi[0]), int(lo[0]))
    # the terms, with the family's counts as observations
    rng = np.random.default_rng(3)
    n = 50000
    sep = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(np.float32)
    sep[::1000] = 0
    st = (sep * rng.uniform(0.5, 2.5, n)).astype(np.float32)
    ob = np.resize(prob.coo_cnt, n).astype(np.int32)
    ob[1::7] = SCORER_FAMILIES[family][1]
    ol.set_mode(ol.MODE_DET)
    p = np.zeros(1, ol.PARAM_DTYPE)
    for k in p.dtype.names:
        p[k] = np.float32(prob.params[k])
    ex, exc, term, q = ol.eval_terms(sep, st, ob, p)
    gex, gexc, gterm, gq = s.ctx.debug_eval_terms(sep, st, ob)
    assert np.array_equal(ex.view(np.uint32), gex.view(np.uint32)) and np.array_equal(exc.view(np.uint32), gexc.view(np.uint32))
    assert np.array_equal(term.view(np.uint64), gterm.view(np.uint64)) and np.array_equal(q, gq)
    # 150 moves through the batch path against the oracle stepping one by one from the same generator state
    lo_tool = _long_oracle()
    frags = np.random.permutation(prob.n_frags)[:150].astype(np.int32)
    state = np.random.get_state()
    res = s.step_sampler_batch(frags, 5)
    after = np.random.get_state()
    np.random.set_state(state)
    for t, (f, r) in enumerate(zip(frags, res)):
        cands = [c for c in o.return_neighbours(int(f), 5) if c != int(f)]
        b = o.step_sampler(int(f), 5, o.dt, candidates=cands)
        assert lo_tool._row(r) == (float(b[0]), float(b[1]), int(b[2]), int(b[3]), float(np.float32(b[4])), int(b[5])), (family, t)
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17())
    assert np.array_equal(np.array(s.ctx.valid_insert(), np.int32), np.array(o.gpu_list_valid_insert, np.int32))
    sums, _ = s.ctx.debug_globals()
    _, _, limbs = s.ctx.full_likelihood(0)
    assert [int(x) for x in sums[:5]] == [int(x) for x in limbs[:5]]  # the maintained sums against a from-scratch pass
    # which form the slice entries took
    stats = s.ctx.debug_screen_stats()
    pool = s.ctx.scratch_bytes()[1]
    if family == "packed_max":
        assert stats[2] > 0 and stats[4] > 0 and pool > 0 and pool % 8 == 0
    else:
        assert stats[2] == 0 and stats[4] == 0 and pool > 0 and pool % 12 == 0  # no column screened
        packed = hip_sampler(**_scorer_prob("packed_max").sampler_kwargs(), device_id=0)
        packed.set_param_simu(prob.params)
        packed.eval_likelihood_init()
        packed.step_sampler_batch(frags[:24], 5)
        # the same number of entries, 12 bytes each instead of 8.  (The two handles have run 150 and 24 moves: the pool is sized when the
        # move buffers are made -- min(candidates x Z, max(2^22, 2 Z)) entries, here candidates x Z, its ceiling, so no batch can grow
        # it -- and IG_POOL_ENTRIES, which would size it otherwise, is dropped at the head of this test.)
        assert 8 * pool == 12 * packed.ctx.scratch_bytes()[1]
        packed.free_gpu()
    s.free_gpu()


def test_packed_family_with_and_without_screening(monkeypatch):
    import test_hip_screen as tsc

    prob = _scorer_prob("packed_max")
    np.random.seed(33)
    frags = np.resize(np.random.permutation(prob.n_frags), 300).astype(np.int32)
    exact, _, _ = tsc._run(prob, frags, 7, {"IG_SCREEN": "0"}, monkeypatch)
    verified, stats, _ = tsc._run(prob, frags, 7, {"IG_SCREEN_VERIFY": "1"}, monkeypatch)  # raises on a violated bound (error 7)
    screened, stats2, _ = tsc._run(prob, frags, 7, {}, monkeypatch)
    assert verified == exact and screened == exact
    assert stats[0] < 0.5 and stats2[2] > 0


# ---- the upload


def test_upload_contacts_refuses_what_int32_cannot_hold():
    from instagraal_amd.sampler import problem_to_context

    prob = _prob("base")
    M = prob.n_sub_frags
    ctx = problem_to_context(prob)
    before = ctx.contact_map(37)[0]
    wrapped = prob.coo_cnt.astype(np.int64)
    wrapped[5] = 2 ** 31  # (as int32: -2^31)
    halves = prob.coo_cnt.astype(np.float64)
    halves[7] = 2.5
    far = prob.coo_row.astype(np.int64)
    far[-1] = 2 ** 32 + 3
    for name, args in (("cnt", (prob.coo_row, prob.coo_col, wrapped)), ("cnt", (prob.coo_row, prob.coo_col, halves)), ("row", (far, prob.coo_col, prob.coo_cnt)),
                       ("col", (prob.coo_row, far, prob.coo_cnt))):
        with pytest.raises(ValueError, match=name):
            ctx.upload_contacts(*args, M)
        assert np.array_equal(ctx.contact_map(37)[0], before)  # the handle keeps the contacts it had
    largest = prob.coo_cnt.astype(np.int64)
    largest[5] = 2 ** 31 - 1
    ctx.upload_contacts(prob.coo_row.astype(np.int64), prob.coo_col.astype(np.float64), largest, M)  # (what fits goes through, whatever its type)
    assert _py_sum(ctx.contact_map(37)[0]) == 2 * sum(largest.tolist())
    ctx.close()
