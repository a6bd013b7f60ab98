"""GPU tests of what the seven reports on the current genome share: the genome view (ig_host_genome.inc) and the row builder
(ig_host_rows.inc).  The reports run against each other on one handle -- in both orders, around a snapshot that stays resident,
behind a refusal, on handles of two sizes in one process, on empty inputs -- and every result is held to its feature's numpy rule
with the comparisons of that feature's own tests.  Exact integer equality throughout; `tiny` and `small` only."""
import numpy as np
import pytest

import test_hip_assembly_contacts as ta
import test_hip_expected_map as te
import test_hip_join_support as tj
import test_hip_placement_support as tp

pytestmark = pytest.mark.gpu

WINDOW = 64
MAX_SIDE = 64
REPORTS = ("map", "law", "junction", "lift_sub", "lift_bin", "join", "emap", "place")


def _order_rule(ctx, prob):
    """the genome order from the downloaded state alone: contigs in ascending id, one only if every bin of it is active, its bins by
    ``pos``, a bin's sub-fragments consecutive in the table and reversed where ``ori == -1``"""
    from instagraal_amd.hip_lib import FRAG_FIELDS

    state = ctx.download_state()
    col = {k: state[i].astype(np.int64) for i, k in enumerate(FRAG_FIELDS)}
    sub_len = col["sub_len"]
    first_sub = np.cumsum(sub_len) - sub_len
    by = np.lexsort((col["pos"], col["id_c"]))
    by = by[~np.isin(col["id_c"][by], np.unique(col["id_c"][col["activ"] != 1]))]
    w = sub_len[by]
    start = np.cumsum(w) - w
    bin_of = np.repeat(np.arange(by.size), w)
    j = np.arange(int(w.sum())) - start[bin_of]
    return (first_sub[by][bin_of] + np.where(col["ori"][by][bin_of] == -1, w[bin_of] - 1 - j, j)).astype(np.int64)


def _rules(ctx, prob, oracle_lib, params, contacts=None):
    """every report's rule for the state of the handle -> {report: the rule's result}; computed once per state, compared many times"""
    from instagraal_amd import assembly_contacts as ac, distance_law as dlaw, expected_map as em, join_support as js
    from instagraal_amd import junction_profile as jp, placement_support as ps
    from instagraal_amd.contact_map import binning

    row, col, cnt = contacts if contacts is not None else (prob.coo_row, prob.coo_col, prob.coo_cnt)
    dist, stot, contig, placed, position, lbp = tj._host_inputs(ctx, prob)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    order = _order_rule(ctx, prob)
    assert np.array_equal(ctx.contact_map_order(), order)
    q = te._model_q(oracle_lib, params)
    T = order.size
    b, side = binning(T, MAX_SIDE)
    pi, pj = position[row] // max(b, 1), position[col] // max(b, 1)
    ok = (position[row] >= 0) & (position[col] >= 0)
    upper = np.bincount(pi[ok] * side + pj[ok], weights=cnt[ok].astype(np.float64), minlength=side * side).astype(np.int64).reshape(side, side)
    edges = np.arange(0, 61.0, 1.0, dtype=np.float32)
    unit = ac.units_along(parent[order])
    return dict(
        order=order, edges=edges, map=(upper + upper.T, b),
        law=dlaw.law_host(dist, stot, contig, placed, row, col, cnt, edges),
        junction=jp.profile_host(dist, stot, contig, placed, position, row, col, cnt, WINDOW, model_q=q),
        lift_sub=ac.lift_host(position, row, col, cnt, None), lift_bin=ac.lift_host(position, row, col, cnt, unit),
        join=js.support_host(dist, stot, contig, placed, position, lbp, row, col, cnt, WINDOW, model_q=q),
        emap=em.expected_host(dist, stot, contig.astype(np.int64), position, MAX_SIDE, q),
        place=ps.support_host(stot, contig, placed, position, parent, prob.n_frags, row, col, cnt, WINDOW, WINDOW))


def _lift_equal(ctx, res, want, what):
    res = dict(res)
    res["col"], res["count"] = ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
    ta._assert_equal(res, want, what)


def _check(ctx, rules, report, what):
    """runs one report on the handle and holds it to its rule"""
    from instagraal_amd import distance_law as dlaw, expected_map as em, junction_profile as jp

    what = (what, report)
    want = rules[report]
    if report == "map":
        assert np.array_equal(ctx.contact_map_order(), rules["order"]), what
        img, b = ctx.contact_map(MAX_SIDE)
        assert b == want[1] and img.dtype == np.int64 and np.array_equal(img, want[0]), what
    elif report == "law":
        got = ctx.distance_law(rules["edges"])
        assert all(np.array_equal(got[k], want[k]) for k in ("observed", "pairs")) and all(got[k] == want[k] for k in dlaw.SCALARS), what
    elif report == "junction":
        got = ctx.junction_profile(WINDOW)
        assert got["n_placed"] == want["n_placed"] and all(np.array_equal(got[k], want[k]) for k in ("observed", "pairs", "expected_q")), what
        assert all(got[k] == want[k] for k in jp.SCALARS), what
    elif report in ("lift_sub", "lift_bin"):
        _lift_equal(ctx, ctx.assembly_contacts(report[5:]), want, what)
    elif report == "join":
        tj._assert_equal(tj._device(ctx, WINDOW, release=False), want, what)
    elif report == "emap":
        got = ctx.expected_map(MAX_SIDE)
        assert (got["side"], got["bin"]) == (want["side"], want["bin"]), what
        assert all(np.array_equal(got[k], want[k]) for k in em.IMAGES) and all(got[k] == want[k] for k in te.COMPARED), what
    else:
        tp._assert_equal(ctx.placement_support(WINDOW, WINDOW), want, what)


def _check_all(ctx, rules, what, reports=REPORTS):
    for report in reports:
        _check(ctx, rules, report, what)


_FRESH = {}


def _fresh(cfg, oracle_lib):
    """a fresh sampler of ``cfg`` and the rules of its state (the same for every fresh handle of that problem: computed once)"""
    prob, s = tj._sampler(cfg, seed=5)
    if cfg not in _FRESH:
        _FRESH[cfg] = _rules(s.ctx, prob, oracle_lib, s.param_simu)
    return prob, s, _FRESH[cfg]


def test_the_reports_interleave_in_both_orders_around_a_resident_snapshot(oracle_lib):
    prob, s = tj._sampler("tiny", seed=6)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:60], 5)
    rules = _rules(s.ctx, prob, oracle_lib, s.param_simu)
    assert rules["lift_bin"]["entries_out"] > 0 and rules["join"]["n_links"] > 0 and rules["place"]["n_guests"] > 0
    _check_all(s.ctx, rules, "forwards")
    # the lift's snapshot stays resident while join support builds its own and placement support comes and goes
    lift = s.ctx.assembly_contacts("bin")
    join = tj._device(s.ctx, WINDOW, release=False)
    tj._assert_equal(join, rules["join"], "join behind a resident lift")
    _check(s.ctx, rules, "place", "between the snapshots")
    _check(s.ctx, rules, "junction", "between the snapshots")
    _lift_equal(s.ctx, lift, rules["lift_bin"], "the lift's snapshot behind join and placement calls")
    col, obs, pairs, expq = s.ctx.join_support_fetch(0, join["n_links"])
    assert np.array_equal(col, rules["join"]["col"]) and np.array_equal(obs, rules["join"]["observed"]) and np.array_equal(expq, rules["join"]["expected_q"])
    _check_all(s.ctx, rules, "backwards", REPORTS[::-1])
    s.ctx.assembly_contacts_release()
    s.ctx.join_support_release()
    s.free_gpu()


def test_handles_of_two_sizes_in_one_process(oracle_lib):
    """(a handle takes one sub-fragment table for life -- ig_upload_contacts refuses another M -- so the sizes alternate between two
    handles that are alive together.  What this does NOT reach: the branch of genome_view that frees and reallocates the view when
    (N, M) change on one handle, and the grow path of rows_reserve on a RowBuf that is kept -- no entry point can change M)"""
    _, tiny, tiny_rules = _fresh("tiny", oracle_lib)
    _check_all(tiny.ctx, tiny_rules, "tiny")
    _, small, small_rules = _fresh("small", oracle_lib)
    _check_all(small.ctx, small_rules, "small")
    _check_all(tiny.ctx, tiny_rules, "tiny again", REPORTS[::-1])
    _check_all(small.ctx, small_rules, "small again", ("lift_bin", "place", "join"))
    tiny.free_gpu()
    small.free_gpu()


def test_a_refusal_in_one_report_leaves_the_next_one_right(oracle_lib):
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s, rules = _fresh("tiny", oracle_lib)
    ctx = s.ctx
    with pytest.raises(hip_lib.HipError, match="ig_junction_profile.*window"):
        ctx.junction_profile(0)
    _check(ctx, rules, "join", "behind a refused junction profile")
    with pytest.raises(hip_lib.HipError, match="ig_join_support_build.*window"):
        ctx.join_support(1025)
    _check(ctx, rules, "place", "behind a refused join support")
    with pytest.raises(hip_lib.HipError, match="ig_placement_support.*min_hosts"):
        ctx.placement_support(WINDOW, 2 * WINDOW + 1)
    _check(ctx, rules, "lift_bin", "behind a refused placement support")
    with pytest.raises(hip_lib.HipError, match="level"):
        ctx.assembly_contacts(2)
    _check(ctx, rules, "emap", "behind a refused lift")
    with pytest.raises(hip_lib.HipError, match="ig_debug_expected_map_time: max_side"):
        ctx.debug_expected_map_time(0)
    _check(ctx, rules, "junction", "behind a refused expected map")
    # the view's own refusal, under every entry point's name: a nuisance step in flight
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    for name, call in (("ig_contact_map_order", ctx.contact_map_order), ("ig_contact_map", lambda: ctx.contact_map(MAX_SIDE)),
                       ("ig_distance_law", lambda: ctx.distance_law(rules["edges"])), ("ig_junction_profile", lambda: ctx.junction_profile(WINDOW)),
                       ("ig_assembly_contacts_build", lambda: ctx.assembly_contacts("sub")), ("ig_join_support_build", lambda: ctx.join_support(WINDOW)),
                       ("ig_expected_map", lambda: ctx.expected_map(MAX_SIDE)), ("ig_placement_support", lambda: ctx.placement_support(WINDOW))):
        with pytest.raises(hip_lib.HipError, match=name + ": a nuisance step is in flight"):
            call()
    ctx.nuis_end()
    _check_all(ctx, _rules(ctx, prob, oracle_lib, s.param_simu), "behind the step")
    s.free_gpu()


def test_empty_inputs_come_back_through_the_no_entries_path(oracle_lib):
    """nothing placed (T == 0) and no contacts (Z == 0): lift, join support and placement support succeed with empty rows, and the
    other reports agree with their rules on the same handles"""
    from instagraal_amd import hip_lib, synth
    from instagraal_amd.sampler import LIST_SIZE, N_INSERT_BLOCKS, PARAM_NAMES, problem_to_context, soa17_from_dict

    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    ctx = problem_to_context(prob)
    for f in range(prob.n_frags):  # nothing placed: a bin of every contig is inactive
        ctx.debug_set_bin_active(f, False)
    rules = _rules(ctx, prob, oracle_lib, prob.params)
    assert rules["order"].size == 0 and rules["lift_sub"]["entries_out"] == 0 == rules["join"]["n_links"] == rules["place"]["entries"]
    for report in ("lift_sub", "lift_bin", "join", "place", "law", "junction"):
        _check(ctx, rules, report, "nothing placed")
    assert ctx.contact_map(MAX_SIDE)[0].size == 0 and ctx.expected_map(MAX_SIDE)["side"] == 0
    for f in range(prob.n_frags):
        ctx.debug_set_bin_active(f, True)
    full = _rules(ctx, prob, oracle_lib, prob.params)
    assert full["lift_bin"]["entries_out"] > 0
    _check_all(ctx, full, "everything placed again")
    ctx.close()
    none = np.zeros(0, np.int32)
    bare = hip_lib.Context(0)
    bare.upload_subfrag_table(prob.np_sub_frags_2_frags)
    bare.upload_contacts(none, none, none, prob.n_sub_frags)
    bare.set_insert_config(LIST_SIZE[:N_INSERT_BLOCKS], int(LIST_SIZE[:N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)))
    bare.upload_state(soa17_from_dict(prob.S_o_A_frags, prob.n_frags))
    mean_kb = np.float32(prob.S_o_A_sub_frags["len_bp"].mean() / 1000.0)
    bare.set_params([np.float32(prob.params[k]) for k in PARAM_NAMES], mean_kb, 0)
    rules = _rules(bare, prob, oracle_lib, prob.params, contacts=(none, none, none))
    assert rules["order"].size == prob.n_sub_frags and rules["lift_sub"]["entries_out"] == 0 == rules["join"]["n_links"] == rules["place"]["entries"]
    _check_all(bare, rules, "no contacts")
    _check_all(bare, rules, "no contacts, backwards", REPORTS[::-1])
    bare.close()
