"""GPU tests of the cut and join scores (ig_cut_scores, ig_join_scores_build; sampler.cut_scores, join_scores, weakest_cuts,
strongest_joins, polish(cuts, joins)) against the rule (instagraal_amd.cut_join, the state given with the handle's own contig ids) and
against the exact scorer (ig_edit_score).  Every comparison is on exact integers; the deltas are compared as bit patterns."""
import os

import numpy as np
import pytest

from test_cut_join_host import assert_representable, exact_fixture
from test_hip_parity import make_ctx
from test_hip_placement_support import _sampler

pytestmark = pytest.mark.gpu

REFUSED = (-1, 0, -2, 0, 0)  # ig_edit_state of a refused edit: the current state as the handle holds it, internal contig ids


@pytest.fixture(scope="module")
def tiny():
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS["tiny"])


def _start(prob):
    from instagraal_amd.sampler import soa17_from_dict

    return soa17_from_dict(prob.S_o_A_frags, prob.n_frags)


def _contigs(state):
    from instagraal_amd import rearrange as ra

    return sorted((ra.contig_bins(state, c) for c in np.unique(state[ra.F["id_c"]]).tolist()), key=lambda b: -b.size)


def _ints(limbs):
    h = [int(x) for x in limbs]
    return ((h[0] << 32) + h[1], (h[2] << 32) + h[3], h[4])


def _against_the_rule(ctx, prob, params=None):
    """both reports of the handle against the rule on the handle's own state -> (cuts, joins) of the device"""
    from instagraal_amd import cut_join as cj

    live, status = ctx.edit_state(REFUSED)
    assert status == 1
    base = ctx.full_likelihood()[2]
    P = cj.Problem.of(prob, params)
    cuts, joins = ctx.cut_scores(), ctx.join_scores()
    want_c, want_j = cj.cut_scores_host(live, P, base), cj.join_scores_host(live, P, base)
    for k in ("valid", "contacts", "limbs"):
        assert np.array_equal(cuts[k], want_c[k]), (k, np.argwhere(cuts[k] != want_c[k])[:5].tolist())
    assert np.array_equal(cuts["delta"].view(np.uint64), want_c["delta"].view(np.uint64))
    assert joins["K"] == want_j["K"] and joins["n_pairs"] == want_j["n_pairs"]
    for k in ("head_bin", "tail_bin", "n_sub", "length_bp", "rowptr", "col", "contacts", "nz", "z", "dni"):
        assert np.array_equal(joins[k], want_j[k]), (k, np.argwhere(joins[k] != want_j[k])[:5].tolist())
    assert np.array_equal(joins["delta"].view(np.uint64), want_j["delta"].view(np.uint64))
    assert np.array_equal(ctx.full_likelihood()[2], base) and np.array_equal(ctx.edit_state(REFUSED)[0], live)  # nothing was changed
    return cuts, joins


def test_tiny_at_start_and_with_a_ring(tiny):
    from instagraal_amd import rearrange as ra

    ctx = make_ctx(tiny)
    cuts, joins = _against_the_rule(ctx, tiny)
    assert cuts["valid"].sum() == 300 - 6 and joins["K"] == 6 and 0 < joins["n_pairs"] <= 15
    start = _start(tiny)
    c = _contigs(start)
    ring = start.copy()
    ring[ra.F["circ"]][c[2]] = 1
    ctx.upload_state(ring)
    cuts, joins = _against_the_rule(ctx, tiny)
    assert not cuts["valid"][c[2]].any() and joins["K"] == 5 and not np.isin(joins["head_bin"], c[2]).any()
    ctx.close()


def test_tiny_with_rare_operands(tiny):
    """slope = 0 (the generic composition of the term, not the one-log evaluation) and a d_max below the longest contig (the prefix
    table of the zero-pixel terms beyond it)"""
    params = dict(tiny.params, slope=0.0, d_max=60.0)
    ctx = make_ctx(tiny, params=params)
    _against_the_rule(ctx, tiny, params)
    ctx.close()


def test_small_behind_300_moves():
    """the handle's own contig ids (gaps, out of order), flipped bins, blocks of several bins"""
    from instagraal_amd import rearrange as ra

    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    live = s.ctx.edit_state(REFUSED)[0]
    ids = np.unique(live[ra.F["id_c"]])
    assert ids.size < ids.max() + 1 and (live[ra.F["ori"]] == -1).any()
    cuts, joins = _against_the_rule(s.ctx, prob)
    assert cuts["valid"].any() and joins["n_pairs"] > 0
    s.free_gpu()


def test_a_bombed_tiny_has_no_cuts_and_many_pairs(tiny):
    from instagraal_amd.hip_lib import CUT_JOIN_LDS_PAIRS

    ctx = make_ctx(tiny)
    ctx.bomb(np.arange(tiny.n_frags, dtype=np.int32))
    cuts, joins = _against_the_rule(ctx, tiny)
    assert not cuts["valid"].any() and not cuts["limbs"].any() and joins["K"] == 300 and joins["n_pairs"] > 4 * CUT_JOIN_LDS_PAIRS
    ctx.close()


def _one_contig(state):
    """every contig of ``state`` joined behind the longest, in the order of their ids"""
    from instagraal_amd import rearrange as ra

    st = state.copy()
    c = _contigs(st)
    for b in c[1:]:
        tail = ra.contig_bins(st, st[ra.F["id_c"]][c[0][0]])[-1]
        st, status = ra.apply_host(st, (int(b[0]), int(b[-1]), int(tail), 0, 0), ra.next_contig_id(st))
        assert status == 0
    return st


def test_one_contig_holding_everything_has_no_links(tiny):
    ctx = make_ctx(tiny)
    ctx.upload_state(_one_contig(_start(tiny)))
    cuts, joins = _against_the_rule(ctx, tiny)
    assert cuts["valid"].sum() == 299 and joins["K"] == 1 and joins["n_pairs"] == 0 and joins["rowptr"].tolist() == [0, 0]
    ctx.close()


def test_both_join_forms_return_the_same_bytes(tiny):
    """pair counts on both sides of the threshold that picks the form: <= 15 pairs (by default: accumulators in LDS) and thousands (by
    default: atomics per run of a wave; forced: LDS in windows of 256 pairs)"""
    from instagraal_amd.hip_lib import CUT_JOIN_LDS_PAIRS

    ctx = make_ctx(tiny)
    for bombed in (False, True):
        if bombed:
            ctx.bomb(np.arange(tiny.n_frags, dtype=np.int32))
        got = []
        for form in (-1, 0, 1, -1):
            ctx.debug_cut_join_form(form)
            j = ctx.join_scores()
            ms, ck = ctx.debug_cut_join_time("joins", 1)
            got.append((j, ck))
            assert ms.shape == (1, 12) and ms[0, 10] > 0 and ms[0, 3] > 0 and not ms[0, :3].any()
        assert (got[0][0]["n_pairs"] > CUT_JOIN_LDS_PAIRS) == bombed
        for j, ck in got[1:]:
            assert ck == got[0][1]
            for k in ("rowptr", "col", "contacts", "nz", "z", "dni"):
                assert np.array_equal(j[k], got[0][0][k]), k
            assert np.array_equal(j["delta"].view(np.uint64), got[0][0]["delta"].view(np.uint64))
        assert got[0][0]["nz"].any()
    ms, ck = ctx.debug_cut_join_time("cuts", 2)
    assert ms.shape == (2, 12) and (ms[:, :3] > 0).all() and not ms[:, 3:].any() and ck == ctx.debug_cut_join_time("cuts", 1)[1]
    with pytest.raises(Exception):
        ctx.debug_cut_join_form(2)
    ctx.close()


def test_on_exactly_representable_dists_the_scores_are_the_exact_scorers(tiny):
    """cut limbs = ig_edit_score's for every junction; link limbs = those of the canonical edit for every unflipped link, and plus the
    delta of the in-place flip of b for every flipped one"""
    from instagraal_amd import cut_join as cj, rearrange as ra

    fx, st = exact_fixture(tiny)
    assert_representable(st, cj.Problem.of(fx))
    ctx = make_ctx(fx)
    cuts, joins = _against_the_rule(ctx, fx)
    base = _ints(ctx.full_likelihood()[2])
    add = lambda d: tuple(a + b for a, b in zip(base, _ints(d)))  # noqa: E731
    bins = np.nonzero(cuts["valid"])[0]
    edits = np.asarray([cj.cut_edit(st, f) for f in bins.tolist()], np.int32)
    status, limbs, _, _ = ctx.edit_score(edits)
    assert not status.any()
    for f, l in zip(bins.tolist(), limbs):
        assert _ints(l) == add(cuts["limbs"][f]), f
    rows = cj.link_rows(joins)
    status, limbs, _, _ = ctx.edit_score(rows["edit"])
    flip_edits = np.asarray([(e[0], e[1], ra.IN_PLACE, 0, 1) for e in rows["edit"]], np.int32)
    fstatus, flimbs, _, _ = ctx.edit_score(flip_edits)
    assert not status.any() and not fstatus.any() and rows["edit"][:, 4].any() and not rows["edit"][:, 4].all()
    moved = 0
    for r, l, fl in zip(rows, limbs, flimbs):
        flip = tuple(a - b for a, b in zip(_ints(fl), base)) if r["edit"][4] else (0, 0, 0)
        assert _ints(l) == tuple(a + b for a, b in zip(add(r["limbs"]), flip)), (r["a"], r["b"], r["sa"], r["sb"])
        moved += flip != (0, 0, 0)
    assert moved
    ctx.close()


def test_planted_join_and_cut_are_rank_one_and_polish_undoes_both(tiny):
    """on unmodified tiny the internal part is not zero: only what is derivable is asserted.  Two contigs joined by an edit: that
    junction is rank 1 of weakest_cuts and of the exact scores of all junctions.  A contig cut in two: that link, in its orientation,
    is rank 1 of strongest_joins and of the exact scores of the listed links.  polish(cuts, joins) undoes both in one round."""
    from instagraal_amd import cut_join as cj, rearrange as ra

    prob, s = _sampler("tiny", seed=23)
    start = _start(prob)
    c = _contigs(start)
    true_like = float(np.ravel(s.likelihood_t)[0])
    join = (int(c[4][0]), int(c[4][-1]), int(c[3][-1]), 0, 0)  # the 6-bin contig behind the tail of the 21-bin one
    cut = (int(c[0][70]), int(c[0][-1]), ra.NEW_CONTIG, 0, 0)  # the 154-bin contig in two
    s.apply_rearrangement(join)
    s.apply_rearrangement(cut)
    assert s.n_contigs == 6
    worst = 0.0
    # the planted join is the weakest junction
    cuts = s.cut_scores()
    wc = s.weakest_cuts(5, cuts)
    assert wc.size >= 1 and wc["bin"][0] == c[4][0] and wc["prev_bin"][0] == c[3][-1] and wc["delta"][0] > 0
    live = s.ctx.download_state()
    bins = np.nonzero(cuts["valid"])[0]
    exact = s.score_rearrangements(np.asarray([cj.cut_edit(live, f) for f in bins.tolist()], np.int32))
    assert not exact["status"].any() and bins[int(np.argmax(exact["delta"]))] == c[4][0]
    worst = max(worst, float(np.abs(exact["delta"] - cuts["delta"][bins]).max()))
    assert any(_ints(e["limbs"])[0] - _ints(s.ctx.full_likelihood()[2])[0] != _ints(cuts["limbs"][f])[0] for e, f in zip(exact, bins.tolist()))  # an internal part exists
    # the planted cut is the strongest link, tail of the first half to head of the second
    joins = s.join_scores()
    sj = s.strongest_joins(10 ** 6, joins)
    top = sj[0]
    assert {int(top["bin_a"]), int(top["bin_b"])} == {int(c[0][69]), int(c[0][70])} and top["delta"] > 0
    e = top["edit"]
    assert e[4] == 0 and ((e[2], e[3]) == (int(c[0][69]), 0) and e[0] == int(c[0][70]) or (e[2], e[3]) == (int(c[0][70]), 1) and e[1] == int(c[0][69]))
    exact = s.score_rearrangements(sj["edit"])
    assert not exact["status"].any() and int(np.argmax(exact["delta"])) == 0
    worst = max(worst, float(np.abs(exact["delta"] - sj["delta"]).max()))
    print("largest |cross part - exact delta|: %.6g" % worst)
    # polish with both kinds of proposal: one round, both plants undone
    st = np.random.get_state()
    log = s.polish(cuts=True, joins=True)
    assert len(log) == 2 and {r["round"] for r in log} == {0} and all(r["delta"] > 0 for r in log)
    kinds = sorted(int(r["edit"][2] == ra.NEW_CONTIG) for r in log)
    assert kinds == [0, 1]
    assert np.array_equal(ra.canonical(s.ctx.download_state()), ra.canonical(start)) and float(s.likelihood_t) == true_like
    after = np.random.get_state()
    assert np.array_equal(st[1], after[1]) and st[2] == after[2]
    s.free_gpu()


def test_the_defaults_of_polish_and_the_proposals_are_unchanged(tiny):
    """cuts = joins = False: the proposals are those of before"""
    from instagraal_amd import rearrange as ra, segment_placement as sp

    prob, s = _sampler("tiny", seed=23)
    c = _contigs(_start(prob))
    s.apply_rearrangement((int(c[1][6]), int(c[1][15]), ra.IN_PLACE, 0, 1))
    s.apply_rearrangement((int(c[0][70]), int(c[0][-1]), ra.NEW_CONTIG, 0, 0))  # (a cut in the wrong place: a link with a positive delta)
    inv = s.inverted_segments(20, level="block")
    mis = [s.misplaced_segments(20, level=level, window=sp.DEFAULT_WINDOW) for level in ("block", "scaffold")]
    want = ra.propose(s.ctx.download_state(), inv, mis, 20, sp.DEFAULT_WINDOW)
    got = s.propose_rearrangements()
    assert np.array_equal(got, want) and got.shape[0] > 0
    more = s.propose_cuts_joins()
    assert more.shape[0] > 0 and not [e for e in more if ra.check(s.ctx.download_state(), e)]
    assert np.array_equal(more, np.concatenate([s.propose_cuts_joins(joins=False), s.propose_cuts_joins(cuts=False)]))
    s.free_gpu()


def test_the_reports_do_not_interfere_with_the_moves():
    outs = []
    for between in (False, True):
        prob, s = _sampler("tiny", seed=21)
        frags = np.random.permutation(prob.n_frags)[:150].astype(np.int32)
        r1 = s.step_sampler_batch(frags[:75], 5).copy()
        if between:
            st = np.random.get_state()
            cuts, joins = s.cut_scores(), s.join_scores()
            assert cuts["valid"].any() and joins["n_pairs"] > 0 and s.weakest_cuts(5, cuts).size <= 5 and s.strongest_joins(5, joins).size <= 5
            after = np.random.get_state()
            assert np.array_equal(st[1], after[1]) and st[2] == after[2]
        r2 = s.step_sampler_batch(frags[75:], 5).copy()
        outs.append((r1, r2, s.gpu_vect_frags.copy_from_gpu().soa17(), list(s.ctx.valid_insert()), np.random.get_state()[1].copy(), np.random.get_state()[2]))
        s.free_gpu()
    a, b = outs
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


def test_the_reports_are_refused_on_a_sharded_handle(tiny):
    from instagraal_amd.hip_lib import HipError

    ctx = make_ctx(tiny)
    ctx.set_shard(0, 2)
    for call in (ctx.cut_scores, ctx.join_scores):
        with pytest.raises(HipError, match="all contacts on one handle"):
            call()
    ctx.close()


def test_contact_terms_host_against_eval_q_on_the_device(tiny):
    """bit for bit, for cis and trans pairs, counts below and beyond the factorial table and the table of log10(ob!), rank distances
    below and beyond the P_z table, separations on both sides of d_max, and under slope = 0 (no one-log evaluation)"""
    from instagraal_amd import hip_lib
    from instagraal_amd.sampler import PARAM_NAMES

    rng = np.random.default_rng(7)
    n = 100_000
    s = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(np.float32)
    s[::1000] = 0
    d = rng.integers(0, 3000, n).astype(np.int32)
    d[::13] = rng.integers(4000, 100_000, d[::13].size)
    trans = (rng.random(n) < 0.3).astype(np.int32)
    ob = rng.integers(0, 40, n).astype(np.int32)
    ob[::17] = rng.integers(0, 5000, ob[::17].size)
    for params in (tiny.params, dict(tiny.params, slope=0.0), dict(tiny.params, d_max=300.0)):
        ctx = make_ctx(tiny, params=params)
        mean_kb = np.float32(tiny.S_o_A_sub_frags["len_bp"].mean() / 1000.0)
        host = hip_lib.contact_terms_host([np.float32(params[k]) for k in PARAM_NAMES], mean_kb, s, d, trans, ob)
        dev = ctx.debug_contact_terms(s, d, trans, ob)
        assert np.array_equal(host, dev), np.argwhere(host != dev)[:5].tolist()
        assert np.unique(host).size > 1000  # (not a vacuous comparison; with slope = 0 a term depends on the count and on P_z alone)
        ctx.close()


def test_a_run_writes_cuts_and_links_and_the_outputs_describe_the_polished_genome(tmp_path):
    from instagraal_amd import cut_join as cj, rearrange as ra, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=1, bomb=True, polish="all", save_cut_join=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    lines = open(os.path.join(folder, "polish.txt")).read().splitlines()
    assert lines[0] == "# " + " ".join(ra.LOG_COLUMNS) and int(lines[-1].split("=")[1]) > 0
    for name, columns, table in (("cuts.txt", cj.CUT_COLUMNS, s.weakest_cuts()), ("links.txt", cj.LINK_COLUMNS, s.strongest_joins())):
        lines = open(os.path.join(folder, name)).read().splitlines()
        assert lines[0] == "# " + " ".join(columns) and len(lines) == len(table) + 2
        rows = [ln.split() for ln in lines if not ln.startswith("#")]
        assert [[int(x) for x in r[-5:]] for r in rows] == table["edit"].tolist()  # written behind the polishing: of the genome the sampler holds
        assert [float(r[len(columns) - 6]) for r in rows] == table["delta"].tolist()
    g = s.gpu_vect_frags.copy_from_gpu()
    assert np.array_equal(g.soa17(), s.ctx.download_state())
    blocks, cur = {}, None
    for ln in open(os.path.join(folder, "info_frags.txt")).read().splitlines():
        if ln.startswith(">"):
            cur = blocks.setdefault(int(ln.rsplit("_", 1)[1]), [])
        elif not ln.startswith("init_contig"):
            cur.append((int(ln.split("\t")[1]), int(ln.split("\t")[2])))
    assert sorted(blocks) == np.unique(g.id_c).tolist() and len(blocks) == int(s.n_contigs)
    for cid, rows_c in blocks.items():
        assert rows_c == [(int(g.id_d[f]), int(g.ori[f])) for f in ra.contig_bins(g.soa17(), cid)], cid
    p2.simulation.release()
