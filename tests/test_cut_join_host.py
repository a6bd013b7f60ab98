"""CPU tests of the cut and join scores' rule (instagraal_amd.cut_join) on problems of at most 60 bins: every cut and every link
against brute force -- ``rearrange.apply_host``, the tables of the edited state, every contact term (``hip_lib.contact_terms_host``) and
every zero-pixel term enumerated --, the identities the device relies on, the proposals and the two writers.  Exact integers
throughout."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def prob():
    from instagraal_amd import synth

    return synth.make_problem(60, 4000, synth.DEFAULT_SEED, 12)


@pytest.fixture(scope="module")
def start(prob):
    from instagraal_amd.sampler import soa17_from_dict

    return soa17_from_dict(prob.S_o_A_frags, prob.n_frags)


@pytest.fixture(scope="module")
def P(prob):
    from instagraal_amd import cut_join as cj

    return cj.Problem.of(prob)


def _terms(state, P):
    """every stored contact's term under the tables of ``state`` (no rings), and whether it is a cis pair"""
    from instagraal_amd import cut_join as cj

    dist, rank = cj.tables(state, P)
    cid = state[cj.F["id_c"]][P.parent]
    i, j = P.row, P.col
    cis = cid[i] == cid[j]
    return P.terms(np.abs(dist[i] - dist[j]).astype(np.float32), np.abs(rank[i] - rank[j]), (~cis).astype(np.int32), P.cnt), cis


def _brute(state, P, edit, cross_of):
    """-> (cross limbs, internal limbs, full difference of the from-scratch sums) of ``edit``; cross_of(cis before, cis behind) marks
    the contacts of the cross part"""
    from instagraal_amd import cut_join as cj, rearrange as ra

    after, status = ra.apply_host(state, edit, ra.next_contig_id(state))
    assert status == 0
    q0, c0 = _terms(state, P)
    q1, c1 = _terms(after, P)
    cross = cross_of(c0, c1)
    dh, dl = cj.limb_diff(q1, q0)
    full = tuple(a - b for a, b in zip(cj.full_sums_host(after, P), cj.full_sums_host(state, P)))
    return (int(dh[cross].sum()), int(dl[cross].sum())), (int(dh[~cross].sum()), int(dl[~cross].sum())), full


def _check_all(state, P):
    """every cut and every link of ``state`` against brute force -> (cuts, links, largest |internal part| in quanta)"""
    from instagraal_amd import cut_join as cj

    cuts, joins = cj.cut_scores_host(state, P), cj.join_scores_host(state, P)
    worst = 0
    for f in np.nonzero(cuts["valid"])[0].tolist():
        cross, internal, full = _brute(state, P, cj.cut_edit(state, f), lambda c0, c1: c0 & ~c1)
        got = tuple(int(x) for x in cuts["limbs"][f])
        assert got[:2] == cross, f
        assert got[2:] == full[2:], f
        assert (got[0] + internal[0], got[1] + internal[1]) == full[:2], f
        worst = max(worst, abs((internal[0] << 32) + internal[1]))
    rows = cj.link_rows(joins)
    for r in rows:
        cross, internal, full = _brute(state, P, r["edit"], lambda c0, c1: ~c0 & c1)
        got = tuple(int(x) for x in r["limbs"])
        assert got[:2] == cross, (r["a"], r["b"], r["sa"], r["sb"])
        assert got[2:] == full[2:]
        assert (got[0] + internal[0], got[1] + internal[1]) == full[:2]
        worst = max(worst, abs((internal[0] << 32) + internal[1]))
    return cuts, rows, worst


def test_every_cut_and_every_link_against_brute_force(start, P):
    cuts, rows, worst = _check_all(start, P)
    assert cuts["valid"].sum() >= 40 and rows.size >= 12  # several contigs, most pairs of them in contact
    assert worst > 0  # the internal part exists: the dists are re-originated


def test_brute_force_on_an_edited_genome_with_flipped_bins_and_other_ids(start, P):
    """behind a few edits: flipped segments (ori = -1), a contig id out of order, a contig of one bin"""
    from instagraal_amd import rearrange as ra

    st = start.copy()
    c = sorted((ra.contig_bins(st, k) for k in np.unique(st[ra.F["id_c"]]).tolist()), key=lambda b: -b.size)
    for e in ((int(c[0][2]), int(c[0][6]), ra.IN_PLACE, 0, 1), (int(c[1][1]), int(c[1][3]), int(c[2][0]), 1, 1), (int(c[0][0]), int(c[0][0]), ra.NEW_CONTIG, 0, 0)):
        st, status = ra.apply_host(st, e, ra.next_contig_id(st))
        assert status == 0
    assert (st[ra.F["ori"]] == -1).any() and (st[ra.F["l_cont"]] == 1).any()
    _check_all(st, P)


def test_a_contigs_scan_ends_at_zero_and_z_is_equal_for_the_four_links(start, P):
    from instagraal_amd import cut_join as cj

    cuts = cj.cut_scores_host(start, P)  # (asserts that every running sum closes at every contig's first bin and behind the last)
    heads = np.nonzero(start[cj.F["pos"]] == 0)[0]
    assert not cuts["valid"][heads].any() and not cuts["limbs"][heads].any() and not cuts["contacts"][heads].any()
    rows = cj.link_rows(cj.join_scores_host(start, P)).reshape(-1, 4)
    assert (rows["limbs"][:, :, 2:] == rows["limbs"][:, :1, 2:]).all()
    assert (rows["limbs"][:, :, :2] != rows["limbs"][:, :1, :2]).any()  # ... and nz is not
    assert (rows["limbs"][:, :, 4] > 0).all() and (cuts["limbs"][cuts["valid"], 4] < 0).all()


@pytest.mark.parametrize("d_max", [30.0, 7000.0, 1e9])
def test_the_closed_form_of_G_is_the_enumeration(prob, d_max):
    """on both sides of the d_max rank p* and of PZ_MAX = 4096 (the P_z table's end on the device)"""
    from instagraal_amd import cut_join as cj
    from instagraal_amd.sampler import PARAM_NAMES

    M = 5000
    sub = np.zeros(M, prob.np_sub_frags_2_frags.dtype)
    p = dict(prob.params, d_max=d_max)
    Q = cj.Problem(sub, [], [], [], [np.float32(p[k]) for k in PARAM_NAMES], np.float32(1.7))
    ps = Q.pstar()
    assert ps == {30.0: 18, 7000.0: 4118, 1e9: M + 1}[d_max]
    for L in sorted({1, 2, 3, ps - 1, ps, ps + 1, ps + 2, ps + 700, 4095, 4096, 4097, 4098, M}):
        if 1 <= L <= M:
            assert Q.G(L) == Q.G_enum(L), L
    assert Q.G(1) == (0, 0) and Q.G(2) != (0, 0)


def test_rings_and_singletons_give_no_cuts_and_no_links_to_rings(start, P):
    from instagraal_amd import cut_join as cj, rearrange as ra

    F = ra.F
    c = sorted((ra.contig_bins(start, k) for k in np.unique(start[F["id_c"]]).tolist()), key=lambda b: -b.size)
    st, status = ra.apply_host(start, (int(c[0][0]), int(c[0][0]), ra.NEW_CONTIG, 0, 0), ra.next_contig_id(start))
    assert status == 0
    st[F["circ"]][c[1]] = 1
    lone = int(c[0][0])
    cuts, joins = cj.cut_scores_host(st, P), cj.join_scores_host(st, P)
    assert not cuts["valid"][c[1]].any() and not cuts["valid"][lone]
    assert not cuts["limbs"][c[1]].any() and not cuts["contacts"][c[1]].any()
    n_lin = np.unique(st[F["id_c"]]).size - 1
    assert joins["K"] == n_lin and not np.isin(joins["head_bin"], c[1]).any()
    k_lone = int(np.nonzero(joins["head_bin"] == lone)[0][0])
    assert joins["tail_bin"][k_lone] == lone and joins["n_sub"][k_lone] == st[F["sub_len"]][lone]
    rows = cj.link_rows(joins)
    assert ((rows["a"] == k_lone) | (rows["b"] == k_lone)).any()  # a contig of one bin has links
    for r in rows:
        assert ra.check(st, r["edit"]) == 0
    # the cuts of the other contigs do not see the ring: they are those of the genome without it
    keep = ~np.isin(np.arange(st.shape[1]), c[1])
    lin = st.copy()
    lin[F["circ"]][:] = 0
    want = cj.cut_scores_host(lin, P)
    assert np.array_equal(cuts["limbs"][keep], want["limbs"][keep]) and np.array_equal(cuts["valid"][keep], want["valid"][keep])


def test_the_canonical_edit_of_every_link_joins_the_named_ends(start, P):
    from instagraal_amd import cut_join as cj, rearrange as ra

    F = ra.F
    joins = cj.join_scores_host(start, P)
    rows = cj.link_rows(joins)
    assert rows.size == 4 * joins["n_pairs"]
    for r in rows:
        a, b, sa, sb = (int(r[k]) for k in ("a", "b", "sa", "sb"))
        e = r["edit"]
        assert (e[0], e[1]) == (joins["head_bin"][b], joins["tail_bin"][b])
        assert (e[2], e[3], e[4]) == ((joins["tail_bin"][a], 0, int(sb == 1)) if sa == 1 else (joins["head_bin"][a], 1, int(sb == 0)))
        after, status = ra.apply_host(start, e, ra.next_contig_id(start))
        assert status == 0
        ea, eb = int(r["bin_a"]), int(r["bin_b"])  # the two ends are neighbours now, a's contig holds both
        assert after[F["id_c"]][ea] == after[F["id_c"]][eb] == start[F["id_c"]][ea]
        assert abs(int(after[F["pos"]][ea]) - int(after[F["pos"]][eb])) == 1
        assert after[F["l_cont"]][ea] == start[F["l_cont"]][ea] + start[F["l_cont"]][eb]


def test_proposals_statuses_and_the_two_writers(start, P, tmp_path):
    from instagraal_amd import cut_join as cj, rearrange as ra

    base = [int(x) for x in cj.full_sums_host(start, P)]
    cuts, joins = cj.cut_scores_host(start, P, base), cj.join_scores_host(start, P, base)
    assert cuts["delta"][cuts["valid"]].any() and joins["delta"].any()
    # a delta is the double ig_full_likelihood's formation gives: here against plain float arithmetic on the exact integers
    f = int(np.nonzero(cuts["valid"])[0][0])
    d = [int(x) for x in cuts["limbs"][f]]
    approx = ((d[0] << 32) + d[1]) / 2.0 ** 32 + cj.LOG_E * (((d[2] << 32) + d[3]) / 2.0 ** 32 + d[4] * float(P.params[7]))
    assert abs(cuts["delta"][f] - approx) < 1e-6 * max(1.0, abs(approx))
    wc, sj = cj.weakest_cuts(start, cuts, 5), cj.strongest_joins(joins, 7)
    assert wc.size <= 5 and sj.size <= 7 and (wc["delta"] > 0).all() and (sj["delta"] > 0).all()
    assert (np.diff(wc["delta"]) <= 0).all() and (np.diff(sj["delta"]) <= 0).all()
    every = cj.weakest_cuts(start, cuts, 10 ** 6)
    assert every.size == int((cuts["valid"] & (cuts["delta"] > 0)).sum())
    for r in every:
        assert ra.check(start, r["edit"]) == 0 and r["edit"][0] == r["bin"] and r["edit"][2] == ra.NEW_CONTIG
        assert start[ra.F["next"]][r["edit"][1]] == -1 and start[ra.F["prev"]][r["bin"]] == r["prev_bin"]
    edits = ra.propose_cuts_joins(start, cuts, joins, 5)
    assert np.array_equal(edits, np.concatenate([wc["edit"], cj.strongest_joins(joins, 5)["edit"]]).astype(np.int32))
    assert ra.propose_cuts_joins(start, None, None).shape == (0, 5)
    assert np.array_equal(ra.propose_cuts_joins(start, cuts, None, 5), wc["edit"])
    # an edit the state refuses is left out: the same tables on a state where the cut contig is a ring
    ring = start.copy()
    ring[ra.F["circ"]][:] = 1
    assert ra.propose_cuts_joins(ring, cuts, joins, 5).shape == (0, 5)
    n = cj.write_cuts(str(tmp_path / "cuts.txt"), wc)
    lines = open(str(tmp_path / "cuts.txt")).read().splitlines()
    assert n == wc.size and lines[0] == "# " + " ".join(cj.CUT_COLUMNS) and lines[-1] == "# cuts=%d" % wc.size and len(lines) == wc.size + 2
    if wc.size:
        w = lines[1].split()
        assert len(w) == len(cj.CUT_COLUMNS) and int(w[0]) == wc["bin"][0] and float(w[3]) == wc["delta"][0] and [int(x) for x in w[4:]] == wc["edit"][0].tolist()
    n = cj.write_links(str(tmp_path / "links.txt"), sj)
    lines = open(str(tmp_path / "links.txt")).read().splitlines()
    assert n == sj.size and lines[0] == "# " + " ".join(cj.LINK_COLUMNS) and lines[-1] == "# links=%d" % sj.size and len(lines) == sj.size + 2
    if sj.size:
        w = lines[1].split()
        assert len(w) == len(cj.LINK_COLUMNS) and w[2] in cj.SIDES and w[3] == cj.SIDES[int(sj["sb"][0])] and float(w[7]) == sj["delta"][0]
        assert [int(x) for x in w[8:]] == sj["edit"][0].tolist()


def test_on_exactly_representable_dists_the_internal_part_is_zero_or_the_flip(prob):
    """every len_bp a multiple of 1 000 and every offset a multiple of 1/64 kb: no sum of a dist rounds (asserted in float64), so the
    internal part of a cut and of a link without a flip is zero, that of a flipped link the delta of the in-place flip of b"""
    from instagraal_amd import cut_join as cj, rearrange as ra

    fx, st = exact_fixture(prob)
    Q = cj.Problem.of(fx)
    assert_representable(st, Q)
    cuts, joins = cj.cut_scores_host(st, Q), cj.join_scores_host(st, Q)
    for f in np.nonzero(cuts["valid"])[0].tolist():
        _, internal, _ = _brute(st, Q, cj.cut_edit(st, f), lambda c0, c1: c0 & ~c1)
        assert internal == (0, 0), f
    flips = 0
    for r in cj.link_rows(joins):
        _, internal, _ = _brute(st, Q, r["edit"], lambda c0, c1: ~c0 & c1)
        if r["edit"][4]:
            _, _, flip = _brute(st, Q, (r["edit"][0], r["edit"][1], ra.IN_PLACE, 0, 1), lambda c0, c1: c0 & ~c0)
            assert internal == flip[:2] and flip[2:] == (0, 0, 0)
            flips += internal != (0, 0)
        else:
            assert internal == (0, 0)
    assert flips  # a flip does move the reference points


def exact_fixture(prob):
    """``prob`` with every bin 1 000 x (its sub-fragments) bp long, the bins of a contig laid end to end, and the watson / crick
    offsets rounded to multiples of 1/64 kb -> (the problem, its start state)"""
    import copy

    from instagraal_amd import rearrange as ra
    from instagraal_amd.sampler import soa17_from_dict

    fx = copy.deepcopy(prob)
    S = fx.S_o_A_frags
    S["len_bp"] = (np.asarray(S["sub_len"]) * 1000).astype(S["len_bp"].dtype)
    st = soa17_from_dict(S, fx.n_frags)
    for c in np.unique(st[ra.F["id_c"]]).tolist():
        ra.rebuild(st, c, ra.contig_bins(st, c))
    S["start_bp"] = st[ra.F["start_bp"]].astype(S["start_bp"].dtype)
    S["l_cont_bp"] = st[ra.F["l_cont_bp"]].astype(S["l_cont_bp"].dtype)
    sub = fx.np_sub_frags_2_frags
    for k in ("y", "z"):
        sub[k] = np.round(sub[k] * 64.0) / 64.0
    return fx, soa17_from_dict(S, fx.n_frags)


def assert_representable(state, P):
    """every dist of the state, and of any state its bins can be rearranged into, is exact: start_bp / 1000 + offset in float64 is the
    float32 value, with bits to spare for every contig below 2^17 kb"""
    from instagraal_amd import cut_join as cj

    assert not (state[cj.F["len_bp"]] % 1000).any() and int(state[cj.F["len_bp"]].astype(np.int64).sum()) < (1 << 17) * 1000
    for off in (P.wat, P.cri):
        assert np.array_equal(off.astype(np.float64) * 64.0, np.round(off.astype(np.float64) * 64.0)) and (np.abs(off) < 1024).all()
    dist, _ = cj.tables(state, P)
    f = P.parent
    ori = state[cj.F["ori"]][f]
    want = state[cj.F["start_bp"]][f].astype(np.float64) / 1000.0 + np.where(ori == 1, P.wat, P.cri).astype(np.float64)
    assert np.array_equal(dist.astype(np.float64), want)
