"""CPU tests of the segment edits' rule (instagraal_amd.rearrange) on ``tiny`` (300 bins in contigs of 154 / 59 / 57 / 21 / 6 / 3): the
round trips, the invariants of a consistent genome behind 200 chained random edits, every status code, the no-ops, and -- with the
oracle's likelihood in DET mode, the zero-pixel part in its nuisance form (the one with the well-defined mean) -- that every planted
error lowers the likelihood, that the limb deltas of edits on disjoint contigs add as exact integers, and that the proposals made from
the reports' host rules contain the exact undos of two planted errors, which one greedy round picks."""
import numpy as np
import pytest

from test_distance_law_host import fill_tables

SIZES = (154, 59, 57, 21, 6, 3)


@pytest.fixture(scope="module")
def prob():
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS["tiny"])


@pytest.fixture(scope="module")
def start(prob):
    from instagraal_amd.sampler import soa17_from_dict

    return soa17_from_dict(prob.S_o_A_frags, prob.n_frags)


def _contigs(state):
    """the contigs of ``state`` by falling length -> list of bin arrays in their order"""
    from instagraal_amd import rearrange as ra

    ids = np.unique(state[ra.F["id_c"]])
    return sorted((ra.contig_bins(state, c) for c in ids.tolist()), key=lambda b: -b.size)


@pytest.fixture(scope="module")
def score(prob, oracle_lib):
    """state -> the five sums of the oracle (DET) as exact integers (nz, z, intra pairs), and nz + z"""
    from oracle.sampler_oracle import OracleSampler

    ol = oracle_lib
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(prob.params)

    def f(state):
        ol.set_mode(ol.MODE_DET)
        for i, k in enumerate(ol.FRAG_FIELDS):
            getattr(o.gpu_vect_frags, k)[:] = state[i]
        o.fill_dist_single()
        z = o.approx_single_likelihood_on_zeros(nuis=True)
        hi, lo = ol.last_limbs()
        zq = (int(hi[0]) << 32) + int(lo[0])
        ni = int(o.gpu_n_vals_intra[0])
        o._full_nz(o.gpu_curr_likelihood_nz, o.param_simu)
        hi, lo = ol.last_limbs()
        nzq = (int(hi[0]) << 32) + int(lo[0])
        return (nzq, zq, ni), float(o.gpu_curr_likelihood_nz[0]) + float(z)

    return f


def _assert_consistent(state):
    from instagraal_amd import rearrange as ra

    F = ra.F
    N = state.shape[1]
    seen = np.zeros(N, np.int64)
    for c in np.unique(state[F["id_c"]]).tolist():
        b = ra.contig_bins(state, c)
        seen[b] += 1
        assert np.array_equal(state[F["pos"]][b], np.arange(b.size))
        sl, lb = state[F["sub_len"]][b].astype(np.int64), state[F["len_bp"]][b].astype(np.int64)
        assert np.array_equal(state[F["sub_pos"]][b], np.cumsum(sl) - sl) and np.array_equal(state[F["start_bp"]][b], np.cumsum(lb) - lb)
        assert (state[F["l_cont"]][b] == b.size).all() and (state[F["sub_l_cont"]][b] == sl.sum()).all() and (state[F["l_cont_bp"]][b] == lb.sum()).all()
        assert np.array_equal(state[F["prev"]][b], np.concatenate([[-1], b[:-1]])) and np.array_equal(state[F["next"]][b], np.concatenate([b[1:], [-1]]))
    assert (seen == 1).all()  # every bin in exactly one contig
    nx, pv = state[F["next"]], state[F["prev"]]
    has = nx >= 0
    assert np.array_equal(pv[nx[has]], np.nonzero(has)[0])  # prev / next mutually inverse
    has = pv >= 0
    assert np.array_equal(nx[pv[has]], np.nonzero(has)[0])


def test_the_synthetic_start_has_the_contigs_the_cases_name(start):
    assert tuple(b.size for b in _contigs(start)) == SIZES


def test_rebuilding_the_start_gives_the_start(start):
    from instagraal_amd import rearrange as ra

    st = start.copy()
    for c in np.unique(start[ra.F["id_c"]]).tolist():
        ra.rebuild(st, c, ra.contig_bins(start, c))
    assert np.array_equal(st, start)
    _assert_consistent(start)


def test_an_inversion_twice_and_a_move_and_back_give_the_start(start):
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    nid = ra.next_contig_id(start)
    a, b = int(c[1][6]), int(c[1][15])
    once, s = ra.apply_host(start, (a, b, ra.IN_PLACE, 0, 1), nid)
    assert s == 0 and not np.array_equal(once, start)
    assert np.array_equal(ra.contig_bins(once, once[ra.F["id_c"]][a])[6:16], c[1][6:16][::-1])
    twice, s = ra.apply_host(once, (b, a, ra.IN_PLACE, 0, 1), nid)
    assert s == 0 and np.array_equal(twice, start)
    # ranks 6..15 of the longest contig, flipped, behind the tail of the third; and back behind rank 5
    a, b, tail = int(c[0][6]), int(c[0][15]), int(c[2][-1])
    moved, s = ra.apply_host(start, (a, b, tail, 0, 1), nid)
    assert s == 0
    _assert_consistent(moved)
    assert np.array_equal(ra.contig_bins(moved, moved[ra.F["id_c"]][tail])[-10:], c[0][6:16][::-1])
    back, s = ra.apply_host(moved, (b, a, int(c[0][5]), 0, 1), nid)
    assert s == 0 and np.array_equal(back, start)
    back, s = ra.apply_host(moved, (b, a, int(c[0][16]), 1, 1), nid)
    assert s == 0 and np.array_equal(back, start)


def test_every_status_code(start):
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    N = start.shape[1]
    a, b = int(c[1][6]), int(c[1][15])
    ring = start.copy()
    ring[ra.F["circ"]][c[2]] = 1
    cases = [((a, b, ra.IN_PLACE, 0, 0), start, 0), ((-1, b, ra.IN_PLACE, 0, 0), start, 1), ((a, N, ra.IN_PLACE, 0, 0), start, 1), ((a, b, N, 0, 0), start, 1),
             ((a, int(c[0][3]), ra.IN_PLACE, 0, 0), start, 2), ((b, a, ra.IN_PLACE, 0, 0), start, 2), ((int(c[2][1]), int(c[2][4]), ra.NEW_CONTIG, 0, 0), ring, 3),
             ((a, b, int(c[2][0]), 0, 0), ring, 3), ((a, b, int(c[1][10]), 0, 0), start, 4), ((a, b, a, 1, 0), start, 4), ((a, b, -3, 0, 0), start, 5),
             ((a, b, ra.IN_PLACE, 2, 0), start, 5), ((a, b, ra.IN_PLACE, 0, -1), start, 5), ((a, N, -3, 0, 0), start, 1), ((b, a, -3, 0, 0), start, 2)]
    for e, st, want in cases:
        assert ra.check(st, e) == want, (e, want)
        out, s = ra.apply_host(st, e, ra.next_contig_id(st))
        assert s == want and (want == 0 or np.array_equal(out, st))
        assert (len(ra.touched_contigs(st, e)) > 0) == (want == 0)
    assert {w for _, _, w in cases} == {0, 1, 2, 3, 4, 5}


def test_no_ops_return_the_state(start):
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    nid = ra.next_contig_id(start)
    a, b = int(c[1][6]), int(c[1][15])
    for e in ((a, b, ra.IN_PLACE, 0, 0), (a, b, int(c[1][5]), 0, 0), (a, b, int(c[1][16]), 1, 0), (int(c[1][0]), b, int(c[1][16]), 1, 0),
              (a, int(c[1][-1]), int(c[1][5]), 0, 0), (a, a, ra.IN_PLACE, 0, 0)):
        out, s = ra.apply_host(start, e, nid)
        assert s == 0 and np.array_equal(out, start), e
    out, s = ra.apply_host(start, (int(c[5][0]), int(c[5][-1]), ra.NEW_CONTIG, 0, 0), nid)  # a whole contig: the same genome, another id
    assert s == 0 and (out[ra.F["id_c"]][c[5]] == nid).all()
    assert np.array_equal(ra.canonical(out), ra.canonical(start))
    rest = np.ones(17, bool)
    rest[ra.F["id_c"]] = False
    assert np.array_equal(out[rest], start[rest])


def _random_edit(rng, state):
    from instagraal_amd import rearrange as ra

    N = state.shape[1]
    fb = int(rng.integers(N))
    bins = ra.contig_bins(state, state[ra.F["id_c"]][fb])
    p = int(state[ra.F["pos"]][fb])
    lb = int(bins[min(bins.size - 1, p + int(rng.integers(0, 12)))])
    kind = int(rng.integers(6))
    anchor = ra.IN_PLACE if kind == 0 else ra.NEW_CONTIG if kind == 1 else int(rng.integers(N))
    return (fb, lb, anchor, int(rng.integers(2)), int(rng.integers(2)))


def test_invariants_behind_200_chained_random_edits(start):
    from instagraal_amd import rearrange as ra

    rng = np.random.default_rng(20)
    st, done, kinds = start.copy(), 0, set()
    while done < 200:
        e = _random_edit(rng, st)
        out, s = ra.apply_host(st, e, ra.next_contig_id(st))
        if s:
            assert np.array_equal(out, st)
            continue
        for k in ("len_bp", "sub_len", "rep", "activ", "id_d", "id"):
            assert np.array_equal(out[ra.F[k]], st[ra.F[k]])
        _assert_consistent(out)
        st, done = out, done + 1
        kinds.add((min(e[2], 0), e[3], e[4]))
    assert len(kinds) >= 8 and len(np.unique(st[ra.F["id_c"]])) != len(SIZES)


def _planted(start):
    """the six kinds of planted error on the true genome: name -> edit"""
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    a, b = int(c[1][6]), int(c[1][15])
    return dict(inversion=(a, b, ra.IN_PLACE, 0, 1), within=(a, b, int(c[1][40]), 0, 0), to_head=(a, b, int(c[2][0]), 1, 0), to_tail_flipped=(a, b, int(c[2][-1]), 0, 1),
                to_tail=(a, b, int(c[3][-1]), 0, 0), excision=(a, b, ra.NEW_CONTIG, 0, 0), split=(int(c[1][30]), int(c[1][-1]), ra.NEW_CONTIG, 0, 0))


def test_every_planted_error_lowers_the_likelihood(start, score):
    from instagraal_amd import rearrange as ra

    _, base = score(start)
    for name, e in _planted(start).items():
        st, s = ra.apply_host(start, e, ra.next_contig_id(start))
        assert s == 0
        _, like = score(st)
        print("%-16s %+.2f" % (name, like - base))
        assert like < base, (name, like - base)


def test_no_ops_score_exactly_zero_and_disjoint_deltas_add(start, score):
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    nid = ra.next_contig_id(start)
    base, _ = score(start)
    st, _ = ra.apply_host(start, (int(c[1][6]), int(c[1][15]), int(c[1][5]), 0, 0), nid)
    assert score(st)[0] == base
    e1 = (int(c[1][6]), int(c[1][15]), ra.IN_PLACE, 0, 1)          # touches the 59-bin contig
    e2 = (int(c[0][6]), int(c[0][15]), int(c[2][-1]), 0, 1)        # the 154- and the 57-bin contigs
    assert not set(ra.touched_contigs(start, e1)) & set(ra.touched_contigs(start, e2))
    s1, _ = ra.apply_host(start, e1, nid)
    s2, _ = ra.apply_host(start, e2, nid)
    s12, _ = ra.apply_host(s1, e2, nid)
    l1, l2, l12 = score(s1)[0], score(s2)[0], score(s12)[0]
    assert all(l12[k] - base[k] == (l1[k] - base[k]) + (l2[k] - base[k]) for k in range(3))
    assert l1 != base and l2 != base


def _reports_host(state, prob, n=20, window=64, orientation_window=8):
    """the tables ``rearrange.propose`` takes, from the reports' host rules (``orientation_support.support_host`` without the model
    part, ``segment_placement.support_host``) on ``state``: the tables by ``fill_tables``, the genome order as
    ``Context.contact_map_order`` states it (contigs by ascending canonical id, sub-fragments by rank)
    -> (inverted, [misplaced at block level, misplaced at scaffold level])"""
    from instagraal_amd import orientation_support as osup, rearrange as ra, segment_placement as sp
    from instagraal_amd.junction_profile import contig_runs

    F = ra.F
    st = ra.canonical(state)
    sub = prob.np_sub_frags_2_frags
    row, col, cnt = prob.coo_row, prob.coo_col, prob.coo_cnt
    parent = sub["x"].astype(np.int64)
    dist, stot, contig, rank, _, placed = fill_tables(st, sub)
    order = np.nonzero(placed)[0]
    order = order[np.lexsort((rank[order], contig[order]))]
    position = np.full(parent.size, -1, np.int64)
    position[order] = np.arange(order.size)
    at = parent[order]
    blocks = osup.block_segments(order, parent, st[F["id_c"]], st[F["ori"]], st[F["id_d"]], prob.S_o_A_frags["id_c"], prob.S_o_A_frags["pos"])
    res = osup.support_host(dist, stot, contig, placed, position, row, col, cnt, blocks["first"], blocks["last"], orientation_window)
    res.update(osup.derived(res))
    res["first_bin"], res["last_bin"] = at[res["first"]], at[res["last"]]
    res["scaffold"] = st[F["id_c"]].astype(np.int64)[res["first_bin"]]
    inverted = osup.inverted_segments(res, n)
    members, start, length = contig_runs(contig, position)
    scaf = sp.scaffold_segments(order, np.repeat(start, length), np.repeat(start + length, length), np.asarray(stot)[members] != 0)
    misplaced = []
    for first, last in ((blocks["first"], blocks["last"]), (scaf["first"], scaf["last"])):
        r = sp.support_host(stot, contig, placed, position, row, col, cnt, first, last, window)
        r.update(sp.densities(r))
        r.update(sp.sites_for_people(r, order, parent, st[F["id_c"]]))
        misplaced.append(sp.misplaced_segments(r, n))
    return inverted, misplaced


def test_the_proposals_contain_both_undos_and_one_round_picks_them(prob, start, score):
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    nid = ra.next_contig_id(start)
    a1, b1 = int(c[1][6]), int(c[1][15])
    a2, b2 = int(c[0][6]), int(c[0][15])
    st, s = ra.apply_host(start, (a1, b1, ra.IN_PLACE, 0, 1), nid)
    assert s == 0
    st, s = ra.apply_host(st, (a2, b2, int(c[2][-1]), 0, 1), nid)
    assert s == 0
    inverted, misplaced = _reports_host(st, prob)
    assert (int(inverted[0]["first_bin"]), int(inverted[0]["last_bin"])) == (b1, a1)  # the planted block ranks first
    edits = ra.propose(st, inverted, misplaced, n=20, window=64)
    have = {tuple(int(x) for x in e) for e in edits}
    undo1 = (b1, a1, ra.IN_PLACE, 0, 1)
    undo2 = (b2, a2, int(c[0][16]), 1, 1)  # (a boundary is proposed once: in front of the bin behind it)
    assert undo1 in have and undo2 in have and (b2, a2, int(c[0][5]), 0, 1) not in have
    assert all(ra.check(st, e) == 0 for e in edits)
    print("%d proposals" % edits.shape[0])
    _, base = score(st)
    delta = np.array([score(ra.apply_host(st, e, nid)[0])[1] - base for e in edits])
    take = ra.polish_round(delta, edits, st, 0.0)
    assert len(take) == 2 and {tuple(int(x) for x in edits[i]) for i in take} == {undo1, undo2}
    out = st
    for i in take:
        out, s = ra.apply_host(out, edits[i], nid)
        assert s == 0
    assert np.array_equal(ra.canonical(out), ra.canonical(start))
    assert abs(float(delta[take].sum()) - (score(start)[1] - base)) < 1e-6 * abs(base)


def test_the_log_file(tmp_path):
    from instagraal_amd import rearrange as ra

    log = [dict(round=0, edit=np.array([3, 9, -2, 0, 1], np.int32), delta=12.5, likelihood=-100.25), dict(round=1, edit=(1, 2, 7, 1, 0), delta=0.5, likelihood=-99.75)]
    assert ra.write_polish_log(str(tmp_path / "polish.txt"), log) == 2
    lines = open(str(tmp_path / "polish.txt")).read().splitlines()
    assert lines[0] == "# " + " ".join(ra.LOG_COLUMNS) and lines[1] == "0 3 9 -2 0 1 12.5 -100.25" and lines[2] == "1 1 2 7 1 0 0.5 -99.75" and lines[3] == "# applied=2"
