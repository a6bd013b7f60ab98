"""GPU tests of the segment edits (ig_edit_score, ig_edit_state, ig_edit_apply; sampler.score_rearrangements, apply_rearrangement,
polish) against the rule's host statement (instagraal_amd.rearrange.apply_host) and the oracle's likelihood (DET) on the rule's
states.  Every comparison is exact: the 17 arrays byte for byte, the five sums as integers, nz and z as the same doubles."""
import copy
import os

import numpy as np
import pytest

from test_hip_parity import make_ctx
from test_hip_placement_support import _sampler

pytestmark = pytest.mark.gpu


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


def _cases(start):
    """the fixed list: every kind of edit the rule knows on the contigs of 154 / 59 / 57 / 21 / 6 / 3 bins, and the refusals"""
    from instagraal_amd import rearrange as ra

    c = _contigs(start)
    N = start.shape[1]
    a, b = int(c[1][6]), int(c[1][15])
    IN, NEW = ra.IN_PLACE, ra.NEW_CONTIG
    one = np.nonzero(start[ra.F["sub_len"]] == 1)[0]
    assert one.size  # a bin with one sub-fragment
    o = int(one[0])
    edits = [
        (a, b, int(c[1][40]), 0, 0), (a, b, int(c[1][40]), 1, 1),                      # forward inside the contig
        (int(c[1][30]), int(c[1][39]), int(c[1][3]), 1, 0), (int(c[1][30]), int(c[1][39]), int(c[1][3]), 0, 1),  # backward
        (a, b, int(c[2][0]), 1, 0), (a, b, int(c[2][0]), 1, 1),                        # another contig's head
        (a, b, int(c[2][-1]), 0, 0), (a, b, int(c[2][-1]), 0, 1),                      # its tail
        (a, b, int(c[2][20]), 0, 0), (a, b, int(c[2][20]), 1, 1),                      # its interior, both sides
        (a, b, IN, 0, 0), (a, b, IN, 0, 1), (a, b, IN, 1, 1),                          # in place
        (a, b, NEW, 0, 0), (int(c[1][0]), int(c[1][9]), NEW, 0, 1), (int(c[1][40]), int(c[1][-1]), NEW, 1, 0),  # excision: middle, prefix, suffix
        (int(c[4][0]), int(c[4][-1]), int(c[3][0]), 1, 0), (int(c[4][0]), int(c[4][-1]), int(c[3][0]), 1, 1),   # a whole contig onto a head
        (int(c[4][0]), int(c[4][-1]), int(c[3][-1]), 0, 0), (int(c[4][0]), int(c[4][-1]), int(c[3][-1]), 0, 1),  # ... onto a tail
        (int(c[5][0]), int(c[5][-1]), NEW, 0, 0), (int(c[5][0]), int(c[5][-1]), NEW, 0, 1),                     # a whole contig as a new one
        (int(c[0][77]), int(c[0][77]), int(c[3][4]), 0, 1), (int(c[0][77]), int(c[0][77]), IN, 0, 1),           # one bin
        (o, o, IN, 0, 1), (o, o, int(c[3][4]) if o not in c[3] else int(c[2][4]), 1, 0),                        # a bin with one sub-fragment
        (int(c[5][0]), int(c[5][1]), int(c[4][2]), 0, 0), (int(c[5][1]), int(c[5][2]), int(c[5][0]), 1, 1),     # the 3-bin contig left with one bin
        (a, b, int(c[1][5]), 0, 0), (a, b, int(c[1][16]), 1, 0), (int(c[1][0]), b, int(c[1][16]), 1, 0),        # no-ops: next to its own place
        (a, int(c[1][-1]), int(c[1][5]), 0, 0),
        (-1, b, IN, 0, 0), (a, N, IN, 0, 0), (a, b, N, 0, 0), (a, int(c[0][3]), IN, 0, 0), (b, a, IN, 0, 0),    # refused: 1, 1, 1, 2, 2
        (a, b, int(c[1][10]), 0, 0), (a, b, a, 1, 0), (a, b, -3, 0, 0), (a, b, IN, 2, 0), (a, b, IN, 0, 2),     # 4, 4, 5, 5, 5
    ]
    noop = [10, 20, 28, 29, 30, 31]
    return np.asarray(edits, np.int32), noop


def _oracle_sums(o, ol, state):
    for i, k in enumerate(ol.FRAG_FIELDS):
        getattr(o.gpu_vect_frags, k)[:] = state[i]
    o.fill_dist_single()
    o.approx_single_likelihood_on_zeros(nuis=True)
    hi, lo = ol.last_limbs()
    zq, ni = (int(hi[0]) << 32) + int(lo[0]), int(o.gpu_n_vals_intra[0])
    o._full_nz(o.gpu_curr_likelihood_nz, o.param_simu)
    hi, lo = ol.last_limbs()
    return ((int(hi[0]) << 32) + int(lo[0]), zq, ni)


def _ints(limbs):
    h = [int(x) for x in limbs]
    return ((h[0] << 32) + h[1], (h[2] << 32) + h[3], h[4])


def test_state_parity_on_the_fixed_list(tiny):
    from instagraal_amd import rearrange as ra

    start = _start(tiny)
    edits, noop = _cases(start)
    ctx = make_ctx(tiny)
    nid = ra.next_contig_id(start)  # (a fresh upload keeps the caller's ids: the internal ids are the table's)
    seen = set()
    for i, e in enumerate(edits):
        want, ws = ra.apply_host(start, e, nid)
        got, gs = ctx.edit_state(e)
        assert gs == ws, (i, e.tolist(), gs, ws)
        bad = [k for k in range(17) if not np.array_equal(got[k], want[k])]
        assert not bad, (i, e.tolist(), [ra.FRAG_FIELDS[k] for k in bad])
        if i in noop:
            assert gs == 0 and np.array_equal(np.delete(got, ra.F["id_c"], 0), np.delete(start, ra.F["id_c"], 0))
        seen.add(gs)
    assert seen == {0, 1, 2, 4, 5}  # (3, a ring: test_a_ring_is_refused)
    assert np.array_equal(ctx.download_state(), ra.canonical(start))  # nothing was committed
    ctx.close()


def test_a_ring_is_refused(tiny):
    from instagraal_amd import rearrange as ra

    start = _start(tiny)
    c = _contigs(start)
    ring = start.copy()
    ring[ra.F["circ"]][c[2]] = 1
    ctx = make_ctx(tiny)
    ctx.upload_state(ring)
    for e in ((int(c[2][1]), int(c[2][4]), ra.NEW_CONTIG, 0, 0), (int(c[1][6]), int(c[1][15]), int(c[2][0]), 0, 0)):
        got, gs = ctx.edit_state(e)
        assert gs == 3 == ra.check(ring, e) and np.array_equal(got, ring)
        status, limbs = ctx.edit_apply(e)
        assert status == 3 and np.array_equal(limbs, ctx.full_likelihood()[2])
    st, _, _, _ = ctx.edit_score([(int(c[1][6]), int(c[1][15]), int(c[3][0]), 0, 0), (int(c[2][1]), int(c[2][4]), ra.IN_PLACE, 0, 1)])
    assert st.tolist() == [0, 3]
    assert np.array_equal(ctx.download_state(), ra.canonical(ring))
    ctx.close()


def _score_parity(prob, params, oracle_lib, edits, noop):
    from instagraal_amd import rearrange as ra
    from oracle.sampler_oracle import OracleSampler

    ol = oracle_lib
    start = _start(prob)
    nid = ra.next_contig_id(start)
    ctx = make_ctx(prob, params=params)
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(params)
    nz0, z0, base = ctx.full_likelihood()
    assert _ints(base) == _oracle_sums(o, ol, start)
    sd, ld, nzd, zd = ctx.edit_score(edits, 0)
    sw, lw, nzw, zw = ctx.edit_score(edits, 1)
    assert np.array_equal(sd, sw) and np.array_equal(ld, lw), np.argwhere(ld != lw)[:5].tolist()
    assert np.array_equal(nzd.view(np.uint64), nzw.view(np.uint64)) and np.array_equal(zd.view(np.uint64), zw.view(np.uint64))
    assert np.array_equal(ctx.full_likelihood()[2], base) and np.array_equal(ctx.download_state(), ra.canonical(start))
    for i, e in enumerate(edits):
        want, ws = ra.apply_host(start, e, nid)
        assert sd[i] == ws
        assert _ints(ld[i]) == _oracle_sums(o, ol, want), (i, e.tolist())
        if ws or i in noop:  # refused, or a no-op: exactly the sums of the current genome
            assert np.array_equal(ld[i], base) and nzd[i] == nz0 and zd[i] == z0
        fresh = make_ctx(prob, params=params)
        status, limbs = fresh.edit_apply(e)
        nz, z, full = fresh.full_likelihood()
        assert status == ws and np.array_equal(limbs, full) and np.array_equal(full, ld[i]), (i, e.tolist())
        assert nz == nzd[i] and z == zd[i]
        assert np.array_equal(fresh.download_state(), ra.canonical(want))
        fresh.close()
    ctx.close()


def test_score_parity_on_the_fixed_list(tiny, oracle_lib):
    edits, noop = _cases(_start(tiny))
    _score_parity(tiny, tiny.params, oracle_lib, edits, noop)


def test_score_parity_with_rare_operands(tiny, oracle_lib):
    """counts >= 256 and >= 1024 (as test_full_likelihood_rare_operands makes them), and slope = 0: the generic composition"""
    import scipy.sparse as sp

    prob = copy.deepcopy(tiny)
    cnt = prob.coo_cnt.copy()
    cnt[::7] *= 60
    cnt[::131] *= 400
    prob.coo_cnt = cnt
    M = prob.n_sub_frags
    prob.sub_csr = sp.csr_matrix((cnt, (prob.coo_row, prob.coo_col)), shape=(M, M), dtype=np.int32)
    prob.sub_csr.sort_indices()
    edits, noop = _cases(_start(prob))
    for params in (prob.params, dict(prob.params, slope=0.0)):
        _score_parity(prob, params, oracle_lib, edits, noop)


def test_chunking(tiny):
    start = _start(tiny)
    edits, _ = _cases(start)
    ctx = make_ctx(tiny)
    one = [ctx.edit_score(e[None, :], 0) for e in edits]
    for n in (1, 63, 64, 65, 130):
        rep = np.resize(edits, (n, 5))
        for form in (0, 1) if n in (1, 65) else (0,):
            s, l, nz, z = ctx.edit_score(rep, form)
            for i in range(n):
                w = one[i % len(edits)]
                assert s[i] == w[0][0] and np.array_equal(l[i], w[1][0]) and nz[i] == w[2][0] and z[i] == w[3][0], (n, form, i)
    # a chunk whose 64 edits all touch the 154-bin contig
    c = _contigs(start)[0]
    rng = np.random.default_rng(5)
    same = []
    for k in range(64):
        a = int(rng.integers(0, 140))
        b = a + int(rng.integers(0, 12))
        t = int(rng.integers(0, 154))
        same.append((int(c[a]), int(c[b]), -2 if a <= t <= b else int(c[t]), k & 1, (k >> 1) & 1))
    same = np.asarray(same, np.int32)
    s, l, nz, z = ctx.edit_score(same, 0)
    assert not s.any() and len({tuple(x) for x in l.tolist()}) > 32
    for i in range(64):
        w = ctx.edit_score(same[i:i + 1], 0)
        assert np.array_equal(l[i], w[1][0]) and nz[i] == w[2][0] and z[i] == w[3][0]
    assert np.array_equal(l, ctx.edit_score(same, 1)[1])
    s, l, nz, z = ctx.edit_score(np.zeros((0, 5), np.int32))
    assert s.size == 0 and l.shape == (0, 5)
    ms, ck0 = ctx.debug_edit_time(same, 0, n=2)
    ms1, ck1 = ctx.debug_edit_time(same, 1)
    assert ms.shape == (2, 6) and ck0 == ck1 and (ms[:, :5] > 0).all() and (ms[:, 5] == 0).all() and ms1[0, 5] > 0 and ms1[0, 3] == 0
    ctx.close()


def test_scoring_does_not_interfere_with_the_moves(tiny):
    from instagraal_amd import rearrange as ra

    start = _start(tiny)
    edits, _ = _cases(start)
    outs = []
    for between in (False, True):
        prob, s = _sampler("tiny", seed=21)
        frags = np.random.permutation(prob.n_frags)[:64].astype(np.int32)
        r1 = s.step_sampler_batch(frags[:32], 5).copy()
        if between:
            st = np.random.get_state()
            # the fixed list (mostly refused by now: the genome has moved on) and edits made for the genome of the moment
            now = s.ctx.download_state()
            c = [b for b in _contigs(now) if b.size >= 4]
            mine = [(int(b[1]), int(b[2]), ra.IN_PLACE, 0, 1) for b in c] + [(int(b[1]), int(b[-1]), int(c[0][0]), 1, k & 1) for k, b in enumerate(c[1:])]
            edits = np.concatenate([edits, np.asarray(mine, np.int32)])
            sc = s.score_rearrangements(edits)
            assert sc["status"].tolist() == [ra.check(now, e) for e in edits] and (sc["status"][-len(mine):] == 0).any() and (sc["delta"] != 0).any()
            assert np.array_equal(sc["limbs"], s.score_rearrangements(edits, form="whole")["limbs"])
            after = np.random.get_state()
            assert np.array_equal(st[1], after[1]) and st[2] == after[2]
        r2 = s.step_sampler_batch(frags[32:], 5).copy()
        outs.append((r1, r2, s.gpu_vect_frags.copy_from_gpu().soa17(), list(s.ctx.valid_insert()), np.random.get_state()[1].copy(), np.random.get_state()[2]))
        s.free_gpu()
    a, b = outs
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


def test_commit_three_edits_then_moves_against_the_oracle(oracle_lib):
    from instagraal_amd import rearrange as ra
    from oracle.sampler_oracle import OracleSampler

    ol = oracle_lib
    prob, s = _sampler("tiny", seed=22)
    start = _start(prob)
    c = _contigs(start)
    want = start
    three = [(int(c[1][6]), int(c[1][15]), ra.IN_PLACE, 0, 1), (int(c[0][6]), int(c[0][15]), int(c[2][-1]), 0, 1), (int(c[0][100]), int(c[0][120]), ra.NEW_CONTIG, 0, 0)]
    for e in three:
        sc = s.score_rearrangements([e])
        like = s.apply_rearrangement(e)
        want, status = ra.apply_host(want, e, ra.next_contig_id(want))
        assert status == 0 and like == sc["score"][0] and np.array_equal(s.last_edit_limbs, sc["limbs"][0])
        assert np.array_equal(s.gpu_vect_frags.soa17(), ra.canonical(want))
    assert s.n_contigs == 7 and list(s.ctx.valid_insert()) == [0] * 12
    before = s.ctx.download_state()
    with pytest.raises(ValueError):  # a refused edit changes nothing
        s.apply_rearrangement((int(c[1][6]), int(c[0][3]), ra.IN_PLACE, 0, 0))
    assert np.array_equal(s.ctx.download_state(), before)
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(prob.params)
    g = ra.canonical(want)
    for i, k in enumerate(ol.FRAG_FIELDS):
        getattr(o.gpu_vect_frags, k)[:] = g[i]
    o.gpu_id_contigs[:] = g[ra.F["id_c"]]
    o.gpu_list_valid_insert[:] = 0
    assert s.dist_inter_genome() == o.dist_inter_genome(o.gpu_vect_frags) > 0
    frags = np.random.permutation(prob.n_frags)[:150].astype(np.int32)
    st = np.random.get_state()
    res = s.step_sampler_batch(frags, 5)
    after = np.random.get_state()
    np.random.set_state(st)
    for t, (f, r) in enumerate(zip(frags, res)):
        b = o.step_sampler(int(f), 5, o.dt)
        row = (float(b[0]), float(b[1]), int(b[2]), int(b[3]), float(np.float32(b[4])), int(b[5]))
        got = (float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), float(np.float32(r["mean_len"])), int(r["n_contigs"]))
        assert got == row, (t, got, row)
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), o.gpu_vect_frags.soa17())
    assert np.array_equal(np.array(s.ctx.valid_insert(), np.int32), np.array(o.gpu_list_valid_insert, np.int32))
    s.free_gpu()


EVOLVED_SEED = 3


def _evolved_edits(state, blocks_first_bin, blocks_last_bin, seed=EVOLVED_SEED, n=30):
    """``n`` seeded edits over the blocks of an evolved genome: a block, and an anchor of every kind"""
    from instagraal_amd import rearrange as ra

    rng = np.random.default_rng(seed)
    N = state.shape[1]
    out = []
    for _ in range(n):
        k = int(rng.integers(len(blocks_first_bin)))
        kind = int(rng.integers(5))
        anchor = ra.IN_PLACE if kind == 0 else ra.NEW_CONTIG if kind == 1 else int(blocks_last_bin[int(rng.integers(len(blocks_last_bin)))]) if kind == 2 else int(rng.integers(N))
        out.append((int(blocks_first_bin[k]), int(blocks_last_bin[k]), anchor, int(rng.integers(2)), int(rng.integers(2))))
    return np.asarray(out, np.int32)


def test_an_evolved_genome(oracle_lib):
    """``small`` behind 300 HIP moves (20 contigs, blocks of several bins, flipped bins), 30 seeded edits over its blocks: with seed 3
    the rule alone finds 29 of them valid, 22 of them with a block of several bins, and one with its anchor inside the segment
    (checked on the CPU: the same 300 moves through the oracle, the blocks from the tables' host restatement).  The rule is given the
    state with the handle's INTERNAL contig ids -- gaps, and a next free id far beyond the largest in use --, so the ids are compared
    too.  Every valid edit is committed: the first, a new contig, on the evolved handle itself, the others on the same state put back
    with its internal ids."""
    from instagraal_amd import orientation_support as osup, rearrange as ra
    from oracle.sampler_oracle import OracleSampler

    ol = oracle_lib
    prob, s = _sampler("small", seed=12)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:300], 5)
    g = s.gpu_vect_frags.copy_from_gpu()
    canon = g.soa17()
    refused = (-1, 0, ra.IN_PLACE, 0, 0)
    live, st1 = s.ctx.edit_state(refused)  # (a refused edit: the current state as the handle holds it)
    nid = int(s.ctx.debug_globals()[1][1])
    ids = np.unique(live[ra.F["id_c"]])
    assert st1 == 1 and np.array_equal(ra.canonical(live), canon) and not np.array_equal(live[ra.F["id_c"]], canon[ra.F["id_c"]])
    assert ids.size < ids.max() + 1 < nid  # gaps, and ids used up by the moves
    order = s.ctx.contact_map_order().astype(np.int64)
    parent = s.np_sub_frags_2_frags["x"].astype(np.int64)
    blocks = osup.block_segments(order, parent, g.id_c, g.ori, g.id_d, s.np_init_id_c, s.np_init_pos)
    edits = _evolved_edits(live, blocks["first_bin"], blocks["last_bin"])
    want = [ra.apply_host(live, e, nid) for e in edits]
    valid = [i for i, (_, st) in enumerate(want) if st == 0]
    print("valid: %d of %d" % (len(valid), len(edits)))
    assert len(valid) >= 15
    sd, ld, nzd, zd = s.ctx.edit_score(edits, 0)
    sw, lw, nzw, zw = s.ctx.edit_score(edits, 1)
    assert sd.tolist() == [st for _, st in want] and np.array_equal(ld, lw) and np.array_equal(nzd, nzw) and np.array_equal(zd, zw)
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(prob.params)
    for i in valid:
        got, gs = s.ctx.edit_state(edits[i])
        assert gs == 0 and np.array_equal(got, want[i][0]), (i, edits[i].tolist())
        assert _ints(ld[i]) == _oracle_sums(o, ol, want[i][0]), (i, edits[i].tolist())
    new_first = sorted(valid, key=lambda i: edits[i][2] != ra.NEW_CONTIG)  # (stable: a new contig first)
    assert edits[new_first[0]][2] == ra.NEW_CONTIG
    for k, i in enumerate(new_first):
        if k:
            s.ctx.upload_state(live)  # (the same genome again, with the internal ids it had)
        status, limbs = s.ctx.edit_apply(edits[i])
        nz, z, full = s.ctx.full_likelihood()
        assert status == 0 and np.array_equal(limbs, ld[i]) and np.array_equal(full, ld[i]) and nz == nzd[i] and z == zd[i], (i, edits[i].tolist())
        assert np.array_equal(s.ctx.download_state(), ra.canonical(want[i][0])), (i, edits[i].tolist())
        if k == 0:  # on the evolved handle: the new contig took the next free id, which is used up
            assert np.array_equal(s.ctx.edit_state(refused)[0], want[i][0]) and int(s.ctx.debug_globals()[1][1]) == nid + 1
    s.free_gpu()


def test_polish_undoes_two_planted_errors():
    from instagraal_amd import rearrange as ra

    prob, s = _sampler("tiny", seed=23)
    start = _start(prob)
    c = _contigs(start)
    nid = ra.next_contig_id(start)
    planted, _ = ra.apply_host(start, (int(c[1][6]), int(c[1][15]), ra.IN_PLACE, 0, 1), nid)
    planted, _ = ra.apply_host(planted, (int(c[0][6]), int(c[0][15]), int(c[2][-1]), 0, 1), nid)
    true_like = float(np.ravel(s.likelihood_t)[0])
    s.ctx.upload_state(planted)
    s.eval_likelihood_init()
    s.gpu_vect_frags.copy_from_gpu()
    low = float(np.ravel(s.likelihood_t)[0])
    st = np.random.get_state()
    log = s.polish()
    assert len(log) == 2 and all(r["delta"] > 0 for r in log) and log[0]["delta"] >= log[1]["delta"]
    assert log[-1]["likelihood"] == float(s.likelihood_t) == true_like and abs(sum(r["delta"] for r in log) - (true_like - low)) < 1e-6 * abs(low)
    assert np.array_equal(ra.canonical(s.ctx.download_state()), ra.canonical(start))
    assert np.array_equal(s.gpu_vect_frags.soa17(), s.ctx.download_state()) and s.n_contigs == 6
    assert s.polish() == []
    after = np.random.get_state()
    assert np.array_equal(st[1], after[1]) and st[2] == after[2]
    s.free_gpu()
    # every entry of the log on a second sampler: the likelihood behind each apply is the one predicted for it on the state in front of it
    prob, s = _sampler("tiny", seed=23)
    s.ctx.upload_state(planted)
    for r in log:
        sc = s.score_rearrangements([r["edit"]])
        like = s.apply_rearrangement(r["edit"])
        assert sc["status"][0] == 0 and sc["delta"][0] > 0 and like == sc["score"][0] == r["likelihood"] and np.array_equal(s.last_edit_limbs, sc["limbs"][0])
    s.free_gpu()


def test_run_instagraal_polish_writes_the_log_and_the_outputs_describe_the_polished_genome(tmp_path):
    from instagraal_amd import rearrange as ra, synth
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    np.random.seed(17)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=1, bomb=True, polish=True,
                        save_segment_placements=True)
    folder = p2.simulation.output_folder
    s = p2.simulation.sampler
    lines = open(os.path.join(folder, "polish.txt")).read().splitlines()
    assert lines[0] == "# " + " ".join(ra.LOG_COLUMNS) and lines[-1].startswith("# applied=")
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert len(rows) == int(lines[-1].split("=")[1]) > 0 and all(float(r[6]) > 0 for r in rows)  # (the bombed one-cycle genome has edits to make)
    assert float(rows[-1][7]) == float(s.likelihood_t)
    assert all(float(a[7]) < float(b[7]) for a, b in zip(rows, rows[1:]))  # every applied edit raised the likelihood
    # info_frags.txt and the report were written behind the polish: they describe the genome the sampler holds now
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
        bins = ra.contig_bins(g.soa17(), cid)
        assert rows_c == [(int(g.id_d[f]), int(g.ori[f])) for f in bins], cid
    tail = [ln for ln in open(os.path.join(folder, "segment_placements.txt")).read().splitlines() if ln.startswith("# window=")][0]
    assert int(dict(kv.split("=") for kv in tail[2:].split())["n_guests"]) == s.segment_placement(level="block")["n_guests"]
    p2.simulation.release()
