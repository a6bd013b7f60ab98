"""The slice kernel walks every touched contig's CSR rows ONCE per move slot, whatever the number of candidates that read them
(k_slice, ig_kernels_score.cuh): crafted candidate lists on the ``small`` shape against the oracle run live (DET mode).

The lists are chosen on the CPU from the ORACLE's genome, move by move, so that every kind of slot occurs -- and the kinds are
counted from that genome, so a case that silently is not produced fails the test:

* all five candidates in the focal contig / none of them;
* two and three candidates in the same OTHER contig;
* a candidate in the focal contig whose slice window spans the whole contig (``CandMeta.windowed`` cleared) and one whose
  window does not;
* a focal contig of one bin;
* all of these interleaved in ONE ``step_sampler_batch`` call, so that slots kept over a launch and slots scored again occur.

Checked bit for bit: the 6-tuple of every move (batch path and one call per move), the 24 x C scores of every move
(``keep_all_scores``, one call per move), the genome, the maintained exact likelihood; and the two counters of
``batch_stats()``: ``slice_contacts_walked`` is the sum of the CSR row lengths over the DISTINCT touched contigs of a slot
(computed here from ``download_state()`` and the contacts), at most ``slice_contacts_walked_per_candidate``.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CAND = 5


def _hip(prob):
    from instagraal_amd.sampler import sampler as hip_sampler

    s = hip_sampler(**prob.sampler_kwargs(), device_id=0)
    s.set_param_simu(prob.params)
    s.eval_likelihood_init()
    return s


class _Genome:
    """what a slot's planes depend on, from a 17 x N state (hip_lib.FRAG_FIELDS order) and the contacts"""

    def __init__(self, prob, slice_nb):
        from instagraal_amd import hip_lib

        self.F = {k: i for i, k in enumerate(hip_lib.FRAG_FIELDS)}
        M = prob.n_sub_frags
        parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
        row_len = np.bincount(prob.coo_row, minlength=M)  # the library's CSR: strict upper triangle, one row per sub-fragment
        self.frag_rows = np.bincount(parent, weights=row_len, minlength=prob.n_frags).astype(np.int64)
        self.slice_nb = int(slice_nb)

    def contig_rows(self, soa, cid):
        return int(self.frag_rows[soa[self.F["id_c"]] == cid].sum())

    def windowed(self, soa, a, b):
        """CandMeta.windowed of candidate b of focal fragment a (k_gather; the slice windows of the reference's slice_sp_mat)"""
        g = lambda k, f: int(soa[self.F[k]][f])  # noqa: E731
        if g("id_c", a) != g("id_c", b) or g("circ", a) != 0:
            return False
        SLA = g("sub_l_cont", a)
        pos = lambda f: max(0, g("sub_pos", f) if g("ori", f) == 1 else g("sub_pos", f) - g("sub_len", f))  # noqa: E731
        up_fa, down_fa = max(0, pos(a) - self.slice_nb - g("sub_len", a)), min(SLA - 1, pos(a) + self.slice_nb + g("sub_len", a))
        up_fb, down_fb = max(0, pos(b) - g("sub_len", b)), min(SLA - 1, pos(b) + g("sub_len", b))
        return not ((up_fa == 0 and down_fa == SLA - 1) or (up_fb == 0 and down_fb == SLA - 1))

    def slot(self, soa, a, cands):
        """-> (kinds of this slot, contacts in the rows walked once per touched contig, ... once per candidate)"""
        idc = soa[self.F["id_c"]]
        cA = int(idc[a])
        cB = [int(idc[b]) for b in cands]
        same = [c == cA for c in cB]
        others = [c for c in cB if c != cA]
        dup = max([others.count(c) for c in set(others)], default=0)
        rows_a = self.contig_rows(soa, cA)
        walked = rows_a + sum(self.contig_rows(soa, c) for c in set(others))
        per_cand = (rows_a if others else 0) + sum(rows_a if sm else self.contig_rows(soa, c) for sm, c in zip(same, cB))
        kinds = set()
        if all(same) and len(cands) == N_CAND:
            kinds.add("all_same")
        if not any(same):
            kinds.add("none_same")
        if dup == 2:
            kinds.add("dup2")
        if dup == 3:
            kinds.add("dup3")
        for b, sm in zip(cands, same):
            if sm:
                kinds.add("same_windowed" if self.windowed(soa, a, b) else "same_whole")
        if int(soa[self.F["l_cont"]][a]) == 1:
            kinds.add("one_bin")
        return kinds, walked, per_cand


def _pick(rng, soa, F, kind, popped):
    """(focal fragment, candidates) of the wanted kind on this genome; the caller counts what it really is"""
    idc, pos, L, SL = soa[F["id_c"]], soa[F["pos"]], soa[F["l_cont"]], soa[F["sub_l_cont"]]
    contigs = {int(c): np.nonzero(idc == c)[0] for c in np.unique(idc)}
    by_len = sorted(contigs, key=lambda c: -len(contigs[c]))
    long_c = [c for c in by_len if len(contigs[c]) >= 8]
    take = lambda c, n, skip=(): [int(x) for x in rng.permutation([f for f in contigs[c] if f not in skip])[:n]]  # noqa: E731

    def others(cA, n):
        return [int(c) for c in rng.permutation([c for c in long_c if c != cA])[:n]]

    if kind == "one_bin":
        a = int(next(f for f in popped if L[f] == 1))
        return a, [take(c, 1)[0] for c in others(int(idc[a]), N_CAND)]
    if kind == "same_windowed":  # the first bin of the longest contig and bins at its far end: the window around A stops short of them
        c = max(contigs, key=lambda c: int(SL[contigs[c][0]]))
        fr = contigs[c][np.argsort(pos[contigs[c]])]
        return int(fr[1]), [int(fr[-2]), int(fr[-4]), int(fr[len(fr) // 2])] + [take(x, 1)[0] for x in others(c, 2)]
    if kind == "same_whole":  # a contig shorter than the window
        c = next(c for c in reversed(by_len) if 4 <= len(contigs[c]) and int(SL[contigs[c][0]]) < 150)
        a = take(c, 1)[0]
        return a, take(c, 2, skip=(a,)) + [take(x, 1)[0] for x in others(c, 3)]
    cA = int(rng.choice(long_c))
    a = take(cA, 1)[0]
    if kind == "all_same":
        return a, take(cA, N_CAND, skip=(a,))
    if kind == "none_same":
        return a, [take(c, 1)[0] for c in others(cA, N_CAND)]
    x, y, z = others(cA, 3)
    if kind == "dup2":
        return a, take(x, 2) + take(y, 1) + take(z, 1) + take(cA, 1, skip=(a,))
    if kind == "dup3":
        return a, take(x, 3) + take(y, 2)
    raise AssertionError(kind)


def _oracle_plan(prob):
    """the oracle alone: three forced pop-outs, then moves whose lists are chosen from its genome and whose kinds are counted
    from its genome -> (forced (a, b, op), moves (a, cands, rows walked, rows walked per candidate), wanted (6-tuple, scores),
    final genome, slots by kind)"""
    from instagraal_amd import sampler as hs
    from oracle import oracle_lib as ol
    from oracle.sampler_oracle import OracleSampler

    ol.build()
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(prob.params)
    o.eval_likelihood_init()
    slice_nb = hs.LIST_SIZE[: hs.N_INSERT_BLOCKS].max() * np.int32(np.round(prob.S_o_A_frags["sub_len"].mean()) + 1)  # CL:418-420
    gen = _Genome(prob, slice_nb)
    F = gen.F
    # three bins popped out of long contigs (CL:2094-2151): contigs of ONE bin to start moves from
    rng = np.random.RandomState(3)
    idc0 = prob.S_o_A_frags["id_c"]
    forced = []
    for c in np.argsort(np.bincount(idc0))[::-1][:3]:
        fr = np.nonzero(idc0 == c)[0]
        a, b = int(fr[len(fr) // 2]), int(fr[2])
        max_id = o.modify_gl_cuda_buffer(a, o.dt)
        o.test_copy_struct(a, b, 0, max_id)
        o.modify_gl_cuda_buffer(a, o.dt)
        forced.append((a, b, 0))
    popped = [f[0] for f in forced]
    start = o.gpu_vect_frags.soa17()
    plan = ["all_same", "none_same", "dup2", "dup3", "same_whole", "same_windowed", "one_bin"] * 6
    plan = [plan[i] for i in rng.permutation(len(plan))]
    moves, want, count = [], [], {}
    for kind in plan:
        soa = o.gpu_vect_frags.soa17()
        if kind == "one_bin" and not any(soa[F["l_cont"]][f] == 1 for f in popped):
            kind = "none_same"  # (every popped bin was put back by an earlier move)
        a, cands = _pick(rng, soa, F, kind, popped)
        cands = sorted(set(cands))
        assert a not in cands and 1 <= len(cands) <= N_CAND
        kinds, walked, per_cand = gen.slot(soa, a, cands)
        for k in kinds:
            count[k] = count.get(k, 0) + 1
        b = o.step_sampler(a, len(cands), o.dt, candidates=cands)
        moves.append((a, cands, walked, per_cand))
        want.append(((float(b[0]), float(b[1]), int(b[2]), int(b[3]), float(b[4]), int(b[5])), o.all_scores.copy()))
    print("slots by kind:", count)
    for k in ("all_same", "none_same", "dup2", "dup3", "same_whole", "same_windowed", "one_bin"):
        assert count.get(k, 0) >= 2, (k, count)  # every crafted case occurs
    return gen, forced, start, moves, want, o.gpu_vect_frags.soa17(), float(o.gpu_curr_likelihood_nz[0])


def test_slice_planes_crafted_candidates_against_the_oracle():
    from instagraal_amd import synth

    prob = synth.make_problem(*synth.CONFIGS["small"])
    gen, forced, start, moves, want, final, _ = _oracle_plan(prob)
    s1, sb = _hip(prob), _hip(prob)  # one library call per move (all scores); the batch path
    for s in (s1, sb):
        for a, b, op in forced:
            s.test_copy_struct(a, b, op)
        assert np.array_equal(s.gpu_vect_frags.copy_from_gpu().soa17(), start)

    def exact(s):
        sums, _ = s.ctx.debug_globals()
        _, _, limbs = s.ctx.full_likelihood(0)
        return int(sums[0]) == int(limbs[0]) and int(sums[1]) == int(limbs[1])

    # ---- one library call per move: scores, records, and the rows walked by each move's one slot
    n_less = 0
    for (a, cands, _, _), (tup, scores) in zip(moves, want):
        kinds, walked, per_cand = gen.slot(s1.ctx.download_state(), a, cands)
        st0 = s1.ctx.batch_stats()
        r = s1.step_sampler(a, len(cands), candidates=cands)
        st1 = s1.ctx.batch_stats()
        assert np.array_equal(s1.all_scores, scores), (a, cands)
        assert (float(r[0]), float(r[1]), int(r[2]), int(r[3]), float(r[4]), int(r[5])) == tup, (a, cands, r, tup)
        d_w = st1["slice_contacts_walked"] - st0["slice_contacts_walked"]
        d_p = st1["slice_contacts_walked_per_candidate"] - st0["slice_contacts_walked_per_candidate"]
        assert (d_w, d_p) == (walked, per_cand), (a, cands, kinds, d_w, walked, d_p, per_cand)
        assert d_w <= d_p
        n_less += int(d_w < d_p)
    assert n_less >= len(moves) // 2  # (most slots have two candidates in one contig)
    assert np.array_equal(s1.gpu_vect_frags.copy_from_gpu().soa17(), final)
    assert exact(s1)

    # ---- all of them in one call of the batch path
    cand_arr = np.full((len(moves), N_CAND), -1, np.int32)
    for i, (_, cands, _, _) in enumerate(moves):
        cand_arr[i, : len(cands)] = cands
    st0 = sb.ctx.batch_stats()
    res = sb.step_sampler_batch(np.array([m[0] for m in moves], np.int32), N_CAND, candidates=cand_arr)
    st1 = sb.ctx.batch_stats()
    for r, (tup, _), m in zip(res, want, moves):
        got = (float(r["o"]), float(r["dist"]), int(r["op_sampled"]), int(r["id_f_sampled"]), float(np.float32(r["mean_len"])), int(r["n_contigs"]))
        assert got == tup, (m[:2], got, tup)
    assert np.array_equal(sb.gpu_vect_frags.copy_from_gpu().soa17(), final)
    assert exact(sb)
    n_batches = st1["batches"] - st0["batches"]
    assert 1 < n_batches <= len(moves), n_batches  # more than one launch chain: slots behind a move that changed their contigs were scored again
    d_w = st1["slice_contacts_walked"] - st0["slice_contacts_walked"]
    d_p = st1["slice_contacts_walked_per_candidate"] - st0["slice_contacts_walked_per_candidate"]
    # every slot is sliced on the genome its move is decided on (a slot scored again adds the walk of its first scoring)
    assert sum(m[2] for m in moves) <= d_w <= d_p, (sum(m[2] for m in moves), d_w, d_p)
    for s in (s1, sb):
        s.free_gpu()
