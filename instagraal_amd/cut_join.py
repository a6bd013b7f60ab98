"""Cut and join scores: the likelihood change of EVERY cut of a linear contig and of EVERY link of two linear contigs, in the units of
the exact scorer (``ig_edit_score``), as far as it has a closed structure.  This module is the single definition of the rule (numpy;
the terms come from ``hip_lib.contact_terms_host`` / ``zero_terms_host``, which need no GPU); the device (``ig_cut_scores``,
``ig_join_scores_build``: csrc/ig_kernels_cutjoin.cuh) reproduces its integers byte for byte from one pass over the contacts each.

State, tables and parameter set 0 are the live ones.  "Linear" means ``circ == 0``; whether a contig is "placed" plays no part.  A
term is the quantised 64-bit value of ``eval_q`` (a stored contact) or ``zero_q`` (a sub-fragment); a sum is kept as two limbs, as
``k_edit_delta`` keeps them: hi = the sum of q >> 32, lo = the sum of (uint32) q; DELTA LIMBS are differences of such limbs
{nz hi, nz lo, z hi, z lo, intra pairs}, not normalised.  G(L) = sum over pos = 1 .. L - 1 of zero_q(pos, L) is the zero-pixel sum of
a linear contig of L sub-fragments.

CUT in front of bin f (f in a linear contig, prev[f] >= 0; the contig has L sub-fragments, j = sub_pos[f] of them in front of the
cut; the edit (f, last bin of the contig, NEW_CONTIG, 0, 0)):
  nz: over the stored contacts whose two sub-fragments lie in this contig in bins on different sides of the junction, eval_q as a trans
      pair minus eval_q under the live coordinates;   z: G(j) + G(L - j) - G(L);   intra pairs: -j (L - j).

LINK.  The linear contigs are numbered k = 0 .. K - 1 in ascending contig id; an end is (k, side), side 0 the head, 1 the tail.
Every pair a < b with a stored contact between them has four links (sa, sb), numbered 2 sa + sb.  The canonical edit of a link keeps
a and moves all of b: sa = tail: behind a's last bin (side 0), flipped where sb = tail; sa = head: in front of a's first bin (side 1),
flipped where sb = head.  In the state ``rearrange.apply_host`` leaves, under the tables ``k_fill_tables``' formula gives there:
  nz: over the contacts between a and b, eval_q (cis, ring-free) minus eval_q as a trans pair;
  z: G(La + Lb) - G(La) - G(Lb), equal for the four links;   intra pairs: La Lb.

``delta`` is a double: (nz + z) of the maintained sums plus the delta limbs minus (nz + z) of the maintained sums, each formed as
``ig_full_likelihood`` forms them (``likelihood_of_limbs``).

RELATION TO THE EXACT SCORER.  For the canonical edit E, the limbs of ``ig_edit_score(E)`` minus the maintained limbs are the CROSS
part above plus an INTERNAL part: the contacts with both ends on one side of a cut, or inside one of the two joined contigs.  Their
rank distance does not change; their f32 separation changes only because ``dist = (float) start_bp / 1000.0f + dfi`` is re-originated
(another rounding) and because a flipped contig mirrors its sub-fragments' reference points.  If every dist of every state involved is
exactly representable (every len_bp a multiple of 1 000, every watson / crick offset a multiple of 1/64 kb, contigs below 2^17 kb),
the internal part of a cut and of a link without a flip is zero, and that of a link with a flip is the delta of the in-place flip of
b, (first, last, IN_PLACE, 0, 1): translation invariance, once no sum rounds.  So the scores here RANK, and ``ig_edit_score`` decides.
"""
from __future__ import annotations

import numpy as np

from . import hip_lib
from .rearrange import F, NEW_CONTIG

HEAD, TAIL = 0, 1
SIDES = ("head", "tail")
LOG_E = 0.43429448190325182
CUT_DTYPE = np.dtype([("bin", np.int32), ("prev_bin", np.int32), ("contacts", np.int64), ("delta", np.float64), ("limbs", np.int64, (5,)), ("edit", np.int32, (5,))])
LINK_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("sa", np.int32), ("sb", np.int32), ("bin_a", np.int32), ("bin_b", np.int32), ("contacts", np.int64),
                       ("delta", np.float64), ("limbs", np.int64, (5,)), ("edit", np.int32, (5,))])
CUT_COLUMNS = ("bin", "prev_bin", "contacts", "delta", "first_bin", "last_bin", "anchor", "side", "flip")
LINK_COLUMNS = ("contig_a", "contig_b", "end_a", "end_b", "bin_a", "bin_b", "contacts", "delta", "first_bin", "last_bin", "anchor", "side", "flip")


class Problem:
    """what the rule reads besides the state: the sub-fragment table (parent bin, watson and crick offsets in kb, index in the bin),
    the stored contacts (row, col, count), the eight parameters in the order of ig_params, the mean sub-fragment length in kb"""

    def __init__(self, sub, row, col, cnt, params8, mean_kb):
        self.parent = np.asarray(sub["x"]).astype(np.int64)
        self.wat, self.cri = np.asarray(sub["y"], np.float32), np.asarray(sub["z"], np.float32)
        self.w = np.asarray(sub["w"]).astype(np.int64)
        self.row, self.col, self.cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int32)
        self.params = np.ascontiguousarray(params8, np.float32)
        self.mean_kb = np.float32(mean_kb)
        self.M = int(self.parent.size)
        self._G, self._T = {}, None

    @classmethod
    def of(cls, prob, params=None):
        """from a ``synth.SynthProblem`` (``params``: a dict, default the problem's)"""
        from .sampler import PARAM_NAMES

        p = prob.params if params is None else params
        return cls(prob.np_sub_frags_2_frags, prob.coo_row, prob.coo_col, prob.coo_cnt, [np.float32(p[k]) for k in PARAM_NAMES],
                   np.float32(prob.S_o_A_sub_frags["len_bp"].mean() / 1000.0))

    # ---- the terms
    def terms(self, s, d, trans, cnt):
        return hip_lib.contact_terms_host(self.params, self.mean_kb, s, d, trans, cnt)

    def trans_terms(self, cnt):
        return self.terms(np.zeros(np.shape(cnt), np.float32), 0, 1, cnt)

    def zero_terms(self, pos, length):
        return hip_lib.zero_terms_host(self.params, self.mean_kb, pos, length)

    # ---- G
    def pstar(self):
        """the first rank p >= 1 whose separation (float) p x mean_kb is not below d_max, M + 1: none up to M"""
        s = np.arange(1, self.M + 1, dtype=np.int64).astype(np.float32) * self.mean_kb
        out = np.nonzero(~(s < self.params[5]))[0]
        return int(out[0]) + 1 if out.size and self.mean_kb > 0 else self.M + 1

    def G_enum(self, L):
        """G(L) by enumeration -> (hi, lo)"""
        return limb_sum(self.zero_terms(np.arange(1, max(int(L), 1), dtype=np.int32), int(L)))

    def G(self, L):
        """G(L) -> (hi, lo): the ranks below p* enumerated, the others from the prefix sums of quantize(-(v_inter k)), which do not
        depend on L"""
        L = int(L)
        if L not in self._G:
            ps = self.pstar()
            hi, lo = limb_sum(self.zero_terms(np.arange(1, max(min(L, ps), 1), dtype=np.int32), L))
            if L > ps:
                if self._T is None:  # T[n] = the limbs of the terms at L - pos = 1 .. n: zero_q at a rank beyond p* is just that
                    k = np.arange(0, self.M + 2, dtype=np.int64)
                    q = self.zero_terms(np.full(k.size, ps, np.int32), (ps + k).astype(np.int32))
                    q[0] = 0
                    self._T = (np.cumsum(q >> 32), np.cumsum(q & 0xFFFFFFFF))
                hi, lo = hi + int(self._T[0][L - ps]), lo + int(self._T[1][L - ps])
            self._G[L] = (hi, lo)
        return self._G[L]


def limb_sum(q):
    """the limbs of the sum of the quantised terms ``q`` -> (hi, lo), Python integers"""
    q = np.asarray(q, np.int64)
    return int((q >> 32).sum()), int((q & 0xFFFFFFFF).sum())


def limb_diff(q1, q0):
    """per term: the limbs of q1 minus the limbs of q0 -> (hi, lo) int64 arrays"""
    q1, q0 = np.asarray(q1, np.int64), np.asarray(q0, np.int64)
    return (q1 >> 32) - (q0 >> 32), (q1 & 0xFFFFFFFF) - (q0 & 0xFFFFFFFF)


def tables(state, P, sbp=None, spos=None, ori=None):
    """numpy float32 restatement of ``k_fill_tables`` -> (dist f32 [M], rank int64 [M]); ``sbp``, ``spos``, ``ori``: per bin, default
    the state's start_bp, sub_pos, ori"""
    st = np.asarray(state)
    f = P.parent
    sbp = st[F["start_bp"]] if sbp is None else sbp
    spos = st[F["sub_pos"]] if spos is None else spos
    ori = st[F["ori"]] if ori is None else ori
    return coords(P, np.arange(P.M), sbp[f], spos[f], st[F["sub_len"]][f], ori[f])


def coords(P, s, sbp, spos, sl, ori):
    """the coordinates ``k_fill_tables`` gives the sub-fragments ``s`` of bins that start at ``sbp`` / ``spos`` (``sl`` sub-fragments)
    with orientation ``ori`` -> (dist f32, rank int64)"""
    fwd = np.asarray(ori) == 1
    dfi = np.where(fwd, P.wat[s], P.cri[s]).astype(np.float32)
    dist = (np.asarray(sbp).astype(np.float32) / np.float32(1000.0) + dfi).astype(np.float32)
    rank = np.where(fwd, np.asarray(spos, np.int64) + P.w[s], np.asarray(spos, np.int64) + (np.asarray(sl, np.int64) - 1) - P.w[s])
    return dist, rank.astype(np.int64)


def cis_terms(P, dist, rank, i, j, cnt):
    """eval_q of the contacts (i, j) as cis pairs of a linear contig under the coordinates (dist, rank) of their ends"""
    di, ri = dist[0], rank[0]
    dj, rj = dist[1], rank[1]
    return P.terms(np.abs(di - dj).astype(np.float32), np.abs(ri - rj), 0, cnt)


def likelihood_of_limbs(h, M, v_inter):
    """(nz, z) of five limbs as ``ig_full_likelihood`` forms them (csrc/ig_host_upload.inc), operation for operation"""
    def acc(hi, lo):
        return float(hi + (lo >> 32)) + float(lo & 0xFFFFFFFF) * (1.0 / 4294967296.0)

    h = [int(x) for x in h]
    n_tot_pxl = float(M) * (float(M) - 1.0) / 2.0
    val_intra = acc(h[2], h[3]) * LOG_E
    val_inter = LOG_E * (n_tot_pxl - float(h[4])) * -1.0 * float(np.float32(v_inter))
    return acc(h[0], h[1]), val_intra + val_inter


def delta_of(P, base_limbs, d):
    """the double the device returns for the delta limbs ``d`` on the maintained sums ``base_limbs``"""
    nz0, z0 = likelihood_of_limbs(base_limbs, P.M, P.params[7])
    nz1, z1 = likelihood_of_limbs([int(a) + int(b) for a, b in zip(base_limbs, d)], P.M, P.params[7])
    return (nz1 + z1) - (nz0 + z0)


def layout(state):
    """-> (slot int64 [N]: the bins in a layout where a contig's bins lie next to each other in their order, contigs by ascending id;
    heads: the first bin of every contig in that order; kof int64 [N]: the number of the bin's contig among the linear ones, -1: a
    ring; lin: the first bins of the linear contigs, by k)"""
    st = np.asarray(state)
    pos, cid, circ = st[F["pos"]].astype(np.int64), st[F["id_c"]].astype(np.int64), st[F["circ"]]
    heads = np.nonzero(pos == 0)[0]
    heads = heads[np.argsort(cid[heads], kind="stable")]
    L = st[F["l_cont"]][heads].astype(np.int64)
    base = np.full(int(cid.max()) + 1, -1, np.int64)
    base[cid[heads]] = np.cumsum(L) - L
    lin = heads[circ[heads] == 0]
    knum = np.full(base.size, -1, np.int64)
    knum[cid[lin]] = np.arange(lin.size)
    return base[cid] + pos, heads, np.where(circ == 0, knum[cid], -1), lin


def cut_scores_host(state, P, base_limbs=None):
    """The rule for the cuts -> dict: valid (bool [N]), contacts (int64 [N]), limbs (int64 [N, 5]), delta (f64 [N]; zeros unless
    ``base_limbs``, the maintained sums, are given); zeros where no cut exists."""
    st = np.asarray(state)
    N = st.shape[1]
    slot, heads, kof, _ = layout(st)
    dist, rank = tables(st, P)
    bi, bj = P.parent[P.row], P.parent[P.col]
    cid = st[F["id_c"]]
    span = (cid[bi] == cid[bj]) & (kof[bi] >= 0) & (bi != bj)
    i, j, cnt = P.row[span], P.col[span], P.cnt[span]
    q0 = cis_terms(P, (dist[i], dist[j]), (rank[i], rank[j]), i, j, cnt)
    dh, dl = limb_diff(P.trans_terms(cnt), q0)
    si, sj = slot[bi[span]], slot[bj[span]]
    lo, hi = np.minimum(si, sj), np.maximum(si, sj)
    prof = []
    for v in (dh, dl, np.ones(dh.size, np.int64)):  # + behind the earlier bin, - behind the later one, then the running sums
        diff = np.zeros(N + 1, np.int64)
        np.add.at(diff, lo + 1, v)
        np.add.at(diff, hi + 1, -v)
        run = np.cumsum(diff)
        assert run[N] == 0 and not run[slot[heads]].any()  # every contribution closes inside its contig
        prof.append(run)
    valid = (kof >= 0) & (st[F["prev"]] >= 0)
    out = dict(valid=valid, contacts=np.where(valid, prof[2][slot], 0), limbs=np.zeros((N, 5), np.int64), delta=np.zeros(N, np.float64))
    for f in np.nonzero(valid)[0].tolist():
        j_, L = int(st[F["sub_pos"]][f]), int(st[F["sub_l_cont"]][f])
        g = [P.G(j_), P.G(L - j_), P.G(L)]
        d = (int(prof[0][slot[f]]), int(prof[1][slot[f]]), g[0][0] + g[1][0] - g[2][0], g[0][1] + g[1][1] - g[2][1], -j_ * (L - j_))
        out["limbs"][f] = d
        if base_limbs is not None:
            out["delta"][f] = delta_of(P, base_limbs, d)
    return out


def link_coords(st, P, x, y, sa, sb):
    """the coordinates of the sub-fragments ``x`` (in a) and ``y`` (in b) in the state the canonical edit of the link (sa, sb) of their
    contigs leaves, by the closed form of ``rearrange.apply_host`` on two whole contigs -> ((dist_x, dist_y), (rank_x, rank_y))"""
    fa, fb = P.parent[x], P.parent[y]
    col = lambda k, f: st[F[k]][f].astype(np.int64)  # noqa: E731
    LBa, SLa, LBb, SLb = col("l_cont_bp", fa), col("sub_l_cont", fa), col("l_cont_bp", fb), col("sub_l_cont", fb)
    if sa == TAIL:  # a stays, b goes behind it
        a = coords(P, x, col("start_bp", fa), col("sub_pos", fa), col("sub_len", fa), col("ori", fa))
        ins_bp, ins_sub, flip = LBa, SLa, sb == TAIL
    else:  # b goes in front, a moves up
        a = coords(P, x, col("start_bp", fa) + LBb, col("sub_pos", fa) + SLb, col("sub_len", fa), col("ori", fa))
        ins_bp, ins_sub, flip = 0, 0, sb == HEAD
    if flip:
        b = coords(P, y, ins_bp + (LBb - (col("start_bp", fb) + col("len_bp", fb))), ins_sub + (SLb - (col("sub_pos", fb) + col("sub_len", fb))),
                   col("sub_len", fb), -col("ori", fb))
    else:
        b = coords(P, y, ins_bp + col("start_bp", fb), ins_sub + col("sub_pos", fb), col("sub_len", fb), col("ori", fb))
    return (a[0], b[0]), (a[1], b[1])


def join_scores_host(state, P, base_limbs=None):
    """The rule for the links -> dict as ``hip_lib.Context.join_scores``: K, n_pairs, head_bin, tail_bin, n_sub, length_bp [K], rowptr
    [K + 1], col, contacts, nz [n_pairs, 4, 2], z [n_pairs, 2], dni, delta [n_pairs, 4] (zeros unless ``base_limbs`` is given)"""
    st = np.asarray(state)
    _, _, kof, lin = layout(st)
    K = int(lin.size)
    tails = np.nonzero((st[F["next"]] < 0) & (kof >= 0))[0]
    tail_bin = np.full(K, -1, np.int32)
    tail_bin[kof[tails]] = tails
    n_sub = st[F["sub_l_cont"]][lin].astype(np.int32)
    out = dict(K=K, head_bin=lin.astype(np.int32), tail_bin=tail_bin, n_sub=n_sub, length_bp=st[F["l_cont_bp"]][lin].astype(np.int32))
    ki, kj = kof[P.parent[P.row]], kof[P.parent[P.col]]
    m = (ki >= 0) & (kj >= 0) & (ki != kj)
    swap = ki[m] > kj[m]
    x, y = np.where(swap, P.col[m], P.row[m]), np.where(swap, P.row[m], P.col[m])
    a, b, cnt = np.minimum(ki[m], kj[m]), np.maximum(ki[m], kj[m]), P.cnt[m]
    key, pair = np.unique(a * max(K, 1) + b, return_inverse=True)
    n_pairs = int(key.size)
    pa, pb = key // max(K, 1), key % max(K, 1)
    rowptr = np.zeros(K + 1, np.int64)
    np.add.at(rowptr, pa + 1, 1)
    nz = np.zeros((n_pairs, 4, 2), np.int64)
    qt = P.trans_terms(cnt)
    for sa in (HEAD, TAIL):
        for sb in (HEAD, TAIL):
            dist, rank = link_coords(st, P, x, y, sa, sb)
            dh, dl = limb_diff(cis_terms(P, dist, rank, x, y, cnt), qt)
            np.add.at(nz[:, 2 * sa + sb, 0], pair, dh)
            np.add.at(nz[:, 2 * sa + sb, 1], pair, dl)
    z = np.zeros((n_pairs, 2), np.int64)
    for p in range(n_pairs):
        La, Lb = int(n_sub[pa[p]]), int(n_sub[pb[p]])
        g = [P.G(La + Lb), P.G(La), P.G(Lb)]
        z[p] = (g[0][0] - g[1][0] - g[2][0], g[0][1] - g[1][1] - g[2][1])
    dni = n_sub[pa].astype(np.int64) * n_sub[pb].astype(np.int64)
    delta = np.zeros((n_pairs, 4), np.float64)
    if base_limbs is not None:
        for p in range(n_pairs):
            for q in range(4):
                delta[p, q] = delta_of(P, base_limbs, (nz[p, q, 0], nz[p, q, 1], z[p, 0], z[p, 1], dni[p]))
    out.update(n_pairs=n_pairs, rowptr=np.cumsum(rowptr), col=pb.astype(np.int32), contacts=np.bincount(pair, minlength=n_pairs).astype(np.int64), nz=nz, z=z, dni=dni,
               delta=delta)
    return out


def full_sums_host(state, P):
    """the five from-scratch sums of a genome WITHOUT rings on the host -> (nz hi, nz lo, z hi, z lo, intra pairs), Python integers,
    not normalised: every stored contact under the tables, every sub-fragment of rank > 0"""
    st = np.asarray(state)
    assert not st[F["circ"]].any()
    dist, rank = tables(st, P)
    cid = st[F["id_c"]][P.parent]
    i, j = P.row, P.col
    q = P.terms(np.abs(dist[i] - dist[j]).astype(np.float32), np.abs(rank[i] - rank[j]), (cid[i] != cid[j]).astype(np.int32), P.cnt)
    L = st[F["sub_l_cont"]][P.parent]
    zq = P.zero_terms(rank[rank > 0].astype(np.int32), L[rank > 0].astype(np.int32))
    ni = int((L[rank == 0].astype(np.int64) * (L[rank == 0].astype(np.int64) - 1) // 2).sum())
    return limb_sum(q) + limb_sum(zq) + (ni,)


# ---------------------------------------------------------------------------------------------------------------- edits and tables
def cut_edit(state, f):
    """the edit of the cut in front of bin ``f``: the tail of its contig from ``f`` on becomes a contig of its own"""
    st = np.asarray(state)
    f = int(f)
    last = np.nonzero((st[F["id_c"]] == st[F["id_c"]][f]) & (st[F["pos"]] == st[F["l_cont"]][f] - 1))[0]
    return (f, int(last[0]), NEW_CONTIG, 0, 0)


def link_edit(head_bin, tail_bin, a, b, sa, sb):
    """the canonical edit of the link (sa, sb) of the contigs a < b: all of b behind a's last bin or in front of a's first"""
    first, last = int(head_bin[b]), int(tail_bin[b])
    if sa == TAIL:
        return (first, last, int(tail_bin[a]), 0, int(sb == TAIL))
    return (first, last, int(head_bin[a]), 1, int(sb == HEAD))


def weakest_cuts(state, cuts, n=20):
    """the ``n`` cuts with the largest positive delta, descending (ties by bin) -> CUT_DTYPE rows with their edits"""
    st = np.asarray(state)
    delta = np.asarray(cuts["delta"], np.float64)
    ok = np.nonzero(np.asarray(cuts["valid"], bool) & (delta > 0))[0]
    ok = ok[np.argsort(-delta[ok], kind="stable")][:max(int(n), 0)]
    out = np.zeros(ok.size, CUT_DTYPE)
    out["bin"], out["prev_bin"], out["contacts"], out["delta"], out["limbs"] = ok, st[F["prev"]][ok], cuts["contacts"][ok], delta[ok], cuts["limbs"][ok]
    for r, f in enumerate(ok.tolist()):
        out["edit"][r] = cut_edit(st, f)
    return out


def link_rows(joins, links=None):
    """one row per link -> LINK_DTYPE rows with their canonical edits.  ``links``: indices 4 pair + (2 sa + sb) into the links of all
    pairs, default every link in the order of the pairs and of 2 sa + sb.  Only the rows asked for are built."""
    P = int(joins["n_pairs"])
    idx = np.arange(4 * P, dtype=np.int64) if links is None else np.asarray(links, np.int64)
    p, q = idx // 4, idx % 4
    sa, sb = q >> 1, q & 1
    a = np.repeat(np.arange(int(joins["K"]), dtype=np.int64), np.diff(joins["rowptr"]))[p]
    b = np.asarray(joins["col"], np.int64)[p]
    head, tail = np.asarray(joins["head_bin"], np.int64), np.asarray(joins["tail_bin"], np.int64)
    out = np.zeros(idx.size, LINK_DTYPE)
    out["a"], out["b"], out["sa"], out["sb"] = a, b, sa, sb
    out["contacts"], out["delta"] = np.asarray(joins["contacts"])[p], np.asarray(joins["delta"])[p, q]
    out["bin_a"], out["bin_b"] = np.where(sa == TAIL, tail[a], head[a]), np.where(sb == TAIL, tail[b], head[b])
    nz, z = np.asarray(joins["nz"]), np.asarray(joins["z"])
    out["limbs"] = np.stack([nz[p, q, 0], nz[p, q, 1], z[p, 0], z[p, 1], np.asarray(joins["dni"])[p]], axis=1) if idx.size else 0
    # the canonical edit (link_edit), for all rows at once: all of b behind a's last bin or in front of a's first
    edit = np.stack([head[b], tail[b], np.where(sa == TAIL, tail[a], head[a]), (sa == HEAD).astype(np.int64), np.where(sa == TAIL, sb == TAIL, sb == HEAD).astype(np.int64)],
                    axis=1) if idx.size else np.zeros((0, 5), np.int64)
    out["edit"] = edit
    return out


def strongest_joins(joins, n=20):
    """the ``n`` links with the largest positive delta, descending (ties by pair, then by 2 sa + sb) -> LINK_DTYPE rows.  The links are
    ranked on the delta array; only the ``n`` rows returned are built."""
    delta = np.asarray(joins["delta"], np.float64).reshape(-1)
    ok = np.nonzero(delta > 0)[0]
    return link_rows(joins, ok[np.argsort(-delta[ok], kind="stable")][:max(int(n), 0)])


def write_cuts(path, table):
    """one line per row of ``weakest_cuts``: the columns of CUT_COLUMNS"""
    with open(path, "w") as f:
        f.write("# " + " ".join(CUT_COLUMNS) + "\n")
        for r in table:
            f.write("%d %d %d %.17g %d %d %d %d %d\n" % ((int(r["bin"]), int(r["prev_bin"]), int(r["contacts"]), float(r["delta"])) + tuple(int(x) for x in r["edit"])))
        f.write("# cuts=%d\n" % len(table))
    return len(table)


def write_links(path, table):
    """one line per row of ``strongest_joins``: the columns of LINK_COLUMNS (ends as head / tail)"""
    with open(path, "w") as f:
        f.write("# " + " ".join(LINK_COLUMNS) + "\n")
        for r in table:
            f.write("%d %d %s %s %d %d %d %.17g %d %d %d %d %d\n" % ((int(r["a"]), int(r["b"]), SIDES[int(r["sa"])], SIDES[int(r["sb"])], int(r["bin_a"]), int(r["bin_b"]),
                                                                     int(r["contacts"]), float(r["delta"])) + tuple(int(x) for x in r["edit"])))
        f.write("# links=%d\n" % len(table))
    return len(table)
