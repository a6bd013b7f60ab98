"""Segment edits: take a run of bins out of its contig, optionally reverse it, and put it somewhere else -- the moves the block-level
reports (``orientation_support.inverted_segments``, ``segment_placement.misplaced_segments``) propose.  This module is the single
definition of the rule (pure numpy, no GPU); the device (``ig_edit_score``, ``ig_edit_state``, ``ig_edit_apply``:
csrc/ig_kernels_edit.cuh) reproduces its states byte for byte and scores them exactly.

A STATE is the 17 x N int32 array of ``hip_lib.FRAG_FIELDS`` (what ``Context.download_state`` returns, with any labelling of the
contigs).  An EDIT is five int32 values ``(first_bin, last_bin, anchor, side, flip)``:

* the SEGMENT S is the bins of one linear contig with pos(first_bin) <= pos <= pos(last_bin);
* S is taken out of its contig and the remainder closes up; a contig left empty disappears;
* with ``flip = 1`` the order of S is reversed and the ``ori`` of each of its bins is negated;
* S goes back where it was (``anchor = IN_PLACE``), becomes a contig of its own with id ``next_cid`` (``anchor = NEW_CONTIG``), or is
  inserted directly behind (``side = 0``) or in front of (``side = 1``) the bin ``anchor >= 0``, a bin outside S in a linear contig
  which may be S's own.

For every contig whose list of bins changed, with its bins b_0 .. b_{L-1} in the new order: ``pos`` = r, ``sub_pos`` and ``start_bp``
the prefix sums of ``sub_len`` and ``len_bp``, ``l_cont``, ``sub_l_cont``, ``l_cont_bp`` the totals, ``prev`` / ``next`` the neighbours
(-1 at the ends), ``circ`` = 0; the destination and the remainder keep their ids.  Every other bin and field stays untouched.

STATUS: 0 ok; 1 a bin (first_bin, last_bin, an anchor >= 0) is out of range; 2 the two bins are not in one contig or in the wrong order;
3 the segment's or the anchor's contig is a ring; 4 the anchor lies inside the segment; 5 anchor < -2, side or flip not 0 / 1.  The
lowest code that applies is returned.  No-ops (``IN_PLACE`` without a flip, a site next to the segment's own place, a whole contig made
a ``NEW_CONTIG``) are valid.
"""
from __future__ import annotations

import numpy as np

from .hip_lib import EDIT_PASSES, FRAG_FIELDS  # noqa: F401  (the passes of ig_debug_edit_time)

IN_PLACE, NEW_CONTIG = -2, -1
OK, BAD_BIN, BAD_SEGMENT, RING, ANCHOR_INSIDE, BAD_FIELD = 0, 1, 2, 3, 4, 5
F = {k: i for i, k in enumerate(FRAG_FIELDS)}
DYNAMIC = ("pos", "sub_pos", "id_c", "start_bp", "circ", "prev", "next", "l_cont", "sub_l_cont", "l_cont_bp", "ori")
FORMS = ("delta", "whole")  # ig_edit_score's form 0 / 1
SCORE_DTYPE = np.dtype([("status", np.int32), ("nz", np.float64), ("z", np.float64), ("score", np.float64), ("delta", np.float64), ("limbs", np.int64, (5,))])
LOG_COLUMNS = ("round", "first_bin", "last_bin", "anchor", "side", "flip", "delta", "likelihood")


def as_edits(edits):
    """-> int32 [n, 5], contiguous"""
    e = np.asarray(edits)
    if e.size == 0:
        return np.zeros((0, 5), np.int32)
    e = np.ascontiguousarray(e, np.int32).reshape(-1, 5)
    return e


def check(state, edit):
    """the status of ``edit`` on ``state``"""
    st = np.asarray(state)
    N = st.shape[1]
    fb, lb, anchor, side, flip = (int(x) for x in edit)
    if not (0 <= fb < N and 0 <= lb < N) or anchor >= N:
        return BAD_BIN
    pos, cid, circ = st[F["pos"]], st[F["id_c"]], st[F["circ"]]
    if cid[fb] != cid[lb] or pos[fb] > pos[lb]:
        return BAD_SEGMENT
    if circ[fb] != 0 or (anchor >= 0 and circ[anchor] != 0):
        return RING
    if anchor >= 0 and cid[anchor] == cid[fb] and pos[fb] <= pos[anchor] <= pos[lb]:
        return ANCHOR_INSIDE
    if anchor < IN_PLACE or side not in (0, 1) or flip not in (0, 1):
        return BAD_FIELD
    return OK


def contig_bins(state, cid):
    """the bins of contig ``cid`` in their order"""
    st = np.asarray(state)
    b = np.nonzero(st[F["id_c"]] == cid)[0]
    return b[np.argsort(st[F["pos"]][b], kind="stable")]


def rebuild(state, cid, bins):
    """writes the fields of the contig ``cid`` made of ``bins`` in this order into ``state`` (in place)"""
    b = np.asarray(bins, np.int64)
    if b.size == 0:
        return
    st = state
    sl, lb = st[F["sub_len"]][b].astype(np.int64), st[F["len_bp"]][b].astype(np.int64)
    st[F["pos"]][b] = np.arange(b.size)
    st[F["sub_pos"]][b] = np.cumsum(sl) - sl
    st[F["start_bp"]][b] = np.cumsum(lb) - lb
    st[F["l_cont"]][b] = b.size
    st[F["sub_l_cont"]][b] = sl.sum()
    st[F["l_cont_bp"]][b] = lb.sum()
    st[F["prev"]][b] = np.concatenate([[-1], b[:-1]])
    st[F["next"]][b] = np.concatenate([b[1:], [-1]])
    st[F["circ"]][b] = 0
    st[F["id_c"]][b] = cid


def new_contigs(state, edit, next_cid):
    """the contigs the edit rewrites -> (status, {contig id: bins in the new order}, the segment in its new order)"""
    status = check(state, edit)
    if status:
        return status, {}, np.zeros(0, np.int64)
    st = np.asarray(state)
    fb, lb, anchor, side, flip = (int(x) for x in edit)
    cs = int(st[F["id_c"]][fb])
    src = contig_bins(st, cs)
    a, b = int(st[F["pos"]][fb]), int(st[F["pos"]][lb])
    seg, rem = src[a:b + 1], np.concatenate([src[:a], src[b + 1:]])
    if flip:
        seg = seg[::-1]
    if anchor == IN_PLACE:
        return OK, {cs: np.concatenate([src[:a], seg, src[b + 1:]])}, seg
    if anchor == NEW_CONTIG:
        return OK, {cs: rem, int(next_cid): seg}, seg
    cd = int(st[F["id_c"]][anchor])
    dst = rem if cd == cs else contig_bins(st, cd)
    k = int(np.nonzero(dst == anchor)[0][0]) + (1 if side == 0 else 0)
    out = {cs: rem}
    out[cd] = np.concatenate([dst[:k], seg, dst[k:]])
    return OK, out, seg


def apply_host(state, edit, next_cid):
    """-> (the edited state: a new 17 x N int32 array, status).  A status other than 0 returns a copy of ``state``."""
    st = np.array(state, dtype=np.int32, copy=True)
    status, contigs, seg = new_contigs(st, edit, next_cid)
    if status:
        return st, status
    if int(edit[4]):
        st[F["ori"]][seg] = -st[F["ori"]][seg]
    for cid, bins in contigs.items():
        rebuild(st, cid, bins)
    return st, OK


def touched_contigs(state, edit):
    """the contig ids (of ``state``) whose list of bins the edit may change; () for an edit that is refused"""
    if check(state, edit):
        return ()
    st = np.asarray(state)
    cs = int(st[F["id_c"]][int(edit[0])])
    if int(edit[2]) >= 0:
        cd = int(st[F["id_c"]][int(edit[2])])
        return (cs,) if cd == cs else (cs, cd)
    return (cs,)


def next_contig_id(state):
    """the id a ``NEW_CONTIG`` gets on a state with this labelling: one more than the largest"""
    return int(np.asarray(state)[F["id_c"]].max()) + 1


def canonical(state):
    """``state`` with the contigs numbered as ``Context.download_state`` numbers them (contigs by ascending index of their head bin,
    stable by length descending, id = n - 1 - rank) and ``id`` = the bin's index: equal genomes -> equal arrays"""
    st = np.array(state, dtype=np.int32, copy=True)
    heads = np.nonzero(st[F["pos"]] == 0)[0]
    order = np.argsort(-st[F["l_cont"]][heads].astype(np.int64), kind="stable")
    lut = np.full(int(st[F["id_c"]].max()) + 1, -1, np.int64)
    lut[st[F["id_c"]][heads[order]]] = heads.size - 1 - np.arange(heads.size)
    st[F["id_c"]] = lut[st[F["id_c"]]]
    st[F["id"]] = np.arange(st.shape[1])
    return st


# ---------------------------------------------------------------------------------------------------------------- the proposals
def _boundary_sites(st, seg_bins, site_bin, site_side, window):
    """the bin boundaries of the contig of ``site_bin``, the segment's bins left out, that lie within ``window`` positions
    (sub-fragments) of the site, each ONCE as (bin, side): in front of every bin (side 1), and behind the last one (side 0)"""
    sp, sl = st[F["sub_pos"]].astype(np.int64), st[F["sub_len"]].astype(np.int64)
    at = sp[site_bin] + (sl[site_bin] if site_side == 0 else 0)
    bins = contig_bins(st, st[F["id_c"]][site_bin])
    bins = bins[~np.isin(bins, seg_bins)]
    out = [(b, 1) for b in bins.tolist() if abs(int(sp[b]) - at) <= window]
    if bins.size and abs(int(sp[bins[-1]] + sl[bins[-1]]) - at) <= window:
        out.append((int(bins[-1]), 0))
    return out


def propose(state, inverted=None, misplaced=(), n=20, window=64):
    """The edits the reports propose, a pure function of their tables and the state -> int32 [n_edits, 5].

    ``inverted``: the table of ``orientation_support.inverted_segments`` (block level): for each of its first ``n`` rows the
    ``IN_PLACE`` flip of [first_bin, last_bin].  ``misplaced``: the tables of ``segment_placement.misplaced_segments`` (block level,
    then scaffold level): for each of the first ``n`` rows of each, every bin boundary of the best scaffold within ``window`` positions
    of the best site (``best_before`` / ``best_after``), once as (bin, side) -- in front of a bin, or behind the last one --, with both
    values of ``flip``; anchors inside the segment are left out.  Equal genomes reached twice (from the block-level and the
    scaffold-level table, or a site next to the segment's own place) are kept: they score the same.  Rows whose bins do not form a
    segment of the state are skipped."""
    st = np.asarray(state)
    edits = []
    if inverted is not None:
        for r in inverted[:max(int(n), 0)]:
            e = (int(r["first_bin"]), int(r["last_bin"]), IN_PLACE, 0, 1)
            if check(st, e) == OK:
                edits.append(e)
    for table in misplaced:
        for r in table[:max(int(n), 0)]:
            fb, lb = int(r["first_bin"]), int(r["last_bin"])
            if check(st, (fb, lb, IN_PLACE, 0, 0)) != OK:
                continue
            after, before = int(r["best_after"]), int(r["best_before"])
            site = (after, 1) if after >= 0 else (before, 0)
            if site[0] < 0 or st[F["circ"]][site[0]] != 0:
                continue
            src = contig_bins(st, st[F["id_c"]][fb])
            seg = src[int(st[F["pos"]][fb]):int(st[F["pos"]][lb]) + 1]
            if site[0] in seg:
                continue
            for b, side in _boundary_sites(st, seg, site[0], site[1], int(window)):
                for flip in (0, 1):
                    edits.append((fb, lb, b, side, flip))
    return as_edits(edits)


def propose_cuts_joins(state, cuts=None, joins=None, n=20):
    """The edits of the ``n`` weakest cuts (``cuts``: what ``sampler.cut_scores`` returns) and of the ``n`` strongest joins (``joins``:
    ``sampler.join_scores``), cuts first, each list by falling delta (``cut_join.weakest_cuts``, ``cut_join.strongest_joins``); either
    may be None.  An edit the rule refuses on ``state`` is left out.  -> int32 [n_edits, 5]"""
    from . import cut_join as cj

    st = np.asarray(state)
    edits = []
    if cuts is not None:
        edits += [tuple(int(x) for x in e) for e in cj.weakest_cuts(st, cuts, n)["edit"]]
    if joins is not None:
        edits += [tuple(int(x) for x in e) for e in cj.strongest_joins(joins, n)["edit"]]
    return as_edits([e for e in edits if check(st, e) == OK])


def polish_round(scores, edits, state, min_gain=0.0):
    """the edits one round applies -> their indices: those with status 0 and delta > ``min_gain``, by descending delta (ties by index),
    skipping any edit that shares a touched contig with one taken before it in this round.  The deltas of edits on disjoint sets of
    contigs add exactly.  ``scores``: what ``sampler.score_rearrangements`` returns (fields status, delta), or the deltas alone."""
    e = as_edits(edits)
    s = np.asarray(scores)
    delta = np.asarray(s["delta"] if s.dtype.names else s, np.float64)
    ok = np.asarray(s["status"] == 0 if s.dtype.names else np.ones(delta.size, bool)) & (delta > float(min_gain))
    taken, used = [], set()
    for i in np.nonzero(ok)[0][np.argsort(-delta[ok], kind="stable")].tolist():
        t = touched_contigs(state, e[i])
        if not t or used.intersection(t):
            continue
        used.update(t)
        taken.append(i)
    return taken


def write_polish_log(path, log):
    """one line per applied edit: the columns of LOG_COLUMNS"""
    with open(path, "w") as f:
        f.write("# " + " ".join(LOG_COLUMNS) + "\n")
        for r in log:
            e = [int(x) for x in r["edit"]]
            f.write("%d %d %d %d %d %d %.17g %.17g\n" % (int(r["round"]), e[0], e[1], e[2], e[3], e[4], float(r["delta"]), float(r["likelihood"])))
        f.write("# applied=%d\n" % len(log))
    return len(log)
