"""Orientation support: which segments of the current genome the contacts would reverse.  A spurious inversion -- a bin, or a run of
co-linear bins, at the right place the wrong way round -- barely shows in the other reports: most contacts that span it stay inside
the junction profile's window, and placement support finds the bin at home.  Here every segment's contacts with the positions on
either side of it are split by the END of the segment they touch.  This module is the single definition of the rule (pure numpy, no
GPU); the device passes (``ig_orientation_support``, csrc/ig_kernels_orient.cuh) reproduce ``support_host`` byte for byte.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs in genome order, 0 .. T - 1; a contig holds
the positions contig_start .. contig_end - 1.  ``window`` w is counted in positions, 1 <= w <= MAX_WINDOW.

SEGMENTS.  The caller gives n_seg intervals [first_k, last_k] of positions, ascending and disjoint, each inside one placed contig;
they need not cover the order.  With n = last - first + 1 the ARM is m = min(n // 2, w): the left arm is [first, first + m - 1], the
right arm [last - m + 1, last], the positions between them are interior.  The FLANKS are the up to w positions of the contig on
either side: left_flank = min(w, first - contig_start), right_flank = min(w, contig_end - 1 - last).

STATUS per segment, the first that fits: 1 fewer than two positions; 2 on a ring (a pair on a ring has two separations); 3 no
flank (both are empty: the segment is its contig); 0 JUDGED.  ``geometry`` holds (status, arm, left_flank, right_flank); arm and
flanks are 0 on a ring.  The rows of ``observed`` and ``expected_q`` of a segment that is not judged are 0.

OBSERVED, four int64 per segment: LL, LR, RL, RR (arm, flank).  A contact of the uploaded strict upper triangle with both ends
placed in the same linear contig lies at positions pa < pb; sa = seg(pa), sb = seg(pb), -1 outside every segment.  If sa == sb >= 0
it is within_segment.  Otherwise its LOWER end counts for sa if sa is judged and pb - last[sa] <= w (pb is in sa's right flank): to
LR if pa is in the left arm, to RR if it is in the right arm; its UPPER end counts for sb if sb is judged and first[sb] - pa <= w
(pa is in sb's left flank): to LL if pb is in the left arm, to RL if it is in the right arm.  A contact between the facing arms of
two neighbouring segments counts once for each.  keep = LL + RR joins each arm with the flank on its own side, flip = LR + RL with
the flank on the other side; each class has pairs = m * (left_flank + right_flank) pairs of positions.  Reversing the segment in
place moves every contact from LL to RL, from LR to RR and back: the quadrants swap exactly, whatever the model.

EXPECTED (optional), two int64 per judged segment: expected_q[keep] and expected_q[flip], each the sum over the pairs of its class
of the model's value at ``s = fabsf(dist_i - dist_k)`` quantised to a multiple of 2^-32 -- the junction profile's q -- added as
integers: the result does not depend on the order of the additions.

The scalars (int64).  Every contact is classified by the first class it fits: ``unplaced`` (an end in a contig that is not
placed), ``trans``, ``ring``, ``within_segment``, ``counted`` (at least one quadrant took it), ``uncounted``; then
``entries_observed`` (the sum of all quadrants) and ``n_judged``.  By construction:

    unplaced + trans + ring + within_segment + counted + uncounted == sum(counts)
    counted <= entries_observed <= 2 * counted
"""
from __future__ import annotations

import numpy as np

from .junction_profile import MAX_WINDOW, Q_ONE, check_window, contig_runs, window_from_kb  # noqa: F401  (the window is the junction profile's)

DEFAULT_WINDOW = 8  # this report's own (the signal was measured at 4 and at 64)
# the order of ig_orientation_support's scalars[8]
SCALARS = ("unplaced", "trans", "ring", "within_segment", "counted", "uncounted", "entries_observed", "n_judged")
CLASS_SCALARS = SCALARS[:6]
STATUS_JUDGED, STATUS_SHORT, STATUS_RING, STATUS_NO_FLANK = 0, 1, 2, 3
STATUS_NAMES = ("judged", "short", "ring", "no_flank")
LL, LR, RL, RR = 0, 1, 2, 3  # the columns of ``observed``: (arm, flank)
KEEP, FLIP = 0, 1            # the columns of ``expected_q``
COLUMNS = ("segment", "first", "last", "first_bin", "last_bin", "scaffold", "status", "arm", "left_flank", "right_flank", "LL", "LR", "RL", "RR",
           "keep", "flip", "pairs", "ratio", "z", "llr")
SEGMENT_DTYPE = np.dtype([(k, np.float64 if k in ("ratio", "z", "llr") else np.int64) for k in COLUMNS])


def check_segments(first, last, n_placed, contig_start):
    """-> (first, last) as int64 arrays; ValueError unless the list is in range, ascending, disjoint and every segment lies inside
    one contig.  ``contig_start``: the first position of the contig of every position"""
    f, l = np.asarray(first), np.asarray(last)
    if f.ndim != 1 or f.shape != l.shape or not (np.issubdtype(f.dtype, np.integer) and np.issubdtype(l.dtype, np.integer)):
        raise ValueError("orientation support: segment list: first and last are integer vectors of one length")
    f, l = f.astype(np.int64), l.astype(np.int64)
    if f.size and (f.min() < 0 or l.max() >= n_placed or np.any(l < f)):
        raise ValueError("orientation support: segment list out of range: 0 <= first <= last < %d" % n_placed)
    if np.any(f[1:] <= l[:-1]):
        raise ValueError("orientation support: segment list not ascending and disjoint")
    cs = np.asarray(contig_start, np.int64)
    if f.size and np.any(cs[f] != cs[l]):
        raise ValueError("orientation support: segment list: a segment spans two contigs")
    return f, l


def segment_geometry(first, last, contig_start, contig_end, ring, window):
    """int32 [n_seg, 4]: (status, arm, left_flank, right_flank).  contig_start, contig_end, ring: per position"""
    w = check_window(window)
    f, l = np.asarray(first, np.int64), np.asarray(last, np.int64)
    geo = np.zeros((f.size, 4), np.int32)
    if f.size == 0:
        return geo
    n = l - f + 1
    on_ring = np.asarray(ring, bool)[f]
    arm = np.where(on_ring, 0, np.minimum(n // 2, w))
    lf = np.where(on_ring, 0, np.minimum(w, f - np.asarray(contig_start, np.int64)[f]))
    rf = np.where(on_ring, 0, np.minimum(w, np.asarray(contig_end, np.int64)[f] - 1 - l))
    geo[:, 0] = np.where(n < 2, STATUS_SHORT, np.where(on_ring, STATUS_RING, np.where(lf + rf == 0, STATUS_NO_FLANK, STATUS_JUDGED)))
    geo[:, 1], geo[:, 2], geo[:, 3] = arm, lf, rf
    return geo


def support_host(dist, stot, contig, placed, position, row, col, cnt, first, last, window, model_q=None):
    """The rule, contact by contact and pair by pair (deliberately naive: no difference arrays, no atomics).

    dist, stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order,
    -1 where not placed; row, col, cnt: the contacts; first, last: the segments; ``model_q``: callable, separations (f32 array) ->
    the model's quantised values (int64), None: ``expected_q`` is None.  -> dict: window, n_placed, n_seg, first, last, geometry
    (int32 [n_seg, 4]), observed (int64 [n_seg, 4]), expected_q (int64 [n_seg, 2]) and the int64 scalars named in SCALARS."""
    w = check_window(window)
    dist = np.asarray(dist, np.float32)
    ring = np.asarray(stot, np.float32) != 0
    contig = np.asarray(contig, np.int64)
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError("orientation support: placed and position disagree")
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    members, start, length = contig_runs(contig, position)
    T = int(members.size)
    c_start, c_end = np.repeat(start, length), np.repeat(start + length, length)
    first, last = check_segments(first, last, T, c_start)
    n_seg = int(first.size)
    geo = segment_geometry(first, last, c_start, c_end, ring[members], w)
    judged = geo[:, 0] == STATUS_JUDGED
    arm = geo[:, 1].astype(np.int64)
    seg = np.full(T, -1, np.int64)
    n_pos = last - first + 1
    seg[np.repeat(first - (np.cumsum(n_pos) - n_pos), n_pos) + np.arange(int(n_pos.sum()), dtype=np.int64)] = np.repeat(np.arange(n_seg, dtype=np.int64), n_pos)

    out = dict(window=w, n_placed=T, n_seg=n_seg, first=first, last=last, geometry=geo)
    both = placed[row] & placed[col]
    out["unplaced"] = int(cnt[~both].sum())
    cis = both & (contig[row] == contig[col])
    out["trans"] = int(cnt[both & ~cis].sum())
    on_ring = cis & ring[row]
    out["ring"] = int(cnt[on_ring].sum())
    lin = cis & ~on_ring
    pa = np.minimum(position[row[lin]], position[col[lin]])
    pb = np.maximum(position[row[lin]], position[col[lin]])
    c = cnt[lin]
    sa, sb = seg[pa], seg[pb]
    within = (sa >= 0) & (sa == sb)
    out["within_segment"] = int(c[within].sum())
    observed = np.zeros((n_seg, 4), np.int64)
    hits = np.zeros(pa.size, np.int64)
    if n_seg:
        # the lower end, for sa: pb lies in sa's right flank
        s = np.maximum(sa, 0)
        ok = ~within & (sa >= 0) & judged[s] & (pb - last[s] <= w)
        for quadrant, in_arm in ((LR, pa < first[s] + arm[s]), (RR, pa > last[s] - arm[s])):
            take = ok & in_arm
            np.add.at(observed[:, quadrant], s[take], c[take])
            hits += take
        # the upper end, for sb: pa lies in sb's left flank
        s = np.maximum(sb, 0)
        ok = ~within & (sb >= 0) & judged[s] & (first[s] - pa <= w)
        for quadrant, in_arm in ((LL, pb < first[s] + arm[s]), (RL, pb > last[s] - arm[s])):
            take = ok & in_arm
            np.add.at(observed[:, quadrant], s[take], c[take])
            hits += take
    out["counted"] = int(c[~within & (hits > 0)].sum())
    out["uncounted"] = int(c[~within & (hits == 0)].sum())
    out["observed"] = observed
    out["entries_observed"] = int(observed.sum())
    out["n_judged"] = int(judged.sum())

    expected_q = None
    if model_q is not None:
        expected_q = np.zeros((n_seg, 2), np.int64)
        d = dist[members]
        for k in np.nonzero(judged)[0].tolist():
            f, l, m, lf, rf = int(first[k]), int(last[k]), int(geo[k, 1]), int(geo[k, 2]), int(geo[k, 3])
            arms = np.concatenate([np.arange(f, f + m), np.arange(l - m + 1, l + 1)])
            flanks = np.concatenate([np.arange(f - lf, f), np.arange(l + 1, l + 1 + rf)])
            sep = np.abs(d[arms][:, None] - d[flanks][None, :])
            assert sep.dtype == np.float32
            q = np.asarray(model_q(sep.ravel()), np.int64).reshape(sep.shape)
            same_side = (np.arange(2 * m) < m)[:, None] == (np.arange(lf + rf) < lf)[None, :]
            expected_q[k, KEEP], expected_q[k, FLIP] = int(q[same_side].sum()), int(q[~same_side].sum())
    out["expected_q"] = expected_q
    return out


def observed_total(result):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(result[k]) for k in CLASS_SCALARS)


def derived(result):
    """-> dict of per-segment columns: keep, flip, pairs (int64), ratio = flip / keep (inf: keep is 0, nan: both are), z =
    (flip - keep) / sqrt(flip + keep) (nan: both are 0) and, with the model, expected_keep, expected_flip (f64) and llr =
    (flip - keep) * ln(E_keep / E_flip): the Poisson log-likelihood ratio of "reversed" against "as placed" for the two classes
    (nan where an expectation is 0)"""
    obs = np.asarray(result["observed"], np.int64).reshape(-1, 4)
    geo = np.asarray(result["geometry"], np.int64).reshape(-1, 4)
    keep, flip = obs[:, LL] + obs[:, RR], obs[:, LR] + obs[:, RL]
    out = dict(keep=keep, flip=flip, pairs=geo[:, 1] * (geo[:, 2] + geo[:, 3]))
    kf, ff = keep.astype(np.float64), flip.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["ratio"] = np.where(keep > 0, ff / np.where(keep > 0, kf, 1.0), np.where(flip > 0, np.inf, np.nan))
        out["z"] = np.where(keep + flip > 0, (ff - kf) / np.sqrt(np.where(keep + flip > 0, kf + ff, 1.0)), np.nan)
        if result.get("expected_q") is not None:
            e = np.asarray(result["expected_q"], np.float64).reshape(-1, 2) / Q_ONE
            out["expected_keep"], out["expected_flip"] = e[:, KEEP], e[:, FLIP]
            ok = (e[:, KEEP] > 0) & (e[:, FLIP] > 0)
            out["llr"] = np.where(ok, (ff - kf) * np.log(np.where(ok, e[:, KEEP], 1.0) / np.where(ok, e[:, FLIP], 1.0)), np.nan)
    return out


def inverted_segments(result, n=20, min_observed=0):
    """the ``n`` judged segments with flip > keep and keep + flip >= ``min_observed``, the most strongly reversed first: by ``llr``
    (by ``z`` where the result has no model part, or no llr) descending, ties by segment index -> a SEGMENT_DTYPE array.
    ``result``: what ``support_host``, ``Context.orientation_support`` or ``sampler.orientation_support`` return"""
    d = result if "keep" in result else dict(result, **derived(result))
    geo = np.asarray(result["geometry"], np.int64).reshape(-1, 4)
    obs = np.asarray(result["observed"], np.int64).reshape(-1, 4)
    keep, flip = np.asarray(d["keep"], np.int64), np.asarray(d["flip"], np.int64)
    llr = np.asarray(d["llr"], np.float64) if d.get("llr") is not None else np.full(keep.size, np.nan)
    score = np.where(np.isfinite(llr), llr, np.asarray(d["z"], np.float64)) if d.get("llr") is not None else np.asarray(d["z"], np.float64)
    ok = np.nonzero((geo[:, 0] == STATUS_JUDGED) & (flip > keep) & (keep + flip >= int(min_observed)))[0]
    pick = ok[np.argsort(-score[ok], kind="stable")[:max(int(n), 0)]]
    t = np.zeros(pick.size, SEGMENT_DTYPE)
    t["segment"] = pick
    t["first"], t["last"] = np.asarray(result["first"], np.int64)[pick], np.asarray(result["last"], np.int64)[pick]
    for k in ("first_bin", "last_bin", "scaffold"):
        t[k] = np.asarray(result[k], np.int64)[pick] if k in result else -1
    for i, k in enumerate(("status", "arm", "left_flank", "right_flank")):
        t[k] = geo[pick, i]
    for i, k in enumerate(("LL", "LR", "RL", "RR")):
        t[k] = obs[pick, i]
    for k in ("keep", "flip", "pairs", "ratio", "z"):
        t[k] = np.asarray(d[k])[pick]
    t["llr"] = llr[pick]
    return t


def write_orientations(path, result, mode="w", title=None):
    """one line per judged segment, the columns of COLUMNS; then the window and the scalars (``mode="a"``: behind what the file
    holds already; ``title``: a comment line in front)"""
    d = result if "keep" in result else dict(result, **derived(result))
    geo = np.asarray(result["geometry"], np.int64).reshape(-1, 4)
    obs = np.asarray(result["observed"], np.int64).reshape(-1, 4)
    llr = np.asarray(d["llr"], np.float64) if d.get("llr") is not None else np.full(geo.shape[0], np.nan)
    some = lambda k, i: int(np.asarray(result[k])[i]) if k in result else -1  # noqa: E731
    with open(path, mode) as f:
        if title:
            f.write("# %s\n" % title)
        f.write("# " + " ".join(COLUMNS) + "\n")
        for i in np.nonzero(geo[:, 0] == STATUS_JUDGED)[0].tolist():
            f.write("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %.9g %.9g %.9g\n" % (
                i, int(np.asarray(result["first"])[i]), int(np.asarray(result["last"])[i]), some("first_bin", i), some("last_bin", i), some("scaffold", i),
                geo[i, 0], geo[i, 1], geo[i, 2], geo[i, 3], obs[i, 0], obs[i, 1], obs[i, 2], obs[i, 3], d["keep"][i], d["flip"][i], d["pairs"][i],
                d["ratio"][i], d["z"][i], llr[i]))
        f.write("# window=%d n_placed=%d n_seg=%d " % (result["window"], result["n_placed"], geo.shape[0]) + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")


# ------------------------------------------------------------------------------------------------------------- the segment builders
def bin_segments(order, parent):
    """one segment per placed bin -> dict: first, last (positions) and first_bin, last_bin (the bins at the segment's ends: here the
    bin itself).  ``order``: the sub-fragment at every position; ``parent``: the bin of every sub-fragment"""
    p = np.asarray(parent, np.int64)[np.asarray(order, np.int64)]
    T = int(p.size)
    if T == 0:
        z = np.zeros(0, np.int64)
        return dict(first=z, last=z.copy(), first_bin=z.copy(), last_bin=z.copy())
    first = np.concatenate([[0], np.nonzero(p[1:] != p[:-1])[0] + 1]).astype(np.int64)
    last = np.concatenate([first[1:] - 1, [T - 1]]).astype(np.int64)
    return dict(first=first, last=last, first_bin=p[first], last_bin=p[last])


def block_segments(order, parent, contig, ori, id_d, init_contig, init_pos):
    """the maximal runs of bins that are neighbours in the order, lie in the same current contig, come from the same initial contig
    and are co-linear: the initial positions of two neighbours differ by +1 with both ``ori == 1``, or by -1 with both ``ori == -1``
    -- the blocks a polishing step reasons about.  contig, ori, id_d: per bin, of the CURRENT state; init_contig, init_pos: per
    initial bin (the fragment table the sampler was built with), indexed through id_d.  -> as ``bin_segments``"""
    b = bin_segments(order, parent)
    bins = b["first_bin"]
    if bins.size == 0:
        return b
    contig, ori = np.asarray(contig, np.int64)[bins], np.asarray(ori, np.int64)[bins]
    src = np.asarray(id_d, np.int64)[bins]
    c0, p0 = np.asarray(init_contig, np.int64)[src], np.asarray(init_pos, np.int64)[src]
    step = p0[1:] - p0[:-1]
    forward = (step == 1) & (ori[1:] == 1) & (ori[:-1] == 1)
    backward = (step == -1) & (ori[1:] == -1) & (ori[:-1] == -1)
    joined = (contig[1:] == contig[:-1]) & (c0[1:] == c0[:-1]) & (forward | backward)
    head = np.concatenate([[0], np.nonzero(~joined)[0] + 1])
    tail = np.concatenate([head[1:] - 1, [bins.size - 1]])
    return dict(first=b["first"][head], last=b["last"][tail], first_bin=bins[head], last_bin=bins[tail])
