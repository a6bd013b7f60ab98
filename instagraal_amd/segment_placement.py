"""Segment placement support: where the contacts say a run of bins belongs, and which way round.  Placement support
(placement_support.py) judges single bins; a block of several bins that sits in the wrong place as a unit is invisible to it -- the
interior bins of the block find their neighbours, the rest of the block, at home.  Here the guest is a SEGMENT of the genome order: a
co-linear block, a whole scaffold or the caller's interval.  This module is the single definition of the rule (pure numpy, no GPU);
the device passes (``ig_segment_placement``, csrc/ig_kernels_segplace.cuh) reproduce its arrays byte for byte.

The rule.  Positions and runs are placement support's: the POSITIONS are the contact map's, 0 .. T - 1, the placed contigs that are
not rings are ``join_support.linear_runs``' runs k = 0 .. K - 1.  The SEGMENTS are orientation support's: n_seg intervals
[first_i, last_i] of positions, ascending, disjoint, each inside one placed contig; they need not cover the order
(``orientation_support.check_segments``).

* GUEST: a segment of a linear contig, n_g = last - first + 1 positions from g0 = first.  A segment on a ring has status 2, its rows
  are zero and its contig fields -1, as for a bin on a ring.
* REDUCED order, SITE (k, u), WINDOW, hosts, HOME, ELIGIBLE (hosts >= min_hosts; in the guest's own contig |u - u_home| >= 2 w), the
  exact comparison with the lower (k, u) among equals, BEST and RUNNER-UP: word for word placement_support's, with "bin" read as
  "segment".  A guest that is a whole contig has no site in its own contig and home_hosts = 0.
* PROFILE: a contact of the uploaded strict upper triangle lies at positions pa and pb; sa = seg(pa), sb = seg(pb), -1 outside every
  segment.  It is classified by the first class that fits: ``unplaced`` (an end in a contig that is not placed), ``ring`` (an end on a
  ring), ``within_segment`` (sa == sb >= 0), ``counted`` (sa >= 0 or sb >= 0), ``uncounted`` (both ends outside every segment).  A
  counted contact adds its count at pb to the row of sa if sa >= 0 and its count at pa to the row of sb if sb >= 0; positions outside
  every segment are hosts only.  ``entries`` is the number of such additions.
* QUADRANTS: the ARM of a guest is orientation support's, m = min(n_g // 2, w): the head arm is [g0, g0 + m - 1], the tail arm
  [g1 - m + 1, g1].  For each of the three sites (home, best, second) four int64 sums HL, HR, TL, TR: the counts of the guest's row
  whose OWN end lies in the head (H) or tail (T) arm and whose other end lies in the left or right part of that site's window; own
  ends in the interior go to no quadrant, a site that does not exist has four zeros.  keep = HL + TR joins each arm with the part of
  the window on its own side, flip = HR + TL with the other part; both classes have m * hosts position pairs and compare without a
  model.

Per segment: the int32 ``INT_ARRAYS`` (placement_support's plus ``arm``) and the int64 ``LONG_ARRAYS`` plus ``quadrants``
[n_seg, 3, 4]; the scalars (int64, ``SCALARS``).  By construction:

    unplaced + ring + within_segment + counted + uncounted == sum(counts)
    (number of counted contacts) <= entries <= 2 * (number of counted contacts)
    HL + TL <= left and HR + TR <= right at every site; both are equalities for a guest with n_g == 2 m
    reversing a guest in place swaps HL <-> TL and HR <-> TR at every site and changes nothing else
    at home: (HL, HR, TL, TR) == orientation_support.support_host(...)["observed"] row (LL, LR, RL, RR), same segments, same w
    with bin_segments of the whole order: every array of placement_support.ARRAYS at segment i == the bin-level array at bin
        first_bin[i]; uncounted == 0, within_segment == within_bin, entries and the other class scalars equal

Overflow guard: placement support's, 2 w sum(counts) >= 2^62 is refused; a quadrant is a part of obs.
"""
from __future__ import annotations

import numpy as np

from . import join_support as js
from . import orientation_support as osup
from . import placement_support as ps
from .junction_profile import contig_runs
from .orientation_support import bin_segments, block_segments  # noqa: F401  (the segment builders are orientation support's)
from .placement_support import DEFAULT_WINDOW, MAX_WINDOW, WAVE_ENTRIES, _argbest, candidate_sites, check_min_hosts, check_window, eligible, site_window, window_from_kb  # noqa: F401

NAME = "segment placement"
INT_ARRAYS = ps.INT_ARRAYS + ("arm",)
LONG_ARRAYS = ps.LONG_ARRAYS
ARRAYS = INT_ARRAYS + LONG_ARRAYS
CONTIG_FIELDS = ps.CONTIG_FIELDS
# the order of ig_segment_placement's scalars[9]
SCALARS = ("unplaced_observed", "ring_observed", "within_segment_observed", "counted_observed", "uncounted_observed", "entries", "n_contigs", "n_guests",
           "n_placed")
OBSERVED_SCALARS = SCALARS[:5]
STATUS_GUEST, STATUS_RING = ps.STATUS_GUEST, ps.STATUS_RING
SITES = ("home", "best", "second")  # the second axis of ``quadrants``
HL, HR, TL, TR = 0, 1, 2, 3         # the third: (arm of the guest, part of the window)
VERDICTS = ("as_placed", "reversed", "undecided")
SEGMENT_COLUMNS = ("segment", "first_bin", "last_bin", "scaffold", "offset", "n_positions", "home_density", "best_scaffold", "best_offset", "best_before",
                   "best_after", "best_density", "ratio", "second_ratio")
SEGMENT_DTYPE = np.dtype([(k, np.float64 if k in ("home_density", "best_density", "ratio", "second_ratio") else np.int64) for k in SEGMENT_COLUMNS])
FILE_COLUMNS = SEGMENT_COLUMNS + ("best_keep", "best_flip", "best_verdict")


def check_segments(first, last, n_placed, contig_start):
    """``orientation_support.check_segments`` under this report's name"""
    try:
        return osup.check_segments(first, last, n_placed, contig_start)
    except ValueError as e:
        raise ValueError(str(e).replace("orientation support", NAME)) from None


def scaffold_segments(order, contig_start, contig_end, ring):
    """one segment per linear placed contig -> dict: first, last (positions).  ``order``: the sub-fragment at every position (its length
    is what is read); contig_start, contig_end, ring: per position, as ``orientation_support.segment_geometry`` takes them"""
    T = int(np.asarray(order).size)
    cs, ce = np.asarray(contig_start, np.int64)[:T], np.asarray(contig_end, np.int64)[:T]
    head = np.nonzero((cs == np.arange(T)) & ~np.asarray(ring, bool)[:T])[0].astype(np.int64)
    return dict(first=head, last=ce[head] - 1)


def _frame(stot, contig, placed, position, row, col, cnt, first, last, window, min_hosts):
    """what the two statements of the rule share: the checks, the runs, the record per segment, the classes of contact, the additions
    (segment, own position, other position, count), the profile as CSR over the segments, the empty arrays"""
    w = check_window(window)
    try:
        mh = check_min_hosts(min_hosts, w)
    except ValueError as e:
        raise ValueError(str(e).replace("placement support", NAME)) from None
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError(NAME + ": placed and position disagree")
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    if 2 * w * int(cnt.sum()) >= 1 << 62:
        raise ValueError(NAME + ": counts too large for this window")
    members, start, length, run = js.linear_runs(stot, contig, position)
    K, T = int(start.size), int(members.size)
    _, all_start, all_length = contig_runs(contig, position)
    first, last = check_segments(first, last, T, np.repeat(all_start, all_length))
    n_seg = int(first.size)
    run_of_pos = run[members] if T else np.zeros(0, np.int64)  # -2: on a ring
    n_pos = last - first + 1
    seg = np.full(T, -1, np.int64)
    seg[np.repeat(first - (np.cumsum(n_pos) - n_pos), n_pos) + np.arange(int(n_pos.sum()), dtype=np.int64)] = np.repeat(np.arange(n_seg, dtype=np.int64), n_pos)
    status = np.where(run_of_pos[first] < 0, STATUS_RING, STATUS_GUEST).astype(np.int32) if n_seg else np.zeros(0, np.int32)
    a, b = run[row], run[col]
    unpl = (a == -1) | (b == -1)
    ring = ~unpl & ((a == -2) | (b == -2))
    lin = ~unpl & ~ring
    pa, pb = position[row], position[col]
    seg_at = lambda p: np.where(lin, seg[np.where(lin, p, 0)], -1) if T else np.full(row.size, -1, np.int64)  # noqa: E731  (-1: outside every segment)
    sa, sb = seg_at(pa), seg_at(pb)
    within = lin & (sa >= 0) & (sa == sb)
    counted = lin & ~within & ((sa >= 0) | (sb >= 0))
    uncounted = lin & ~within & ~counted
    ea, eb = counted & (sa >= 0), counted & (sb >= 0)
    e_seg = np.concatenate([sa[ea], sb[eb]])
    e_own = np.concatenate([pa[ea], pb[eb]])
    e_pos = np.concatenate([pb[ea], pa[eb]])
    e_cnt = np.concatenate([cnt[ea], cnt[eb]])
    out = dict(window=w, min_hosts=mh, n_seg=n_seg, first=first, last=last, unplaced_observed=int(cnt[unpl].sum()), ring_observed=int(cnt[ring].sum()),
               within_segment_observed=int(cnt[within].sum()), counted_observed=int(cnt[counted].sum()), uncounted_observed=int(cnt[uncounted].sum()),
               entries=int(e_seg.size), n_contigs=K, n_guests=int((status == STATUS_GUEST).sum()), n_placed=T, n_counted_contacts=int(counted.sum()),
               first_position=start.astype(np.int32), contig_positions=length.astype(np.int32))
    out["row_entries"] = np.bincount(e_seg, minlength=n_seg).astype(np.int64)
    key = e_seg * max(T, 1) + e_pos
    uniq, inv = np.unique(key, return_inverse=True)
    summed = np.zeros(uniq.size, np.int64)
    np.add.at(summed, inv.ravel(), e_cnt)
    p_seg, p_pos = uniq // max(T, 1), uniq % max(T, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(p_seg, minlength=n_seg))]).astype(np.int64)
    out.update(rowptr=rowptr, col=p_pos.astype(np.int32), count=summed)
    res = {k: np.zeros(n_seg, np.int32) for k in INT_ARRAYS}
    res.update({k: np.zeros(n_seg, np.int64) for k in LONG_ARRAYS})
    res["status"][:] = status
    for k in CONTIG_FIELDS:
        res[k][:] = -1
    guest = status == STATUS_GUEST
    res["arm"][:] = np.where(guest, np.minimum(n_pos // 2, w), 0)
    out.update(res)
    return out, (w, mh, start, length, run_of_pos, status, rowptr, p_pos, summed, (e_seg, e_own, e_pos, e_cnt))


def site_bounds(result, first_position, contig_positions):
    """the three sites of every segment as bounds in the ORIGINAL positions -> (lo, mid, hi), int64 [n_seg, 3]: the left part of the
    window is lo <= q < mid, the right part mid <= q < hi (a guest's own positions never hold the other end of an entry of its row, so
    that is the whole test, at home too); a site that does not exist has lo = mid = hi = 0"""
    start, length = np.asarray(first_position, np.int64), np.asarray(contig_positions, np.int64)
    w = int(result["window"])
    kg, uh, ng = (np.asarray(result[k], np.int64) for k in ("contig", "offset", "n_positions"))
    n_seg = kg.size
    lo, mid, hi = (np.zeros((n_seg, 3), np.int64) for _ in range(3))
    if start.size == 0:
        return lo, mid, hi
    for s, which in enumerate(SITES):
        k = kg if which == "home" else np.asarray(result[which + "_contig"], np.int64)
        u = uh if which == "home" else np.asarray(result[which + "_offset"], np.int64)
        have = k >= 0
        ks = np.where(have, k, 0)
        own = ks == kg
        n_red = length[ks] - np.where(own, ng, 0)
        a, b = site_window(n_red, w, u)
        bound = lambda v: start[ks] + v + np.where(own & (v > uh), ng, 0)  # noqa: E731
        lo[:, s], mid[:, s], hi[:, s] = (np.where(have, bound(v), 0) for v in (a, u, b))
    return lo, mid, hi


def _quadrants(out, additions):
    """the pass over the additions: own end in an arm, other end in a part of a site's window"""
    e_seg, e_own, e_pos, e_cnt = additions
    n_seg = int(out["n_seg"])
    quad = np.zeros((n_seg, 3, 4), np.int64)
    if n_seg and e_seg.size:
        lo, mid, hi = site_bounds(out, out["first_position"], out["contig_positions"])
        m = np.asarray(out["arm"], np.int64)[e_seg]
        head, tail = e_own < out["first"][e_seg] + m, e_own > out["last"][e_seg] - m
        for s in range(3):
            left = (e_pos >= lo[e_seg, s]) & (e_pos < mid[e_seg, s])
            right = (e_pos >= mid[e_seg, s]) & (e_pos < hi[e_seg, s])
            for q, take in ((HL, head & left), (HR, head & right), (TL, tail & left), (TR, tail & right)):
                np.add.at(quad[:, s, q], e_seg[take], e_cnt[take])
    out["quadrants"] = quad
    return out


def support_host(stot, contig, placed, position, row, col, cnt, first, last, window, min_hosts=None):
    """The rule by plain enumeration of every site of every guest; dense over the positions (meant for small problems).

    stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order, -1 where
    not placed; row, col, cnt: the contacts; first, last: the segments.  -> dict: window, min_hosts, n_seg, first, last, the arrays of
    ARRAYS, ``quadrants``, the scalars of SCALARS, first_position and contig_positions (per contig k), and the profile as CSR over
    the segments (``rowptr``, ``col``, ``count``: equal columns summed; ``row_entries``: the entries per row before that)."""
    out, (w, mh, start, length, run_of_pos, status, rowptr, p_pos, summed, additions) = _frame(stot, contig, placed, position, row, col, cnt, first, last, window,
                                                                                           min_hosts)
    res, K, T = out, int(start.size), int(run_of_pos.size)
    for g in np.nonzero(status == STATUS_GUEST)[0].tolist():
        g0, ng = int(out["first"][g]), int(out["last"][g] - out["first"][g] + 1)
        kg = int(run_of_pos[g0])
        uh = g0 - int(start[kg])
        dense = np.zeros(T, np.int64)
        dense[p_pos[rowptr[g]:rowptr[g + 1]]] = summed[rowptr[g]:rowptr[g + 1]]
        reduced = np.delete(dense, np.arange(g0, g0 + ng))
        C = np.concatenate([[0], np.cumsum(reduced)])
        s_red = start - np.where(start > g0, ng, 0)
        n_red = length.copy()
        n_red[kg] -= ng
        n_sites = np.where((np.arange(K) == kg) & (n_red == 0), 0, n_red + 1)
        sk = np.repeat(np.arange(K, dtype=np.int64), n_sites)
        su = np.arange(int(n_sites.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_sites) - n_sites, n_sites)
        lo, hi = site_window(n_red[sk], w, su)
        left = C[s_red[sk] + su] - C[s_red[sk] + lo]
        right = C[s_red[sk] + hi] - C[s_red[sk] + su]
        hosts, obs = hi - lo, left + right
        res["contig"][g], res["offset"][g], res["n_positions"][g] = kg, uh, ng
        if n_red[kg] > 0:
            h = int(np.nonzero((sk == kg) & (su == uh))[0][0])
            res["home_hosts"][g], res["home_left"][g], res["home_right"][g] = hosts[h], left[h], right[h]
        ok = (hosts >= mh) & ~((sk == kg) & (np.abs(su - uh) < 2 * w))
        i = _argbest(obs, hosts, ok)
        if i < 0:
            continue
        res["best_contig"][g], res["best_offset"][g], res["best_hosts"][g] = sk[i], su[i], hosts[i]
        res["best_left"][g], res["best_right"][g] = left[i], right[i]
        j = _argbest(obs, hosts, ok & ~((sk == sk[i]) & (np.abs(su - su[i]) < 2 * w)))
        if j < 0:
            continue
        res["second_contig"][g], res["second_offset"][g], res["second_hosts"][g] = sk[j], su[j], hosts[j]
        res["second_left"][g], res["second_right"][g] = left[j], right[j]
    return _quadrants(out, additions)


def support_sparse(stot, contig, placed, position, row, col, cnt, first, last, window, min_hosts=None):
    """The same result the way the device computes it (csrc/ig_kernels_segplace.cuh), sparse over the positions: per guest only the
    candidate sites of its row's entries (``candidate_sites``), every window sum two binary searches in the ORIGINAL positions of the
    row and a difference of prefix sums, then a pass over the contacts for the quadrants.  tests/test_segment_placement_host.py holds
    the two to the same bytes."""
    out, (w, mh, start, length, run_of_pos, status, rowptr, p_pos, summed, additions) = _frame(stot, contig, placed, position, row, col, cnt, first, last, window,
                                                                                           min_hosts)
    res = out
    for g in np.nonzero(status == STATUS_GUEST)[0].tolist():
        g0, ng = int(out["first"][g]), int(out["last"][g] - out["first"][g] + 1)
        kg = int(run_of_pos[g0])
        uh = g0 - int(start[kg])
        P = p_pos[rowptr[g]:rowptr[g + 1]].astype(np.int64)
        pre = np.concatenate([[0], np.cumsum(summed[rowptr[g]:rowptr[g + 1]])])

        def windows(k, u):
            """left, right, hosts of the sites (k, u)"""
            s0, n_red = start[k], length[k] - np.where(k == kg, ng, 0)
            lo, hi = site_window(n_red, w, u)
            bound = lambda v: s0 + v + np.where((k == kg) & (v > uh), ng, 0)  # noqa: E731
            a, m, b = (pre[np.searchsorted(P, bound(v), side="left")] for v in (lo, u, hi))
            return m - a, b - m, hi - lo

        res["contig"][g], res["offset"][g], res["n_positions"][g] = kg, uh, ng
        left, right, hosts = windows(np.array([kg]), np.array([uh]))
        res["home_hosts"][g], res["home_left"][g], res["home_right"][g] = hosts[0], left[0], right[0]
        ke = run_of_pos[P]
        own = ke == kg
        x = P - start[ke] - np.where(own & (P - start[ke] > uh), ng, 0)
        zone = None
        for which in ("best", "second"):
            ks, us = [], []
            for k in np.unique(ke).tolist():
                n_red = int(length[k]) - (ng if k == kg else 0)
                u = candidate_sites(n_red, w, mh, x[ke == k], home=uh if k == kg else None, exclude=zone[1] if zone and zone[0] == k else None)
                u = u[eligible(n_red, w, mh, u, home=uh if k == kg else None, exclude=zone[1] if zone and zone[0] == k else None)]
                ks.append(np.full(u.size, k, np.int64))
                us.append(u)
            if not ks:
                break
            sk, su = np.concatenate(ks), np.concatenate(us)
            left, right, hosts = windows(sk, su)
            i = _argbest(left + right, hosts, np.ones(sk.size, bool))
            if i < 0:
                break
            res[which + "_contig"][g], res[which + "_offset"][g], res[which + "_hosts"][g] = sk[i], su[i], hosts[i]
            res[which + "_left"][g], res[which + "_right"][g] = left[i], right[i]
            zone = (int(sk[i]), int(su[i]))
    return _quadrants(out, additions)


def observed_total(result):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(result[k]) for k in OBSERVED_SCALARS)


def densities(result):
    """-> dict of f64 [n_seg]: ``home_density``, ``best_density``, ``ratio`` and ``second_ratio`` as ``placement_support.densities``
    defines them, with the guest's n_g for n_positions"""
    return ps.densities(result)


def orientation_at(result):
    """the orientation the contacts give every guest at each of its three sites -> dict: ``keep`` = HL + TR, ``flip`` = HR + TL (int64
    [n_seg, 3], the sites in the order of SITES) and ``verdict`` ([n_seg, 3] of VERDICTS: "undecided" where keep == flip or the
    guest has no arm)"""
    q = np.asarray(result["quadrants"], np.int64).reshape(-1, 3, 4)
    keep, flip = q[:, :, HL] + q[:, :, TR], q[:, :, HR] + q[:, :, TL]
    arm = np.asarray(result["arm"], np.int64)[:, None]
    verdict = np.where((arm == 0) | (keep == flip), "undecided", np.where(keep > flip, "as_placed", "reversed"))
    return dict(keep=keep, flip=flip, verdict=verdict)


def sites_for_people(result, order, parent, contig_of_bin, first_position=None, contig_positions=None):
    """the segments and their sites translated -> dict of int64 [n_seg]: ``first_bin``, ``last_bin`` (the bins at the segment's ends, as
    orientation support reports them), ``scaffold`` (the canonical id of the guest's scaffold, -1: no guest) and for which in (best,
    second): ``<which>_scaffold``, ``<which>_before`` and ``<which>_after``, the bins in front of and behind the site in the reduced
    order (-1: none).  first_position, contig_positions: per linear contig k (default: the result's own)"""
    order, parent = np.asarray(order, np.int64), np.asarray(parent, np.int64)
    contig_of_bin = np.asarray(contig_of_bin, np.int64)
    start = np.asarray(result["first_position"] if first_position is None else first_position, np.int64)
    n = np.asarray(result["contig_positions"] if contig_positions is None else contig_positions, np.int64)
    first, last = np.asarray(result["first"], np.int64), np.asarray(result["last"], np.int64)
    n_seg = first.size
    at = parent[order]
    kg, uh, ng = (np.asarray(result[k], np.int64) for k in ("contig", "offset", "n_positions"))
    out = dict(first_bin=at[first], last_bin=at[last])
    out["scaffold"] = np.where(kg >= 0, contig_of_bin[out["first_bin"]] if n_seg else -1, -1)
    for which in ("best", "second"):
        k, u = np.asarray(result[which + "_contig"], np.int64), np.asarray(result[which + "_offset"], np.int64)
        have = k >= 0
        ks = np.where(have, k, 0)
        s0, n_red = (start[ks], n[ks] - np.where(ks == kg, ng, 0)) if start.size else (np.zeros(n_seg, np.int64), np.zeros(n_seg, np.int64))
        own = have & (ks == kg)

        def bin_at(r, ok):
            p = np.clip(s0 + r + np.where(own & (r >= uh), ng, 0), 0, max(order.size - 1, 0))
            return np.where(ok, at[p] if order.size else -1, -1)

        out[which + "_before"] = bin_at(u - 1, have & (u >= 1))
        out[which + "_after"] = bin_at(u, have & (u < n_red))
        anchor = np.where(out[which + "_after"] >= 0, out[which + "_after"], out[which + "_before"])
        out[which + "_scaffold"] = np.where(anchor >= 0, contig_of_bin[np.maximum(anchor, 0)], -1)
    return out


def misplaced_segments(result, n=20, min_ratio=1.0):
    """the ``n`` guests with the highest ``ratio`` above ``min_ratio`` as a SEGMENT_DTYPE array: inf first, ties by segment index.
    ``result``: what ``sampler.segment_placement`` returns"""
    ratio = np.asarray(result["ratio"], np.float64)
    ok = np.nonzero((np.asarray(result["status"]) == STATUS_GUEST) & (np.asarray(result["best_contig"]) >= 0) & (ratio > float(min_ratio)))[0]
    pick = ok[np.argsort(-ratio[ok], kind="stable")[:max(int(n), 0)]]
    t = np.zeros(pick.size, SEGMENT_DTYPE)
    t["segment"] = pick
    for k in SEGMENT_COLUMNS[1:]:
        t[k] = np.asarray(result[k])[pick]
    return t


def write_segment_placements(path, result, n=None, min_ratio=1.0, mode="w", title=None):
    """the ranked table (every segment above ``min_ratio``, or the first ``n``), one line per segment: the columns of SEGMENT_COLUMNS
    with the scaffolds by the names of genome.fasta and ``-`` for no bin, then the best site's keep, flip and verdict; then the window,
    min_hosts and the scalars (``mode="a"``: behind what the file holds already; ``title``: a comment line in front)"""
    from .assembly_contacts import scaffold_names

    t = misplaced_segments(result, np.asarray(result["status"]).size if n is None else n, min_ratio)
    at = result if "verdict" in result else orientation_at(result)
    name = lambda c: scaffold_names([c])[0] if c >= 0 else "-"  # noqa: E731
    some = lambda b: str(int(b)) if b >= 0 else "-"  # noqa: E731
    with open(path, mode) as f:
        if title:
            f.write("# %s\n" % title)
        f.write("# " + " ".join(FILE_COLUMNS) + "\n")
        for r in t:
            i = int(r["segment"])
            f.write("%d %d %d %s %d %d %.9g %s %d %s %s %.9g %.9g %.9g %d %d %s\n" % (
                i, r["first_bin"], r["last_bin"], name(r["scaffold"]), r["offset"], r["n_positions"], r["home_density"], name(r["best_scaffold"]),
                r["best_offset"], some(r["best_before"]), some(r["best_after"]), r["best_density"], r["ratio"], r["second_ratio"],
                int(at["keep"][i, 1]), int(at["flip"][i, 1]), at["verdict"][i, 1]))
        f.write("# window=%d min_hosts=%d " % (result["window"], result["min_hosts"]) + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")
    return int(t.size)
