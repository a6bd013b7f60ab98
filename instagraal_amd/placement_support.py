"""Placement support: where the contacts say each bin belongs.  The junction profile (junction_profile.py) judges the joins the
sampler made, the join support (join_support.py) the joins between scaffold ends it did not make; this is the third question, at the
resolution the sampler works at: is this bin sitting in the wrong place, and if so, at which site of which scaffold do its contacts
concentrate?  The statistic needs no model: a bin's contacts with the flanks it has now are compared with its contacts with the
flanks it would have at another site, at the same distances; the bin's own coverage cancels in the ratio.  This module is the single
definition of the rule (pure numpy, no GPU); the device passes (``ig_placement_support``, csrc/ig_kernels_place.cuh) reproduce its
arrays byte for byte.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs in genome order, 0 .. T - 1.  The placed
contigs that are not rings are ``join_support.linear_runs``' runs k = 0 .. K - 1: first position start_k, n_k positions.

* GUEST: a placed bin of a linear contig; its positions [g0, g1] are consecutive in the order, n_g of them.  The REDUCED order of a
  guest is the order with those positions taken out: contig k has n'_k positions there, n_k - n_g for the guest's own contig.
* SITE (k, u), 0 <= u <= n'_k: the gap in front of reduced offset u of contig k (u = 0: off the head, u = n'_k: off the tail),
  ordered by (k, u).  A guest that is a whole contig has no site in its own contig.
* WINDOW w (``junction_profile.check_window``: 1 .. 1024) of a site: left = the reduced offsets [max(0, u - w), u - 1], right =
  [u, min(n'_k, u + w) - 1]; hosts = |left| + |right|.
* PROFILE: a contact of the uploaded strict upper triangle between two DIFFERENT bins, both ends placed in linear contigs, adds its
  count at the position of each end to the row of the other end's bin.  left_obs / right_obs of a site: the sums of the guest's
  row over the two parts of the window; obs = left_obs + right_obs.
* HOME: the site (k_g, g0 - start_{k_g}), where the guest sits now (home_hosts = 0 for a guest that is a whole contig).
* A site is ELIGIBLE if hosts >= min_hosts (1 .. 2 w, default w) and, in the guest's own contig, |u - u_home| >= 2 w (the window is
  then disjoint from home's).  Sites are compared by density with exact integers: x beats y iff obs_x hosts_y > obs_y hosts_x, on
  equality the lower (k, u) wins.  BEST: the maximum over the eligible sites with obs > 0 (none: best_contig = -1).
* RUNNER-UP (second_*): the same maximum over the eligible sites that lie in another contig than the best, or at least 2 w sites
  from it.

Per bin, arrays of length N: the int32 ``INT_ARRAYS`` (status: 0 guest, 1 unplaced, 2 on a ring) and the int64 ``LONG_ARRAYS``; rows
with status != 0 are zero with the contig fields at -1.  The scalars (int64, ``SCALARS``); a contact is classified by the first class
it fits: an end in a contig that is not placed, else an end on a ring, else both ends in one bin, else counted.  ``entries``: the
(contact, row) pairs before equal columns are summed.  By construction:

    unplaced + ring + within_bin + counted == sum(counts)
    entries == 2 * (number of counted contacts);  the sum of the whole profile == 2 * counted_observed
    w >= max n_k: a contig other than the guest's has one window, the whole contig, at every site: obs is the guest's total with
    that contig, and ties pick u = 0

Overflow guard: 2 w sum(counts) >= 2^62 is refused ("counts too large for this window"): obs * hosts stays below 2^62.

The device need not visit every site: between two consecutive EVENTS (an entry at reduced offset x enters the window on the right at
u = x - w + 1 and leaves it on the left at u = x + w + 1) obs is constant and hosts(u) is piecewise linear, so the density is
monotone on every stretch without an event or a kink, and its maximum -- the lowest u among equals -- is at an end of a stretch.
The stretch ends are stated once, in ``candidate_sites``; tests/test_placement_support_host.py holds them against the enumeration.
"""
from __future__ import annotations

import numpy as np

from . import join_support as js
from .junction_profile import DEFAULT_WINDOW, MAX_WINDOW, check_window, window_from_kb  # noqa: F401  (one definition: the junction profile's)

INT_ARRAYS = ("status", "contig", "offset", "n_positions", "home_hosts", "best_contig", "best_offset", "best_hosts", "second_contig",
              "second_offset", "second_hosts")
LONG_ARRAYS = ("home_left", "home_right", "best_left", "best_right", "second_left", "second_right")
ARRAYS = INT_ARRAYS + LONG_ARRAYS
CONTIG_FIELDS = ("contig", "best_contig", "second_contig")
# the order of ig_placement_support's scalars[7]
SCALARS = ("unplaced_observed", "ring_observed", "within_bin_observed", "counted_observed", "entries", "n_contigs", "n_guests")
OBSERVED_SCALARS = SCALARS[:4]
STATUS_GUEST, STATUS_UNPLACED, STATUS_RING = 0, 1, 2
WAVE_ENTRIES = 128  # PLACE_WAVE_ENTRIES of csrc/ig_kernels_place.cuh: rows of more summed entries get a wave in the scan, the others a thread
PLACEMENT_COLUMNS = ("bin", "scaffold", "offset", "n_positions", "home_density", "best_scaffold", "best_offset", "best_before", "best_after",
                     "best_density", "ratio", "second_ratio")
PLACEMENT_DTYPE = np.dtype([("bin", np.int64), ("scaffold", np.int64), ("offset", np.int64), ("n_positions", np.int64), ("home_density", np.float64),
                            ("best_scaffold", np.int64), ("best_offset", np.int64), ("best_before", np.int64), ("best_after", np.int64),
                            ("best_density", np.float64), ("ratio", np.float64), ("second_ratio", np.float64)])


def check_min_hosts(min_hosts, window):
    """-> min_hosts as an int (None: the window); ValueError unless it is a whole number in 1 .. 2 w"""
    w = check_window(window)
    if min_hosts is None:
        return w
    m = int(min_hosts)
    if m != min_hosts or not 1 <= m <= 2 * w:
        raise ValueError("placement support: 1 <= min_hosts <= 2 * window = %d (got %r)" % (2 * w, min_hosts))
    return m


def site_window(n_reduced, window, u):
    """the window of site u of a contig of ``n_reduced`` positions in the reduced order -> (lo, hi): left = [lo, u - 1],
    right = [u, hi - 1]; hosts = hi - lo.  Arrays or scalars."""
    u, n, w = np.asarray(u, np.int64), np.asarray(n_reduced, np.int64), np.int64(window)
    return np.maximum(0, u - w), np.minimum(n, u + w)


def eligible(n_reduced, window, min_hosts, u, home=None, exclude=None):
    """which of the sites ``u`` of one contig are eligible: hosts >= min_hosts, and at least 2 w sites from ``home`` (the guest's own
    contig) and from ``exclude`` (the runner-up: the best site, where it lies in this contig)"""
    u = np.asarray(u, np.int64)
    lo, hi = site_window(n_reduced, window, u)
    ok = (u >= 0) & (u <= n_reduced) & (hi - lo >= min_hosts)
    for z in (home, exclude):
        if z is not None:
            ok &= np.abs(u - int(z)) >= 2 * int(window)
    return ok


def candidate_sites(n_reduced, window, min_hosts, entries, home=None, exclude=None):
    """The sites of one contig (``n_reduced`` positions in the guest's reduced order) that can hold the maximum of the density
    over the eligible sites with obs > 0, lowest u among equals: -> the candidates 0 <= u <= n_reduced, ascending, each once
    (eligible or not: the caller filters).  ``entries``: the reduced offsets of the guest's row in this contig.

    Why these.  obs(u) changes only at an event: the entry at x is in the window of u iff x - w + 1 <= u <= x + w.  hosts(u) =
    min(n', u + w) - max(0, u - w) is linear between its kinks u = w and u = n' - w.  hosts is concave and symmetric, so
    {hosts >= min_hosts} is the interval [ua, n' - ua], ua = max(0, min_hosts - w) (empty where min(n', 2 w) < min_hosts); the
    exclusions cut the open intervals (z - 2 w, z + 2 w) out of it.  On a stretch of eligible sites without an event or a kink inside
    obs is constant and hosts is linear: the density is monotone (or constant: the lowest u wins), its maximum is at the first or
    the last site of the stretch.  A stretch begins at an event, at a kink or at the first site of an eligible interval and ends
    one site in front of an event, at a kink or at the last site of an eligible interval: four sites per entry and at most ten
    per contig."""
    n, w = int(n_reduced), int(window)
    x = np.asarray(entries, np.int64).ravel()
    ua = max(0, int(min_hosts) - w)
    fixed = [0, n, w, n - w, ua, n - ua]
    for z in (home, exclude):
        if z is not None:
            fixed += [int(z) - 2 * w, int(z) + 2 * w]
    u = np.concatenate([np.asarray(fixed, np.int64), x - w, x - w + 1, x + w, x + w + 1])
    return np.unique(u[(u >= 0) & (u <= n)])


def _argbest(obs, hosts, ok):
    """the index of the best site among ``ok`` with obs > 0 (-1: none).  The sites come in (k, u) order: only a strictly denser
    one replaces an earlier one.  Float densities shortlist, exact integers decide."""
    idx = np.nonzero(ok & (obs > 0))[0]
    if idx.size == 0:
        return -1
    d = obs[idx] / hosts[idx]
    short = idx[d >= d.max() * (1.0 - 1e-9)]
    best = int(short[0])
    for i in short[1:].tolist():
        if int(obs[i]) * int(hosts[best]) > int(obs[best]) * int(hosts[i]):
            best = i
    return best


def bin_records(run, position, parent, n_bins):
    """per bin: status, first position g0 (-1: not a guest), positions n_g.  ValueError unless a guest's positions are consecutive."""
    parent = np.asarray(parent, np.int64)
    N = int(n_bins)
    n_sub = np.bincount(parent, minlength=N).astype(np.int64)
    worst = np.full(N, 0, np.int64)  # the lowest run over the bin's sub-fragments: -2 a ring, -1 not placed
    np.minimum.at(worst, parent, np.minimum(run, 0))
    status = np.where(n_sub == 0, STATUS_UNPLACED, np.where(worst == -1, STATUS_UNPLACED, np.where(worst == -2, STATUS_RING, STATUS_GUEST)))
    big = np.iinfo(np.int64).max
    g0, g1 = np.full(N, big, np.int64), np.full(N, -1, np.int64)
    np.minimum.at(g0, parent, np.where(position >= 0, position, big))
    np.maximum.at(g1, parent, position)
    guest = status == STATUS_GUEST
    if np.any(g1[guest] - g0[guest] + 1 != n_sub[guest]):
        raise ValueError("placement support: the positions of a bin are not consecutive")
    return status.astype(np.int32), np.where(guest, g0, -1), np.where(guest, n_sub, 0)


def _frame(stot, contig, placed, position, parent, n_bins, row, col, cnt, window, min_hosts):
    """what the two statements of the rule below share: the checks, the runs, the records per bin, the classes of contact, the profile
    as CSR over the bins, the empty arrays"""
    w = check_window(window)
    mh = check_min_hosts(min_hosts, w)
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    parent = np.asarray(parent, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError("placement support: placed and position disagree")
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    if 2 * w * int(cnt.sum()) >= 1 << 62:
        raise ValueError("placement support: counts too large for this window")
    N = int(n_bins)
    members, start, length, run = js.linear_runs(stot, contig, position)
    K, T = int(start.size), int(members.size)
    status, g0, n_g = bin_records(run, position, parent, N)
    a, b = run[row], run[col]
    unpl = (a == -1) | (b == -1)
    ring = ~unpl & ((a == -2) | (b == -2))
    within = ~unpl & ~ring & (parent[row] == parent[col])
    counted = ~unpl & ~ring & ~within
    out = dict(window=w, min_hosts=mh, unplaced_observed=int(cnt[unpl].sum()), ring_observed=int(cnt[ring].sum()),
               within_bin_observed=int(cnt[within].sum()), counted_observed=int(cnt[counted].sum()), entries=2 * int(counted.sum()), n_contigs=K,
               n_guests=int((status == STATUS_GUEST).sum()), first_position=start.astype(np.int32), contig_positions=length.astype(np.int32))
    # the profile: the row of a bin, by position
    r, c, v = row[counted], col[counted], cnt[counted]
    e_bin = np.concatenate([parent[r], parent[c]])
    e_pos = np.concatenate([position[c], position[r]])
    e_cnt = np.concatenate([v, v])
    out["row_entries"] = np.bincount(e_bin, minlength=N).astype(np.int64)
    key = e_bin * max(T, 1) + e_pos
    uniq, inv = np.unique(key, return_inverse=True)
    summed = np.zeros(uniq.size, np.int64)
    np.add.at(summed, inv, e_cnt)
    p_bin, p_pos = uniq // max(T, 1), uniq % max(T, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(p_bin, minlength=N))]).astype(np.int64)
    out.update(rowptr=rowptr, col=p_pos.astype(np.int32), count=summed)
    res = {k: np.zeros(N, np.int32) for k in INT_ARRAYS}
    res.update({k: np.zeros(N, np.int64) for k in LONG_ARRAYS})
    res["status"][:] = status
    for k in CONTIG_FIELDS:
        res[k][:] = -1
    pos_run = np.repeat(np.arange(K, dtype=np.int64), length)  # the run of every position of a linear contig ...
    lin_pos = (np.repeat(start, length) + np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)).astype(np.int64)
    run_of_pos = np.full(T, -1, np.int64)
    run_of_pos[lin_pos] = pos_run
    out.update(res)
    return out, (w, mh, start, length, run_of_pos, status, g0, n_g, rowptr, p_pos, summed)


def support_host(stot, contig, placed, position, parent, n_bins, row, col, cnt, window, min_hosts=None):
    """The rule by plain enumeration of every site of every guest; dense over the positions (meant for small problems).

    stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order, -1 where
    not placed; parent: int [M], the bin of every sub-fragment; row, col, cnt: the contacts.  -> dict: window, min_hosts, the
    arrays of ARRAYS, the scalars of SCALARS, first_position and contig_positions (per contig k), and the profile as CSR over the
    bins (``rowptr``, ``col``, ``count``: equal columns summed; ``row_entries``: the entries per row before that)."""
    out, (w, mh, start, length, run_of_pos, status, g0, n_g, rowptr, p_pos, summed) = _frame(stot, contig, placed, position, parent, n_bins, row, col, cnt, window,
                                                                                       min_hosts)
    res, K, T = out, int(start.size), int(run_of_pos.size)
    for g in np.nonzero(status == STATUS_GUEST)[0].tolist():
        first, ng = int(g0[g]), int(n_g[g])
        kg = int(run_of_pos[first])
        uh = first - int(start[kg])
        dense = np.zeros(T, np.int64)
        dense[p_pos[rowptr[g]:rowptr[g + 1]]] = summed[rowptr[g]:rowptr[g + 1]]
        reduced = np.delete(dense, np.arange(first, first + ng))
        C = np.concatenate([[0], np.cumsum(reduced)])
        s_red = start - np.where(start > first, ng, 0)
        n_red = length.copy()
        n_red[kg] -= ng
        # every site of every contig, in (k, u) order; a guest that is a whole contig has no site in its own
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
    return out




def support_sparse(stot, contig, placed, position, parent, n_bins, row, col, cnt, window, min_hosts=None):
    """The same result the way the device computes it (csrc/ig_kernels_place.cuh), sparse over the positions: per guest only the
    candidate sites of its row's entries (``candidate_sites``), every window sum two binary searches in the ORIGINAL positions of the
    row and a difference of prefix sums -- the shift to the reduced order is monotone (``bound``).  For problems ``support_host`` is
    too dense for; tests/test_placement_support_host.py holds the two to the same bytes."""
    out, (w, mh, start, length, run_of_pos, status, g0, n_g, rowptr, p_pos, summed) = _frame(stot, contig, placed, position, parent, n_bins, row, col, cnt, window,
                                                                                       min_hosts)
    res = out
    for g in np.nonzero(status == STATUS_GUEST)[0].tolist():
        first, ng = int(g0[g]), int(n_g[g])
        kg = int(run_of_pos[first])
        uh = first - int(start[kg])
        P = p_pos[rowptr[g]:rowptr[g + 1]]
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
    return out


def observed_total(result):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(result[k]) for k in OBSERVED_SCALARS)


def densities(result):
    """-> dict of f64 [N]: ``home_density`` and ``best_density`` (obs / (n_positions * hosts); 0 where there is no such site),
    ``ratio`` = best_density / home_density (inf where home is 0 with a best site, nan with neither), ``second_ratio`` = the
    runner-up's density over the best's (nan without a best site).  Bins that are no guests: nan everywhere."""
    n = np.asarray(result["n_positions"], np.float64)
    guest = np.asarray(result["status"]) == STATUS_GUEST

    def dens(which):
        obs = np.asarray(result[which + "_left"], np.float64) + np.asarray(result[which + "_right"], np.float64)
        area = n * np.asarray(result[which + "_hosts"], np.float64)
        d = np.zeros(n.size)
        np.divide(obs, area, out=d, where=area > 0)
        return np.where(guest, d, np.nan)

    home, best, second = dens("home"), dens("best"), dens("second")
    has_best = guest & (np.asarray(result["best_contig"]) >= 0)
    ratio = np.full(n.size, np.nan)
    np.divide(best, home, out=ratio, where=guest & (home > 0))
    ratio[has_best & (home == 0)] = np.inf
    second_ratio = np.full(n.size, np.nan)
    np.divide(second, best, out=second_ratio, where=has_best)
    return dict(home_density=home, best_density=best, ratio=ratio, second_ratio=second_ratio)


def contig_table(result, order, parent):
    """per contig k, from the result's own arrays and the genome order: (first position, positions)"""
    K = int(result["n_contigs"])
    order, parent = np.asarray(order, np.int64), np.asarray(parent, np.int64)
    first_of_bin = np.full(np.asarray(result["status"]).size, -1, np.int64)
    first_of_bin[parent[order[::-1]]] = np.arange(order.size - 1, -1, -1)
    guest = np.nonzero(np.asarray(result["status"]) == STATUS_GUEST)[0]
    k = np.asarray(result["contig"], np.int64)[guest]
    start, n = np.zeros(K, np.int64), np.zeros(K, np.int64)
    start[k] = first_of_bin[guest] - np.asarray(result["offset"], np.int64)[guest]
    np.add.at(n, k, np.asarray(result["n_positions"], np.int64)[guest])
    return start, n


def sites_for_people(result, order, parent, contig_of_bin):
    """the sites translated: -> dict of int64 [N]: ``scaffold`` (the canonical id of the guest's scaffold: its name is
    ``assembly_contacts.scaffold_names``'), and for which in (best, second): ``<which>_scaffold``, ``<which>_before`` and
    ``<which>_after``, the bins in front of and behind the site in the reduced order (-1: none -- off an end, or no such site)."""
    order, parent = np.asarray(order, np.int64), np.asarray(parent, np.int64)
    contig_of_bin = np.asarray(contig_of_bin, np.int64)
    start, n = contig_table(result, order, parent)
    N = np.asarray(result["status"]).size
    kg, uh, ng = (np.asarray(result[k], np.int64) for k in ("contig", "offset", "n_positions"))
    out = dict(scaffold=np.where(kg >= 0, contig_of_bin[np.arange(N)], -1))
    for which in ("best", "second"):
        k, u = np.asarray(result[which + "_contig"], np.int64), np.asarray(result[which + "_offset"], np.int64)
        have = k >= 0
        ks = np.where(have, k, 0)
        s0, n_red = (start[ks], n[ks] - np.where(ks == kg, ng, 0)) if start.size else (np.zeros(N, np.int64), np.zeros(N, np.int64))
        own = have & (ks == kg)

        def bin_at(r, ok):
            p = np.clip(s0 + r + np.where(own & (r >= uh), ng, 0), 0, max(order.size - 1, 0))
            return np.where(ok, parent[order[p]] if order.size else -1, -1)

        out[which + "_before"] = bin_at(u - 1, have & (u >= 1))
        out[which + "_after"] = bin_at(u, have & (u < n_red))
        anchor = np.where(out[which + "_after"] >= 0, out[which + "_after"], out[which + "_before"])
        out[which + "_scaffold"] = np.where(anchor >= 0, contig_of_bin[np.maximum(anchor, 0)], -1)
    return out


def misplaced_bins(result, n=20, min_ratio=1.0):
    """the ``n`` guests with the highest ``ratio`` above ``min_ratio`` as a PLACEMENT_DTYPE array: inf first, ties by bin id.
    ``result``: what ``sampler.placement_support`` returns."""
    ratio = np.asarray(result["ratio"], np.float64)
    ok = np.nonzero((np.asarray(result["status"]) == STATUS_GUEST) & (np.asarray(result["best_contig"]) >= 0) & (ratio > float(min_ratio)))[0]
    pick = ok[np.argsort(-ratio[ok], kind="stable")[:max(int(n), 0)]]
    t = np.zeros(pick.size, PLACEMENT_DTYPE)
    t["bin"] = pick
    for k in PLACEMENT_COLUMNS[1:]:
        t[k] = np.asarray(result[k])[pick]
    return t


def write_placements(path, result, n=None, min_ratio=1.0):
    """the ranked table (every bin above ``min_ratio``, or the first ``n``), one line per bin: the columns of PLACEMENT_COLUMNS with
    the scaffolds by the names of genome.fasta and ``-`` for no bin; then the window, min_hosts and the scalars."""
    from .assembly_contacts import scaffold_names

    t = misplaced_bins(result, np.asarray(result["status"]).size if n is None else n, min_ratio)
    name = lambda c: scaffold_names([c])[0] if c >= 0 else "-"  # noqa: E731
    some = lambda b: str(int(b)) if b >= 0 else "-"  # noqa: E731
    with open(path, "w") as f:
        f.write("# " + " ".join(PLACEMENT_COLUMNS) + "\n")
        for r in t:
            f.write("%d %s %d %d %.9g %s %d %s %s %.9g %.9g %.9g\n" % (r["bin"], name(r["scaffold"]), r["offset"], r["n_positions"], r["home_density"],
                                                                    name(r["best_scaffold"]), r["best_offset"], some(r["best_before"]),
                                                                    some(r["best_after"]), r["best_density"], r["ratio"], r["second_ratio"]))
        f.write("# window=%d min_hosts=%d " % (result["window"], result["min_hosts"]) + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")
    return int(t.size)
