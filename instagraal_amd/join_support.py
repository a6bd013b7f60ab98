"""Join support: which scaffold ends the contacts of the current genome would link.  The junction profile (junction_profile.py)
judges the joins the sampler made; this is the same question for the joins it did NOT make: for every pair of scaffold ends the
contacts that would span the join inside a window, the sub-fragment pairs that could, and what the model in use would expect of
them if the two ends were adjacent.  This module is the single definition of the rule (pure numpy, no GPU); the device passes
(``ig_join_support_build``, csrc/ig_kernels_join.cuh) reproduce it entry for entry.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs in genome order, 0 .. T - 1.  The placed
contigs that are not rings are runs k = 0 .. K - 1 of that order (in that order), first position start_k, n_k positions.  A contig
has two ENDS, e = 2 k + side: side 0 is the head (position start_k), side 1 the tail.  The DEPTH of position r of contig k is
r - start_k at the head and start_k + n_k - 1 - r at the tail.  ``window`` w is counted in positions, 1 <= w <= MAX_WINDOW
(junction_profile's).

* observed: a contact of the uploaded strict upper triangle whose ends are placed in two DIFFERENT linear contigs a != b at the
  positions pa, pb has, for each of the four (sa, sb), gap = depth(pa, sa) + depth(pb, sb) + 1: the separation in positions the two
  would have if end (a, sa) were joined to end (b, sb).  Where gap <= w the contact adds its count to the LINK (lo, hi) = (min, max)
  of the two end ids.  One contact counts for up to four links (contigs shorter than the window).
* pairs(link): the position pairs (i in a, j in b) with depth(i, sa) + depth(j, sb) + 1 <= w (closed form: ``pairs_closed_form``).
* expected_q(link): the sum over those pairs of the model's value at s = depth_kb(i, sa) + depth_kb(j, sb) (an f32 sum), quantised
  to a multiple of 2^-32 and added as a 64-bit integer; depth_kb(i, 0) = dist_i, depth_kb(i, 1) = fabsf(L_kb - dist_i) with
  L_kb = (float) l_cont_bp / 1000.0f, l_cont_bp the contig's length in bp: the separation the coordinates would give behind the
  join with no gap between the scaffolds.  expected = expected_q / 2^32, ratio = observed / expected.

Only links with at least one contact are listed, as CSR over the 2 K ends: ``rowptr`` (int64 [2 K + 1]), ``col`` (int32, strictly
ascending inside a row), ``observed``, ``pairs``, ``expected_q`` (int64 per link).

The scalars (int64, SCALARS): a contact with an end in a contig that is not placed is ``unplaced``; else one with an end in a ring
is ``ring``; else one with both ends in the same contig is ``cis``; what is left -- trans between linear placed contigs -- is
``in_reach`` if it counts for at least one link, else ``out_of_reach``.  ``contributions`` = sum of count * number of links the
contact counts for.  By construction:

    in_reach + out_of_reach + cis + ring + unplaced == sum(counts)
    sum(observed) == contributions
    w >= n_a + n_b - 1 for every pair of contigs  =>  contributions == 4 (in_reach + out_of_reach), out_of_reach == 0
    w == 1  =>  observed of a link is the count of the one contact between the two end sub-fragments, pairs == 1
"""
from __future__ import annotations

import numpy as np

from . import junction_profile as jp
from .junction_profile import MAX_WINDOW, Q_ONE, check_window, window_from_kb  # noqa: F401  (one definition: the junction profile's)

DEFAULT_WINDOW = jp.DEFAULT_WINDOW
# the order of ig_join_support_build's scalars[8]
SCALARS = ("in_reach_observed", "out_of_reach_observed", "cis_observed", "ring_observed", "unplaced_observed", "contributions",
           "n_contigs", "n_links")
OBSERVED_SCALARS = SCALARS[:5]
SUMMED_SCALARS = SCALARS[:6]  # what the shards of a sharded handle add up in
LINK_ARRAYS = ("col", "observed", "pairs", "expected_q")
ENDS_DTYPE = np.dtype([("scaffold", np.int64), ("side", np.int64), ("bin", np.int64), ("sub_frag", np.int64), ("n_positions", np.int64),
                       ("length_bp", np.int64)])
JOIN_COLUMNS = ("scaffold_a", "side_a", "scaffold_b", "side_b", "observed", "pairs", "expected", "ratio")
JOIN_DTYPE = np.dtype([("end_a", np.int64), ("end_b", np.int64), ("observed", np.int64), ("pairs", np.int64), ("expected", np.float64),
                       ("ratio", np.float64), ("runner_up_a", np.float64), ("runner_up_b", np.float64)])
SIDE_NAMES = ("head", "tail")


def pairs_closed_form(n_a, n_b, window):
    """``pairs`` of a link between an end of a contig of ``n_a`` positions and an end of one of ``n_b``: the position of depth u,
    u = 0 .. min(w, n_a) - 1, pairs with the min(n_b, w - u) positions of the other contig of depth below w - u.  The first
    r = clamp(w - n_b + 1, 0, min(w, n_a)) depths see all n_b, the others w - u.  Arrays or scalars -> int64."""
    na, nb, w = np.asarray(n_a, np.int64), np.asarray(n_b, np.int64), np.int64(window)
    ua = np.minimum(w, na)
    r = np.clip(w - nb + 1, 0, ua)
    return (r * nb + (ua - r) * w - (ua - 1 + r) * (ua - r) // 2).astype(np.int64)


def linear_runs(stot, contig, position):
    """the placed contigs that are not rings as runs of the genome order -> (members: the sub-fragments by position, start, length:
    per linear contig, run: the run index of every sub-fragment, -1: not placed, -2: on a ring)"""
    members, start, length = jp.contig_runs(contig, position)
    ring = np.asarray(stot, np.float32)[members[start]] != 0 if start.size else np.zeros(0, bool)
    by_position = np.repeat(np.where(ring, -2, np.cumsum(~ring) - 1), length).astype(np.int64)
    run = np.full(np.asarray(position).size, -1, np.int64)
    run[members] = by_position
    return members, start[~ring], length[~ring], run


def support_host(dist, stot, contig, placed, position, l_cont_bp, row, col, cnt, window, model_q=None, chunk=1 << 22):
    """The rule by enumeration: every trans contact tried against the four pairs of ends, the pairs of every link laid out one by one.

    dist, stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order,
    -1 where not placed; l_cont_bp: int [M], the length in bp of the sub-fragment's contig; row, col, cnt: the contacts;
    ``model_q``: callable, separations (f32 array) -> the model's quantised values (int64), None: ``pairs`` and ``expected_q``
    are None.  -> dict: window, rowptr, col, observed, pairs, expected_q, first_position, n_positions (per contig k), entries and row_entries
    (the (contact, link) pairs, in all and per lower end) and the int64 scalars named in SCALARS."""
    w = check_window(window)
    dist = np.asarray(dist, np.float32)
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError("join support: placed and position disagree")
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    members, start, length, run = linear_runs(stot, contig, position)
    K = int(start.size)
    a, b = run[row], run[col]
    unpl = (a == -1) | (b == -1)
    ring = ~unpl & ((a == -2) | (b == -2))
    cis = ~unpl & ~ring & (a == b)
    trans = ~unpl & ~ring & (a != b)
    out = dict(window=w, unplaced_observed=int(cnt[unpl].sum()), ring_observed=int(cnt[ring].sum()), cis_observed=int(cnt[cis].sum()),
               n_contigs=K, first_position=start.astype(np.int32), n_positions=length.astype(np.int32))
    pa, pb, ka, kb, c = position[row[trans]], position[col[trans]], a[trans], b[trans], cnt[trans]
    depth = ((pa - start[ka], start[ka] + length[ka] - 1 - pa), (pb - start[kb], start[kb] + length[kb] - 1 - pb)) if K else None
    keys, vals, n_of = [], [], np.zeros(c.size, np.int64)
    for sa in (0, 1):
        for sb in (0, 1):
            if not K:
                break
            ok = depth[0][sa] + depth[1][sb] + 1 <= w
            ea, eb = 2 * ka[ok] + sa, 2 * kb[ok] + sb
            keys.append(np.minimum(ea, eb) * (2 * K) + np.maximum(ea, eb))
            vals.append(c[ok])
            n_of += ok
    out["in_reach_observed"] = int(c[n_of > 0].sum())
    out["out_of_reach_observed"] = int(c[n_of == 0].sum())
    out["contributions"] = int((c * n_of).sum())
    key = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    out["entries"] = int(key.size)  # (contact, link) pairs: what the device's counting sort holds before the equal links are summed
    out["row_entries"] = np.bincount(key // max(2 * K, 1), minlength=2 * K).astype(np.int64)  # ... per row: what picks a row's sort form
    uniq, inv = np.unique(key, return_inverse=True)
    observed = np.zeros(uniq.size, np.int64)
    np.add.at(observed, inv, np.concatenate(vals) if vals else np.zeros(0, np.int64))
    lo, hi = (uniq // (2 * K), uniq % (2 * K)) if K else (uniq, uniq)
    out["rowptr"] = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=2 * K))]).astype(np.int64)
    out["col"] = hi.astype(np.int32)
    out["observed"] = observed
    out["n_links"] = int(uniq.size)
    out["pairs"] = out["expected_q"] = None
    if model_q is None:
        return out
    l_kb = np.zeros(K, np.float32)
    if K:
        l_kb = np.asarray(l_cont_bp)[members[start]].astype(np.float32) / np.float32(1000.0)
    na, nb = length[lo >> 1] if K else lo, length[hi >> 1] if K else hi
    ua, vb = np.minimum(w, na), np.minimum(w, nb)
    pairs, expected_q = np.zeros(uniq.size, np.int64), np.zeros(uniq.size, np.int64)
    cum = np.concatenate([[0], np.cumsum(ua * vb)])  # the depth rectangles of the links, laid out cell by cell
    side_lo, side_hi, k_lo, k_hi = lo & 1, hi & 1, lo >> 1, hi >> 1
    g0 = 0
    while g0 < uniq.size:  # links g0 .. g1 - 1: at most `chunk` cells (one link at least)
        g1 = max(g0 + 1, int(np.searchsorted(cum, cum[g0] + chunk, side="right")) - 1)
        off = cum[g0:g1] - cum[g0]
        n_cells = np.diff(cum[g0:g1 + 1])
        g = np.repeat(np.arange(g0, g1), n_cells)
        t = np.arange(int(n_cells.sum()), dtype=np.int64) - np.repeat(off, n_cells)
        u, v = t // vb[g], t % vb[g]
        m = u + v + 1 <= w
        g, u, v = g[m], u[m], v[m]
        da = dist[members[np.where(side_lo[g] == 0, start[k_lo[g]] + u, start[k_lo[g]] + length[k_lo[g]] - 1 - u)]]
        db = dist[members[np.where(side_hi[g] == 0, start[k_hi[g]] + v, start[k_hi[g]] + length[k_hi[g]] - 1 - v)]]
        da = np.where(side_lo[g] == 0, da, np.abs(l_kb[k_lo[g]] - da))
        db = np.where(side_hi[g] == 0, db, np.abs(l_kb[k_hi[g]] - db))
        s = da + db
        assert s.dtype == np.float32
        np.add.at(pairs, g, 1)
        np.add.at(expected_q, g, np.asarray(model_q(s), np.int64))
        g0 = g1
    out["pairs"], out["expected_q"] = pairs, expected_q
    return out


def observed_total(result):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(result[k]) for k in OBSERVED_SCALARS)


def rows_of(rowptr):
    """the row (the lower end) of every link"""
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def expected(result):
    """expected_q / 2^32 as f64"""
    return np.asarray(result["expected_q"], np.float64) / Q_ONE


def ratio(result):
    """observed / expected per link as f64, nan where expected is 0"""
    obs, ex = np.asarray(result["observed"], np.float64), expected(result)
    out = np.full(obs.shape, np.nan)
    np.divide(obs, ex, out=out, where=ex != 0)
    return out


def merge_shards(parts):
    """the results of the ranks of a sharded handle -> the whole: the links merged by key (lower end, upper end), ``observed`` and
    the summed scalars added, ``pairs`` / ``expected_q`` (the same on every rank that has the link) taken once"""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_shards: nothing to merge")
    first = parts[0]
    n_ends = np.asarray(first["rowptr"]).size - 1
    if any(np.asarray(p["rowptr"]).size - 1 != n_ends or p["window"] != first["window"] for p in parts):
        raise ValueError("merge_shards: the parts are not of one genome and one window")
    key = np.concatenate([rows_of(p["rowptr"]) * max(n_ends, 1) + np.asarray(p["col"], np.int64) for p in parts])
    uniq, where, inv = np.unique(key, return_index=True, return_inverse=True)
    out = {k: v for k, v in first.items() if k not in LINK_ARRAYS and k not in SCALARS and k != "rowptr"}
    out["observed"] = np.zeros(uniq.size, np.int64)
    np.add.at(out["observed"], inv, np.concatenate([np.asarray(p["observed"], np.int64) for p in parts]))
    for k in ("pairs", "expected_q"):
        if any(p[k] is None for p in parts):
            out[k] = None
            continue
        every = np.concatenate([np.asarray(p[k], np.int64) for p in parts])
        out[k] = every[where]
        if not np.array_equal(out[k][inv], every):
            raise ValueError("merge_shards: the parts disagree on %s" % k)
    lo = uniq // max(n_ends, 1)
    out["col"] = (uniq % max(n_ends, 1)).astype(np.int32)
    out["rowptr"] = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=n_ends))]).astype(np.int64)
    for k in SUMMED_SCALARS:
        out[k] = sum(int(p[k]) for p in parts)
    out["n_contigs"] = int(first["n_contigs"])
    out["n_links"] = int(uniq.size)
    return out


def ends_table(first_position, n_positions, order, parent, contig_of_bin, len_bp):
    """one row per end e = 2 k + side (ENDS_DTYPE): the canonical id of its scaffold (its name: ``assembly_contacts.scaffold_names``),
    the side, the bin and the sub-fragment at the end, the contig's positions and bp.  order: the sub-fragment at every position;
    parent: the bin of every sub-fragment; contig_of_bin: the downloaded state's id_c; len_bp: per sub-fragment."""
    start, n = np.asarray(first_position, np.int64), np.asarray(n_positions, np.int64)
    order = np.asarray(order, np.int64)
    t = np.zeros(2 * start.size, ENDS_DTYPE)
    if start.size == 0:
        return t
    at = np.stack([start, start + n - 1], axis=1).ravel()
    t["side"] = np.tile([0, 1], start.size)
    t["sub_frag"] = order[at]
    t["bin"] = np.asarray(parent, np.int64)[t["sub_frag"]]
    t["scaffold"] = np.asarray(contig_of_bin, np.int64)[t["bin"]]
    t["n_positions"] = np.repeat(n, 2)
    run = np.concatenate([[0], np.cumsum(np.asarray(len_bp, np.int64)[order])])
    t["length_bp"] = np.repeat(run[start + n] - run[start], 2)
    return t


def default_min_pairs(window):
    """half of a full window's pairs (the junction profile's): below that a link is between ends too short to be judged"""
    return jp.default_min_pairs(window)


def best_joins(result, n=20, min_pairs=None):
    """the ``n`` links with the highest observed / expected among those with at least ``min_pairs`` pairs (default: half a full
    window) and a ratio, as a JOIN_DTYPE array, best first.  ``runner_up_a`` / ``runner_up_b``: the best ratio among the OTHER
    eligible links of the link's lower / upper end (nan: it has no other) -- a join is convincing when its ends have no close
    second."""
    if result.get("pairs") is None:
        raise ValueError("best_joins: the result has no model part")
    mp = default_min_pairs(result["window"]) if min_pairs is None else int(min_pairs)
    lo, hi = rows_of(result["rowptr"]), np.asarray(result["col"], np.int64)
    r = ratio(result)
    ok = np.nonzero((np.asarray(result["pairs"]) >= mp) & np.isfinite(r))[0]
    pick = ok[np.argsort(-r[ok], kind="stable")[:max(int(n), 0)]]
    t = np.zeros(pick.size, JOIN_DTYPE)
    t["end_a"], t["end_b"] = lo[pick], hi[pick]
    t["observed"], t["pairs"] = np.asarray(result["observed"])[pick], np.asarray(result["pairs"])[pick]
    t["expected"], t["ratio"] = expected(result)[pick], r[pick]
    for i, g in enumerate(pick.tolist()):
        for name, e in (("runner_up_a", lo[g]), ("runner_up_b", hi[g])):
            others = ok[((lo[ok] == e) | (hi[ok] == e)) & (ok != g)]
            t[name][i] = r[others].max() if others.size else np.nan
    return t


def write_joins(path, result):
    """one line per link: the columns of JOIN_COLUMNS (scaffolds by the names of genome.fasta, sides as head / tail); then the
    window and the scalars.  ``result``: what ``sampler.join_support`` returns (``ends``: the ends table)."""
    from .assembly_contacts import scaffold_names

    ends = result["ends"]
    names = scaffold_names(ends["scaffold"])
    lo, hi = rows_of(result["rowptr"]), np.asarray(result["col"], np.int64)
    have = result.get("pairs") is not None
    prs = np.asarray(result["pairs"]) if have else np.zeros(lo.size, np.int64)
    ex = expected(result) if have else np.full(lo.size, np.nan)
    r = ratio(result) if have else np.full(lo.size, np.nan)
    obs = np.asarray(result["observed"])
    with open(path, "w") as f:
        f.write("# " + " ".join(JOIN_COLUMNS) + "\n")
        for g in range(lo.size):
            a, b = int(lo[g]), int(hi[g])
            f.write("%s %s %s %s %d %d %.9g %.9g\n" % (names[a], SIDE_NAMES[int(ends["side"][a])], names[b], SIDE_NAMES[int(ends["side"][b])],
                                                        obs[g], prs[g], ex[g], r[g]))
        f.write("# window=%d " % result["window"] + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")
    return int(lo.size)
