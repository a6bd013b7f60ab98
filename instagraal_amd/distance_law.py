"""The distance law P(s) of the current genome as the data shows it: observed contacts and sub-fragment pairs per bin of genomic
separation.  This module is the single definition of the rule (pure numpy, no GPU, no matplotlib); the device pass
(``ig_distance_law``, csrc/ig_kernels_law.cuh) reproduces it entry for entry.

The rule.  Per sub-fragment: ``dist`` (f32, kb: Tables.dist), ``stot`` (f32, nonzero: its contig is a ring), a contig id, and whether
its contig is PLACED -- exactly as for the contact map: every bin of the contig is active.  The contacts are the uploaded ones (row,
column, count; strict upper triangle).  ``edges``: ascending f32, 2 <= len(edges) <= MAX_EDGES.

* A pair of sub-fragments of one placed contig that is not a ring has the separation ``s = fabsf(dist_i - dist_j)``, computed in
  f32 -- the value the exact cis term feeds the model.  It falls into the bin b with ``edges[b] <= s < edges[b + 1]``:
  ``observed[b]`` takes the count of a contact between the two, ``pairs[b]`` counts the pair whether it has a contact or not.
  With ``s < edges[0]`` or ``s >= edges[-1]`` the pair goes to ``out_of_range_pairs`` / ``out_of_range_observed``.
* A pair inside a RING contig has two separations (the two ways round), and which of them the model uses depends on the ring's
  length: such pairs are left out of the law and counted in ``ring_pairs`` / ``ring_observed``.
* Both ends placed, in different contigs: ``trans_pairs`` / ``trans_observed``.  The pairs are counted from the contigs'
  sub-fragment counts: T (T - 1) / 2 - placed_pairs, T the number of placed sub-fragments.
* A contact with an end in a contig that is not placed: ``unplaced_observed``.
* ``placed_pairs`` = sum over the placed contigs of M_c (M_c - 1) / 2.

All outputs are int64 and two identities hold by construction:

    sum(observed) + out_of_range_observed + trans_observed + ring_observed + unplaced_observed == sum(counts)
    sum(pairs) + out_of_range_pairs + ring_pairs == placed_pairs
"""
from __future__ import annotations

import numpy as np

MAX_EDGES = 4097  # at most 4096 bins
# the order of ig_distance_law's scalars[8]
SCALARS = ("out_of_range_observed", "out_of_range_pairs", "trans_observed", "trans_pairs", "ring_observed", "ring_pairs",
           "unplaced_observed", "placed_pairs")
OBSERVED_SCALARS = ("out_of_range_observed", "trans_observed", "ring_observed", "unplaced_observed")


def check_edges(edges):
    """-> the edges as a contiguous f32 array; ValueError unless finite, ascending (equal neighbours allowed: an empty bin) and
    2 <= len <= MAX_EDGES"""
    e = np.ascontiguousarray(edges, np.float32).ravel()
    if not 2 <= e.size <= MAX_EDGES:
        raise ValueError("distance law: 2 <= len(edges) <= %d (got %d)" % (MAX_EDGES, e.size))
    if not np.all(np.isfinite(e)):
        raise ValueError("distance law: the edges must be finite")
    if np.any(e[1:] < e[:-1]):
        raise ValueError("distance law: the edges must be ascending")
    return e


def _bins(s, edges):
    """bin of every separation (f32 against f32: comparisons only), -1: out of range"""
    b = np.searchsorted(edges, s, side="right").astype(np.int64) - 1  # edges[b] <= s < edges[b + 1]
    b[b >= edges.size - 1] = -1
    return b


def law_host(dist, stot, contig, placed, row, col, cnt, edges, pairs=True, chunk=1 << 22):
    """The rule by brute force: O(M_c^2) per placed contig, no assumption about the order of ``dist`` inside a contig.

    dist, stot: f32 [M]; contig: int [M] (any labelling: equal <=> same contig); placed: bool [M]; row, col, cnt: the contacts;
    ``pairs=False`` leaves the pair counts out (``pairs`` is None, the pair scalars -1).  -> dict: observed, pairs (int64 [n_bins]),
    edges, and the int64 scalars named in SCALARS."""
    edges = check_edges(edges)
    nb = edges.size - 1
    dist = np.asarray(dist, np.float32)
    ring = np.asarray(stot, np.float32) != 0
    contig = np.asarray(contig, np.int64)
    placed = np.asarray(placed, bool)
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    cnt = np.asarray(cnt, np.int64)

    out = dict(edges=edges)
    both = placed[row] & placed[col]
    out["unplaced_observed"] = int(cnt[~both].sum())
    cis = both & (contig[row] == contig[col])
    out["trans_observed"] = int(cnt[both & ~cis].sum())
    on_ring = cis & ring[row]
    out["ring_observed"] = int(cnt[on_ring].sum())
    lin = cis & ~on_ring
    s = np.abs(dist[row[lin]] - dist[col[lin]])  # f32 - f32 -> f32
    assert s.dtype == np.float32
    b = _bins(s, edges)
    c = cnt[lin]
    out["out_of_range_observed"] = int(c[b < 0].sum())
    observed = np.zeros(nb, np.int64)
    np.add.at(observed, b[b >= 0], c[b >= 0])
    out["observed"] = observed

    if not pairs:
        out["pairs"] = None
        for k in ("out_of_range_pairs", "trans_pairs", "ring_pairs", "placed_pairs"):
            out[k] = -1
        return out
    pair_hist = np.zeros(nb, np.int64)
    oor = ring_pairs = placed_pairs = 0
    idx = np.nonzero(placed)[0]
    T = int(idx.size)
    by = idx[np.argsort(contig[idx], kind="stable")]
    ids, start, length = np.unique(contig[by], return_index=True, return_counts=True)
    for st, ln in zip(start.tolist(), length.tolist()):
        n_pairs = ln * (ln - 1) // 2
        placed_pairs += n_pairs
        members = by[st:st + ln]
        if ring[members[0]]:
            ring_pairs += n_pairs
            continue
        d = dist[members]
        rows_per = max(1, chunk // max(ln, 1))
        for i0 in range(0, ln - 1, rows_per):
            i1 = min(ln - 1, i0 + rows_per)
            sep = np.abs(d[i0:i1, None] - d[None, :])  # f32
            keep = np.arange(ln)[None, :] > np.arange(i0, i1)[:, None]  # every unordered pair once
            bb = _bins(sep[keep], edges)
            oor += int((bb < 0).sum())
            pair_hist += np.bincount(bb[bb >= 0], minlength=nb)
    out["pairs"] = pair_hist
    out["out_of_range_pairs"] = int(oor)
    out["ring_pairs"] = int(ring_pairs)
    out["placed_pairs"] = int(placed_pairs)
    out["trans_pairs"] = T * (T - 1) // 2 - int(placed_pairs)
    return out


def observed_total(law):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return int(law["observed"].sum()) + sum(int(law[k]) for k in OBSERVED_SCALARS)


def pairs_total(law):
    """the left-hand side of the second identity (== law["placed_pairs"])"""
    return int(law["pairs"].sum()) + int(law["out_of_range_pairs"]) + int(law["ring_pairs"])


def default_edges(mean_kb, longest_kb, per_octave=8):
    """Geometric edges from ``mean_kb / 2`` to beyond ``longest_kb`` (the longest placed contig), ``per_octave`` bins per factor of
    two, at most MAX_EDGES - 1 bins (a longer range gets wider bins) -> f32, strictly ascending"""
    lo = float(mean_kb) / 2.0
    if not (lo > 0 and np.isfinite(lo)):
        raise ValueError("default_edges: mean_kb must be positive and finite")
    hi = max(float(longest_kb), 2.0 * lo) * 1.001
    n = int(np.ceil(np.log2(hi / lo) * per_octave))
    n = max(1, min(n, MAX_EDGES - 1))
    e = (lo * np.power(hi / lo, np.arange(n + 1) / n)).astype(np.float32)
    e[-1] = np.nextafter(np.float32(max(e[-1], np.float32(longest_kb))), np.float32(np.inf))
    e = np.unique(e)  # (f32 rounding may merge neighbours of a very fine grid)
    return e


def mean_per_pair(law):
    """observed / pairs per bin as f64, nan where a bin holds no pair"""
    obs = np.asarray(law["observed"], np.float64)
    prs = np.asarray(law["pairs"], np.float64)
    out = np.full(obs.shape, np.nan)
    np.divide(obs, prs, out=out, where=prs > 0)
    return out


def bin_centres(edges):
    """geometric centre of a bin whose lower edge is positive, else the arithmetic one"""
    e = np.asarray(edges, np.float64)
    lo, hi = e[:-1], e[1:]
    return np.where(lo > 0, np.sqrt(np.abs(lo * hi)), 0.5 * (lo + hi))


def write_law(path, law):
    """one line per bin: edge_lo edge_hi observed pairs"""
    e = law["edges"]
    with open(path, "w") as f:
        f.write("# edge_lo_kb edge_hi_kb observed pairs\n")
        for b in range(e.size - 1):
            f.write("%.9g %.9g %d %d\n" % (e[b], e[b + 1], law["observed"][b], law["pairs"][b]))
        f.write("# " + " ".join("%s=%d" % (k, law[k]) for k in SCALARS) + "\n")
