"""The junction support profile of the current genome: for every junction between two neighbouring positions of the genome order,
the contacts that span it inside a window, next to the number of sub-fragment pairs that could and to what the model in use
predicts for them.  A misjoin is a dip of observed over expected.  This module is the single definition of the rule (pure numpy,
no GPU, no matplotlib); the device passes (``ig_junction_profile``, csrc/ig_kernels_junc.cuh) reproduce it entry for entry.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs (every bin of the contig active) in genome
order, 0 .. T - 1.  JUNCTION j, 1 <= j <= T - 1, lies between the positions j - 1 and j; every array has length T, entry 0 is 0.
A junction is INTERNAL if both positions are in the same contig and that contig is not a ring; at a contig BOUNDARY and inside a
RING (a pair on a ring has two separations: the distance law leaves rings out for the same reason) all three values are 0.
``window`` w is counted in positions, 1 <= w <= MAX_WINDOW.

* ``observed[j]``: the sum of the counts of the uploaded contacts (strict upper triangle) with both ends placed in the same
  contig that is not a ring, whose positions pa < pb satisfy pb - pa <= w and pa < j <= pb.
* ``pairs[j]``: the number of pairs of positions (i, k) of that contig with i < j <= k and k - i <= w, with or without a contact
  (closed form: ``pairs_closed_form``).
* ``expected_q[j]``: the sum over the same pairs of the model's value at ``s = fabsf(dist_i - dist_k)`` (f32: what the exact cis
  term feeds the model), quantised to a multiple of 2^-32 (round half even) and added as a 64-bit integer: the result does not
  depend on the order of the additions.  ``expected = expected_q / 2^32``.

The scalars (int64): ``in_window_observed``; ``beyond_window_observed`` (same linear contig, pb - pa > w); ``trans_observed``;
``ring_observed``; ``unplaced_observed`` (an end in a contig that is not placed); ``internal_junctions``; ``spanned_observed``
(= sum(observed)).  By construction:

    in_window + beyond_window + trans + ring + unplaced == sum(counts)
    sum(observed) == sum of count * (pb - pa) over the in-window contacts
    sum(pairs) == sum over the placed linear contigs of sum_{d = 1 .. min(w, n_c - 1)} d * (n_c - d)
"""
from __future__ import annotations

import numpy as np

MAX_WINDOW = 1024
DEFAULT_WINDOW = 64
# the order of ig_junction_profile's scalars[8] (the last word is not used)
SCALARS = ("in_window_observed", "beyond_window_observed", "trans_observed", "ring_observed", "unplaced_observed",
           "internal_junctions", "spanned_observed")
OBSERVED_SCALARS = SCALARS[:5]
KIND_BOUNDARY, KIND_INTERNAL, KIND_RING = 0, 1, 2
KIND_NAMES = ("boundary", "internal", "ring")
BIN_COLUMNS = ("left_frag", "right_frag", "contig", "position", "observed", "pairs", "expected", "ratio")
BIN_DTYPE = np.dtype([("left_frag", np.int64), ("right_frag", np.int64), ("contig", np.int64), ("position", np.int64),
                      ("observed", np.int64), ("pairs", np.int64), ("expected", np.float64), ("ratio", np.float64)])
Q_ONE = 4294967296.0  # 2^32: one unit of the model's value in expected_q


def check_window(window):
    """-> the window as an int; ValueError unless it is a whole number of positions in 1 .. MAX_WINDOW"""
    w = int(window)
    if w != window or not 1 <= w <= MAX_WINDOW:
        raise ValueError("junction profile: the window is a whole number of positions, 1 <= window <= %d (got %r)" % (MAX_WINDOW, window))
    return w


def window_from_kb(kb, mean_kb):
    """a window given in kb as a number of positions: max(1, ceil(kb / mean_kb)), ``mean_kb`` the mean sub-fragment length"""
    kb, mean_kb = float(kb), float(mean_kb)
    if not (kb > 0 and mean_kb > 0 and np.isfinite(kb) and np.isfinite(mean_kb)):
        raise ValueError("window_from_kb: kb and mean_kb must be positive and finite")
    return max(1, int(np.ceil(kb / mean_kb)))


def pairs_closed_form(rank, length, window):
    """``pairs`` of the junction in front of the sub-fragment of local rank ``rank`` (1 .. length - 1) of a linear contig of
    ``length`` positions: the i on its left within reach are rank - u, u = 1 .. a = min(rank, w), and such an i pairs with
    min(length - rank, w - u + 1) positions k on the right, so pairs = F(w) - F(w - a) with
    F(x) = sum_{v = 1 .. x} min(b, v), b = length - rank.  Arrays or scalars -> int64."""
    l, n, w = np.asarray(rank, np.int64), np.asarray(length, np.int64), np.int64(window)
    a, b = np.minimum(l, w), n - l

    def F(x):
        return np.where(x <= b, x * (x + 1) // 2, b * (b + 1) // 2 + (x - b) * b)

    return np.where((l >= 1) & (l < n), F(w) - F(w - a), 0).astype(np.int64)


def pairs_total_closed_form(lengths, window):
    """the right-hand side of the third identity for linear placed contigs of these lengths"""
    tot = 0
    for n in np.asarray(lengths, np.int64).tolist():
        d = np.arange(1, min(int(window), n - 1) + 1, dtype=np.int64)
        tot += int((d * (n - d)).sum())
    return tot


def contig_runs(contig, position):
    """the placed contigs as runs of the genome order -> (members: the sub-fragments by position, start, length: per contig);
    ValueError unless the positions are 0 .. T - 1 once each and every contig is one run"""
    contig, position = np.asarray(contig, np.int64), np.asarray(position, np.int64)
    members = np.nonzero(position >= 0)[0]
    members = members[np.argsort(position[members], kind="stable")]
    T = int(members.size)
    if not np.array_equal(position[members], np.arange(T)):
        raise ValueError("junction profile: the positions of the placed sub-fragments must be 0 .. T - 1, each once")
    if T == 0:
        return members, np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = contig[members]
    start = np.concatenate([[0], np.nonzero(c[1:] != c[:-1])[0] + 1]).astype(np.int64)
    if np.unique(c[start]).size != start.size:
        raise ValueError("junction profile: a contig is not contiguous in the genome order")
    return members, start, np.diff(np.concatenate([start, [T]])).astype(np.int64)


def junction_kinds(stot, contig, position):
    """kind of every junction (KIND_BOUNDARY / KIND_INTERNAL / KIND_RING; entry 0: boundary) -> int8 [T]"""
    members, _, _ = contig_runs(contig, position)
    kind = np.zeros(members.size, np.int8)
    if members.size > 1:
        c = np.asarray(contig, np.int64)[members]
        ring = np.asarray(stot, np.float32)[members] != 0
        same = c[1:] == c[:-1]
        kind[1:] = np.where(same, np.where(ring[1:], KIND_RING, KIND_INTERNAL), KIND_BOUNDARY)
    return kind


def profile_host(dist, stot, contig, placed, position, row, col, cnt, window, model_q=None, chunk=1 << 22):
    """The rule by enumeration (deliberately not the device's difference arrays): every in-window contact is expanded to the
    junctions it spans and counted; the pairs of every contig are enumerated separation by separation.

    dist, stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order,
    -1 where not placed; row, col, cnt: the contacts; ``model_q``: callable, separations (f32 array) -> the model's quantised
    values (int64), None: ``expected_q`` is None.  -> dict: window, n_placed, observed, pairs, expected_q (int64 [T]) and the
    int64 scalars named in SCALARS."""
    w = check_window(window)
    dist = np.asarray(dist, np.float32)
    ring = np.asarray(stot, np.float32) != 0
    contig = np.asarray(contig, np.int64)
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError("junction profile: placed and position disagree")
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    cnt = np.asarray(cnt, np.int64)
    members, start, length = contig_runs(contig, position)
    T = int(members.size)

    out = dict(window=w, n_placed=T)
    both = placed[row] & placed[col]
    out["unplaced_observed"] = int(cnt[~both].sum())
    cis = both & (contig[row] == contig[col])
    out["trans_observed"] = int(cnt[both & ~cis].sum())
    on_ring = cis & ring[row]
    out["ring_observed"] = int(cnt[on_ring].sum())
    lin = cis & ~on_ring
    pa = np.minimum(position[row[lin]], position[col[lin]])
    pb = np.maximum(position[row[lin]], position[col[lin]])
    c = cnt[lin]
    near = pb - pa <= w
    out["in_window_observed"] = int(c[near].sum())
    out["beyond_window_observed"] = int(c[~near].sum())
    pa, span, c = pa[near], (pb - pa)[near], c[near]
    observed = np.zeros(T, np.int64)
    per = max(1, chunk // w)  # contacts per chunk: at most `chunk` (contact, junction) entries
    for k0 in range(0, pa.size, per):
        a, n, v = pa[k0:k0 + per], span[k0:k0 + per], c[k0:k0 + per]
        if int(v.sum()) >= 1 << 53:
            raise ValueError("junction profile: counts beyond what a float64 bincount adds exactly")
        first = np.cumsum(n) - n  # every contact's entries: junctions a + 1 .. a + n
        j = np.repeat(a + 1 - first, n) + np.arange(int(n.sum()), dtype=np.int64)
        observed += np.bincount(j, weights=np.repeat(v, n).astype(np.float64), minlength=T)[:T].astype(np.int64)
    out["observed"] = observed
    out["spanned_observed"] = int(observed.sum())

    pairs = np.zeros(T, np.int64)
    expected_q = np.zeros(T, np.int64) if model_q is not None else None
    internal = 0
    for st, n in zip(start.tolist(), length.tolist()):
        if ring[members[st]] or n < 2:
            continue
        internal += n - 1
        d_c = dist[members[st:st + n]]
        l = np.arange(1, n, dtype=np.int64)  # local rank of the sub-fragment behind the junction
        for d in range(1, min(w, n - 1) + 1):  # the pairs (i, i + d), i = 0 .. n - 1 - d: junction l is spanned by max(0, l - d) <= i < min(l, n - d)
            lo, hi = np.maximum(l - d, 0), np.minimum(l, n - d)
            pairs[st + 1:st + n] += hi - lo
            if model_q is not None:
                s = np.abs(d_c[:n - d] - d_c[d:])
                assert s.dtype == np.float32
                q = np.concatenate([[0], np.cumsum(np.asarray(model_q(s), np.int64))])
                expected_q[st + 1:st + n] += q[hi] - q[lo]
    out["pairs"] = pairs
    out["expected_q"] = expected_q
    out["internal_junctions"] = int(internal)
    return out


def observed_total(profile):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(profile[k]) for k in OBSERVED_SCALARS)


def expected(profile):
    """expected_q / 2^32 as f64"""
    return np.asarray(profile["expected_q"], np.float64) / Q_ONE


def ratio(profile):
    """observed / expected per junction as f64, nan where expected is 0"""
    obs, ex = np.asarray(profile["observed"], np.float64), expected(profile)
    out = np.full(obs.shape, np.nan)
    np.divide(obs, ex, out=out, where=ex != 0)
    return out


def default_min_pairs(window):
    """half of a full window's pairs, w (w + 1) / 2: below that a junction sits too close to an end of its contig to be judged"""
    w = check_window(window)
    return (w * (w + 1) // 2 + 1) // 2


def bin_table(profile, kind, parent, contig_of_position):
    """the internal junctions at which the parent bin changes -- the joins the sampler's moves made or could break -- as a
    BIN_DTYPE array.  ``parent``, ``contig_of_position``: the bin and the contig id of the sub-fragment at every position"""
    parent = np.asarray(parent, np.int64)
    T = parent.size
    j = np.zeros(0, np.int64)
    if T > 1:
        j = np.nonzero((np.asarray(kind)[1:] == KIND_INTERNAL) & (parent[1:] != parent[:-1]))[0] + 1
    t = np.zeros(j.size, BIN_DTYPE)
    t["left_frag"], t["right_frag"] = parent[j - 1], parent[j]
    t["contig"] = np.asarray(contig_of_position, np.int64)[j]
    t["position"] = j
    t["observed"] = np.asarray(profile["observed"])[j]
    t["pairs"] = np.asarray(profile["pairs"])[j]
    t["expected"] = expected(profile)[j]
    t["ratio"] = ratio(profile)[j]
    return t


def weakest(table, n=20, min_pairs=0):
    """the n rows of a bin-level table with the lowest ratio among those with at least ``min_pairs`` pairs and a ratio"""
    t = table[(table["pairs"] >= min_pairs) & np.isfinite(table["ratio"])]
    return t[np.argsort(t["ratio"], kind="stable")[:max(int(n), 0)]]


def write_profile(path, profile):
    """one line per bin-level junction (``profile["bins"]``): the columns of BIN_COLUMNS; then the window and the scalars"""
    with open(path, "w") as f:
        f.write("# " + " ".join(BIN_COLUMNS) + "\n")
        for r in profile["bins"]:
            f.write("%d %d %d %d %d %d %.9g %.9g\n" % tuple(r[k] for k in BIN_COLUMNS))
        f.write("# window=%d n_placed=%d " % (profile["window"], profile["n_placed"]) + " ".join("%s=%d" % (k, profile[k]) for k in SCALARS) + "\n")
