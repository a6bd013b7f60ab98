"""Gap support: the distance the contacts put across each join of the current genome.  Every other report scores a join as if its two
sides touched: the separation of a pair across a junction is |ds_i - ds_m|, the sub-fragments in between and nothing for sequence the
assembly does not hold.  A true join across a missing repeat and a misjoin then look the same -- observed far below expected.  They
differ in HOW the contacts across the join fall off: across a true join with a gap g they still decay with distance, as P(s + g);
across a misjoin they sit at the trans level whatever the distance.  One profile likelihood over a grid of gaps per join tells the
two apart and sizes the gap.  This module is the single definition of the rule (pure numpy, no GPU); the device passes
(``ig_gap_support``, csrc/ig_kernels_gap.cuh) reproduce ``support_host`` byte for byte.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs in genome order, 0 .. T - 1; a contig holds
the positions start .. end - 1.  JUNCTION j lies between the positions j - 1 and j.  ``ds`` is the genome view's distance per position
(what ``ig_junction_profile`` uses).

INPUTS.  ``window`` w in positions, 1 <= w <= MAX_WINDOW = 256 (this report's own cap: a junction costs K w (w + 1) / 2 model values
where the junction profile pays 2 w per position).  n_j >= 1 JUNCTIONS, strictly ascending, each in 1 .. T - 1 and internal to one
placed contig (the positions j - 1 and j share a contig); anything else is an error of the whole call, not a status.  K GAPS in kb
as float32, 2 <= K <= MAX_GAPS = 64, finite, strictly ascending, gaps[0] == 0.

STATUS per junction: 0 JUDGED; 2 the contig is a ring (a pair on a ring has two separations: the distance law leaves rings out for
the same reason), its row is all zeros.  ``geometry`` holds (contig, left, right, 0): the canonical id of the contig,
left = min(w, j - start), right = min(w, end - j) (both 0 on a ring); the fourth word is reserved.

``pairs[j]``: the number of (i, m), start <= i < j <= m < end, m - i <= w (``junction_profile.pairs_closed_form``).
``observed[j]``: the sum of ``cnt`` over the contacts of that linear contig at positions pa < pb with pb - pa <= w and pa < j <= pb.

THE TWO MODEL SUMS.  A pair at separation s = fabsf(ds_i - ds_m) has the SHIFTED separation s_k = s + gaps[k] -- one float32
addition -- and E_k = ig_rippe(s_k, p) under parameter set 0 (beyond d_max that is v_inter: a huge gap is the "apart" hypothesis).

* ``expected_q[j][k]`` = the sum over the pairs of ig_quantize((double) E_k);
* ``log_q[j][k]`` = the sum over the spanning contacts of cnt * ig_quantize(ig_log10((double) E_k)),

both int64 in units of 2^-32, added as integers (unsigned wrap on the way; the device's guards, the second of them stated here as
``log_sum_fits``, make the final value fit), so the result does not depend on the order of the additions.  It is a profile PER
JUNCTION: a pair that also spans another listed junction takes that junction's gap as 0.

The scalars (int64, SCALARS).  Every contact falls in the first class that fits -- ``unplaced`` (an end in a contig that is not
placed), ``trans``, ``ring``, ``counted`` (cis on a linear contig, in window, spanning at least one judged listed junction),
``uncounted`` (the other cis contacts) -- then ``contributions`` (the number of (contact, junction) updates: the sum over the contacts
of the judged listed junctions they span), ``n_judged`` and ``n_placed``.  By construction:

    unplaced + trans + ring + counted + uncounted == sum(cnt)
    counted contacts <= contributions;  sum(observed) is its count-weighted form

``derived`` (float64 on the host; not compared byte for byte): ll[j][k] = ln(10) log_q / 2^32 - expected_q / 2^32, the Poisson
log-likelihood up to the term that does not depend on the gap; ll_apart[j] the same with every pair at v_inter (from observed, pairs
and the quantised v_inter alone); best = argmax_k ll (ties: the lowest k); gap_kb = gaps[best]; llr_gap = ll[best] - ll[0];
llr_apart = ll_apart - ll[best]; gap_lo, gap_hi the smallest and the largest grid gap whose ll is within 1.92 of the maximum -- half
the 95 % quantile of chi^2 with one degree of freedom, 3.84 / 2: the standard profile-likelihood interval (Wilks 1938; Venzon &
Moolgavkar 1988) --; verdict "apart" if llr_apart >= 0, else "adjacent" if best == 0 or llr_gap < 1.92, else "gap" ("none" for a
junction that is not judged).

``default_gaps``: 32 float32 values, 0 and 31 values spaced geometrically from a quarter of the mean sub-fragment length to d_max.
"""
from __future__ import annotations

import numpy as np

from .junction_profile import Q_ONE, contig_runs, pairs_closed_form, window_from_kb  # noqa: F401

MAX_WINDOW = 256  # this report's own: K w (w + 1) / 2 model values per junction
DEFAULT_WINDOW = 64
MIN_GAPS, MAX_GAPS, DEFAULT_N_GAPS = 2, 64, 32
HALF_CHI2_95 = 1.92  # chi^2_1 at 95 % is 3.84; a profile log-likelihood within half of it of its maximum is the 95 % interval
# the order of ig_gap_support's scalars[8]
SCALARS = ("unplaced", "trans", "ring", "counted", "uncounted", "contributions", "n_judged", "n_placed")
CLASS_SCALARS = SCALARS[:5]
STATUS_JUDGED, STATUS_RING = 0, 2
VERDICTS = ("adjacent", "gap", "apart")
COLUMNS = ("scaffold", "left_bin", "right_bin", "observed", "pairs", "gap_kb", "gap_lo", "gap_hi", "llr_gap", "llr_apart", "verdict")
JOIN_DTYPE = np.dtype([("index", np.int64), ("junction", np.int64), ("scaffold", np.int64), ("left_bin", np.int64), ("right_bin", np.int64),
                       ("observed", np.int64), ("pairs", np.int64), ("gap_kb", np.float64), ("gap_lo", np.float64), ("gap_hi", np.float64),
                       ("llr_gap", np.float64), ("llr_apart", np.float64), ("score", np.float64), ("verdict", "U8")])


def check_window(window):
    """-> the window as an int; ValueError unless it is a whole number of positions in 1 .. MAX_WINDOW"""
    w = int(window)
    if w != window or not 1 <= w <= MAX_WINDOW:
        raise ValueError("gap support: the window is a whole number of positions, 1 <= window <= %d (got %r)" % (MAX_WINDOW, window))
    return w


def check_gaps(gaps_kb):
    """-> the gaps as float32; ValueError unless there are MIN_GAPS .. MAX_GAPS of them, finite, strictly ascending, the first 0"""
    g = np.asarray(gaps_kb)
    if g.ndim != 1 or not MIN_GAPS <= g.size <= MAX_GAPS:
        raise ValueError("gap support: %d .. %d gaps in one vector (got shape %r)" % (MIN_GAPS, MAX_GAPS, g.shape))
    g = g.astype(np.float32)
    if not np.all(np.isfinite(g)) or g[0] != 0 or np.any(g[1:] <= g[:-1]):
        raise ValueError("gap support: the gaps are finite, strictly ascending as float32 and start at 0")
    return g


def default_gaps(mean_subfrag_kb, d_max, n=DEFAULT_N_GAPS):
    """0 and n - 1 values spaced geometrically from a quarter of the mean sub-fragment length to d_max, as float32, strictly
    ascending after the cast (ValueError if the two ends leave no room for that)"""
    lo, hi = float(mean_subfrag_kb) / 4.0, float(d_max)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo < hi):
        raise ValueError("default_gaps: 0 < mean_subfrag_kb / 4 < d_max, both finite (got %r, %r)" % (mean_subfrag_kb, d_max))
    return check_gaps(np.concatenate([[0.0], np.geomspace(lo, hi, int(n) - 1)]).astype(np.float32))


def check_junctions(junctions, n_placed, contig_start):
    """-> the junctions as int64; ValueError unless the list is not empty, strictly ascending, in 1 .. T - 1 and every junction is
    internal to one contig.  ``contig_start``: the first position of the contig of every position"""
    j = np.asarray(junctions)
    if j.ndim != 1 or j.size < 1 or not np.issubdtype(j.dtype, np.integer):
        raise ValueError("gap support: junction list: one integer vector of at least one junction")
    j = j.astype(np.int64)
    if j.min() < 1 or j.max() >= n_placed:
        raise ValueError("gap support: junction list out of range: 1 <= junction <= %d" % (n_placed - 1))
    if np.any(j[1:] <= j[:-1]):
        raise ValueError("gap support: junction list not strictly ascending")
    cs = np.asarray(contig_start, np.int64)
    if np.any(cs[j - 1] != cs[j]):
        raise ValueError("gap support: junction list: a junction on a contig boundary")
    return j


def log_sum_fits(observed_max, max_abs_log_q):
    """the device's second guard (``ig_gap_support``: "too many contacts across one junction for this model"): a word of ``log_q`` adds
    at most max_j observed[j] counts times the largest |quantised log10| of a counted contact; the call is refused unless that product
    stays below 2^62.  Python integers -> bool"""
    return int(observed_max) * int(max_abs_log_q) < 1 << 62


def support_host(dist, stot, contig, placed, position, row, col, cnt, junctions, gaps_kb, window, model, want_expected=True, canonical=None,
                 check=True):
    """The rule, pair by pair and contact by contact (deliberately not the device's algorithm: no painted counts, no atomics).

    dist, stot: f32 [M]; contig: int [M] (any labelling); placed: bool [M]; position: int [M], the position in the genome order,
    -1 where not placed; row, col, cnt: the contacts; ``model``: callable, separations (f32 array) -> (e_q, l_q), the quantised
    model value and the quantised log10 of it (int64 arrays); ``canonical``: int [M], the canonical contig id of every sub-fragment
    (None: ``contig`` is reported).  -> dict: window, n_junctions, junction, gaps_kb, status (int32 [n_j]), geometry (int32 [n_j, 4]),
    observed, pairs (int64 [n_j]), log_q, expected_q (int64 [n_j, K]; expected_q None without ``want_expected``), apart_q (the model's
    two values at an infinite separation: v_inter), max_abs_log_q (the largest |l_q| of a counted contact under any gap) and the int64
    scalars named in SCALARS.  ValueError where ``log_sum_fits`` fails, as the device refuses (``check=False``: the result comes back,
    its ``log_q`` wrapped modulo 2^64)."""
    w = check_window(window)
    gaps = check_gaps(gaps_kb)
    K = int(gaps.size)
    dist = np.asarray(dist, np.float32)
    ring = np.asarray(stot, np.float32) != 0
    contig = np.asarray(contig, np.int64)
    placed = np.asarray(placed, bool)
    position = np.asarray(position, np.int64)
    if not np.array_equal(placed, position >= 0):
        raise ValueError("gap support: placed and position disagree")
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    members, start, length = contig_runs(contig, position)
    T = int(members.size)
    c_start, c_end = np.repeat(start, length), np.repeat(start + length, length)
    junc = check_junctions(junctions, T, c_start)
    n_j = int(junc.size)
    on_ring = ring[members][junc]
    label = contig if canonical is None else np.asarray(canonical, np.int64)

    status = np.where(on_ring, STATUS_RING, STATUS_JUDGED).astype(np.int32)
    geo = np.zeros((n_j, 4), np.int32)
    geo[:, 0] = label[members][junc]
    geo[:, 1] = np.where(on_ring, 0, np.minimum(w, junc - c_start[junc]))
    geo[:, 2] = np.where(on_ring, 0, np.minimum(w, c_end[junc] - junc))
    pairs = np.where(on_ring, 0, pairs_closed_form(junc - c_start[junc], c_end[junc] - c_start[junc], w)).astype(np.int64)
    apart = model(np.array([np.inf], np.float32))
    out = dict(window=w, n_placed=T, n_junctions=n_j, junction=junc, gaps_kb=gaps, status=status, geometry=geo, pairs=pairs,
               apart_q=(int(np.asarray(apart[0])[0]), int(np.asarray(apart[1])[0])))

    # ---- the contacts, one by one
    both = placed[row] & placed[col]
    out["unplaced"] = int(cnt[~both].sum())
    cis = both & (contig[row] == contig[col])
    out["trans"] = int(cnt[both & ~cis].sum())
    ringed = cis & ring[row]
    out["ring"] = int(cnt[ringed].sum())
    lin = cis & ~ringed
    pa = np.minimum(position[row[lin]], position[col[lin]])
    pb = np.maximum(position[row[lin]], position[col[lin]])
    sep = np.abs(dist[row[lin]] - dist[col[lin]])
    assert sep.dtype == np.float32
    c = cnt[lin]
    lo, hi = np.searchsorted(junc, pa, side="right"), np.searchsorted(junc, pb, side="right")  # the listed junctions pa < j <= pb
    spans = np.where(pb - pa <= w, hi - lo, 0)
    hit = spans > 0
    out["counted"] = int(c[hit].sum())
    out["uncounted"] = int(c[~hit].sum())
    out["contributions"] = int(spans.sum())
    out["n_judged"] = int((status == STATUS_JUDGED).sum())
    observed = np.zeros(n_j, np.int64)
    log_q = np.zeros((n_j, K), np.int64)
    lo, n, v, s = lo[hit], spans[hit], c[hit], sep[hit]
    out["max_abs_log_q"] = 0
    if n.size:
        first = np.cumsum(n) - n
        which = np.repeat(lo - first, n) + np.arange(int(n.sum()), dtype=np.int64)  # every contact's junctions lo .. lo + n - 1
        np.add.at(observed, which, np.repeat(v, n))
        shifted = s[:, None] + gaps[None, :]
        assert shifted.dtype == np.float32
        lq = np.asarray(model(shifted.ravel())[1], np.int64).reshape(shifted.shape)
        out["max_abs_log_q"] = max(abs(int(lq.max())), abs(int(lq.min())))
        with np.errstate(over="ignore"):
            np.add.at(log_q, which, np.repeat(v[:, None] * lq, n, axis=0))
    out["observed"], out["log_q"] = observed, log_q
    if check and not log_sum_fits(observed.max() if n_j else 0, out["max_abs_log_q"]):
        raise ValueError("gap support: too many contacts across one junction for this model (%d contacts, the largest |log10| %.6g: their product does "
                         "not fit the 64-bit sum)" % (int(observed.max()), out["max_abs_log_q"] / Q_ONE))

    # ---- the pairs of every contig that holds a listed junction, separation by separation
    expected_q = None
    if want_expected:
        expected_q = np.zeros((n_j, K), np.int64)
        d = dist[members]
        for st, n_c in zip(start.tolist(), length.tolist()):
            idx = np.nonzero((junc > st) & (junc < st + n_c) & ~on_ring)[0]
            if idx.size == 0:
                continue
            l = junc[idx] - st  # local rank of the position behind the junction
            d_c = d[st:st + n_c]
            for sp in range(1, min(w, n_c - 1) + 1):  # the pairs (i, i + sp): junction l is spanned by max(0, l - sp) <= i < min(l, n_c - sp)
                a, b = np.maximum(l - sp, 0), np.minimum(l, n_c - sp)
                i0, i1 = int(a.min()), int(b.max())
                if i1 <= i0:
                    continue
                s = np.abs(d_c[i0:i1] - d_c[i0 + sp:i1 + sp])
                shifted = s[:, None] + gaps[None, :]
                assert shifted.dtype == np.float32
                eq = np.asarray(model(shifted.ravel())[0], np.int64).reshape(shifted.shape)
                cum = np.concatenate([np.zeros((1, K), np.int64), np.cumsum(eq, axis=0)])
                expected_q[idx] += cum[b - i0] - cum[a - i0]
    out["expected_q"] = expected_q
    return out


def observed_total(result):
    """the left-hand side of the first identity: every contact's count, wherever it went"""
    return sum(int(result[k]) for k in CLASS_SCALARS)


def derived(result):
    """-> dict of per-junction columns (float64 on the host): ll [n_j, K], ll_apart, best (int64), gap_kb, llr_gap, llr_apart,
    gap_lo, gap_hi and verdict ("adjacent", "gap", "apart"; "none": not judged).  Needs ``expected_q`` and ``apart_q``."""
    if result.get("expected_q") is None:
        raise ValueError("gap support: derived needs the model part (expected_q)")
    gaps = np.asarray(result["gaps_kb"], np.float64)
    lq, eq = np.asarray(result["log_q"], np.float64), np.asarray(result["expected_q"], np.float64)
    ll = np.log(10.0) * lq / Q_ONE - eq / Q_ONE
    e_inf, l_inf = (float(x) for x in result["apart_q"])
    obs, prs = np.asarray(result["observed"], np.float64), np.asarray(result["pairs"], np.float64)
    ll_apart = np.log(10.0) * (obs * l_inf) / Q_ONE - (prs * e_inf) / Q_ONE  # (the products first: what the sums hold where every pair sits at v_inter)
    best = np.argmax(ll, axis=1).astype(np.int64)  # (numpy: the first of equal maxima)
    rows = np.arange(ll.shape[0])
    top = ll[rows, best]
    llr_gap = top - ll[:, 0]
    llr_apart = ll_apart - top
    near = ll >= (top - HALF_CHI2_95)[:, None]
    gap_lo = gaps[np.argmax(near, axis=1)]
    gap_hi = gaps[ll.shape[1] - 1 - np.argmax(near[:, ::-1], axis=1)]
    judged = np.asarray(result["status"]) == STATUS_JUDGED
    verdict = np.where(~judged, "none", np.where(llr_apart >= 0, "apart", np.where((best == 0) | (llr_gap < HALF_CHI2_95), "adjacent", "gap")))
    return dict(ll=ll, ll_apart=ll_apart, best=best, gap_kb=gaps[best], llr_gap=llr_gap, llr_apart=llr_apart, gap_lo=gap_lo, gap_hi=gap_hi,
                verdict=verdict.astype("U8"))


def _people(result, k, size):
    return np.asarray(result[k], np.int64) if k in result else np.full(size, -1, np.int64)


def gapped_joins(result, n=20, min_observed=0):
    """the ``n`` joins whose verdict is "gap" or "apart" with at least ``min_observed`` contacts across, ranked by
    max(llr_gap, ll_apart - ll[0]) -- how much better than "adjacent" the better of the two other readings is -- descending, ties by
    junction -> a JOIN_DTYPE array"""
    d = result if "verdict" in result else dict(result, **derived(result))
    score = np.maximum(np.asarray(d["llr_gap"]), np.asarray(d["ll_apart"]) - np.asarray(d["ll"])[:, 0])
    obs = np.asarray(result["observed"], np.int64)
    ok = np.nonzero(np.isin(d["verdict"], ("gap", "apart")) & (obs >= int(min_observed)))[0]
    pick = ok[np.argsort(-score[ok], kind="stable")[:max(int(n), 0)]]
    t = np.zeros(pick.size, JOIN_DTYPE)
    t["index"], t["junction"] = pick, np.asarray(result["junction"], np.int64)[pick]
    for k in ("scaffold", "left_bin", "right_bin"):
        t[k] = _people(result, k, obs.size)[pick]
    t["observed"], t["pairs"] = obs[pick], np.asarray(result["pairs"], np.int64)[pick]
    for k in ("gap_kb", "gap_lo", "gap_hi", "llr_gap", "llr_apart", "verdict"):
        t[k] = np.asarray(d[k])[pick]
    t["score"] = score[pick]
    return t


def write_gaps(path, result, mode="w", title=None):
    """one line per junction, the columns of COLUMNS; then the window, the number of gaps and the scalars (``mode="a"``: behind what
    the file holds already; ``title``: a comment line in front)"""
    d = result if "verdict" in result else dict(result, **derived(result))
    n_j = int(np.asarray(result["junction"]).size)
    who = [_people(result, k, n_j) for k in ("scaffold", "left_bin", "right_bin")]
    with open(path, mode) as f:
        if title:
            f.write("# %s\n" % title)
        f.write("# " + " ".join(COLUMNS) + "\n")
        for i in range(n_j):
            f.write("%d %d %d %d %d %.9g %.9g %.9g %.9g %.9g %s\n" % (who[0][i], who[1][i], who[2][i], result["observed"][i], result["pairs"][i], d["gap_kb"][i],
                                                                  d["gap_lo"][i], d["gap_hi"][i], d["llr_gap"][i], d["llr_apart"][i], d["verdict"][i]))
        f.write("# window=%d n_junctions=%d n_gaps=%d " % (result["window"], n_j, np.asarray(result["gaps_kb"]).size)
                + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")


# ------------------------------------------------------------------------------------------------------------ the junction builders
def _between(seg, scaffold_of_bin):
    """the junctions between two consecutive segments of one scaffold -> dict: junction, left_bin, right_bin, scaffold"""
    first, last = np.asarray(seg["first"], np.int64), np.asarray(seg["last"], np.int64)
    fb, lb = np.asarray(seg["first_bin"], np.int64), np.asarray(seg["last_bin"], np.int64)
    if first.size < 2:
        z = np.zeros(0, np.int64)
        return dict(junction=z, left_bin=z.copy(), right_bin=z.copy(), scaffold=z.copy())
    sc = np.asarray(scaffold_of_bin, np.int64)
    k = np.nonzero((first[1:] == last[:-1] + 1) & (sc[fb[1:]] == sc[lb[:-1]]))[0] + 1
    return dict(junction=first[k], left_bin=lb[k - 1], right_bin=fb[k], scaffold=sc[fb[k]])


def bin_junctions(order, parent, contig):
    """the internal junctions at which the parent bin changes.  ``order``: the sub-fragment at every position; ``parent``: the bin
    of every sub-fragment; ``contig``: the scaffold of every bin (the current state's id_c)"""
    from .orientation_support import bin_segments

    return _between(bin_segments(order, parent), contig)


def block_junctions(order, parent, contig, ori, id_d, init_contig, init_pos):
    """the junctions where one block of ``orientation_support.block_segments`` ends and the next block of the same scaffold begins:
    the only places where a gap can exist (inside a block the input assembly vouches for adjacency).  Arguments as
    ``block_segments``"""
    from .orientation_support import block_segments

    return _between(block_segments(order, parent, contig, ori, id_d, init_contig, init_pos), contig)
