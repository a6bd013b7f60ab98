"""Balancing the contact map of the current genome: one weight per unit (sub-fragment, bin or pixel) that removes its coverage bias
-- iterative correction (ICE), the update of ``cooler balance``.  Every other report on the current genome reads raw counts; a raw
count times the weights of its two units (``balanced``) is what a Hi-C viewer shows.  This module is the single definition of the
rule (pure numpy, no GPU); the device passes (``ig_balance_build`` / ``ig_balance_run``, csrc/ig_kernels_bal.cuh) reproduce its arrays
byte for byte.

The rule.  UNITS -- level ``"sub"``: the positions of the genome order; ``"bin"``: the placed bins along it
(``assembly_contacts.units_along``); ``"map"``: the pixels of ``contact_map(max_side)`` (``contact_map.binning``).  ``key[s]`` is the
unit of sub-fragment s, -1 where it is not placed.

* ENTRIES: every contact whose two sub-fragments are placed, with units u != v and |u - v| >= ``ignore_diags`` (an integer >= 1: no
  diagonal is held), gives the two entries (u, v, c) and (v, u, c).  The others are counted into the scalars ``unplaced_observed``,
  ``within_observed`` (u == v) and ``band_observed`` and dropped.  Rows sorted by column, equal columns summed (int64): ``rowptr``,
  ``col``, ``count``; per unit ``nnz`` (its entries) and ``total`` (their sum).  A total >= 2^53 is refused: every count converts to
  a double exactly.  By construction

      unplaced_observed + within_observed + band_observed + kept_observed == sum(counts);  entries == 2 * (kept contacts)
      count.sum() == total.sum() == 2 * kept_observed

* MASK (host side, here and in the product): a unit is masked if nnz < ``min_nnz``, or total < ``min_count``, or -- ``mad_max`` > 0,
  cooler's filter -- log(total) lies more than ``mad_max`` median absolute deviations below the median over the units not masked so
  far (those with total > 0).  b0 = 1.0 for the kept units, 0.0 for the masked.
* THE ORDERED SUM, ``lane_sum(values, rowptr)``, per row: 64 accumulators start at +0.0; accumulator l adds the row's entries l,
  l + 64, l + 128, ... in that order; the accumulators are combined by the fixed tree a[l] += a[l + h], h = 32, 16, 8, 4, 2, 1; the sum
  is a[0].  ``vec_sum(x)``: the same over one row of all of x.  The order is a wave's: lane l of 64 holds accumulator l, reads
  coalesced, and the tree is six shuffles -- stated here so that numpy and the device add the same doubles in the same order.
* ONE ITERATION (cooler's update, every sum through the ordered sum):

      t    = float64(count) * b[col]
      marg = lane_sum(t, rowptr) * b
      nz   = marg != 0;  k = nz.sum()            (k == 0: stop, not converged, n_iters as reached)
      mean = vec_sum(marg) / k
      m    = where(nz, marg / mean, 1.0)
      b    = b / m
      d    = where(nz, m - 1.0, 0.0)
      var  = vec_sum(d * d) / k

  Stop after the first iteration with var < ``tol``, or after ``max_iters``.  One more marg is computed from the final b;
  scale = vec_sum(marg_final) / k_final, weight = b / sqrt(scale), nan where the unit is masked or marg_final == 0.

THE ENTRIES OF A BUILT MAP (``entries_of_rows``; the device: ``ig_balance_build_snapshot``, csrc/ig_kernels_balsnap.cuh).  Every map
the project builds is an upper-triangular CSR snapshot (col >= row, the columns of a row strictly ascending, int64 counts, the
diagonal allowed); its entries are the rule's ENTRIES without a pass over the contacts.  An entry (u, v, c), by the first test it
meets: u == v -> ``within_observed``; v - u < ``ignore_diags`` -> ``band_observed``; outside the MODE -> ``other_observed`` ("cis"
keeps group[u] == group[v], "trans" group[u] != group[v], "all" everything; ``group``: the scaffold of every unit); otherwise kept as
(u, v, c) and (v, u, c).  The kept entries are distinct, so nothing is summed and a single count is NOT limited to 32 bits (a pixel
of the scaffold matrix holds everything between two scaffolds); a unit's total still has to stay below 2^53.

      within_observed + band_observed + other_observed + kept_observed == count.sum();  entries == 2 * (kept entries) == entries_out
"""
from __future__ import annotations

import numpy as np

LEVELS = ("sub", "bin", "map")
# the order of ig_balance_build's scalars[8]
SCALARS = ("unplaced_observed", "within_observed", "band_observed", "kept_observed", "entries", "n_placed", "n_units", "entries_out")
OBSERVED_SCALARS = SCALARS[:4]
LANES = 64
DEFAULTS = dict(ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200)
MAX_TOTAL = 1 << 53
MODES = ("all", "cis", "trans")
# the order of ig_balance_build_snapshot's scalars[8]
SNAPSHOT_SCALARS = ("within_observed", "band_observed", "other_observed", "kept_observed", "entries", "entries_in", "n_units", "entries_out")
SNAPSHOT_OBSERVED_SCALARS = SNAPSHOT_SCALARS[:4]
BALANCE_COLUMNS = ("unit", "scaffold", "start", "end", "weight")


def check_level(level):
    """-> 0 "sub", 1 "bin", 2 "map"; ValueError otherwise"""
    if level not in LEVELS:
        raise ValueError("balance: level is one of %r (got %r)" % (LEVELS, level))
    return LEVELS.index(level)


def check_ignore_diags(ignore_diags):
    d = int(ignore_diags)
    if d != ignore_diags or d < 1:
        raise ValueError("balance: ignore_diags is a whole number >= 1 (the device holds no diagonal), got %r" % (ignore_diags,))
    return d


def check_run(tol, max_iters):
    """-> (tol as a float, max_iters as an int); ValueError for a negative (or nan) tol and for max_iters < 1"""
    t = float(tol)
    if not t >= 0.0:
        raise ValueError("balance: tol >= 0 (got %r)" % (tol,))
    n = int(max_iters)
    if n != max_iters or n < 1:
        raise ValueError("balance: max_iters is a whole number >= 1 (got %r)" % (max_iters,))
    return t, n


def keys_of(position, level="sub", unit=None, max_side=2048):
    """the unit of every sub-fragment (-1: not placed) and the number of units.  position: int [M], -1 where not placed; ``unit``:
    level "bin", the unit of every position (``assembly_contacts.units_along``) -> (key int64 [M], U)"""
    from .contact_map import binning

    lv = check_level(level)
    position = np.asarray(position, np.int64)
    placed = position >= 0
    T = int(placed.sum())
    key = np.full(position.size, -1, np.int64)
    if lv == 0:
        key[placed], U = position[placed], T
    elif lv == 1:
        unit = np.asarray(unit, np.int64)
        if unit.size != T:
            raise ValueError("balance: unit has one entry per position")
        key[placed] = unit[position[placed]]
        U = int(unit[-1]) + 1 if T else 0
    else:
        b, U = binning(T, max_side)
        key[placed] = position[placed] // b
    return key, int(U)


def entries_host(key, n_units, row, col, cnt, ignore_diags=2):
    """The entries of the rule.  key: int [M] (``keys_of``); row, col, cnt: the contacts -> dict: rowptr (int64 [U + 1]), col (int32),
    count (int64), nnz and total (int64 [U]) and the scalars of SCALARS"""
    d = check_ignore_diags(ignore_diags)
    key = np.asarray(key, np.int64)
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    U = int(n_units)
    a, b = key[row], key[col]
    unpl = (a < 0) | (b < 0)
    within = ~unpl & (a == b)
    band = ~unpl & ~within & (np.abs(a - b) < d)
    kept = ~unpl & ~within & ~band
    u, v, c = a[kept], b[kept], cnt[kept]
    e_row, e_col, e_cnt = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([c, c])
    flat = e_row * max(U, 1) + e_col
    keys, inverse = np.unique(flat, return_inverse=True)
    summed = np.zeros(keys.size, np.int64)
    np.add.at(summed, inverse, e_cnt)
    o_row, o_col = keys // max(U, 1), keys % max(U, 1)
    nnz = np.bincount(o_row, minlength=U).astype(np.int64)[:U]
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(nnz)
    total = np.zeros(U, np.int64)
    np.add.at(total, o_row, summed)
    if total.size and int(total.max()) >= MAX_TOTAL:
        raise ValueError("balance: a unit's contacts sum to 2^53 or more (counts must convert to doubles exactly)")
    return dict(rowptr=rowptr, col=o_col.astype(np.int32), count=summed, nnz=nnz, total=total, unplaced_observed=int(cnt[unpl].sum()),
                within_observed=int(cnt[within].sum()), band_observed=int(cnt[band].sum()), kept_observed=int(c.sum()), entries=2 * int(kept.sum()),
                n_placed=int((key >= 0).sum()), n_units=U, entries_out=int(keys.size))


def check_mode(mode):
    """-> 0 "all", 1 "cis", 2 "trans"; ValueError otherwise"""
    if mode not in MODES:
        raise ValueError("balance: mode is one of %r (got %r)" % (MODES, mode))
    return MODES.index(mode)


def check_rows(rowptr, col, count):
    """an upper-triangular CSR map -> (rowptr int64 [U + 1], col int64, count int64, the row of every entry); ValueError where it is
    not one: rowptr from 0 and non-decreasing, ending at the number of entries; col >= row, below U, strictly ascending in a row;
    no negative count"""
    rowptr = np.asarray(rowptr, np.int64)
    col, count = np.asarray(col, np.int64), np.asarray(count, np.int64)
    if rowptr.ndim != 1 or rowptr.size < 1 or rowptr[0] != 0 or (np.diff(rowptr) < 0).any():
        raise ValueError("balance: rowptr has n_units + 1 words, starts at 0 and does not decrease")
    U = rowptr.size - 1
    if col.ndim != 1 or col.shape != count.shape or col.size != int(rowptr[-1]):
        raise ValueError("balance: col and count have rowptr[-1] = %d entries each (got %d, %d)" % (int(rowptr[-1]), col.size, count.size))
    row = np.repeat(np.arange(U, dtype=np.int64), np.diff(rowptr))
    if col.size:
        if (col < row).any() or (col >= U).any():
            raise ValueError("balance: the map is upper triangular: row <= col < %d" % U)
        same = row[1:] == row[:-1]
        if (col[1:][same] <= col[:-1][same]).any():
            raise ValueError("balance: the columns of a row ascend strictly")
        if (count < 0).any():
            raise ValueError("balance: a negative count")
    return rowptr, col, count, row


def check_group(group, n_units, mode):
    """-> group as int64 [U], or None where the mode needs none; ValueError for a mode other than "all" without one, a wrong length
    and a negative group"""
    if check_mode(mode) == 0:
        return None
    if group is None:
        raise ValueError("balance: mode %r needs the group (the scaffold) of every unit" % (mode,))
    g = np.asarray(group, np.int64)
    if g.shape != (int(n_units),):
        raise ValueError("balance: group has one entry per unit (%d, got shape %r)" % (int(n_units), g.shape))
    if g.size and int(g.min()) < 0:
        raise ValueError("balance: a negative group")
    return g


def entries_of_rows(rowptr, col, count, ignore_diags=2, group=None, mode="all"):
    """The entries of the rule from a built map (the module's docstring).  rowptr, col, count: an upper-triangular CSR map; group:
    int [U] for ``mode`` "cis" / "trans" -> the dict of ``entries_host`` (rowptr, col int32, count int64, nnz, total) with the scalars
    of SNAPSHOT_SCALARS"""
    d = check_ignore_diags(ignore_diags)
    m = check_mode(mode)
    rowptr, v, c, u = check_rows(rowptr, col, count)
    U = rowptr.size - 1
    g = check_group(group, U, mode)
    within = u == v
    band = ~within & (v - u < d)
    other = np.zeros(u.size, bool)
    if m:
        same = g[u] == g[v]
        other = ~within & ~band & (~same if m == 1 else same)
    kept = ~within & ~band & ~other
    ku, kv, kc = u[kept], v[kept], c[kept]
    e_row, e_col, e_cnt = np.concatenate([ku, kv]), np.concatenate([kv, ku]), np.concatenate([kc, kc])
    o = np.lexsort((e_col, e_row))
    e_row, e_col, e_cnt = e_row[o], e_col[o], e_cnt[o]
    nnz = np.bincount(e_row, minlength=U).astype(np.int64)[:U]
    out_ptr = np.zeros(U + 1, np.int64)
    out_ptr[1:] = np.cumsum(nnz)
    psum = lambda a: int(a.sum(dtype=object)) if a.size else 0  # (a sum of int64 wraps silently: Python integers)
    hi, lo = np.zeros(U, np.int64), np.zeros(U, np.int64)  # the halves summed apart: neither sum can wrap below 2^31 entries
    np.add.at(hi, e_row, e_cnt >> 32)
    np.add.at(lo, e_row, e_cnt & 0xffffffff)
    too_much = (hi >= (1 << 21)) | (lo >= MAX_TOTAL)
    total = np.where(too_much, 0, (hi << 32) + lo)
    if (too_much | (total >= MAX_TOTAL)).any():
        raise ValueError("balance: a unit's contacts sum to 2^53 or more (counts must convert to doubles exactly)")
    return dict(rowptr=out_ptr, col=e_col.astype(np.int32), count=e_cnt, nnz=nnz, total=total, within_observed=psum(c[within]), band_observed=psum(c[band]),
                other_observed=psum(c[other]), kept_observed=psum(kc), entries=2 * int(kept.sum()), entries_in=int(c.size), n_units=U, entries_out=int(e_cnt.size))


def snapshot_observed_total(result):
    """every count of the map, wherever it went"""
    return sum(int(result[k]) for k in SNAPSHOT_OBSERVED_SCALARS)


def observed_total(result):
    """every contact's count, wherever it went"""
    return sum(int(result[k]) for k in OBSERVED_SCALARS)


def mask_units(nnz, total, min_nnz=10, min_count=0, mad_max=0):
    """-> bool [U]: the masked units"""
    nnz, total = np.asarray(nnz, np.int64), np.asarray(total, np.int64)
    masked = (nnz < int(min_nnz)) | (total < int(min_count))
    if mad_max > 0:
        ok = ~masked & (total > 0)
        if ok.any():
            lg = np.log(total[ok].astype(np.float64))
            med = np.median(lg)
            dev = np.median(np.abs(lg - med))
            low = np.zeros(total.size, bool)
            low[ok] = lg < med - float(mad_max) * dev
            masked |= low
    return masked


def lane_sum(values, rowptr):
    """the ordered sum of every row -> f64 [n_rows].  Vectorised: ceil(longest row / 64) steps over the rows still running, then the
    six halvings.  (A lane with no entry at a step adds +0.0: an accumulator starts at +0.0 and can never become -0.0, so that is
    exact.)"""
    values = np.asarray(values, np.float64)
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.size - 1
    acc = np.zeros((max(n, 0), LANES), np.float64)
    if n <= 0:
        return np.zeros(0, np.float64)
    first, lens = rowptr[:-1], np.diff(rowptr)
    lanes = np.arange(LANES, dtype=np.int64)
    live = np.nonzero(lens > 0)[0]
    done = 0
    while live.size:
        idx = first[live, None] + done + lanes[None, :]
        ok = lanes[None, :] < (lens[live, None] - done)
        acc[live] += np.where(ok, values[np.where(ok, idx, 0)] if values.size else 0.0, 0.0)
        done += LANES
        live = live[lens[live] > done]
    h = LANES // 2
    while h >= 1:
        acc[:, :h] += acc[:, h:2 * h]
        h //= 2
    return acc[:, 0].copy()


def lane_sum_loop(values, rowptr):
    """the same by a plain loop (the statement the tests hold ``lane_sum`` against)"""
    values = np.asarray(values, np.float64)
    out = np.zeros(len(rowptr) - 1, np.float64)
    for r in range(len(rowptr) - 1):
        a = [np.float64(0.0)] * LANES
        for i, e in enumerate(range(int(rowptr[r]), int(rowptr[r + 1]))):
            a[i % LANES] = a[i % LANES] + values[e]
        h = LANES // 2
        while h >= 1:
            for l in range(h):
                a[l] = a[l] + a[l + h]
            h //= 2
        out[r] = a[0]
    return out


def vec_sum(x):
    """the ordered sum over one row of all of x -> f64"""
    x = np.asarray(x, np.float64).ravel()
    return lane_sum(x, np.array([0, x.size], np.int64))[0]


def marginals(rowptr, col, count_f, b):
    return lane_sum(count_f * b[col], rowptr) * b


def iterate(rowptr, col, count, b0, tol=1e-5, max_iters=200):
    """The iterations of the rule from b0 -> dict: b, marg_final, variance (f64 [n_iters]), n_iters, converged"""
    tol, max_iters = check_run(tol, max_iters)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    count = np.asarray(count, np.int64)
    if count.size and int(count.max()) >= MAX_TOTAL:
        raise ValueError("balance: a count of 2^53 or more")
    cf = count.astype(np.float64)
    b = np.array(b0, np.float64)
    if b.size != rowptr.size - 1:
        raise ValueError("balance: b0 has one entry per unit")
    variance, converged = [], False
    with np.errstate(all="ignore"):
        for _ in range(max_iters):
            marg = marginals(rowptr, col, cf, b)
            nz = marg != 0
            k = int(nz.sum())
            if k == 0:
                break
            mean = vec_sum(marg) / np.float64(k)
            m = np.where(nz, marg / mean, 1.0)
            b = b / m
            d = np.where(nz, m - 1.0, 0.0)
            var = vec_sum(d * d) / np.float64(k)
            variance.append(var)
            if var < tol:
                converged = True
                break
        marg_final = marginals(rowptr, col, cf, b)
    return dict(b=b, marg_final=marg_final, variance=np.array(variance, np.float64), n_iters=len(variance), converged=converged)


def finish(b, marg_final, masked):
    """-> (weight f64 [U], scale): scale = vec_sum(marg_final) / k_final, weight = b / sqrt(scale), nan where the unit is masked or
    marg_final == 0 (and everywhere where no unit is left)"""
    b, marg_final = np.asarray(b, np.float64), np.asarray(marg_final, np.float64)
    nz = marg_final != 0
    k = int(nz.sum())
    with np.errstate(all="ignore"):
        scale = float(vec_sum(marg_final) / np.float64(k)) if k else float("nan")
        weight = b / np.sqrt(np.float64(scale))
    weight[np.asarray(masked, bool) | ~nz] = np.nan
    return weight, scale


def balance_entries(ent, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
    """mask, iterate and finish over built entries (``entries_host``'s dict, or the device's) -> the entries' dict plus weight, b,
    marg_final, masked, variance, n_iters, converged, scale and the parameters"""
    tol, max_iters = check_run(tol, max_iters)
    masked = mask_units(ent["nnz"], ent["total"], min_nnz, min_count, mad_max)
    out = dict(ent)
    out.update(iterate(ent["rowptr"], ent["col"], ent["count"], np.where(masked, 0.0, 1.0), tol, max_iters))
    out["weight"], out["scale"] = finish(out["b"], out["marg_final"], masked)
    out.update(masked=masked, min_nnz=int(min_nnz), min_count=int(min_count), mad_max=mad_max, tol=tol, max_iters=max_iters)
    return out


def balance_host(position, row, col, cnt, level="bin", unit=None, max_side=2048, ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5,
                 max_iters=200):
    """The whole rule from the positions and the contacts."""
    key, U = keys_of(position, level, unit, max_side)
    ent = entries_host(key, U, row, col, cnt, ignore_diags)
    out = balance_entries(ent, min_nnz, min_count, mad_max, tol, max_iters)
    out.update(level=level, max_side=int(max_side), ignore_diags=int(ignore_diags))
    return out


def balance_rows_host(rowptr, col, count, group=None, mode="all", ignore_diags=2, min_nnz=10, min_count=0, mad_max=0, tol=1e-5, max_iters=200):
    """The whole rule from a built map: ``entries_of_rows``, then the mask, the iterations and the finish of ``balance_host``."""
    ent = entries_of_rows(rowptr, col, count, ignore_diags, group, mode)
    out = balance_entries(ent, min_nnz, min_count, mad_max, tol, max_iters)
    out.update(level="units", mode=mode, ignore_diags=int(ignore_diags))
    return out


def balanced(count, row, col, weight):
    """count * weight[row] * weight[col] -> f64 (nan where a unit has no weight)"""
    w = np.asarray(weight, np.float64)
    return np.asarray(count, np.float64) * w[np.asarray(row, np.int64)] * w[np.asarray(col, np.int64)]


def write_weights(path, table, result):
    """one line per unit: the columns of BALANCE_COLUMNS (the scaffold by its name in genome.fasta, the weight with 17 digits: it
    reads back to the same double; ``nan`` for none), then the parameters and the scalars.  ``table``:
    ``assembly_contacts.bins_table`` of the same units.  -> the number of units written"""
    from .assembly_contacts import SCAFFOLD_PREFIX

    w = np.asarray(result["weight"], np.float64)
    if table.size != w.size:
        raise ValueError("balance: the table has %d units, the result %d" % (table.size, w.size))
    with open(path, "w") as f:
        f.write("# " + "\t".join(BALANCE_COLUMNS) + "\n")
        for u, (c, s, e, x) in enumerate(zip(table["contig"].tolist(), table["start"].tolist(), table["end"].tolist(), w.tolist())):
            f.write("%d\t%s%d\t%d\t%d\t%s\n" % (u, SCAFFOLD_PREFIX, c, s, e, "nan" if x != x else "%.17g" % x))
        f.write("# " + " ".join("%s=%s" % (k, result[k]) for k in ("level", "ignore_diags", "min_nnz", "min_count", "mad_max", "tol", "max_iters", "n_iters",
                                                                     "converged", "scale") if k in result)
                + " " + " ".join("%s=%d" % (k, result[k]) for k in SCALARS if k in result) + "\n")
    return int(w.size)


def write_snapshot_weights(path, table, result):
    """``write_weights`` for a result balanced from a built map (``balance_rows_host``, or the device's), and one more comment line
    behind it: the mode and the scalars only that route has (``other_observed``, ``entries_in``) -- a file written under "cis" tells so.
    ``read_weights`` reads both forms.  -> the number of units written"""
    n = write_weights(path, table, result)
    with open(path, "a") as f:
        f.write("# source=snapshot mode=%s other_observed=%d entries_in=%d\n" % (result["mode"], result["other_observed"], result["entries_in"]))
    return n


def read_weights(path):
    """-> (unit int64, scaffold names, start int64, end int64, weight f64) of a file ``write_weights`` wrote"""
    unit, name, start, end, weight = [], [], [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            u, n, s, e, w = line.rstrip("\n").split("\t")
            unit.append(int(u)), name.append(n), start.append(int(s)), end.append(int(e)), weight.append(float(w))
    return np.array(unit, np.int64), np.array(name, dtype=object), np.array(start, np.int64), np.array(end, np.int64), np.array(weight, np.float64)
