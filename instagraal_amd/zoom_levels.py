"""Fixed-resolution maps of the current genome: the contacts at a bin size in bp, at several zoom levels, and scaffold by scaffold
-- what ``cooler load`` and ``cooler zoomify`` are used for, in the form ``assembly_contacts`` writes.  This module is the single
definition of the rule (pure numpy, no GPU); the device passes (``ig_assembly_contacts_build_units``,
``ig_assembly_contacts_coarsen``, csrc/ig_kernels_zoom.cuh) reproduce its arrays byte for byte.

The rule.  The scaffolds are the placed contigs in genome order, ``size_k`` bp long (``assembly_contacts.chrom_sizes`` of the
sub-fragment table).  At bin size B scaffold k has ``nb_k = max(1, ceil(size_k / B))`` FIXED BINS ``(i B, min((i + 1) B, size_k))``,
numbered from ``off_k``, the running sum of the ``nb``.  The UNIT of a position is the fixed bin that holds the midpoint of its
sub-fragment: ``off_k + min(((start + end) // 2) // B, nb_k - 1)``, in exact integers.  Units are non-decreasing along the order and
may step by more than one: a sub-fragment longer than B leaves units without a position, whose rows are empty
(``units_without_position`` counts them: the resolution is below what the fragments carry).  At scaffold level the unit of a
position is the rank of its scaffold.

The contacts are lifted as at level "bin" of ``assembly_contacts`` with that unit table (``lift_units_host``): keys (min unit, max
unit), equal keys summed into int64, lo == hi kept, unplaced ends counted apart.

The identity that makes a zoom chain legitimate: with ``coarse_map(B, f)`` -- per scaffold ``off'_k + (u - off_k) // f`` --

    coarsen_host(lift_units_host(units at B), coarse_map(B, f)) == lift_units_host(units at f B)      entry for entry,

because (mid // B) // f = mid // (f B), (nb - 1) // f = ceil(nb / f) - 1 and ceil(ceil(s / B) / f) = ceil(s / (f B)).  So a level
whose bin size is a multiple of the level built just before it may be made from that level alone, without another pass over the
contacts (``plan``): the bytes do not depend on the plan, it is a cost choice only.
"""
from __future__ import annotations

import os

import numpy as np

from . import assembly_contacts as ac

DEFAULT_RESOLUTIONS = (10_000, 20_000, 50_000, 100_000, 200_000, 500_000, 1_000_000)
FIXED_BINS_DTYPE = np.dtype([("contig", np.int64), ("start", np.int64), ("end", np.int64)])
MAX_UNITS = (1 << 31) - 1  # a column is an int32


def check_binsize(binsize):
    b = int(binsize)
    if b != binsize or b < 1:
        raise ValueError("zoom levels: a bin size is a whole number of bp >= 1 (got %r)" % (binsize,))
    return b


def _sizes(chrom_sizes):
    ids, sizes = chrom_sizes
    ids, sizes = np.asarray(ids, np.int64).ravel(), np.asarray(sizes, np.int64).ravel()
    if ids.size != sizes.size or (sizes.size and sizes.min() < 0):
        raise ValueError("zoom levels: chrom_sizes is (contig ids, sizes >= 0) of one length")
    return ids, sizes


def bins_per_scaffold(chrom_sizes, binsize):
    """-> (nb int64 [K], off int64 [K + 1]): the fixed bins of every scaffold and the running sum from 0 (off[K]: all units)"""
    B = check_binsize(binsize)
    _, sizes = _sizes(chrom_sizes)
    nb = np.maximum(1, -(-sizes // B))
    off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    if int(off[-1]) > MAX_UNITS:
        raise ValueError("zoom levels: %d bins of %d bp are more than 2^31 - 1 units" % (int(off[-1]), B))
    return nb.astype(np.int64), off


def binnify(chrom_sizes, binsize):
    """the fixed bins of ``binsize`` bp of the scaffolds in genome order, the last of a scaffold cut at its end (a scaffold of 0 bp
    keeps one empty bin) -> FIXED_BINS_DTYPE array [U].  chrom_sizes: (contig ids, sizes)"""
    B = check_binsize(binsize)
    ids, sizes = _sizes(chrom_sizes)
    nb, off = bins_per_scaffold((ids, sizes), B)
    t = np.zeros(int(off[-1]), FIXED_BINS_DTYPE)
    k = np.repeat(np.arange(ids.size, dtype=np.int64), nb)
    i = np.arange(t.size, dtype=np.int64) - off[:-1][k]
    t["contig"] = ids[k]
    t["start"] = i * B
    t["end"] = np.minimum((i + 1) * B, sizes[k])
    return t


def scaffold_units(table_sub):
    """the unit of every position at scaffold level: the rank of its scaffold in genome order -> (unit int64 [T], U).  table_sub:
    ``assembly_contacts.bins_table(..., "sub")``"""
    c = np.asarray(table_sub["contig"], np.int64)
    if c.size == 0:
        return np.zeros(0, np.int64), 0
    unit = np.cumsum(np.concatenate([[True], c[1:] != c[:-1]])) - 1
    return unit.astype(np.int64), int(unit[-1]) + 1


def scaffold_table(table_sub):
    """one row per scaffold: (contig, 0, size)"""
    ids, sizes = ac.chrom_sizes(table_sub)
    t = np.zeros(ids.size, FIXED_BINS_DTYPE)
    t["contig"], t["end"] = ids, sizes
    return t


def units_of_positions(table_sub, binsize):
    """the unit of every position at ``binsize`` bp: the fixed bin that holds the midpoint of its sub-fragment -> (unit int64 [T],
    U); U counts every fixed bin, with a position or without"""
    B = check_binsize(binsize)
    nb, off = bins_per_scaffold(ac.chrom_sizes(table_sub), B)
    k, _ = scaffold_units(table_sub)
    mid = (np.asarray(table_sub["start"], np.int64) + np.asarray(table_sub["end"], np.int64)) // 2
    unit = off[:-1][k] + np.minimum(mid // B, nb[k] - 1)
    return unit.astype(np.int64), int(off[-1])


def units_without_position(unit, n_units):
    """the units no position falls into: their rows are empty whatever the contacts"""
    return int(n_units) - int(np.unique(np.asarray(unit, np.int64)).size)


def check_units(unit, n_units, n_positions=None):
    """a caller's unit table: one unit per position, non-decreasing, inside 0 .. n_units - 1, n_units < 2^31 -> (int64 [T], U)"""
    unit = np.asarray(unit)
    U = int(n_units)
    if unit.ndim != 1 or not (np.issubdtype(unit.dtype, np.integer) or unit.size == 0):
        raise ValueError("zoom levels: the unit table is one vector of integers")
    unit = unit.astype(np.int64)
    if n_positions is not None and unit.size != int(n_positions):
        raise ValueError("zoom levels: the unit table has %d entries, the genome %d positions" % (unit.size, int(n_positions)))
    if U < 0 or U > MAX_UNITS:
        raise ValueError("zoom levels: n_units is 0 .. 2^31 - 1 (got %d)" % U)
    if unit.size and (unit.min() < 0 or unit.max() >= U or np.any(np.diff(unit) < 0)):
        raise ValueError("zoom levels: the units are non-decreasing along the order and inside 0 .. n_units - 1")
    return unit, U


def _csr(lo, hi, c, U):
    """(lo, hi, c) entries with equal keys summed -> rowptr, col, count"""
    flat = lo * max(U, 1) + hi
    keys, inverse = np.unique(flat, return_inverse=True)
    out_c = np.zeros(keys.size, np.int64)
    np.add.at(out_c, inverse.ravel(), c)
    out_lo, out_hi = keys // max(U, 1), keys % max(U, 1)
    rowptr = np.zeros(U + 1, np.int64)
    if U:
        rowptr[1:] = np.cumsum(np.bincount(out_lo, minlength=U)[:U])
    return rowptr, out_hi.astype(np.int32), out_c.astype(np.int64)


def lift_units_host(position, row, col, cnt, unit, n_units):
    """The rule of ``assembly_contacts.lift_host`` at level "bin" with a caller's unit table, which may have gaps.  position: int
    [M], -1 where not placed; row, col, cnt: the contacts (row < col); unit: int [T]; -> dict: rowptr (int64 [U + 1]), col (int32,
    strictly ascending inside a row), count (int64) and the scalars of ``assembly_contacts.SCALARS``"""
    position = np.asarray(position, np.int64)
    row, col, cnt = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(cnt, np.int64)
    placed = position >= 0
    T = int(placed.sum())
    if T and not np.array_equal(np.sort(position[placed]), np.arange(T)):
        raise ValueError("zoom levels: the positions of the placed sub-fragments must be 0 .. T - 1, each once")
    if row.size and not np.all(row < col):
        raise ValueError("zoom levels: the contacts are the strict upper triangle (row < col)")
    unit, U = check_units(unit, n_units, T)
    key = np.full(position.size, -1, np.int64)
    key[placed] = unit[position[placed]]
    a, b = key[row], key[col]
    kept = (a >= 0) & (b >= 0)
    c = cnt[kept]
    rowptr, out_col, out_c = _csr(np.minimum(a, b)[kept], np.maximum(a, b)[kept], c, U)
    out = dict(rowptr=rowptr, col=out_col, count=out_c)
    out.update(entries_in=int(row.size), entries_kept=int(kept.sum()), contacts_kept=int(c.sum()), entries_unplaced=int((~kept).sum()),
               contacts_unplaced=int(cnt[~kept].sum()), n_placed=T, n_units=U, entries_out=int(out_c.size))
    return out


def check_coarse_map(coarse_of_unit, n_coarse, n_units=None):
    m = np.asarray(coarse_of_unit)
    C = int(n_coarse)
    if m.ndim != 1 or not (np.issubdtype(m.dtype, np.integer) or m.size == 0):
        raise ValueError("zoom levels: the coarse map is one vector of integers")
    m = m.astype(np.int64)
    if n_units is not None and m.size != int(n_units):
        raise ValueError("zoom levels: the coarse map has %d entries, the level %d units" % (m.size, int(n_units)))
    if C < 0 or C > MAX_UNITS:
        raise ValueError("zoom levels: n_coarse is 0 .. 2^31 - 1 (got %d)" % C)
    if m.size and (m.min() < 0 or m.max() >= C or np.any(np.diff(m) < 0)):
        raise ValueError("zoom levels: the coarse map is non-decreasing and inside 0 .. n_coarse - 1")
    return m, C


def coarsen_host(rowptr, col, count, coarse_of_unit, n_coarse):
    """entry (lo, hi, c) of a CSR level goes to (coarse_of_unit[lo], coarse_of_unit[hi]), equal keys summed -> (rowptr int64
    [n_coarse + 1], col int32, count int64) of the same form"""
    rowptr = np.asarray(rowptr, np.int64)
    m, C = check_coarse_map(coarse_of_unit, n_coarse, rowptr.size - 1)
    lo = m[ac.rows_of(rowptr)]
    hi = m[np.asarray(col, np.int64)]
    return _csr(lo, hi, np.asarray(count, np.int64), C)


def coarse_map(chrom_sizes, binsize, factor):
    """the fixed bins of ``binsize`` bp -> those of ``factor * binsize`` bp: per scaffold off'_k + (u - off_k) // factor ->
    (coarse_of_unit int64 [U], n_coarse)"""
    f = int(factor)
    if f != factor or f < 1:
        raise ValueError("zoom levels: a factor is a whole number >= 1 (got %r)" % (factor,))
    B = check_binsize(binsize)
    nb, off = bins_per_scaffold(chrom_sizes, B)
    _, off2 = bins_per_scaffold(chrom_sizes, B * f)
    k = np.repeat(np.arange(nb.size, dtype=np.int64), nb)
    u = np.arange(int(off[-1]), dtype=np.int64)
    return (off2[:-1][k] + (u - off[:-1][k]) // f).astype(np.int64), int(off2[-1])


def scaffold_map(chrom_sizes, binsize):
    """the fixed bins of ``binsize`` bp -> the scaffolds -> (coarse_of_unit int64 [U], K)"""
    nb, _ = bins_per_scaffold(chrom_sizes, binsize)
    return np.repeat(np.arange(nb.size, dtype=np.int64), nb), int(nb.size)


def check_resolutions(resolutions):
    res = [check_binsize(b) for b in resolutions]
    if not res:
        raise ValueError("zoom levels: at least one resolution")
    if len(set(res)) != len(res):
        raise ValueError("zoom levels: the resolutions are distinct (got %r)" % (res,))
    if res != sorted(res):
        raise ValueError("zoom levels: the resolutions are ascending (got %r)" % (res,))
    return tuple(res)


def plan(resolutions):
    """how every level is made, in order: ``("coarsen", factor)`` where the bin size is a multiple of the level built immediately
    before it (the only one resident), else ``("direct",)``"""
    res = check_resolutions(resolutions)
    out = []
    for i, b in enumerate(res):
        out.append(("coarsen", b // res[i - 1]) if i and b % res[i - 1] == 0 else ("direct",))
    return out


def level_folder(folder, binsize):
    return os.path.join(folder, "resolutions", str(check_binsize(binsize)))


def scaffold_folder(folder):
    return os.path.join(folder, "scaffolds")


def write_level(folder, table, rowptr, fetch, block_rows=ac.DEFAULT_BLOCK_ROWS, diag=None, weights=None):
    """bins.bed, pixels.tsv and chrom.sizes of one level into ``folder`` (``assembly_contacts.write_all`` over the fixed bins);
    ``weights``: a ``balance`` result over the same units, written as weights.tsv beside them -> the number of pixels written"""
    n = ac.write_all(folder, table, rowptr, fetch, block_rows, diag)
    if weights is not None:
        from . import balance as bal

        bal.write_weights(os.path.join(folder, "weights.tsv"), table, weights)
    return n


def fetch_of(col, count):
    """``fetch(first, n)`` over host arrays, for the writers"""
    return lambda first, n: (col[first:first + n], count[first:first + n])


def read_pixels(path):
    """-> (bin1 int64, bin2 int64, count int64) of a pixels.tsv"""
    a = np.loadtxt(path, dtype=np.int64, ndmin=2) if os.path.getsize(path) else np.zeros((0, 3), np.int64)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def read_bins_bed(path):
    """-> FIXED_BINS_DTYPE array of a bins.bed"""
    rows = []
    with open(path) as f:
        for line in f:
            name, s, e = line.rstrip("\n").split("\t")
            rows.append((int(name[len(ac.SCAFFOLD_PREFIX):]), int(s), int(e)))
    return np.array(rows, FIXED_BINS_DTYPE) if rows else np.zeros(0, FIXED_BINS_DTYPE)
