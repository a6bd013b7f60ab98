"""The contacts in the coordinates of the current genome: every Hi-C contact re-indexed from sub-fragment ids to the scaffolded
assembly, sorted, at full resolution -- the data behind the contact map, the distance law and the junction profile, in the form
``cooler load -f coo bins.bed pixels.tsv`` takes.  This module is the single definition of the rule (pure numpy, no GPU); the device
passes (``ig_assembly_contacts_build``, csrc/ig_kernels_lift.cuh, csrc/ig_kernels_rows.cuh) reproduce its arrays byte for byte.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs (contigs in ascending canonical id, a
contig placed only if every one of its bins is active, ``full_order_high`` inside it), 0 .. T - 1; ``position[s]`` is the place of
sub-fragment ``s``, -1 where it is not placed.  The contacts are ``(row, col, cnt)`` with ``row < col`` in sub-fragment ids.

* Level ``"sub"``: a UNIT is a position, U = T.  A contact with both ends placed becomes ``(lo, hi, cnt)``, lo = min and hi = max of
  the two positions; ``position`` is injective on the placed sub-fragments, so lo < hi and no key occurs twice.
* Level ``"bin"``: the unit of a position is the rank of its parent bin among the placed bins in genome order (``unit[r]``,
  non-decreasing, one head per bin: the sub-fragments of a bin are neighbours in the order).  Keys are (min unit, max unit), equal
  keys are summed into int64, entries with lo == hi (two sub-fragments of one bin) are kept.
* A contact with an end that is not placed is counted apart (``entries_unplaced``, ``contacts_unplaced``), never dropped silently.

The result is the CSR form of the upper triangle: ``rowptr`` int64 [U + 1], ``col`` int32 [n_out] strictly ascending inside a
row, ``count`` int64 [n_out], and the eight int64 scalars named in SCALARS.  By construction:

    contacts_kept + contacts_unplaced == cnt.sum()
    count.sum() == contacts_kept
    entries_out == entries_kept at level "sub"
"""
from __future__ import annotations

import numpy as np

LEVELS = ("sub", "bin")
# the order of ig_assembly_contacts_build's scalars[8]
SCALARS = ("entries_in", "entries_kept", "contacts_kept", "entries_unplaced", "contacts_unplaced", "n_placed", "n_units", "entries_out")
SUMMED_SCALARS = SCALARS[:5]  # what the shards of a sharded handle add up in (entries_out too at level "sub")
BINS_DTYPE = np.dtype([("contig", np.int64), ("start", np.int64), ("end", np.int64), ("bin", np.int64), ("ori", np.int64)])
SCAFFOLD_PREFIX = "3C-assembly-contig_"  # io_frags.write_assembly's name of the same scaffold in genome.fasta
DEFAULT_BLOCK_ROWS = 4096


def check_level(level):
    """-> 0 for "sub", 1 for "bin"; ValueError otherwise"""
    if level not in LEVELS:
        raise ValueError("assembly contacts: level is one of %r (got %r)" % (LEVELS, level))
    return LEVELS.index(level)


def positions_of(order, n_sub_frags):
    """``order[r]`` = the sub-fragment at position r -> ``position[s]``, -1 where s is not in the order"""
    order = np.asarray(order, np.int64)
    position = np.full(int(n_sub_frags), -1, np.int64)
    position[order] = np.arange(order.size)
    return position


def units_along(parent_by_position):
    """the unit of every position at level "bin": the heads are where the parent bin changes along the order -> int64 [T],
    non-decreasing from 0"""
    p = np.asarray(parent_by_position, np.int64)
    if p.size == 0:
        return np.zeros(0, np.int64)
    head = np.concatenate([[True], p[1:] != p[:-1]])
    return np.cumsum(head) - 1


def lift_host(position, row, col, cnt, unit=None):
    """The rule.  position: int [M]; row, col, cnt: the contacts; ``unit``: None (level "sub") or the unit of every position
    (level "bin", int [T]).  -> dict: rowptr, col, count and the scalars."""
    position = np.asarray(position, np.int64)
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    cnt = np.asarray(cnt, np.int64)
    placed = position >= 0
    T = int(placed.sum())
    if T and not np.array_equal(np.sort(position[placed]), np.arange(T)):
        raise ValueError("assembly contacts: the positions of the placed sub-fragments must be 0 .. T - 1, each once")
    if row.size and not np.all(row < col):
        raise ValueError("assembly contacts: the contacts are the strict upper triangle (row < col)")
    if unit is None:
        key, U = position, T
    else:
        unit = np.asarray(unit, np.int64)
        if unit.size != T or (T and (unit[0] != 0 or np.any(np.diff(unit) < 0) or np.any(np.diff(unit) > 1))):
            raise ValueError("assembly contacts: unit has one entry per position, from 0, non-decreasing in steps of at most one")
        U = int(unit[-1]) + 1 if T else 0
        key = np.full(position.size, -1, np.int64)
        key[placed] = unit[position[placed]]
    a, b = key[row], key[col]
    kept = (a >= 0) & (b >= 0)
    lo, hi, c = np.minimum(a, b)[kept], np.maximum(a, b)[kept], cnt[kept]
    flat = lo * max(U, 1) + hi
    if unit is None:
        by = np.argsort(flat, kind="stable")
        if by.size > 1 and np.any(np.diff(flat[by]) == 0):
            raise ValueError("assembly contacts: a key occurs twice at level sub (the contacts are not distinct)")
        out_lo, out_hi, out_c = lo[by], hi[by], c[by]
    else:
        keys, inverse = np.unique(flat, return_inverse=True)
        out_c = np.zeros(keys.size, np.int64)
        np.add.at(out_c, inverse, c)
        out_lo, out_hi = keys // max(U, 1), keys % max(U, 1)
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(out_lo, minlength=U)[:U]) if U else 0
    out = dict(rowptr=rowptr, col=out_hi.astype(np.int32), count=out_c.astype(np.int64))
    out.update(entries_in=int(row.size), entries_kept=int(kept.sum()), contacts_kept=int(c.sum()), entries_unplaced=int((~kept).sum()),
               contacts_unplaced=int(cnt[~kept].sum()), n_placed=T, n_units=U, entries_out=int(out_c.size))
    return out


def rows_of(rowptr):
    """the row of every entry of a CSR result -> int64 [n_out]"""
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def merge_diagonal(first_row, rowptr, col, count, diag):
    """Entries (u, u, diag[u]) merged into the rows first_row .. first_row + len(diag) - 1 of a CSR block, first in their rows:
    added to the row's own (u, u) entry where there is one (level "bin"), inserted otherwise.  rowptr: the block's, from 0.
    -> (rowptr, col, count) of the merged block"""
    rowptr, col, count, diag = np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(count, np.int64).copy(), np.asarray(diag, np.int64)
    n = diag.size
    rows = first_row + np.arange(n, dtype=np.int64)
    has = np.zeros(n, bool)
    nonempty = rowptr[1:] > rowptr[:-1]
    has[nonempty] = col[rowptr[:-1][nonempty]] == rows[nonempty]
    add = (diag != 0) & has
    count[rowptr[:-1][add]] += diag[add]
    ins = (diag != 0) & ~has
    col = np.insert(col, rowptr[:-1][ins], rows[ins].astype(np.int32))
    count = np.insert(count, rowptr[:-1][ins], diag[ins])
    lens = np.diff(rowptr) + ins
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col, count


def bins_table(order, parent, contig_of_bin, ori_of_bin, len_bp, level="sub"):
    """The units of the genome as a BINS_DTYPE array, one row per unit in genome order: the canonical id of its scaffold (its name:
    ``scaffold_names``), ``start`` and ``end`` in bp inside the scaffold -- the running sum of ``len_bp`` over the sub-fragments in
    genome order, from 0 with every contig --, the parent bin and its orientation.  order: the sub-fragment at every position;
    parent: the bin of every sub-fragment; contig_of_bin, ori_of_bin: per bin (the downloaded state's id_c and ori); len_bp: per
    sub-fragment.  Level "bin": the table of level "sub" merged by unit."""
    check_level(level)
    order = np.asarray(order, np.int64)
    b = np.asarray(parent, np.int64)[order]
    t = np.zeros(order.size, BINS_DTYPE)
    if order.size == 0:
        return t
    t["bin"] = b
    t["contig"] = np.asarray(contig_of_bin, np.int64)[b]
    t["ori"] = np.asarray(ori_of_bin, np.int64)[b]
    ln = np.asarray(len_bp, np.int64)[order]
    run = np.cumsum(ln)
    head = np.concatenate([[True], t["contig"][1:] != t["contig"][:-1]])
    base = np.repeat((run - ln)[head], np.diff(np.concatenate([np.nonzero(head)[0], [order.size]])))
    t["end"] = run - base
    t["start"] = t["end"] - ln
    if level == "bin":
        unit = units_along(b)
        first = np.concatenate([[True], unit[1:] != unit[:-1]])
        last = np.concatenate([first[1:], [True]])
        merged = t[first].copy()
        merged["end"] = t["end"][last]
        return merged
    return t


def scaffold_names(contig):
    """the names ``io_frags.write_assembly`` gives the scaffolds of these canonical ids in genome.fasta"""
    return np.array([SCAFFOLD_PREFIX + str(int(c)) for c in np.asarray(contig).ravel()], dtype=object)


def chrom_sizes(table):
    """-> (contig ids, sizes): per scaffold of a bins table, in its order, the last ``end``"""
    if table.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    last = np.concatenate([table["contig"][1:] != table["contig"][:-1], [True]])
    return table["contig"][last].copy(), table["end"][last].copy()


def write_bins_bed(path, table, block_rows=1 << 16):
    """``chrom\\tstart\\tend`` per unit, block by block"""
    with open(path, "w") as f:
        for a in range(0, table.size, int(block_rows)):
            t = table[a:a + int(block_rows)]
            f.write("".join("%s%d\t%d\t%d\n" % (SCAFFOLD_PREFIX, c, s, e) for c, s, e in zip(t["contig"].tolist(), t["start"].tolist(), t["end"].tolist())))


def write_chrom_sizes(path, table):
    ids, sizes = chrom_sizes(table)
    with open(path, "w") as f:
        for c, n in zip(ids.tolist(), sizes.tolist()):
            f.write("%s%d\t%d\n" % (SCAFFOLD_PREFIX, c, n))


def write_pixels(path, rowptr, fetch, block_rows=DEFAULT_BLOCK_ROWS, diag=None):
    """``bin1_id\\tbin2_id\\tcount`` per entry, zero-based, sorted by (bin1, bin2), upper-triangular: the ``pixels.tsv`` of
    ``cooler load -f coo``.  The entries come through ``fetch(first, n) -> (col, count)`` by blocks of ``block_rows`` rows, and only a
    block's text is ever held.  ``diag`` (int64 per unit, or None): self-contacts merged in as ``merge_diagonal`` does.
    -> the number of lines written"""
    rowptr = np.asarray(rowptr, np.int64)
    U = rowptr.size - 1
    step = max(int(block_rows), 1)
    n_lines = 0
    with open(path, "w") as f:
        for r0 in range(0, U, step):
            r1 = min(r0 + step, U)
            e0, e1 = int(rowptr[r0]), int(rowptr[r1])
            col, count = fetch(e0, e1 - e0)
            ptr = rowptr[r0:r1 + 1] - e0
            if diag is not None:
                ptr, col, count = merge_diagonal(r0, ptr, col, count, np.asarray(diag, np.int64)[r0:r1])
            if ptr[-1] == 0:
                continue
            b1 = r0 + rows_of(ptr)
            f.write("".join("%d\t%d\t%d\n" % x for x in zip(b1.tolist(), np.asarray(col).tolist(), np.asarray(count).tolist())))
            n_lines += int(ptr[-1])
    return n_lines


def write_all(folder, table, rowptr, fetch, block_rows=DEFAULT_BLOCK_ROWS, diag=None):
    """bins.bed, pixels.tsv and chrom.sizes into ``folder`` (created if need be) -> the number of pixels written"""
    import os

    os.makedirs(folder, exist_ok=True)
    write_bins_bed(os.path.join(folder, "bins.bed"), table)
    write_chrom_sizes(os.path.join(folder, "chrom.sizes"), table)
    return write_pixels(os.path.join(folder, "pixels.tsv"), rowptr, fetch, block_rows, diag)
