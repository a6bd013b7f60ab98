"""The contact levels of the pyramid, stated once: numpy, no GPU.

``pyramid.build_and_filter`` turns the contact list of the input folder into the filtered level 0 and every binned level by
re-indexing the list through a table and summing the equal pairs again.  This module is that rule, and the device path
(``csrc/ig_kernels_pyr.cuh``, ``hip_lib.Context.pyr_*``) reproduces its arrays word for word.

All ids are 0-based.  ``lut[old] = new``, or -1 for a fragment the filter destroyed.  A level is three int64 arrays
``(row, col, total)``: the upper-triangular sum over ``(min, max)``, rows ascending, columns ascending inside a row, 64-bit sums.

* For a canonical list (``canonical``) the level is the list itself, and it is ``pyramid.fill_sparse_pyramid_level``'s ``data3``.
  ``pre``, the filter and every binning write canonical lists.
* For a list that is not canonical the reference orders the columns of a row by their first appearance in the file.  Only level 0 of
  ``pyramid_1_no_thresh`` and level 0 of a ``build()`` pyramid can see such a list, and for that one matrix the device path calls the
  existing host function (``fill_sparse_pyramid_level``); the device only reports that the list is not canonical.  Everything made
  FROM such a list (the degrees, the filtered level, the binned levels) is a sum, which does not depend on the order.
* A sum of 2^31 or more anywhere is refused (``LevelOverflow``) naming the level and the pixel, here and on the device: the host path
  of ``pyramid.py`` would wrap it silently when it stores int32.  2^31 - 1 passes.
"""
from __future__ import annotations

import numpy as np

LIMIT = 1 << 31  # PYR_LIMIT (csrc/ig_kernels_pyr.cuh)
SCALARS = ("entries_in", "skipped", "dropped_by_lut", "entries_kept", "pixels", "largest_sum")  # ig_pyr_remap


class LevelOverflow(ValueError):
    """a pixel's sum does not fit the level's int32"""


def _i64(x):
    return np.ascontiguousarray(x, np.int64).ravel()


def canonical(a, b):
    """true when every entry has ``a <= b`` and the pairs ``(a, b)`` are strictly ascending in file order"""
    a, b = _i64(a), _i64(b)
    if a.size != b.size:
        raise ValueError("canonical: one a and one b per entry")
    if a.size == 0:
        return True
    if np.any(a > b):
        return False
    return bool(np.all((a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] > b[:-1]))))


def refuse_overflow(row, col, total, level=None):
    """raises ``LevelOverflow`` naming the first pixel whose sum is 2^31 or more"""
    bad = np.nonzero(total >= LIMIT)[0]
    if bad.size:
        k = int(bad[0])
        raise LevelOverflow("level %s: the sum of the pixel (%d, %d) is %d: 2^31 or more does not fit the level's int32"
                            % ("?" if level is None else level, int(row[k]), int(col[k]), int(total[k])))


def level_matrix(a, b, count, level=None):
    """the upper-triangular sum over ``(min, max)`` -> ``(row, col, total)``, int64, rows ascending, columns ascending; an entry whose
    counts sum to zero stays (a stored zero).  ``level``: named by the refusal of a sum >= 2^31."""
    a, b, count = _i64(a), _i64(b), _i64(count)
    if not (a.size == b.size == count.size):
        raise ValueError("level_matrix: one a, one b and one count per entry")
    if a.size and (min(int(a.min()), int(b.min())) < 0 or int(count.min()) < 0):
        raise ValueError("level_matrix: negative id or count")
    if a.size == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    lo, hi, cnt = lo[order], hi[order], count[order]
    head = np.concatenate(([True], (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])))
    starts = np.nonzero(head)[0]
    # exact: the partial sums are checked in float64 first, where 2^31 * entries is far below 2^53 only for short runs -- so sum in
    # Python integers wherever an int64 could wrap
    if float(cnt.astype(np.float64).sum()) < 2.0 ** 62:
        total = np.add.reduceat(cnt, starts)
    else:
        ends = np.concatenate((starts[1:], [cnt.size]))
        total = np.array([min(sum(int(v) for v in cnt[s:e]), (1 << 63) - 1) for s, e in zip(starts, ends)], np.int64)
    row, col = lo[starts], hi[starts]
    refuse_overflow(row, col, total, level)
    return row, col, total


def degrees(M, n):
    """``deg[i]``: the number of ``j`` with ``(M + M^T)[i, j] != 0`` -- a stored zero count is no partner, a diagonal entry counts
    once (scipy's ``csr + csr.T`` drops the zeros: what ``remove_problematic_fragments`` counts)"""
    row, col, total = (_i64(x) for x in M)
    nz = total != 0
    deg = np.bincount(row[nz], minlength=int(n)).astype(np.int64)
    off = nz & (row != col)
    deg += np.bincount(col[off], minlength=int(n))
    return deg


def remap(a, b, count, lut, skip_first, level=None, scalars=None):
    """the next level: entry 0 of the list dropped when ``skip_first`` (quirk Q-P1: binning loses the first contact of the file; the
    filter reads all of them), both ends through ``lut``, an entry dropped when either end is -1, ``level_matrix`` of the rest.
    ``scalars``: a dict that gets ``SCALARS``."""
    a, b, count, lut = _i64(a), _i64(b), _i64(count), _i64(lut)
    n_in = a.size
    first = 1 if (skip_first and n_in) else 0
    a, b, count = a[first:], b[first:], count[first:]
    if a.size and (min(int(a.min()), int(b.min())) < 0 or max(int(a.max()), int(b.max())) >= lut.size):
        raise ValueError("remap: an id outside the table")
    na, nb = lut[a], lut[b]
    keep = (na >= 0) & (nb >= 0)
    M = level_matrix(na[keep], nb[keep], count[keep], level)
    if scalars is not None:
        scalars.update(entries_in=n_in, skipped=first, dropped_by_lut=int((~keep).sum()), entries_kept=int(keep.sum()), pixels=int(M[0].size),
                       largest_sum=int(M[2].max()) if M[2].size else 0)
    return M


def data3(M):
    """a level as the ``(3, nnz)`` int32 array of the ``SparseStore``"""
    return np.stack([_i64(x) for x in M]).astype(np.int32) if len(M[0]) else np.zeros((3, 0), np.int32)
