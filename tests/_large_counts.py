"""Synthetic problems whose contact counts reach 2^25 - 1, 2^25 and 2^31 - 1 (tests/test_large_counts_host.py,
tests/test_hip_large_counts.py): the counts at which the reports pick the `int` or the `long long` form of their segmented wave scan,
and at which every sum leaves 32 bits.  A helper module: nothing here is collected.

DENSE ROWS.  The contact list is the union of the synth contacts and of eight dense rows: on the longest contig of the fresh genome,
the sub-fragment at position p of the contig gets a contact with each of the positions p + 1 .. p + 192.  A row's contacts are
consecutive in the row-major list (the synth contacts of the same pairs are replaced, the row's other contacts lie before and behind
them), so the 192 contain a whole aligned block of 64 consecutive contacts: a wave whose 64 lanes all hold that row.  The rows sit at
odd offsets two or more apart, so that [p - 1, p] can be a segment of the orientation support that ends at p.

FAMILIES (`make(cfg, family)`): see FAMILIES below."""
import copy

import numpy as np
import scipy.sparse as sp

N_DENSE, DENSE_LEN = 8, 192
MIN_CONTIG = 200 + N_DENSE
INT_MAX = 2 ** 31 - 1
FAMILIES = {
    "base": "the synth counts on the merged list (the new contacts of the dense rows count 1): the control",
    "narrow_max": "dense rows 2^25 - 1, the rest as base: the largest upload of the `int` form, a full wave sums to 2^31 - 64",
    "wide_min": "dense rows 2^25: the first upload of the `long long` form, the same wave sums to 2^31",
    "int_max": "dense rows and every 7th other contact 2^31 - 1: every sum beyond 2^32",
    "one_wide": "the synth list untouched but for one trans contact of 2^25: one contact picks the form for all",
}
_cache = {}


def _synth(cfg):
    from instagraal_amd import synth

    if cfg not in _cache:
        _cache[cfg] = synth.make_problem(*synth.CONFIGS[cfg])
    return _cache[cfg]


def longest_contig(prob):
    """-> (first sub-fragment, number of sub-fragments) of the longest contig of the fresh genome (its sub-fragments are consecutive
    in the table, and the fresh genome order is the table's)"""
    c = np.asarray(prob.S_o_A_sub_frags["id_c"], np.int64)
    assert np.all(np.diff(c) >= 0)
    ids, first, n = np.unique(c, return_index=True, return_counts=True)
    k = int(np.argmax(n))
    return int(first[k]), int(n[k])


def smallest_config():
    """the smallest of tiny / small / bigctg whose longest contig holds the dense rows"""
    for cfg in ("tiny", "small", "bigctg"):
        if longest_contig(_synth(cfg))[1] >= MIN_CONTIG:
            return cfg
    raise AssertionError("no config has a contig of %d sub-fragments" % MIN_CONTIG)


def dense_rows(prob):
    """the sub-fragments of the eight dense rows, ascending (consecutive sub-fragments of a contig are consecutive positions of the
    fresh genome: sub-fragment i + d lies at the position of i plus d)"""
    first, n = longest_contig(prob)
    assert n >= MIN_CONTIG, (n, MIN_CONTIG)
    step = (n - 2 - DENSE_LEN) // (N_DENSE - 1)
    assert step >= 2
    rows = first + 1 + step * np.arange(N_DENSE, dtype=np.int64)
    assert rows[-1] + DENSE_LEN <= first + n - 1
    return rows


def _rebuild(prob, row, col, cnt):
    M = prob.n_sub_frags
    assert row.size == np.unique(row.astype(np.int64) * M + col).size and np.all(row < col)  # distinct, strict upper triangle
    assert np.all(np.diff(row.astype(np.int64) * M + col) > 0)  # row-major sorted
    assert cnt.min() >= 1 and cnt.max() <= INT_MAX
    out = copy.deepcopy(prob)
    out.coo_row, out.coo_col, out.coo_cnt = row.astype(np.int32), col.astype(np.int32), cnt.astype(np.int32)
    out.n_contacts = int(row.size)
    out.sub_csr = sp.csr_matrix((out.coo_cnt, (out.coo_row, out.coo_col)), shape=(M, M), dtype=np.int32)
    out.sub_csr.sort_indices()
    return out


def make(cfg, family):
    """a deep copy of the synth problem ``cfg`` with coo_row / coo_col / coo_cnt and sub_csr rebuilt under ``family``"""
    assert family in FAMILIES, family
    prob = _synth(cfg)
    M = prob.n_sub_frags
    key = prob.coo_row.astype(np.int64) * M + prob.coo_col
    cnt = prob.coo_cnt.astype(np.int64)
    if family == "one_wide":
        c_of = np.asarray(prob.S_o_A_sub_frags["id_c"])
        trans = np.nonzero(c_of[key // M] != c_of[key % M])[0]
        cnt = cnt.copy()
        cnt[trans[trans.size // 2]] = 2 ** 25
        return _rebuild(prob, key // M, key % M, cnt)
    rows = dense_rows(prob)
    dkey = (rows[:, None] * M + rows[:, None] + 1 + np.arange(DENSE_LEN, dtype=np.int64)[None, :]).ravel()
    allk = np.union1d(key, dkey)
    dense = np.isin(allk, dkey)
    out = np.ones(allk.size, np.int64)
    out[np.searchsorted(allk, key)] = cnt  # base: the synth counts, 1 for the contacts only the dense rows have
    if family == "narrow_max":
        out[dense] = 2 ** 25 - 1
    elif family == "wide_min":
        out[dense] = 2 ** 25
    elif family == "int_max":
        out[dense] = INT_MAX
        other = np.nonzero(~dense)[0]
        out[other[::7]] = INT_MAX
    return _rebuild(prob, allk // M, allk % M, out)


def with_dense_count(prob, count):
    """``prob`` (made by ``make`` with dense rows) with the dense rows' counts replaced by ``count``"""
    M = prob.n_sub_frags
    rows = dense_rows(prob)
    r, c = prob.coo_row.astype(np.int64), prob.coo_col.astype(np.int64)
    dense = np.isin(r, rows) & (c - r >= 1) & (c - r <= DENSE_LEN)
    assert int(dense.sum()) == N_DENSE * DENSE_LEN
    cnt = prob.coo_cnt.astype(np.int64)
    cnt[dense] = int(count)
    return _rebuild(prob, r, c, cnt)


def wave_stats(dest, cnt):
    """``dest``: one destination per contact in list order (negative: none); the lanes of a wave hold an aligned block of 64
    consecutive contacts.  -> (the longest run of equal non-negative destinations inside one block, the largest sum of the counts
    of such a run -- a Python int)"""
    dest, cnt = np.asarray(dest, np.int64), np.asarray(cnt, np.int64)
    n = dest.size
    if n == 0:
        return 0, 0
    k = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = (dest[1:] != dest[:-1]) | (k[1:] % 64 == 0)
    run = np.cumsum(head) - 1
    ok = dest >= 0
    length = np.bincount(run[ok], minlength=run[-1] + 1)
    hi, lo = np.bincount(run[ok], weights=(cnt[ok] >> 16).astype(np.float64)), np.bincount(run[ok], weights=(cnt[ok] & 0xFFFF).astype(np.float64))
    sums = [(int(h) << 16) + int(l) for h, l in zip(hi.tolist(), lo.tolist())] or [0]  # (at most 64 terms below 2^16 each: exact)
    return int(length.max()) if length.size else 0, max(sums)


def fresh_order(prob):
    """the order of the fresh genome (what ``ig_contact_map_order`` returns before any move): every contig placed, the contigs in
    ascending canonical id -- enumerated by their first bin, stable sort by length in bins descending, id = (n - 1) - rank (the
    reference's modify_gl_cuda_buffer, CL:2715-2881) --, each contig's sub-fragments in table order -> the sub-fragment at every position"""
    S = prob.S_o_A_frags
    heads = np.nonzero(np.asarray(S["pos"]) == 0)[0]
    by_length = heads[np.argsort(-np.asarray(S["l_cont"], np.int64)[heads], kind="stable")]
    sub_c = np.asarray(prob.S_o_A_sub_frags["id_c"], np.int64)
    return np.concatenate([np.nonzero(sub_c == S["id_c"][h])[0] for h in by_length[::-1]]).astype(np.int64)


def fresh_position(prob):
    """-> (position [M] of every sub-fragment in ``fresh_order``, contig [M])"""
    order = fresh_order(prob)
    position = np.full(prob.n_sub_frags, -1, np.int64)
    position[order] = np.arange(order.size)
    assert np.all(position >= 0)
    return position, np.asarray(prob.S_o_A_sub_frags["id_c"], np.int64)


def map_keys(prob, max_side):
    """the contact map's key of every contact on the fresh genome: pixel pair min * side + max (csrc/ig_kernels_map.cuh)"""
    from instagraal_amd.contact_map import binning

    pos, _ = fresh_position(prob)
    b, side = binning(pos.size, max_side)
    pi, pj = pos[prob.coo_row] // b, pos[prob.coo_col] // b
    return np.minimum(pi, pj) * side + np.maximum(pi, pj)


def junction_plus_words(prob, window):
    """the junction profile's + word of every contact on the fresh genome (no rings): pa + 1 for an in-window cis contact, else -1"""
    pos, contig = fresh_position(prob)
    pa, pb = pos[prob.coo_row], pos[prob.coo_col]
    ok = (contig[prob.coo_row] == contig[prob.coo_col]) & (pb - pa <= window)
    return np.where(ok, pa + 1, -1)


def dense_segments(prob):
    """the custom segment list of the orientation support, in positions of the fresh genome: [p - 1, p] for every dense row p, so that the 192 columns of the row lie
    in the segment's right flank and the row's end in its right arm (quadrant RR) at windows >= 192"""
    rows = fresh_position(prob)[0][dense_rows(prob)]
    assert np.all(np.diff(rows) >= 2)
    return rows - 1, rows.copy()


def orientation_row_words(prob, first, last, window):
    """the orientation support's word of the ROW end of every contact on the fresh genome (no rings), where the row is the lower
    position: 4 * segment + quadrant (LR = 1, RR = 3), -1: not counted (csrc/ig_kernels_orient.cuh, the lower end)"""
    pos, contig = fresh_position(prob)
    first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
    seg = np.full(pos.size, -1, np.int64)
    for k, (f, l) in enumerate(zip(first.tolist(), last.tolist())):
        seg[f:l + 1] = k
    arm = np.minimum((last - first + 1) // 2, window)
    pa, pb = pos[prob.coo_row], pos[prob.coo_col]
    sa, sb = seg[pa], seg[pb]
    s = np.maximum(sa, 0)
    ok = (contig[prob.coo_row] == contig[prob.coo_col]) & (sa >= 0) & (sa != sb) & (arm[s] > 0) & (pb - last[s] <= window)
    word = np.where(pa < first[s] + arm[s], 4 * s + 1, np.where(pa > last[s] - arm[s], 4 * s + 3, -1))
    return np.where(ok, word, -1)


def map_host(position, row, col, cnt, max_side):
    """the contact map's rule in numpy integers (no float bincount): every contact with both ends placed adds its count to the pixel
    pair of its ends and to the mirrored one (inside one pixel: twice) -> (image int64 [side, side], bin)"""
    from instagraal_amd.contact_map import binning, pixel_of

    position = np.asarray(position, np.int64)
    b, side = binning(int((position >= 0).sum()), max_side)
    pa, pb = position[np.asarray(row, np.int64)], position[np.asarray(col, np.int64)]
    ok = (pa >= 0) & (pb >= 0)
    pi, pj, c = pixel_of(pa[ok], b), pixel_of(pb[ok], b), np.asarray(cnt, np.int64)[ok]
    image = np.zeros(side * side, np.int64)
    np.add.at(image, pi * side + pj, c)
    np.add.at(image, pj * side + pi, c)
    return image.reshape(side, side), b
