"""Host helpers of the contact map of the current genome (``sampler.display_current_matrix``, CL:2555-2605): the order of the
genome as the reference builds it, and the binning rule of the device image (``ig_contact_map``).  Pure numpy, no GPU."""
from __future__ import annotations

import numpy as np


def genome_order(pos, id_c, activ, id_d, ori, np_sub_frags_id):
    """CL:2556-2585 on downloaded state arrays -> (full_order, dict_contig, full_order_high).

    Contigs in ascending id (``np.unique``); a contig whose bins are not all active is left out of the two orders and keeps an empty
    list in ``dict_contig`` (CL:2568-2571); inside a contig the bins by ``pos``; ``full_order_high``: per bin its sub-fragment ids
    (``np_sub_frags_id`` x, y, z, of which w are in use) in table order, reversed where ``ori == -1`` (CL:2576-2585)."""
    pos, id_c, activ, id_d, ori = (np.asarray(a) for a in (pos, id_c, activ, id_d, ori))
    sub_ids = np.stack([np_sub_frags_id["x"], np_sub_frags_id["y"], np_sub_frags_id["z"]], axis=1).astype(np.int64)
    n_sub = np.asarray(np_sub_frags_id["w"]).astype(np.int64)
    by = np.lexsort((pos, id_c))  # contig by contig, each in genome order
    keys, starts = np.unique(id_c[by], return_index=True)
    ends = np.append(starts[1:], by.size)
    dict_contig, bins = {}, []
    for k, a, b in zip(keys, starts, ends):
        idx = by[a:b]
        if np.all(activ[idx] == 1):
            ordered = id_d[idx]
            dict_contig[k] = ordered.tolist()
            bins.append(ordered)
        else:
            dict_contig[k] = []
    full = np.concatenate(bins).astype(np.int64) if bins else np.zeros(0, np.int64)
    # sub-fragment j of bin i in genome direction: table index j, or w - 1 - j on the reverse strand
    w = n_sub[full]
    first = np.cumsum(w) - w
    bin_of = np.repeat(np.arange(full.size), w)
    j = np.arange(int(w.sum())) - first[bin_of]
    rev = ori[full][bin_of] == -1
    high = sub_ids[full[bin_of], np.where(rev, w[bin_of] - 1 - j, j)]
    return full.tolist(), dict_contig, high.tolist()


def binning(n_placed, max_side):
    """the image of ``n_placed`` positions under ``max_side``: ``bin = max(1, ceil(T / max_side))`` positions per pixel,
    ``side = ceil(T / bin)`` pixels -> (bin, side)"""
    T, m = int(n_placed), int(max_side)
    if m < 1:
        raise ValueError("max_side must be >= 1")
    b = max(1, -(-T // m))
    return b, -(-T // b)


def pixel_of(position, bin):  # noqa: A002 - the rule's own word
    """pixel of a position (or an array of them) in the order"""
    return np.asarray(position) // int(bin)
