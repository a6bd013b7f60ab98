"""The expected contact map of the current genome: for every pixel of the contact map's image what the model in use predicts of
the sub-fragment pairs that fall into it, and the residuals of the observed image against it.  A misplaced or inverted block shows
as a pixel off the diagonal with far more contacts than P(s) allows at that separation, and as a band near the diagonal with far
fewer.  This module is the single definition of the rule (pure numpy, no GPU, no matplotlib); the device passes
(``ig_expected_map``, csrc/ig_kernels_emap.cuh) reproduce the three images entry for entry.

The rule.  The POSITIONS are the contact map's: the sub-fragments of the placed contigs (every bin of the contig active) in genome
order, 0 .. T - 1; ``bin, side = contact_map.binning(T, max_side)``, the pixel of position r is ``r // bin``, ``n_a`` the number of
positions in pixel a (the last pixel may hold fewer).  Every unordered pair {i, k}, i < k, of positions has one class: LINEAR CIS
(same contig, not a ring: ``stot == 0``), RING (same contig, a ring) or TRANS (different contigs).  Every image is int64
[side, side], symmetric, in ``ig_contact_map``'s convention: a pair with its ends in the pixels a != b adds to [a][b] and to [b][a],
a pair inside one pixel adds twice to [a][a] -- so the image at ``bin = B`` is the B x B block sum of the image at ``bin = 1``,
whose diagonal is zero.

* ``cis_pairs``: the number of linear cis pairs.
* ``cis_q``: over the same pairs the sum of the model's value at ``s = fabsf(dist_i - dist_k)`` (f32: what the exact cis term feeds
  the model), quantised to a multiple of 2^-32 (round half even) and added as a 64-bit integer.
* ``ring_pairs``: the number of ring pairs.  A pair on a ring has two separations (the distance law and the junction profile leave
  rings out for the same reason): no model value, the pixels are masked in the residuals.

``compose`` adds what needs no device: ``total[a][b] = n_a n_b`` (``n_a (n_a - 1)`` on the diagonal),
``trans_pairs = total - cis_pairs - ring_pairs``, ``expected_q = cis_q + trans_pairs * q_trans`` with ``q_trans`` the quantised
trans level ``v_inter``, and ``expected = expected_q / 2^32`` (f64).

The scalars (int64): ``n_placed``, ``linear_cis_pairs``, ``ring_pairs_total``, ``max_q`` (the largest |quantised value| seen),
``tiles_evaluated``, ``tiles_constant`` (how the device's tile form got there; 0 under its row form and here).  By construction:

    cis_pairs.sum() == 2 * linear_cis_pairs          ring_pairs.sum() == 2 * ring_pairs_total
    total.sum() == T (T - 1)                         linear_cis_pairs + ring_pairs_total == placed_pairs of the distance law
    at bin = 1: expected_q[j] of the junction profile under window w == sum of cis_q[i][k] over i < j <= k, k - i <= w
"""
from __future__ import annotations

import numpy as np

from .contact_map import binning
from .junction_profile import contig_runs

# the order of ig_expected_map's scalars[8] (the last two words are not used)
SCALARS = ("n_placed", "linear_cis_pairs", "ring_pairs_total", "max_q", "tiles_evaluated", "tiles_constant")
IMAGES = ("cis_q", "cis_pairs", "ring_pairs")
Q_ONE = 4294967296.0  # 2^32: one unit of the model's value in cis_q / expected_q
Q_CLAMP = 1048576.0   # ig_quantize clamps to +- 2^20
CLIP_LOG2 = 3.0       # display_residual_matrix clips log2(O / E) here
FORMS = ("default", "rows", "tiles", "tiles_plain")  # ig_debug_expected_map_form
STRONGEST_COLUMNS = ("pixel_a", "pixel_b", "first_a", "last_a", "first_b", "last_b", "contig_a", "contig_b", "pairs", "observed",
                     "expected", "z")
STRONGEST_DTYPE = np.dtype([(k, np.float64 if k in ("expected", "z") else np.int64) for k in STRONGEST_COLUMNS])


def quantize(value):
    """ig_quantize of a scalar: nan -> 0, clamped to +- 2^20, times 2^32, rounded half even -> int"""
    t = float(value)
    if t != t:
        return 0
    return int(np.rint(min(max(t, -Q_CLAMP), Q_CLAMP) * Q_ONE))


def pixel_sizes(n_placed, bin, side):  # noqa: A002 - the rule's own word
    """n_a: positions per pixel -> int64 [side]"""
    n = np.full(int(side), int(bin), np.int64)
    if side:
        n[-1] = int(n_placed) - (int(side) - 1) * int(bin)
    return n


def _add_exact(flat, keys, values):
    """flat[keys] += values with repeated keys, exactly: int64 values go through float64 bincounts in three limbs of 21 bits (a
    limb's sum stays below 2^53 for up to 2^32 entries per key); ``values`` None: every entry counts 1"""
    if values is None:
        flat += np.bincount(keys, minlength=flat.size)
        return
    v = np.asarray(values, np.int64)
    for shift in (0, 21):
        flat += np.bincount(keys, weights=((v >> shift) & 0x1FFFFF).astype(np.float64), minlength=flat.size).astype(np.int64) << shift
    flat += np.bincount(keys, weights=(v >> 42).astype(np.float64), minlength=flat.size).astype(np.int64) << 42  # (the signed top)


def _add_pairs(image, pa, pb, value):
    """every pair (pa <= pb) adds ``value`` at [a][b] and at [b][a] (a == b: twice into that pixel)"""
    side = image.shape[0]
    upper = np.zeros(side * side, np.int64)
    _add_exact(upper, pa * side + pb, value)
    upper = upper.reshape(side, side)
    image += upper + upper.T


def expected_host(ds, stot, contig, position, max_side, model_q):
    """The rule by enumeration, contig by contig and separation by separation, with no shortcut: every pair of a contig is listed
    with its two pixels and, on a linear contig, the model's value at its own separation; a contig's pairs are then added up.

    ds, stot: f32 [M]; contig: int [M] (any labelling); position: int [M], the position in the genome order, -1 where not placed;
    ``model_q``: callable, separations (f32 array) -> the model's quantised values (int64).  -> dict: side, bin, the int64
    [side, side] images named in IMAGES and the int64 scalars named in SCALARS."""
    ds = np.asarray(ds, np.float32)
    ring = np.asarray(stot, np.float32) != 0
    members, start, length = contig_runs(contig, position)
    T = int(members.size)
    b, side = binning(T, max_side)
    out = dict(side=side, bin=b, n_placed=T, tiles_evaluated=0, tiles_constant=0)
    img = {k: np.zeros((side, side), np.int64) for k in IMAGES}
    linear = rings = max_q = 0
    for st, n in zip(start.tolist(), length.tolist()):
        if n < 2:
            continue
        on_ring = bool(ring[members[st]])
        d_c = ds[members[st:st + n]]
        i = np.arange(st, st + n, dtype=np.int64)
        pa, pb, q = [], [], []
        for d in range(1, n):  # the pairs (i, i + d)
            pa.append(i[:n - d] // b)
            pb.append(i[d:] // b)
            if not on_ring:
                s = np.abs(d_c[:n - d] - d_c[d:])
                assert s.dtype == np.float32
                q.append(np.asarray(model_q(s), np.int64))
        pa, pb = np.concatenate(pa), np.concatenate(pb)
        if on_ring:
            _add_pairs(img["ring_pairs"], pa, pb, None)
            rings += pa.size
            continue
        q = np.concatenate(q)
        _add_pairs(img["cis_pairs"], pa, pb, None)
        _add_pairs(img["cis_q"], pa, pb, q)
        linear += pa.size
        max_q = max(max_q, int(np.abs(q).max()))
    out.update(img)
    out.update(linear_cis_pairs=linear, ring_pairs_total=rings, max_q=max_q)
    return out


def tile_census(ds, stot, contig, position, max_side, d_max):
    """The work list of the device's tile form, stated on the host: pixel a lists the pixels b from a up to the pixel of the last
    position of the contig that a's last position lies in.  A listed tile off the diagonal whose contig is linear is CONSTANT where
    its smallest separation, fabsf(ds[first k] - ds[last i]) in f32, is >= ``d_max`` (the device writes pairs x one value there);
    every other listed tile is EVALUATED.  Of the evaluated linear tiles off the diagonal, ``below`` have their largest separation
    under d_max and ``straddling`` do not.  -> dict of counts: listed, diagonal, constant, evaluated, ring, below, straddling, and
    max_contigs_per_pixel"""
    ds = np.asarray(ds, np.float32)
    members, start, length = contig_runs(contig, position)
    T = int(members.size)
    b, side = binning(T, max_side)
    out = dict(listed=0, diagonal=0, constant=0, evaluated=0, ring=0, below=0, straddling=0, max_contigs_per_pixel=0)
    if T == 0:
        return out
    d = ds[members]
    on_ring = (np.asarray(stot, np.float32) != 0)[members]
    c_start = np.repeat(start, length)
    c_end = c_start + np.repeat(length, length)
    first = np.zeros(T, np.int64)
    first[start] = 1
    per_pixel = np.add.reduceat(first, np.arange(0, T, b)) + (first[np.arange(0, T, b)] == 0)
    out["max_contigs_per_pixel"] = int(per_pixel.max())
    d_max = np.float32(d_max)
    for a in range(side):
        la = min((a + 1) * b, T) - 1
        end = int(c_end[la])
        for bb in range(a, (end - 1) // b + 1):
            out["listed"] += 1
            if bb == a:
                out["diagonal"] += 1
                out["evaluated"] += 1
                continue
            if on_ring[la]:
                out["ring"] += 1
                out["evaluated"] += 1
                continue
            k0 = bb * b
            if np.abs(d[k0] - d[la]) >= d_max:
                out["constant"] += 1
                continue
            out["evaluated"] += 1
            i_first, k_last = max(a * b, int(c_start[la])), min((bb + 1) * b, T, end) - 1
            out["below" if np.abs(d[k_last] - d[i_first]) < d_max else "straddling"] += 1
    return out


def block_sum(image, bin, side):  # noqa: A002
    """the image at ``bin`` positions per pixel from the one at one position per pixel"""
    image = np.asarray(image, np.int64)
    T = image.shape[0]
    edges = np.arange(0, max(T, 1), int(bin))[:int(side)]
    if T == 0:
        return np.zeros((0, 0), np.int64)
    return np.add.reduceat(np.add.reduceat(image, edges, axis=0), edges, axis=1)


def compose(result, q_trans):
    """adds ``total``, ``trans_pairs``, ``expected_q`` (int64 images) and ``expected`` (f64) to a device or host result -> the same
    dict.  ``q_trans``: the quantised trans level, ``quantize(v_inter)``."""
    n = pixel_sizes(result["n_placed"], result["bin"], result["side"])
    total = np.outer(n, n)
    if n.size:
        total[np.diag_indices(n.size)] = n * (n - 1)
    trans = total - np.asarray(result["cis_pairs"], np.int64) - np.asarray(result["ring_pairs"], np.int64)
    if (trans < 0).any():
        raise ValueError("expected map: a pixel holds more cis and ring pairs than pairs")
    q_trans = int(q_trans)
    b = max(int(result["bin"]), 1)
    if 2 * b * b * max(abs(q_trans), int(result["max_q"])) >= 1 << 62:
        raise ValueError("expected map: model value too large for this pixel size")
    result["total"] = total
    result["trans_pairs"] = trans
    result["q_trans"] = q_trans
    result["expected_q"] = np.asarray(result["cis_q"], np.int64) + trans * np.int64(q_trans)
    result["expected"] = result["expected_q"].astype(np.float64) / Q_ONE
    return result


def residuals(observed, result):
    """``observed``: the device's image (``Context.contact_map(max_side)``: without the input matrix's diagonal -- self-contacts
    have no model term) under the same ``max_side`` as the composed ``result`` -> dict: observed, expected, ``log2_ratio`` =
    log2(O / E) (-inf where O == 0) and ``z`` = (O - E) / sqrt(E), both nan where E == 0 or the pixel holds a ring pair; ``mask``:
    where they are nan; plus side, bin, n_placed, total"""
    obs = np.asarray(observed, np.float64)
    ex = np.asarray(result["expected"], np.float64)
    if obs.shape != ex.shape:
        raise ValueError("expected map: the observed image is %r, the expected one %r" % (obs.shape, ex.shape))
    mask = (ex == 0) | (np.asarray(result["ring_pairs"]) != 0)
    safe = np.where(mask, 1.0, ex)
    with np.errstate(divide="ignore"):
        lr = np.log2(obs / safe)
    z = (obs - safe) / np.sqrt(safe)
    lr[mask] = np.nan
    z[mask] = np.nan
    return dict(observed=np.asarray(observed, np.int64), expected=ex, log2_ratio=lr, z=z, mask=mask, side=result["side"], bin=result["bin"],
                n_placed=result["n_placed"], total=np.asarray(result["total"], np.int64))


def default_min_pairs(bin):  # noqa: A002
    """half of a full pixel's pairs, bin^2: below that a pixel sits at the ragged end of the image"""
    return (int(bin) * int(bin) + 1) // 2


def strongest(res, n=20, min_pairs=None, contig_of_position=None):
    """the ``n`` pixels a < b of a ``residuals`` result with the largest z among those with ``total >= min_pairs`` (default: half of
    bin^2) and a z, as a STRONGEST_DTYPE array: both pixels, the range of positions of each, the contig at their first positions
    (``contig_of_position``: the contig id at every position; -1 without it), the pairs, O, E and z.  The sort is stable."""
    side, b, T = int(res["side"]), int(res["bin"]), int(res["n_placed"])
    mp = default_min_pairs(b) if min_pairs is None else int(min_pairs)
    a, c = np.triu_indices(side, k=1)
    z = np.asarray(res["z"])[a, c]
    keep = np.isfinite(z) & (np.asarray(res["total"])[a, c] >= mp)
    a, c, z = a[keep], c[keep], z[keep]
    top = np.argsort(-z, kind="stable")[:max(int(n), 0)]
    a, c = a[top].astype(np.int64), c[top].astype(np.int64)
    t = np.zeros(top.size, STRONGEST_DTYPE)
    t["pixel_a"], t["pixel_b"] = a, c
    t["first_a"], t["last_a"] = a * b, np.minimum((a + 1) * b, T) - 1
    t["first_b"], t["last_b"] = c * b, np.minimum((c + 1) * b, T) - 1
    cp = None if contig_of_position is None else np.asarray(contig_of_position, np.int64)
    t["contig_a"] = -1 if cp is None else cp[t["first_a"]]
    t["contig_b"] = -1 if cp is None else cp[t["first_b"]]
    t["pairs"] = np.asarray(res["total"])[a, c]
    t["observed"] = np.asarray(res["observed"])[a, c]
    t["expected"] = np.asarray(res["expected"])[a, c]
    t["z"] = z[top]
    return t


def write_residuals(path, table, result):
    """one line per listed pixel (``strongest``): the columns of STRONGEST_COLUMNS; then the image's size and the scalars"""
    with open(path, "w") as f:
        f.write("# " + " ".join(STRONGEST_COLUMNS) + "\n")
        for r in table:
            f.write("%d %d %d %d %d %d %d %d %d %d %.9g %.9g\n" % tuple(r[k] for k in STRONGEST_COLUMNS))
        f.write("# side=%d bin=%d " % (result["side"], result["bin"]) + " ".join("%s=%d" % (k, result[k]) for k in SCALARS) + "\n")
