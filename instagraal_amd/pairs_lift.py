"""Read pairs lifted onto the current genome: every Hi-C read pair, aligned to the input contigs, re-expressed in the coordinates of
the scaffolds as they stand (those of ``genome.fasta`` and of ``assembly_contacts.bins_table``), then binned at any resolution and
counted by distance and strand combination -- bp-resolution maps and P(s) of the assembly, which the sub-fragment contact matrix
cannot give.  This module is the single definition of the rule (pure numpy, no GPU); the device passes (``ig_pairs_lift``,
``ig_pairs_pixels_build``, ``ig_pairs_law``, csrc/ig_kernels_pairs.cuh) reproduce its arrays byte for byte.  The reference does the
same one line and one dictionary lookup at a time (post.py: ``_pos_to_new_coords``, ``_pairs_to_lifted_pixels``,
``_pairs_to_fixed_bin_pixels``, ``_compute_ps``).

The rule.  The SOURCE TABLE has one interval per sub-fragment: ``[src_start, src_end)`` on input contig ``src_contig``, 0-based and
half-open, sorted by (src_contig, src_start), with ``src_rowptr`` over the contig ids.  From the genome order every interval also
has the rank of its scaffold among the placed ones (-1: its sub-fragment is not placed), ``new_start`` inside the scaffold,
``reversed`` (the parent bin's ori == -1) and its position in the order.

An END (contig c, 1-based position p): ``pos0 = p - 1``; ``i = searchsorted(starts of c, pos0, "right") - 1``; the end MISSES if c is
unknown, i < 0 or pos0 >= end[i]; else ``off = pos0 - start[i]`` and ``new0 = new_start[i] + off``, or
``new_start[i] + (len - 1 - off)`` where the interval is reversed.  A PAIR has one status: kept; end 1 not covered; end 2 not covered
(end 1 is); an end on an unplaced sub-fragment (both covered).  Nothing is dropped silently: the scalars count every status.

Pixels: the unit of an end is its position (``"sub"``), the rank of its parent bin among the placed bins (``"bin"``: the rows of
info_frags.txt), ``first_unit[scaffold] + new0 // binsize`` (a bin size in bp: the bins of ``zoom_levels.binnify``; a pair counts
where it falls, not at a fragment's midpoint) or its scaffold (``"scaffold"``).  Keys are (min, max), equal keys are summed into
int64, the diagonal is kept; the result is CSR as ``assembly_contacts.lift_host``'s.

The law: over the kept pairs with both ends on one scaffold, ``idx = clip(searchsorted(edges, |pos2 - pos1|, "right") - 1, 0,
n_edges - 2)``, counted per strand combination ``++ +- -+ --``; with ``flip_strands`` an end on a reversed interval has its strand
flipped (the read now lies on the other strand of the scaffold), without it the strands stay as read, as the reference leaves them.

The text side (``read_pairs``, ``write_lifted_pairs``) parses and formats lines in Python and is bound by that; the arrays are the
fast path.  ``read_pairs_device`` is ``read_pairs`` with the parse on the device (the rule: ``pairs_text.py``), asked for by name."""
from __future__ import annotations

import gzip

import numpy as np

from . import assembly_contacts as ac, zoom_levels as zl

STATUS = ("kept", "end1_not_covered", "end2_not_covered", "unplaced")
KEPT, END1_NOT_COVERED, END2_NOT_COVERED, UNPLACED = range(4)
# the order of ig_pairs_lift's scalars[8]
SCALARS = ("pairs_in", "pairs_kept", "end1_not_covered", "end2_not_covered", "unplaced", "pairs_stored", "reserved6", "reserved7")
UNIT_KINDS = ("sub", "bin", "binsize", "scaffold")  # ig_pairs_pixels_build's kind
STRAND_COMBOS = ("++", "+-", "-+", "--")
MAX_BP = (1 << 31) - 1
MAX_EDGES = 512
TABLE_DTYPE = np.dtype([("src_contig", np.int64), ("src_start", np.int64), ("src_end", np.int64), ("scaffold", np.int64), ("new_start", np.int64),
                        ("reversed", np.int8), ("position", np.int64), ("sub", np.int64)])
_BIG = 1 << 32


def source_table(sub_contig, len_bp, order, parent, contig_of_bin, ori_of_bin, start_bp=None, names=None):
    """The intervals the pairs are looked up in.  sub_contig, len_bp: input contig id (>= 0) and length of every sub-fragment;
    start_bp: its 0-based start on that contig, None: the running sum of ``len_bp`` in sub-fragment id order inside each contig;
    order, parent, contig_of_bin, ori_of_bin: as ``assembly_contacts.bins_table``; names: {contig name: id} or a list of names by
    id (optional: what lets ``contig_ids`` map names).  -> dict: ``intervals`` (TABLE_DTYPE, sorted by (src_contig, src_start)),
    ``src_rowptr`` (int64 [max id + 2]), ``scaffold_ids`` (the canonical ids of the placed scaffolds in genome order),
    ``scaffold_len`` (int64), ``bin_unit`` (int64 [T]: the unit of every position at "bin"), ``n_bin_units``, ``n_positions``,
    ``names``.  ValueError: overlapping intervals on one contig, a scaffold or a contig beyond 2^31 - 1 bp."""
    sub_contig, len_bp = np.asarray(sub_contig, np.int64).ravel(), np.asarray(len_bp, np.int64).ravel()
    M = sub_contig.size
    if len_bp.size != M or (M and (sub_contig.min() < 0 or len_bp.min() < 0)):
        raise ValueError("pairs lift: one contig id >= 0 and one length >= 0 per sub-fragment")
    if start_bp is None:
        by = np.argsort(sub_contig, kind="stable")
        run = np.cumsum(len_bp[by]) - len_bp[by]
        c = sub_contig[by]
        head = np.concatenate([[True], c[1:] != c[:-1]]) if M else np.zeros(0, bool)
        base = np.repeat(run[head], np.diff(np.concatenate([np.nonzero(head)[0], [M]]))) if M else run
        start = np.zeros(M, np.int64)
        start[by] = run - base
    else:
        start = np.asarray(start_bp, np.int64).ravel()
        if start.size != M or (M and start.min() < 0):
            raise ValueError("pairs lift: one start >= 0 per sub-fragment")
    order = np.asarray(order, np.int64).ravel()
    t = ac.bins_table(order, parent, contig_of_bin, ori_of_bin, len_bp, "sub")
    k, K = zl.scaffold_units(t)
    ids, sizes = ac.chrom_sizes(t)
    if sizes.size and int(sizes.max()) > MAX_BP:
        raise ValueError("pairs lift: scaffold %s%d is %d bp long, more than 2^31 - 1" % (ac.SCAFFOLD_PREFIX, int(ids[np.argmax(sizes)]), int(sizes.max())))
    iv = np.zeros(M, TABLE_DTYPE)
    iv["src_contig"], iv["src_start"], iv["src_end"], iv["sub"] = sub_contig, start, start + len_bp, np.arange(M)
    iv["scaffold"], iv["position"] = -1, -1
    iv["scaffold"][order], iv["new_start"][order], iv["reversed"][order], iv["position"][order] = k, t["start"], t["ori"] == -1, np.arange(order.size)
    if M and int(iv["src_end"].max()) > MAX_BP:
        raise ValueError("pairs lift: an input contig reaches %d bp, more than 2^31 - 1" % int(iv["src_end"].max()))
    iv = iv[np.lexsort((iv["src_start"], iv["src_contig"]))]
    same = iv["src_contig"][1:] == iv["src_contig"][:-1]
    bad = np.nonzero(same & (iv["src_start"][1:] < iv["src_end"][:-1]))[0]
    if bad.size:
        a, b = iv[bad[0]], iv[bad[0] + 1]
        raise ValueError("pairs lift: overlapping intervals on contig %d: sub-fragment %d [%d, %d) and sub-fragment %d [%d, %d)"
                         % (a["src_contig"], a["sub"], a["src_start"], a["src_end"], b["sub"], b["src_start"], b["src_end"]))
    n_c = int(sub_contig.max()) + 1 if M else 0
    rowptr = np.zeros(n_c + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(iv["src_contig"], minlength=n_c))
    bin_unit = ac.units_along(t["bin"])
    if names is not None and not isinstance(names, dict):
        names = {str(n): i for i, n in enumerate(names)}
    return dict(intervals=iv, src_rowptr=rowptr, scaffold_ids=ids, scaffold_len=sizes.astype(np.int64), bin_unit=bin_unit.astype(np.int64),
                n_bin_units=int(bin_unit[-1]) + 1 if bin_unit.size else 0, n_positions=int(order.size), names=names)


def table_of_state(state17, np_sub_frags_id, parent, sub_contig, len_bp, start_bp=None, names=None):
    """``source_table`` of a downloaded state (17 x N in the order of ``hip_lib.FRAG_FIELDS``), the genome order made on the host
    (``contact_map.genome_order``): what the device session gets from ``sampler.pairs_begin``"""
    from .contact_map import genome_order

    st = np.asarray(state17)
    pos, id_c, ori, activ, id_d = st[0], st[2], st[13], st[15], st[16]
    _, _, high = genome_order(pos, id_c, activ, id_d, ori, np_sub_frags_id)
    return source_table(sub_contig, len_bp, np.asarray(high, np.int64), parent, id_c, ori, start_bp=start_bp, names=names)


def identity_table(scaffold_len, names=None):
    """the table of a genome whose contigs are its scaffolds, each one interval: lifted pairs lift to themselves under it"""
    n = np.asarray(scaffold_len, np.int64).ravel()
    K = n.size
    return source_table(np.arange(K), n, np.arange(K), np.arange(K), np.arange(K), np.ones(K, np.int64), names=names)


def contig_ids(table, contig):
    """ids as they are, names through ``table["names"]`` (an unknown name: -1) -> int64"""
    a = np.asarray(contig)
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    names = table.get("names")
    if names is None:
        raise ValueError("pairs lift: the contigs are given by name and the table has no names")
    return np.array([names.get(str(x), -1) for x in a.ravel()], np.int64).reshape(a.shape)


def _lift_end(table, c, p):
    iv, rowptr = table["intervals"], table["src_rowptr"]
    c, p = np.asarray(c, np.int64).ravel(), np.asarray(p, np.int64).ravel()
    n = c.size
    known = (c >= 0) & (c < rowptr.size - 1)
    cc = np.where(known, c, 0)
    pos0 = p - 1
    out = dict(scaffold=np.full(n, -1, np.int32), pos=np.zeros(n, np.int32), unit=np.full(n, -1, np.int32), rev=np.zeros(n, np.uint8))
    if iv.size == 0 or n == 0:
        return np.zeros(n, bool), out
    key = iv["src_contig"] * _BIG + iv["src_start"]
    i = np.searchsorted(key, cc * _BIG + np.clip(pos0, -1, _BIG - 1), side="right") - 1
    hit = known & (i >= rowptr[cc]) & (i < rowptr[np.minimum(cc + 1, rowptr.size - 1)])
    ii = np.where(hit, i, 0)
    hit &= pos0 < iv["src_end"][ii]
    h = iv[ii]
    off = pos0 - h["src_start"]
    new0 = h["new_start"] + np.where(h["reversed"] != 0, h["src_end"] - h["src_start"] - 1 - off, off)
    ok = hit & (h["scaffold"] >= 0)
    out["scaffold"][ok] = h["scaffold"][ok]
    out["pos"][ok] = new0[ok] + 1
    out["unit"][ok] = h["position"][ok]
    out["rev"][ok] = h["reversed"][ok]
    return hit, out


def lift_host(table, c1, p1, c2, p2):
    """The rule, end by end.  c1, c2: contig ids (``contig_ids``); p1, p2: 1-based positions.  -> dict: ``scaffold1``, ``pos1``
    (1-based; -1 and 0 where the end is not lifted), ``unit1`` (its position in the genome order, -1), ``rev1`` (uint8) and the same
    for end 2, all int32 but the bits; ``status`` (uint8: KEPT, END1_NOT_COVERED, END2_NOT_COVERED, UNPLACED) and the scalars"""
    hit1, e1 = _lift_end(table, c1, p1)
    hit2, e2 = _lift_end(table, c2, p2)
    if hit1.size != hit2.size:
        raise ValueError("pairs lift: the four arrays of the pairs have one length")
    status = np.full(hit1.size, KEPT, np.uint8)
    status[(e1["scaffold"] < 0) | (e2["scaffold"] < 0)] = UNPLACED
    status[~hit2] = END2_NOT_COVERED
    status[~hit1] = END1_NOT_COVERED
    out = dict(scaffold1=e1["scaffold"], pos1=e1["pos"], unit1=e1["unit"], rev1=e1["rev"], scaffold2=e2["scaffold"], pos2=e2["pos"], unit2=e2["unit"],
               rev2=e2["rev"], status=status)
    counts = np.bincount(status, minlength=4)
    out.update(pairs_in=int(status.size), pairs_kept=int(counts[KEPT]), end1_not_covered=int(counts[END1_NOT_COVERED]),
               end2_not_covered=int(counts[END2_NOT_COVERED]), unplaced=int(counts[UNPLACED]))
    return out


def concat_lifted(parts):
    """the lifted chunks of one input, in order, as one"""
    parts = list(parts)
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("scaffold1", "pos1", "unit1", "rev1", "scaffold2", "pos2", "unit2", "rev2", "status")}
    out.update((k, sum(int(p[k]) for p in parts)) for k in SCALARS[:5])
    return out


def check_units(table, units):
    """-> (kind, binsize, first_unit or None, n_units) of ``units``: "sub", "bin", "scaffold" or a bin size in bp"""
    K = table["scaffold_len"].size
    if isinstance(units, str):
        if units not in ("sub", "bin", "scaffold"):
            raise ValueError("pairs lift: units is \"sub\", \"bin\", \"scaffold\" or a bin size in bp (got %r)" % (units,))
        return units, 0, None, {"sub": table["n_positions"], "bin": table["n_bin_units"], "scaffold": K}[units]
    B = zl.check_binsize(units)
    if B > MAX_BP:
        raise ValueError("pairs lift: a bin size is at most 2^31 - 1 bp (got %d)" % B)
    _, off = zl.bins_per_scaffold((table["scaffold_ids"], table["scaffold_len"]), B)
    return "binsize", B, off[:-1].astype(np.int64), int(off[-1])


def units_of(lifted, table, units):
    """the two units of every kept pair -> (a, b, n_units)"""
    kind, B, first, U = check_units(table, units)
    keep = lifted["status"] == KEPT
    s1, s2 = lifted["scaffold1"][keep].astype(np.int64), lifted["scaffold2"][keep].astype(np.int64)
    if kind == "sub":
        return lifted["unit1"][keep].astype(np.int64), lifted["unit2"][keep].astype(np.int64), U
    if kind == "bin":
        return table["bin_unit"][lifted["unit1"][keep]], table["bin_unit"][lifted["unit2"][keep]], U
    if kind == "scaffold":
        return s1, s2, U
    return first[s1] + (lifted["pos1"][keep].astype(np.int64) - 1) // B, first[s2] + (lifted["pos2"][keep].astype(np.int64) - 1) // B, U


def pixels_host(lifted, table, units):
    """The pixels of the kept pairs -> dict: rowptr (int64 [n_units + 1]), col (int32, strictly ascending inside a row), count
    (int64), n_units, entries_in (the kept pairs) and entries_out"""
    a, b, U = units_of(lifted, table, units)
    rowptr, col, count = zl._csr(np.minimum(a, b), np.maximum(a, b), np.ones(a.size, np.int64), U)
    return dict(rowptr=rowptr, col=col, count=count, n_units=U, entries_in=int(a.size), entries_out=int(col.size))


def check_edges(edges_bp):
    e = np.asarray(edges_bp)
    if e.ndim != 1 or not 2 <= e.size <= MAX_EDGES or e.dtype.kind not in "iu":
        raise ValueError("pairs lift: 2 <= len(edges) <= %d whole numbers of bp" % MAX_EDGES)
    e = e.astype(np.int64)
    if e.min() < 0 or np.any(np.diff(e) < 0):
        raise ValueError("pairs lift: the edges are >= 0 and ascending")
    return np.ascontiguousarray(e)


def default_edges_bp(mean_kb, longest_kb):
    """the distance law's default edges (``distance_law.default_edges``), in whole bp, distinct, at most MAX_EDGES"""
    from . import distance_law as dlaw

    for per_octave in (8, 4, 2, 1):
        e = np.unique(np.round(np.asarray(dlaw.default_edges(mean_kb, longest_kb, per_octave), np.float64) * 1000.0).astype(np.int64))
        if e.size <= MAX_EDGES:
            break
    return e[:MAX_EDGES]


def strand_codes(strand1, strand2):
    """'+' / '-' (or 0 / 1) per end -> uint8 codes: bit 0 set where end 1 is on '-', bit 1 where end 2 is"""
    def minus(s):
        s = np.asarray(s)
        return (s == "-") if s.dtype.kind in "US" else (s.astype(np.int64) != 0)
    return (minus(strand1).astype(np.uint8) | (minus(strand2).astype(np.uint8) << 1)).astype(np.uint8)


def law_host(lifted, strands, edges_bp, flip_strands=True):
    """-> int64 [4][n_edges - 1]: the kept pairs with both ends on one scaffold by strand combination (STRAND_COMBOS) and distance
    bin.  strands: ``strand_codes`` per pair, None: all '+'"""
    e = check_edges(edges_bp)
    keep = (lifted["status"] == KEPT) & (lifted["scaffold1"] == lifted["scaffold2"])
    code = np.zeros(keep.size, np.uint8) if strands is None else np.asarray(strands, np.uint8).ravel()
    if code.size != keep.size:
        raise ValueError("pairs lift: one strand code per pair")
    s1, s2 = (code & 1)[keep], ((code >> 1) & 1)[keep]
    if flip_strands:
        s1, s2 = s1 ^ lifted["rev1"][keep], s2 ^ lifted["rev2"][keep]
    d = np.abs(lifted["pos2"][keep].astype(np.int64) - lifted["pos1"][keep].astype(np.int64))
    idx = np.clip(np.searchsorted(e, d, side="right") - 1, 0, e.size - 2)
    counts = np.zeros((4, e.size - 1), np.int64)
    np.add.at(counts, (s1.astype(np.int64) * 2 + s2, idx), 1)
    return counts


def normalise(counts, edges_bp, widths=None):
    """the reference's ``norm_p``: counts over the combination's total, over the bin width (``widths``: given, else the edges'
    differences) -> f64 [4][n_edges - 1], nan where a combination has no pair"""
    counts = np.asarray(counts, np.int64)
    w = np.diff(np.asarray(edges_bp, np.int64)).astype(np.float64) if widths is None else np.asarray(widths, np.float64)
    tot = counts.sum(axis=1, keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return counts / tot / w


def write_law(path, counts, edges_bp):
    """one line per bin: edge_lo edge_hi and the four counts"""
    e = np.asarray(edges_bp, np.int64)
    with open(path, "w") as f:
        f.write("# edge_lo_bp edge_hi_bp " + " ".join(STRAND_COMBOS) + "\n")
        for b in range(e.size - 1):
            f.write("%d %d %d %d %d %d\n" % ((e[b], e[b + 1]) + tuple(int(counts[k][b]) for k in range(4))))


# ---------------------------------------------------------------- the text side (host-bound)
DEFAULT_COLUMNS = ("readID", "chr1", "pos1", "chr2", "pos2", "strand1", "strand2")
DEFAULT_CHUNK_PAIRS = 1 << 20


def _opener(path):
    return gzip.open if str(path).endswith((".gz", ".bgz")) else open


def _columns(line, cols):
    """the column indices behind a ``#columns:`` line: chr1, pos1, chr2, pos2 change together (or not at all), the strands likewise"""
    names = line.strip().split()[1:]
    try:
        cols = [names.index("chr1"), names.index("pos1"), names.index("chr2"), names.index("pos2")] + cols[4:]
    except ValueError:
        return cols
    try:
        cols = cols[:4] + [names.index("strand1"), names.index("strand2")]
    except ValueError:
        pass
    return cols


def _parse(parts, cols, names):
    """-> (c1, p1, c2, p2, strand code) of a data line's fields, None where the line is malformed (as the reference: a missing
    field or a position that is no integer); an unknown contig name is -1; a missing strand column is '+'"""
    try:
        n1, p1, n2, p2 = parts[cols[0]], int(parts[cols[1]]), parts[cols[2]], int(parts[cols[3]])
    except (IndexError, ValueError):
        return None
    s = 0
    if cols[4] < len(parts) and parts[cols[4]] == "-":
        s |= 1
    if cols[5] < len(parts) and parts[cols[5]] == "-":
        s |= 2
    return names.get(n1, -1), p1, names.get(n2, -1), p2, s


def read_pairs(path, names, chunk_pairs=DEFAULT_CHUNK_PAIRS, with_lines=False):
    """A 4DN pairs file (``.gz`` / ``.bgz`` by extension) chunk by chunk.  names: {contig name: id}.  Yields dicts: ``c1``, ``p1``,
    ``c2``, ``p2`` (int64), ``strands`` (uint8 codes), ``malformed`` (data lines skipped so far, as the reference skips them), and
    with ``with_lines`` the fields of every parsed line and the column indices.  ``#columns:`` is honoured wherever it stands."""
    chunk_pairs = max(int(chunk_pairs), 1)
    cols = [1, 2, 3, 4, 5, 6]
    rows, lines, malformed = [], [], 0

    def flush():
        a = np.array(rows, np.int64).reshape(-1, 5)
        out = dict(c1=a[:, 0].copy(), p1=a[:, 1].copy(), c2=a[:, 2].copy(), p2=a[:, 3].copy(), strands=a[:, 4].astype(np.uint8), malformed=malformed)
        if with_lines:
            out.update(lines=list(lines), columns=list(cols))
        rows.clear()
        lines.clear()
        return out

    with _opener(path)(path, "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                if line.startswith("#columns:"):
                    if rows:
                        yield flush()
                    cols = _columns(line, cols)
                continue
            parts = line.rstrip("\n").split("\t")
            rec = _parse(parts, cols, names)
            if rec is None:
                malformed += 1
                continue
            rows.append(rec)
            if with_lines:
                lines.append(parts)
            if len(rows) >= chunk_pairs:
                yield flush()
    if rows or malformed:
        yield flush()


def device_parse(ctx, feed=False):
    """``pairs_text.walk``'s ``parse`` on an open text session of ``ctx`` (``Context.text_begin``): the four passes on the device, then
    the arrays to the host -- or, with ``feed``, nothing but the scalars: the DATA pairs stay on the device for ``text_feed_pre`` /
    ``text_feed_pairs``, and ``line_start`` and ``deferred`` come only where a line is deferred or starts with ``#columns:``"""
    def parse(seg, cols):
        res = ctx.text_parse(seg, cols)
        if not feed:
            return ctx.text_fetch(res)
        if res["counts"]["deferred"] or res["first_columns_line"] >= 0:
            return ctx.text_fetch(res, ("line_start", "deferred"))
        res["deferred"] = ()
        return res
    return parse


def feed_device(path, names, ctx, feed, add, chunk_bytes=None):
    """A pairs file parsed on the device and fed to a live session of ``ctx`` without a round trip: ``feed()`` after every parsed
    stretch (``Context.text_feed_pre`` / ``text_feed_pairs``), ``add(c1, p1, c2, p2, strands)`` (int64, uint8) for what Python had to
    decide: the deferred lines that ``_parse`` takes and the chunks refused whole.  -> the malformed lines"""
    from . import pairs_text

    def late(rows):
        if rows:
            a = np.array(rows, np.int64).reshape(-1, 5)
            add(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), a[:, 4].astype(np.uint8))

    malformed = 0
    ctx.text_begin(names)
    try:
        for ev in pairs_text.walk(path, names, device_parse(ctx, feed=True), chunk_bytes or pairs_text.DEFAULT_CHUNK_BYTES):
            if ev[0] == "parsed":
                res, seg, cols = ev[1:]
                feed()  # (in front of the next parse: the session holds one chunk's result)
                malformed += res["counts"]["malformed"]
                recs = [_parse(parts, cols, names) for parts in pairs_text.deferred_lines(res, seg)]
                malformed += sum(r is None for r in recs)
                late([r for r in recs if r is not None])
            elif ev[0] == "rows":
                late(ev[1])
                malformed += ev[2]
    finally:
        ctx.text_end()
    return malformed


def read_pairs_device(path, names, ctx, chunk_bytes=None):
    """``read_pairs`` (without ``with_lines``) with the lines, fields, integers and names parsed on the device (``ig_text_parse``; the
    rule: ``pairs_text.py``): the same yields chunk for chunk of bytes, a flush at every ``#columns:`` line.  ctx: a ``hip_lib.Context``
    with no text session open; the session is this call's own."""
    from . import pairs_text

    ctx.text_begin(names)
    try:
        yield from pairs_text.read_pairs_bytes(path, names, device_parse(ctx), chunk_bytes or pairs_text.DEFAULT_CHUNK_BYTES)
    finally:
        ctx.text_end()


def check_reader(reader):
    if reader not in ("host", "device"):
        raise ValueError("pairs: reader is \"host\" (the Python line loop) or \"device\" (pairs_text on the device), got %r" % (reader,))
    return reader


def read_header(path):
    """-> (format line, the other header lines kept, the columns line) as the reference's ``_write_lifted_pairs`` sorts them"""
    fmt, other, columns = "## pairs format v1.0", [], "#columns: " + " ".join(DEFAULT_COLUMNS)
    with _opener(path)(path, "rt") as fh:
        for line in fh:
            if not line.startswith("#"):
                break
            s = line.rstrip("\n")
            if s.startswith("## "):
                fmt = s
            elif s.startswith("#columns:"):
                columns = s
            elif s.startswith(("#chromsize:", "#chromosomes:", "#sorted:")):
                pass
            else:
                other.append(s)
    return fmt, other, columns


def write_lifted_pairs(pairs_path, out_path, table, lift=None, chunk_pairs=DEFAULT_CHUNK_PAIRS):
    """Rewrites a pairs file in the coordinates of the current genome, gzip-compressed.  The header as the reference's: the format
    line, ``#sorted: none``, the other lines kept, ``#chromosomes:`` and ``#chromsize:`` of the scaffolds under their genome.fasta
    names (``assembly_contacts.scaffold_names``), the columns line; the kept pairs in input order, every other field as it was.
    lift: ``(c1, p1, c2, p2, strands) -> lifted`` (the device's, which also stores what it keeps, or None: ``lift_host``).  -> dict of the scalars plus ``malformed`` and
    ``lines`` (data lines read).  The lines are read by the Python reader whatever the other calls use: every field of every kept line is
    written out again, and the output side is bound by gzip."""
    if table.get("names") is None:
        raise ValueError("pairs lift: the table has no contig names")
    names = ac.scaffold_names(table["scaffold_ids"])
    lift = lift or (lambda c1, p1, c2, p2, strands: lift_host(table, c1, p1, c2, p2))
    fmt, other, columns = read_header(pairs_path)
    total = dict.fromkeys(SCALARS[:5], 0)
    malformed = 0
    with gzip.open(out_path, "wt") as out:
        out.write(fmt + "\n#sorted: none\n")
        for m in other:
            out.write(m + "\n")
        out.write("#chromosomes: %s\n" % " ".join(names))
        for n, size in zip(names, table["scaffold_len"].tolist()):
            out.write("#chromsize: %s %d\n" % (n, size))
        out.write(columns + "\n")
        for ch in read_pairs(pairs_path, table["names"], chunk_pairs, with_lines=True):
            malformed = ch["malformed"]
            if not ch["lines"]:
                continue
            res = lift(ch["c1"], ch["p1"], ch["c2"], ch["p2"], ch["strands"])
            for k in total:
                total[k] += int(res[k])
            cols = ch["columns"]
            for j in np.nonzero(res["status"] == KEPT)[0].tolist():
                parts = ch["lines"][j]
                parts[cols[0]], parts[cols[1]] = names[res["scaffold1"][j]], str(int(res["pos1"][j]))
                parts[cols[2]], parts[cols[3]] = names[res["scaffold2"][j]], str(int(res["pos2"][j]))
                out.write("\t".join(parts) + "\n")
    total.update(malformed=malformed, lines=total["pairs_in"] + malformed)
    return total
