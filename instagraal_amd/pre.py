"""The input folder from an assembly FASTA and a 4DN pairs file: what the reference's ``pre`` step makes with Biopython, pandas and
cooler, stated once in numpy and plain Python (no GPU).  The device (``hip_lib.Context.pre_*``, csrc/ig_kernels_pre.cuh)
reproduces the arrays of this module byte for byte.

* **Enzymes.**  ``enzyme(spec)`` -> ``(site, cut)``: an upper-case IUPAC site of 1 .. 16 letters and ``0 <= cut <= len(site)``; a name
  of ``ENZYMES`` or a literal site with one ``^``.  ``expand_enzymes`` takes a list (or a comma-separated string) and knows ``Arima`` as
  DpnII + HinfI.  A site that is not its own reverse complement is refused: Biopython searches both strands for those.
* **Matching** is Biopython's regular expression restated: the sequence is upper-cased; a site letter ``N`` matches any sequence letter,
  any other site letter only those of A, C, G, T its IUPAC set holds (an ambiguity code in the sequence matches nothing but ``N``);
  matches may overlap; a match lies inside its record.  A sequence character outside ``ABCDGHKMNRSTVWY`` is refused.
* **Digest.**  A match at 0-based ``s`` cuts at ``s + cut``; the cuts of all enzymes of a record, with 0 and the record's length,
  de-duplicated and sorted, bound its fragments ``[start, end)``.
* **GC.**  G and C of either case per fragment, an integer; the fraction is ``count / length`` as a Python float.
* **Fragment of a position.**  1-based ``p`` of a record: ``searchsorted(starts, p - 1, "right") - 1``; ``p <= 0`` and an unknown record
  have none; a position beyond the record's end falls into its last fragment, as in the reference, and is counted (``ends_beyond_record``:
  every end of a known record with ``p`` beyond its length, whatever becomes of the pair).
* **Pixels.**  Every pair whose two ends have a fragment adds 1 at ``(min, max)`` of the global fragment ids, the diagonal included.

The one place where the reader differs from the reference's: the pairs are read by ``pairs_lift.read_pairs``, which COUNTS the
malformed data lines (a missing field, a position that is no integer) and reports them (``malformed_lines``); the reference skips them
in silence.  The numbers that come out are the same."""
import gzip
import os

import numpy as np

from . import pairs_lift

ENZYMES = {
    "DpnII": "^GATC", "MboI": "^GATC", "Sau3AI": "^GATC", "HinfI": "G^ANTC", "DdeI": "C^TNAG", "MseI": "T^TAA", "NlaIII": "CATG^",
    "HindIII": "A^AGCTT", "EcoRI": "G^AATTC", "NcoI": "C^CATGG", "BglII": "A^GATCT", "Csp6I": "G^TAC",
}
ENZYME_SETS = {"Arima": ("DpnII", "HinfI")}
MAX_SITE = 16       # PRE_MAX_SITE (csrc/ig_kernels_pre.cuh)
MAX_ENZYMES = 4     # PRE_MAX_ENZYMES
MAX_RECORD = (1 << 31) - 2  # a position clipped to 2^31 - 1 (_clip32) is still beyond the longest record
ALPHABET = "ABCDGHKMNRSTVWY"
IUPAC = dict(A="A", C="C", G="G", T="T", R="AG", Y="CT", S="CG", W="AT", K="GT", M="AC", B="CGT", D="AGT", H="ACT", V="ACG", N="ACGT")
COMPLEMENT = dict(A="T", C="G", G="C", T="A", R="Y", Y="R", S="S", W="W", K="M", M="K", B="V", V="B", D="H", H="D", N="N")
# a base's code: one bit per plain letter and the "valid letter" bit; a site letter's mask: the bits it accepts (N: the valid bit)
BIT_A, BIT_C, BIT_G, BIT_T, BIT_VALID = 1, 2, 4, 8, 16
SCALARS = ("pairs_in", "pairs_kept", "end1_without_fragment", "end2_without_fragment", "ends_beyond_record", "pixels")
DEFAULT_CHUNK_PAIRS = pairs_lift.DEFAULT_CHUNK_PAIRS


def _code_table():
    t = np.zeros(256, np.uint8)
    for ch in ALPHABET:
        v = BIT_VALID | {"A": BIT_A, "C": BIT_C, "G": BIT_G, "T": BIT_T}.get(ch, 0)
        t[ord(ch)] = t[ord(ch.lower())] = v
    return t


CODE = _code_table()


# ---------------------------------------------------------------- enzymes
def enzyme(spec):
    """-> (site, cut) of a name of ``ENZYMES`` or of a literal site with one ``^``"""
    spec = str(spec).strip()
    text = ENZYMES.get(spec)
    if text is None:
        if spec in ENZYME_SETS:
            raise ValueError("%r is a set of enzymes (%s): expand_enzymes takes it" % (spec, " + ".join(ENZYME_SETS[spec])))
        if "^" not in spec:
            raise ValueError("Unknown restriction enzyme: %r" % spec)
        text = spec
    if text.count("^") != 1:
        raise ValueError("a literal site has one '^' (got %r)" % text)
    cut = text.index("^")
    site = text.replace("^", "").upper()
    if not 1 <= len(site) <= MAX_SITE:
        raise ValueError("a site has 1 .. %d letters (got %r)" % (MAX_SITE, text))
    bad = [ch for ch in site if ch not in IUPAC]
    if bad:
        raise ValueError("%r is no IUPAC letter (site %r)" % (bad[0], text))
    if "".join(COMPLEMENT[ch] for ch in reversed(site)) != site:
        raise ValueError("the site %r is not its own reverse complement: both strands would have to be searched, which is not built" % text)
    return site, cut


def expand_enzymes(specs):
    """a list of names or sites, or one comma-separated string -> [(site, cut)], the sets of ``ENZYME_SETS`` expanded"""
    if isinstance(specs, str):
        specs = [s for s in specs.split(",") if s.strip()]
    out = []
    for s in specs:
        if isinstance(s, tuple):
            out.append((str(s[0]), int(s[1])))
            continue
        for name in ENZYME_SETS.get(str(s).strip(), (s,)):
            out.append(enzyme(name))
    if not 1 <= len(out) <= MAX_ENZYMES:
        raise ValueError("1 .. %d enzymes (got %d)" % (MAX_ENZYMES, len(out)))
    return out


def site_masks(site):
    """uint8 [MAX_SITE]: per site letter the bits of a base's code it accepts, 0 behind the site"""
    m = np.zeros(MAX_SITE, np.uint8)
    for j, ch in enumerate(site):
        m[j] = BIT_VALID if ch == "N" else sum({"A": BIT_A, "C": BIT_C, "G": BIT_G, "T": BIT_T}[b] for b in IUPAC[ch])
    return m


# ---------------------------------------------------------------- FASTA
def read_fasta(path):
    """a plain or ``.gz`` FASTA -> [(id, sequence bytes)] in the file's order; id: the header up to the first white space"""
    opener = gzip.open if str(path).endswith(".gz") else open
    out, name, parts = [], None, []
    with opener(path, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                fields = line[1:].split()
                name, parts = (fields[0].decode() if fields else ""), []
            elif name is not None:
                parts.append(b"".join(line.split()))
            elif line.strip():
                raise ValueError("%s: sequence before the first header" % path)
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def check_records(records):
    """the refusals of the rule that need no enzyme: an empty or repeated record, a character outside the alphabet"""
    seen = set()
    if not records:
        raise ValueError("no record")
    for name, seq in records:
        if name in seen:
            raise ValueError("the record name %r is repeated" % name)
        seen.add(name)
        if len(seq) == 0:
            raise ValueError("the record %r is empty" % name)
        if len(seq) > MAX_RECORD:
            raise ValueError("the record %r has %d bases: more than 2^31 - 2" % (name, len(seq)))
        bad = np.flatnonzero(CODE[np.frombuffer(seq, np.uint8)] == 0)
        if bad.size:
            raise ValueError("record %r, position %d: the character %r is not one of %s" % (name, int(bad[0]) + 1, chr(seq[int(bad[0])]), ALPHABET))


def concatenate(records):
    """-> (bytes uint8 [sum(len) + R], offsets int64 [R], lengths int64 [R]): the records one behind the other, a zero byte behind each"""
    lens = np.array([len(s) for _, s in records], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens + 1)[:-1])).astype(np.int64)
    buf = np.zeros(int(lens.sum()) + len(records), np.uint8)
    for (_, s), o in zip(records, offs):
        buf[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
    return buf, offs, lens


# ---------------------------------------------------------------- digest, GC
def match_starts(seq, site):
    """0-based starts of the site in one record's bytes"""
    code = CODE[np.frombuffer(seq, np.uint8)]
    n, L = code.size, len(site)
    if n < L:
        return np.zeros(0, np.int64)
    m = site_masks(site)
    ok = np.ones(n - L + 1, bool)
    for j in range(L):
        ok &= (code[j:n - L + 1 + j] & m[j]) != 0
    return np.flatnonzero(ok).astype(np.int64)


def digest(records, enzymes):
    """-> dict: names, rec_len (int64 [R]), rec_first (int64 [R + 1]: the first global fragment of every record), frag_rec (int32),
    start, end (int64 [n_frags], 0-based, half-open, inside the record), n_frags"""
    enzymes = expand_enzymes(enzymes)
    check_records(records)
    starts, ends, recs, first = [], [], [], [0]
    for r, (_, seq) in enumerate(records):
        cuts = [np.array([0, len(seq)], np.int64)] + [match_starts(seq, site) + cut for site, cut in enzymes]
        cuts = np.unique(np.concatenate(cuts))
        starts.append(cuts[:-1])
        ends.append(cuts[1:])
        recs.append(np.full(cuts.size - 1, r, np.int32))
        first.append(first[-1] + cuts.size - 1)
    return dict(names=[n for n, _ in records], rec_len=np.array([len(s) for _, s in records], np.int64), rec_first=np.array(first, np.int64),
                frag_rec=np.concatenate(recs), start=np.concatenate(starts), end=np.concatenate(ends), n_frags=first[-1], enzymes=enzymes)


def gc_counts(records, dig):
    """int64 [n_frags]: the letters G and C of either case of every fragment"""
    out = np.zeros(dig["n_frags"], np.int64)
    for r, (_, seq) in enumerate(records):
        is_gc = (CODE[np.frombuffer(seq, np.uint8)] & (BIT_C | BIT_G)) != 0
        pre = np.concatenate(([0], np.cumsum(is_gc, dtype=np.int64)))
        a, b = int(dig["rec_first"][r]), int(dig["rec_first"][r + 1])
        out[a:b] = pre[dig["end"][a:b]] - pre[dig["start"][a:b]]
    return out


def gc_fraction(gc, length):
    return int(gc) / int(length)


# ---------------------------------------------------------------- fragment of a position, pixels
def fragment_of(dig, rec, pos):
    """rec: record index (-1 or beyond the records: unknown), pos: 1-based -> (global fragment id int64, -1: none; bool: the end lies
    beyond its record's end)"""
    rec, pos = np.asarray(rec, np.int64), np.asarray(pos, np.int64)
    R = len(dig["names"])
    frag, beyond = np.full(rec.shape, -1, np.int64), np.zeros(rec.shape, bool)
    known = (rec >= 0) & (rec < R)
    for r in np.unique(rec[known]):
        sel = np.flatnonzero(known & (rec == r))
        a, b = int(dig["rec_first"][r]), int(dig["rec_first"][r + 1])
        idx = np.searchsorted(dig["start"][a:b], pos[sel] - 1, side="right") - 1
        frag[sel] = np.where(idx >= 0, a + idx, -1)
        beyond[sel] = pos[sel] > dig["rec_len"][r]
    return frag, beyond


def pixels_host(dig, c1, p1, c2, p2):
    """-> dict: rowptr (int64 [n_frags + 1]), col, count (int64), sorted by (bin1, bin2), and the scalars of ``SCALARS``"""
    f1, b1 = fragment_of(dig, c1, p1)
    f2, b2 = fragment_of(dig, c2, p2)
    n = dig["n_frags"]
    miss1 = f1 < 0
    miss2 = ~miss1 & (f2 < 0)
    keep = ~miss1 & ~miss2
    lo, hi = np.minimum(f1[keep], f2[keep]), np.maximum(f1[keep], f2[keep])
    key, count = np.unique(lo * n + hi, return_counts=True) if lo.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    rows = key // max(n, 1)
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    out = dict(rowptr=np.cumsum(rowptr), col=(key % max(n, 1)).astype(np.int64), count=count.astype(np.int64))
    out.update(pairs_in=int(f1.size), pairs_kept=int(keep.sum()), end1_without_fragment=int(miss1.sum()), end2_without_fragment=int(miss2.sum()),
               ends_beyond_record=int(b1.sum()) + int(b2.sum()), pixels=int(key.size))
    return out


def merge_pixels(parts, n_frags):
    """the pixels of several chunks as one (the rule's form of a store that grows): rows, columns and scalars summed"""
    if not parts:
        out = dict(rowptr=np.zeros(n_frags + 1, np.int64), col=np.zeros(0, np.int64), count=np.zeros(0, np.int64))
        out.update({k: 0 for k in SCALARS})
        return out
    n = max(n_frags, 1)
    keys = np.concatenate([np.repeat(np.arange(n_frags, dtype=np.int64), np.diff(p["rowptr"])) * n + p["col"] for p in parts])
    cnts = np.concatenate([p["count"] for p in parts])
    key, inv = np.unique(keys, return_inverse=True)
    count = np.zeros(key.size, np.int64)
    np.add.at(count, inv, cnts)
    rowptr = np.zeros(n_frags + 1, np.int64)
    np.add.at(rowptr, key // n + 1, 1)
    out = dict(rowptr=np.cumsum(rowptr), col=key % n, count=count)
    for k in SCALARS[:5]:
        out[k] = sum(p[k] for p in parts)
    out["pixels"] = int(key.size)
    return out


# ---------------------------------------------------------------- writers
def write_fragments_list(path, dig, gc):
    with open(path, "w") as fh:
        fh.write("id\tchrom\tstart_pos\tend_pos\tsize\tgc_content\n")
        names, first = dig["names"], dig["rec_first"]
        for r, name in enumerate(names):
            for i, f in enumerate(range(int(first[r]), int(first[r + 1])), start=1):
                s, e = int(dig["start"][f]), int(dig["end"][f])
                fh.write(f"{i}\t{name}\t{s}\t{e}\t{e - s}\t{gc_fraction(gc[f], e - s)}\n")


def write_info_contigs(path, dig):
    with open(path, "w") as fh:
        fh.write("contig\tlength\tn_frags\tcumul_length\n")
        first = dig["rec_first"]
        for r, name in enumerate(dig["names"]):
            fh.write(f"{name}\t{int(dig['rec_len'][r])}\t{int(first[r + 1] - first[r])}\t{int(first[r])}\n")


def write_abs_contacts(path, n_frags, rowptr, col, count):
    rows = np.repeat(np.arange(n_frags, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))
    with open(path, "w") as fh:
        fh.write(f"{n_frags}\t{n_frags}\t{len(col)}\n")
        for a, b, c in zip(rows.tolist(), np.asarray(col).tolist(), np.asarray(count).tolist()):
            fh.write(f"{a}\t{b}\t{c}\n")


def display_matrix(rowptr, col, count, max_display_bins=1000):
    """The matrix of the pre-assembly picture (float32, symmetric): the fragments are grouped in runs of ``group`` consecutive ones,
    the least number that leaves at most ``max_display_bins`` groups; a pixel counts for the cell of its two groups and, off the
    diagonal of the groups, for the mirrored cell too; the cells are then ``log1p`` of their sums."""
    rowptr = np.asarray(rowptr, np.int64)
    n_frags = rowptr.size - 1
    group = max(1, -(-n_frags // int(max_display_bins)))
    side = -(-n_frags // group)
    ga = np.repeat(np.arange(n_frags, dtype=np.int64) // group, np.diff(rowptr))
    gb = np.asarray(col, np.int64) // group
    w = np.asarray(count, np.float64)
    cells = np.bincount(ga * side + gb, weights=w, minlength=side * side)
    mirrored = ga != gb
    cells += np.bincount(gb[mirrored] * side + ga[mirrored], weights=w[mirrored], minlength=side * side)
    return np.log1p(cells.reshape(side, side).astype(np.float32))


def _plot(path, image, title):
    """the picture as ``sampler.display_current_matrix`` draws its own: a figure on an Agg canvas of its own (no pyplot: the process's
    backend is left alone), the colour scale cut at the 98th percentile of the cells that hold anything"""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    filled = image[image > 0]
    fig = Figure(figsize=(8, 8))
    FigureCanvasAgg(fig)
    ax = fig.subplots()
    ax.imshow(image, cmap="YlOrRd", vmin=0.0, vmax=float(np.percentile(filled, 98)) if filled.size else 1.0, interpolation="nearest")
    ax.set_title(title)
    ax.axis("off")
    fig.savefig(str(path), dpi=150, bbox_inches="tight")


# ---------------------------------------------------------------- the whole step
def _clip32(p):
    """positions as the device takes them: 2^31 - 1 and anything beyond it is beyond every record (MAX_RECORD), below 0 is as 0"""
    return np.clip(p, 0, (1 << 31) - 1).astype(np.int32)


def run_pre(fasta, pairs, enzymes, output_dir, device=True, plot=False, chunk_pairs=DEFAULT_CHUNK_PAIRS):
    """FASTA + pairs -> ``fragments_list.txt``, ``info_contigs.txt``, ``abs_fragments_contacts_weighted.txt`` in ``output_dir``; returns
    the scalars of ``SCALARS`` plus ``n_frags``, ``n_records`` and ``malformed_lines``.  ``device``: True (a handle of its own on device
    0), a ``hip_lib.Context``, or False: the rule alone.  The pairs are read by the Python line loop (``pairs_lift.read_pairs``);
    ``run_pre_reader`` is this call with the reader chosen."""
    return run_pre_reader(fasta, pairs, enzymes, output_dir, "host", device, plot, chunk_pairs)


def run_pre_reader(fasta, pairs, enzymes, output_dir, reader="host", device=True, plot=False, chunk_pairs=DEFAULT_CHUNK_PAIRS):
    """``run_pre`` with the reader of the pairs text chosen: "host" (``pairs_lift.read_pairs``, the Python line loop) or "device": the
    text is parsed by ``pairs_text`` -- on the device, which feeds the store without a round trip, or with ``device=False`` by the rule
    on the host; the files and the dict are the same.  (``run_pre``'s own parameter list is pinned, so the choice lives here.)"""
    from . import pairs_text

    pairs_lift.check_reader(reader)
    chunk_bytes = pairs_text.DEFAULT_CHUNK_BYTES
    enzymes = expand_enzymes(enzymes)
    records = read_fasta(fasta)
    check_records(records)
    os.makedirs(output_dir, exist_ok=True)
    names = {n: k for k, (n, _) in enumerate(records)}
    malformed = 0
    ctx = own = None
    if device is not False and device is not None:
        from . import hip_lib

        ctx = device if isinstance(device, hip_lib.Context) else hip_lib.Context(0)
        own = ctx if ctx is not device else None
    try:
        if ctx is None:
            dig = digest(records, enzymes)
            gc = gc_counts(records, dig)
            parts = []
            for chunk in pairs_lift.read_pairs(pairs, names, chunk_pairs) if reader == "host" else pairs_text.read_pairs_bytes(pairs, names, None, chunk_bytes):
                malformed = chunk["malformed"]
                parts.append(pixels_host(dig, chunk["c1"], chunk["p1"], chunk["c2"], chunk["p2"]))
            px = merge_pixels(parts, dig["n_frags"])
        else:
            buf, offs, lens = concatenate(records)
            ctx.pre_begin(buf, offs, lens)
            try:
                dig = ctx.pre_digest(enzymes)
                dig["names"] = [n for n, _ in records]
                gc = dig.pop("gc_count")

                def add(c1, p1, c2, p2, strands=None):
                    ctx.pre_add_pairs(c1.astype(np.int32), _clip32(p1), c2.astype(np.int32), _clip32(p2))

                if reader == "device":
                    malformed = pairs_lift.feed_device(pairs, names, ctx, ctx.text_feed_pre, add, chunk_bytes)
                else:
                    for chunk in pairs_lift.read_pairs(pairs, names, chunk_pairs):
                        malformed = chunk["malformed"]
                        add(chunk["c1"], chunk["p1"], chunk["c2"], chunk["p2"])
                px = ctx.pre_pixels()
            finally:
                ctx.pre_end()
    finally:
        if own is not None:
            own.close()
    write_fragments_list(os.path.join(output_dir, "fragments_list.txt"), dig, gc)
    write_info_contigs(os.path.join(output_dir, "info_contigs.txt"), dig)
    write_abs_contacts(os.path.join(output_dir, "abs_fragments_contacts_weighted.txt"), dig["n_frags"], px["rowptr"], px["col"], px["count"])
    if plot:
        stem = os.path.basename(str(pairs))
        for _ in range(2):
            stem, ext = os.path.splitext(stem)
            if not ext:
                break
        _plot(os.path.join(output_dir, stem + "_hic_map.png"), display_matrix(px["rowptr"], px["col"], px["count"]), stem + " - pre-assembly Hi-C map")
    out = {k: int(px[k]) for k in SCALARS}
    out.update(n_frags=int(dig["n_frags"]), n_records=len(records), malformed_lines=int(malformed))
    return out
