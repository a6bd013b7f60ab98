"""The polish step behind a run: what the reference's ``instagraal-polish`` does to an ``info_frags.txt`` and the input FASTA, stated
once in numpy and plain Python.  The device (``hip_lib.Context.seq_*``, csrc/ig_kernels_seq.cuh) reproduces ``stitch``
and ``composition`` byte for byte.

* **Data.**  A scaffold is a list of bins ``[init_contig, id_frag, start, end, ori]``; a genome a dict of scaffolds in file order.
  ``records`` is what ``pre.read_fasta`` returns: ``[(id, bytes)]``.
* **Corrections** (the reference's results on any input): ``remove_spurious_insertions``, ``correct_spurious_inversions``,
  ``rearrange_intra_scaffolds``, ``reorient_consecutive_blocks``.  Scaffolds of two bins or fewer are left alone where the reference
  leaves them alone, a tie in orientation goes to ``+``, the larger group wins a rearrangement and the first one a tie.
* **Lost DNA.**  ``find_lost_dna`` by interval arithmetic with the reference's semantics: a bin removes ``[start, end]`` INCLUSIVE.
  ``integrate_lost_dna(mode="reference")`` reproduces the reference with what it does wrong; ``mode="once"`` puts every base no bin
  covers (true half-open bounds) back exactly once.  ``coverage`` counts what a set of scaffolds covers, loses and duplicates.
* **Stitching.**  ``stitch_plan`` lays the polished FASTA out as tables without touching a base; ``stitch`` makes the file's bytes.
  Reverse complement: Biopython's ``ambiguous_dna_complement`` over ``ABCDGHKMNRSTVWY``, the case kept.
* ``polish_assembly`` is the seven modes of the reference's command; ``python -m instagraal_amd.scaffold_polish`` its command line.

Not built: ``plot_contig_composition`` (no ``contig_composition.png`` is written), ``parse_bed``, ``correct_scaffolds``."""
import argparse
import itertools
import os
import sys
import threading
import time

import numpy as np

from . import assembly_stats, pre

NEW_INFO_FRAGS_NAME = "new_info_frags.txt"
POLISHED_GENOME_NAME = "polished_genome.fa"
LOST_DNA_NAME = "lost_dna.fa"
STATS_NAME = "assembly_stats.txt"
MODES = ("fasta", "singleton", "inversion", "inversion2", "rearrange", "reincorporation", "polishing")
CRITERIA = ("cis", "colinear", "contiguous")
CLASSES = ("A", "C", "G", "T", "N", "other", "lower", "bases")  # SEQ_NC classes (csrc/ig_kernels_seq.cuh): a letter of either case
DEFAULT_WIDTH = 60
DEFAULT_WINDOW = 1 << 28
INFO_FRAGS_HEADER = "\t".join(("init_contig", "id_frag", "orientation", "start", "end"))


def _complement_table():
    t = np.arange(256, dtype=np.uint8)
    for a, b in pre.COMPLEMENT.items():
        t[ord(a)], t[ord(a.lower())] = ord(b), ord(b.lower())
    return t


COMPLEMENT = _complement_table()


def _class_table():
    """[256, 8]: what a byte adds to each of ``CLASSES``"""
    t = np.zeros((256, len(CLASSES)), np.int64)
    for ch in pre.ALPHABET:
        for b in (ord(ch), ord(ch.lower())):
            t[b, CLASSES.index(ch) if ch in "ACGTN" else 5] = 1
            t[b, 7] = 1
        t[ord(ch.lower()), 6] = 1
    return t


CLASS_OF = _class_table()


# ---------------------------------------------------------------- info_frags
def parse_info_frags(path):
    scaffolds, current = {}, None
    with open(path, "r") as fh:
        for no, line in enumerate(fh, start=1):
            text = line[:-1] if line.endswith("\n") else line
            if text.startswith(">"):
                current = text[1:]
                scaffolds[current] = []
            elif text.startswith("init_contig"):
                continue
            else:
                fields = text.split("\t")
                try:
                    if len(fields) != 5 or current is None:
                        raise ValueError
                    contig, frag, ori, start, end = fields[0], int(fields[1]), int(fields[2]), int(fields[3]), int(fields[4])
                except ValueError:
                    raise ValueError("%s, line %d: not a bin of a scaffold (init_contig, id_frag, orientation, start, end): %r" % (path, no, text)) from None
                if start < 0 or start >= end:
                    raise ValueError("%s, line %d: a bin runs from %d to %d" % (path, no, start, end))
                if ori not in (-1, 1):
                    raise ValueError("%s, line %d: the orientation %d is neither -1 nor 1" % (path, no, ori))
                scaffolds[current].append([contig, frag, start, end, ori])
    return scaffolds


def _scaffolds(x):
    return x if isinstance(x, dict) else parse_info_frags(x)


def info_frags_text(scaffolds):
    out = []
    for name, scaffold in _scaffolds(scaffolds).items():
        out.append(">%s\n%s\n" % (name, INFO_FRAGS_HEADER))
        for contig, frag, start, end, ori in scaffold:
            if ori not in (-1, 1):
                raise ValueError("scaffold %r: the orientation %r is neither -1 nor 1" % (name, ori))
            out.append("%s\t%s\t%s\t%s\t%s\n" % (contig, frag, ori, start, end))
    return "".join(out)


def write_info_frags(scaffolds, path=NEW_INFO_FRAGS_NAME):
    text = info_frags_text(scaffolds)
    with open(path, "w") as fh:
        fh.write(text)


def filter_scaffolds(scaffolds, min_scaffold_size=0, min_scaffold_length=0):
    """more than ``min_scaffold_size`` bins, and at least ``min_scaffold_length`` bp"""
    return {n: s for n, s in scaffolds.items() if len(s) > min_scaffold_size and sum(b[3] - b[2] for b in s) >= min_scaffold_length}


def _copy(scaffold):
    return [list(b) for b in scaffold]


def _blocks(scaffold):
    """the runs of neighbouring bins of one input contig"""
    return [list(g) for _, g in itertools.groupby(scaffold, key=lambda b: b[0])]


# ---------------------------------------------------------------- corrections
def remove_spurious_insertions(scaffolds):
    """a bin whose two neighbours (at an end: the two bins next to it) are of one contig that is not its own is dropped"""
    out = {}
    for name, s in _scaffolds(scaffolds).items():
        n = len(s)
        if n <= 2:
            out[name] = _copy(s)
            continue
        keep = []
        for i, b in enumerate(s):
            a, c = (s[1], s[2]) if i == 0 else (s[n - 2], s[n - 3]) if i == n - 1 else (s[i - 1], s[i + 1])
            if not (a[0] == c[0] and a[0] != b[0]):
                keep.append(list(b))
        out[name] = keep
    return out


def correct_spurious_inversions(scaffolds, criterion="colinear"):
    """every neighbourhood (a run of bins each of which follows the one before it under the criterion) gets its majority orientation"""
    follows = {"cis": lambda a, b: a[0] == b[0], "colinear": lambda a, b: a[0] == b[0] and a[3] <= b[2],
               "contiguous": lambda a, b: a[0] == b[0] and a[3] == b[2]}
    if criterion not in follows:
        raise ValueError("the criterion %r is none of %s" % (criterion, ", ".join(CRITERIA)))
    test = follows[criterion]
    out = {}
    for name, s in _scaffolds(scaffolds).items():
        if len(s) <= 2:
            out[name] = _copy(s)
            continue
        new, run = [], []
        for b in s:
            if run and not test(run[-1], b):
                new += _oriented(run)
                run = []
            run.append(list(b))
        out[name] = new + _oriented(run)
    return out


def _oriented(run):
    ori = 1 if sum(b[4] for b in run) >= 0 else -1
    return [b[:4] + [ori] for b in run]


def rearrange_intra_scaffolds(scaffolds):
    """the blocks of one contig brought together at the place of its largest block (the first of the largest), each block kept whole"""
    out = {}
    for name, s in _scaffolds(scaffolds).items():
        blocks = _blocks(s)
        place = {}
        for k, blk in enumerate(blocks):
            if blk[0][0] not in place or len(blk) > place[blk[0][0]][1]:
                place[blk[0][0]] = (k, len(blk))
        out[name] = [list(b) for blk in sorted(blocks, key=lambda blk: place[blk[0][0]][0]) for b in blk]
    return out


def reorient_consecutive_blocks(scaffolds, mode="blocks"):
    """``blocks``: a block gets its majority orientation and the order of its fragment ids, ascending for ``+``; ``sequences``: inside a
    block, a bin followed by the next (the previous) fragment id becomes ``+`` (``-``), and the last bin of such a run goes with it"""
    if mode not in ("blocks", "sequences"):
        raise ValueError("the mode %r is neither 'blocks' nor 'sequences'" % (mode,))
    out = {}
    for name, s in _scaffolds(scaffolds).items():
        new = []
        for blk in _blocks(s):
            if mode == "blocks":
                ori = 1 if sum(b[4] for b in blk) >= 0 else -1
                new += [b[:4] + [ori] for b in sorted(blk, key=lambda b: b[1], reverse=ori < 0)]
                continue
            run_ori = 0
            for k, b in enumerate(blk):
                step = (blk[k + 1][1] if k + 1 < len(blk) else -2) - b[1]  # (-2: the id of the reference's closing sentinel)
                if len(blk) > 1 and step in (1, -1):
                    run_ori = step
                    new.append(b[:4] + [step])
                else:
                    new.append(b[:4] + [run_ori if run_ori else b[4]])
                    run_ori = 0
        out[name] = new
    return out


# ---------------------------------------------------------------- lost DNA
def _uncovered(length, spans):
    """the stretches of ``[0, length)`` outside the half-open ``spans``, ascending"""
    out, at = [], 0
    for a, b in sorted(spans):
        a, b = max(a, 0), min(b, length)
        if a > at:
            out.append((at, a))
        at = max(at, b)
    if at < length:
        out.append((at, length))
    return out


def find_lost_dna(records, scaffolds):
    """-> ``{contig: [[contig, -1, first, last + 1, 1], ...]}`` of the records that lost something, the longest record first.  As in the
    reference a bin takes the base AT its end with it (``[start, end]`` inclusive)."""
    scaffolds = _scaffolds(scaffolds)
    spans = {}
    for s in scaffolds.values():
        for contig, _, start, end, _ in s:
            spans.setdefault(contig, []).append((start, end + 1))
    lost = {}
    for name, seq in sorted(records, key=lambda r: len(r[1]), reverse=True):
        gaps = _uncovered(len(seq), spans.get(name, ()))
        if gaps:
            lost[name] = [[name, -1, a, b, 1] for a, b in gaps]
    return lost


def lost_dna_text(records, lost):
    seqs = dict(records)
    return "".join(">%s_%d_%d\n%s\n" % (name, b[2], b[3], seqs[name][b[2]:b[3]].decode()) for name, chunks in lost.items() for b in chunks)


def integrate_lost_dna(scaffolds, lost, mode="reference", records=None):
    """``reference``: the reference's integration of ``find_lost_dna``'s stretches; ``once``: ``integrate_lost_dna_once``, which works from
    the ``records`` (``lost``, cut under the inclusive rule, does not say which bases are uncovered)"""
    scaffolds = _scaffolds(scaffolds)
    if mode == "reference":
        return _integrate_reference(scaffolds, lost)
    if mode != "once":
        raise ValueError("the mode %r is neither 'reference' nor 'once'" % (mode,))
    if records is None:
        raise ValueError("mode 'once' needs the records of the input FASTA")
    return integrate_lost_dna_once(records, scaffolds)


def _integrate_reference(scaffolds, lost):
    """The reference's integration, kept with its faults: a stretch that begins one base behind a bin's end is put in
    widened by a base on either side; one that ends at, before or behind a bin's start is put in two places before where the bin is
    believed to be; the first hit drops the contig's whole list from what is appended at the end, a second hit of the same contig ends
    the walk over that contig's stretches; of what remains only the last stretch of a contig becomes a scaffold, under the contig's name."""
    remaining = {k: _copy(v) for k, v in lost.items()}
    out = {}
    for name, scaffold in scaffolds.items():
        edited, at = _copy(scaffold), 0
        for contig, _, start, end, ori in scaffold:
            for stretch in lost.get(contig, ()):
                ls, le = stretch[2], stretch[3]
                if end == ls - 1:
                    edited.insert(at + 1 - (ori < 0), [contig, -1, ls - 1, le + 1, ori])
                elif start in (le - 1, le, le + 1):
                    edited.insert(at - 1, [contig, -1, ls, le, ori])
                else:
                    continue
                if contig not in remaining:
                    break
                del remaining[contig]
                at += 1
            at += 1
        out[name] = edited
    for contig, stretches in remaining.items():
        for b in stretches:
            out[contig] = [[contig, -1, b[2], b[3], 1]]
    return out


def integrate_lost_dna_once(records, scaffolds):
    """Every base of the input that no bin covers -- a bin is ``[start, end)`` here -- exactly once: next to the first bin of its contig
    that it abuts, in that bin's orientation (behind the bin's end, in front of its start; the other way round for a reversed bin), or
    as a scaffold of its own, ``<contig>_<first>_<end>``."""
    scaffolds = _scaffolds(scaffolds)
    spans, by_end, by_start = {}, {}, {}
    for name, s in scaffolds.items():
        for k, (contig, _, start, end, _) in enumerate(s):
            spans.setdefault(contig, []).append((start, end))
            by_end.setdefault((contig, end), (name, k))
            by_start.setdefault((contig, start), (name, k))
    before, behind, own = {}, {}, {}
    for contig, seq in records:
        for a, b in _uncovered(len(seq), spans.get(contig, ())):
            hit, at_end = (by_end[(contig, a)], True) if (contig, a) in by_end else (by_start.get((contig, b)), False)
            if hit is None:
                own["%s_%d_%d" % (contig, a, b)] = [[contig, -1, a, b, 1]]
                continue
            ori = scaffolds[hit[0]][hit[1]][4]
            (behind if at_end == (ori > 0) else before).setdefault(hit, []).append([contig, -1, a, b, ori])
    out = {}
    for name, s in scaffolds.items():
        out[name] = [x for k, b in enumerate(s) for x in before.get((name, k), []) + [list(b)] + behind.get((name, k), [])]
    for name, s in own.items():
        if name in out:
            raise ValueError("a lost stretch would be named %r, which is a scaffold already" % name)
        out[name] = s
    return out


def coverage(records, scaffolds):
    """what the bins (half-open, clipped to their record) make of the input: ``bases_input``; ``bases_covered_once``; ``bases_lost``
    (under no bin); ``bases_duplicated`` (the copies beyond the first).  Stitched length = input - lost + duplicated."""
    events = {}
    lens = {name: len(seq) for name, seq in records}
    for s in _scaffolds(scaffolds).values():
        for contig, _, start, end, _ in s:
            a, b = min(max(start, 0), lens[contig]), min(max(end, 0), lens[contig])
            if b > a:
                events.setdefault(contig, []).extend(((a, 1), (b, -1)))
    once = lost = dup = 0
    for name, n in lens.items():
        at = depth = 0
        for x, d in sorted(events.get(name, ())) + [(n, 0)]:
            span = x - at
            once += span if depth == 1 else 0
            lost += span if depth == 0 else 0
            dup += span * (depth - 1) if depth > 1 else 0
            at, depth = x, depth + d
    return dict(bases_input=sum(lens.values()), bases_covered_once=once, bases_lost=lost, bases_duplicated=dup)


# ---------------------------------------------------------------- stitching
def stitch_plan(records, scaffolds, junction="", width=DEFAULT_WIDTH):
    """The layout of the polished FASTA.  Per output record: ``names``, ``hdr_lit`` / ``hdr_len`` (the header ``>name\\n`` in
    ``literal``), ``body_len`` (bases), ``rec_off`` (int64 [n + 1]: the file offset of every header, the file's size last), ``piece_first``
    (int64 [n + 1]).  Per piece: ``src`` (the input record, -1: ``literal``), ``start`` (in the record, or in ``literal``), ``length``,
    ``ori``, ``body`` (the offset of its first base in its record's body).  A body of ``L`` bases takes ``L + ceil(L / width)`` bytes."""
    width = int(width)
    if width < 1:
        raise ValueError("a line has at least one base (width %d)" % width)
    index = {name: r for r, (name, _) in enumerate(records)}
    junction = junction.encode() if isinstance(junction, str) else bytes(junction or b"")
    literal = bytearray(junction)
    names, hdr_lit, hdr_len, body_len, rec_off, piece_first = [], [], [], [], [0], [0]
    src, start, length, ori, body = [], [], [], [], []
    clipped = 0
    for name, scaffold in _scaffolds(scaffolds).items():
        header = (">%s\n" % name).encode()
        names.append(name)
        hdr_lit.append(len(literal))
        hdr_len.append(len(header))
        literal += header
        at, previous = 0, None
        for contig, _, a, b, o in scaffold:
            if contig not in index:
                raise ValueError("scaffold %r: the contig %r is not in the FASTA" % (name, contig))
            if o not in (-1, 1):
                raise ValueError("scaffold %r: the orientation %r is neither -1 nor 1" % (name, o))
            if a < 0 or a >= b:
                raise ValueError("scaffold %r: a bin of %r runs from %d to %d" % (name, contig, a, b))
            if junction and previous not in (None, contig):
                src.append(-1), start.append(0), length.append(len(junction)), ori.append(1), body.append(at)
                at += len(junction)
            previous = contig
            n = len(records[index[contig]][1])
            lo, hi = min(a, n), min(b, n)
            clipped += hi - lo < b - a
            if hi > lo:
                src.append(index[contig]), start.append(lo), length.append(hi - lo), ori.append(o), body.append(at)
                at += hi - lo
        body_len.append(at)
        piece_first.append(len(src))
        rec_off.append(rec_off[-1] + len(header) + at + -(-at // width))
    i64 = lambda x: np.array(x, np.int64)  # noqa: E731
    return dict(names=names, width=width, literal=np.frombuffer(bytes(literal), np.uint8).copy(), hdr_lit=i64(hdr_lit), hdr_len=np.array(hdr_len, np.int32),
                body_len=i64(body_len), rec_off=i64(rec_off), piece_first=i64(piece_first), src=np.array(src, np.int32), start=i64(start), length=i64(length),
                ori=np.array(ori, np.int32), body=i64(body), pieces_clipped=int(clipped), file_bytes=int(rec_off[-1]))


def composition(records):
    """int64 [R, 8] (``CLASSES``): A, C, G, T, N of either case, the other letters, the lower-case letters, all bases"""
    out = np.zeros((len(records), len(CLASSES)), np.int64)
    for r, (_, seq) in enumerate(records):
        out[r] = np.bincount(np.frombuffer(seq, np.uint8), minlength=256) @ CLASS_OF
    return out


def stitch(records, plan):
    """-> (the file's bytes as uint8 [file_bytes], int64 [n, 8]: the composition of every output record's body)"""
    seqs = [np.frombuffer(s, np.uint8) for _, s in records]
    lit, w = plan["literal"], plan["width"]
    out = np.empty(plan["file_bytes"], np.uint8)
    counts = np.zeros((len(plan["names"]), len(CLASSES)), np.int64)
    for j in range(len(plan["names"])):
        at = int(plan["rec_off"][j])
        h = int(plan["hdr_len"][j])
        out[at:at + h] = lit[int(plan["hdr_lit"][j]):int(plan["hdr_lit"][j]) + h]
        parts = []
        for p in range(int(plan["piece_first"][j]), int(plan["piece_first"][j + 1])):
            a, n = int(plan["start"][p]), int(plan["length"][p])
            part = (lit if plan["src"][p] < 0 else seqs[plan["src"][p]])[a:a + n]
            parts.append(part if plan["ori"][p] > 0 else COMPLEMENT[part[::-1]])
        bases = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        L = bases.size
        assert L == plan["body_len"][j]
        counts[j] = np.bincount(bases, minlength=256) @ CLASS_OF
        at += h
        full = L // w
        lines = out[at:at + full * (w + 1)].reshape(full, w + 1)
        lines[:, :w] = bases[:full * w].reshape(full, w)
        lines[:, w] = 10
        at += full * (w + 1)
        if L % w:
            out[at:at + L % w] = bases[full * w:]
            out[at + L % w] = 10
    return out, counts


def stitch_device(ctx, records, plan, sink, window=DEFAULT_WINDOW, times=None):
    """the same file through the device, window by window: ``sink(bytes-like)`` gets every window in order, from a second thread while
    the next one is computed -> (int64 [R, 8]: the input's composition, int64 [n, 8]: the output's)"""
    window = max(16, int(window) // 16 * 16)
    buf, offs, lens = pre.concatenate(records)
    ctx.seq_begin(buf, offs, lens)
    try:
        comp = ctx.seq_composition(times=times)
        ctx.seq_plan(plan)
        total = plan["file_bytes"]
        bufs = [np.empty(min(window, max(total, 1)), np.uint8) for _ in range(2)]
        writer, failure = None, []

        def put(view):
            try:
                sink(view)
            except BaseException as e:  # noqa: BLE001  (handed to the caller's thread below)
                failure.append(e)

        for k, first in enumerate(range(0, total, window)):
            n = min(window, total - first)
            view = bufs[k & 1][:n]  # (the writer of window k - 1 holds the other buffer; that of k - 2 was joined before k - 1 began)
            ctx.seq_window(first, view, times=times)
            if writer is not None:
                writer.join()
            if failure:
                raise failure[0]
            writer = threading.Thread(target=put, args=(view,))
            writer.start()
        if writer is not None:
            writer.join()
        if failure:
            raise failure[0]
        return comp, ctx.seq_out_composition(len(plan["names"]))
    finally:
        ctx.seq_end()


# ---------------------------------------------------------------- the command
def _stats_of(counts):
    return assembly_stats.compute_assembly_stats(counts[:, 7], counts[:, 2] + counts[:, 1])


def polish_assembly(info_frags, fasta=None, output_dir="out", mode="polishing", criterion=None, min_scaffold_size=0, min_scaffold_length=0, junction="", lost="reference",
                    device=True, width=DEFAULT_WIDTH, window=DEFAULT_WINDOW, device_id=0, times=None):
    """The reference's ``instagraal-polish``: the seven ``MODES``, its file names.  ``lost``: how the lost DNA goes back in
    (``integrate_lost_dna``).  ``device``: the FASTA is stitched and counted on the GPU (a missing library or device is an error), else
    by ``stitch``.  ``times``: a dict that gets the seconds ``read_s``, ``lists_s`` and ``stitch_s`` (with the device also the kernels' ms: ``composition``, ``stitch``).  Writes ``new_info_frags.txt`` (every mode but ``fasta``), ``polished_genome.fa`` and ``assembly_stats.txt`` (``fasta``
    and ``polishing``), ``lost_dna.fa`` (``reincorporation`` and ``polishing``).  -> dict: the scaffolds, the files, the coverage."""
    mode = (mode or "polishing").lower()
    if mode not in MODES:
        raise ValueError("the mode %r is none of %s" % (mode, ", ".join(MODES)))
    if lost not in ("reference", "once"):
        raise ValueError("lost=%r is neither 'reference' nor 'once'" % (lost,))
    if mode in ("fasta", "reincorporation", "polishing") and fasta is None:
        raise ValueError("a reference FASTA file must be provided for the mode %r" % mode)
    os.makedirs(output_dir, exist_ok=True)
    clock = [time.perf_counter()]

    def lap(key):
        clock.append(time.perf_counter())
        if times is not None:
            times[key] = times.get(key, 0.0) + clock[-1] - clock[-2]

    parsed = parse_info_frags(info_frags)
    scaffolds = filter_scaffolds(parsed, min_scaffold_size, min_scaffold_length)
    result = dict(mode=mode, scaffolds_in=len(parsed), scaffolds_kept=len(scaffolds), files=[])
    records = None
    if fasta is not None and mode in ("fasta", "reincorporation", "polishing"):
        records = pre.read_fasta(fasta)
        pre.check_records(records)
    lap("read_s")

    def integrate(s):
        removed = find_lost_dna(records, s)
        with open(os.path.join(output_dir, LOST_DNA_NAME), "w") as fh:
            fh.write(lost_dna_text(records, removed))
        result["files"].append(LOST_DNA_NAME)
        return integrate_lost_dna(s, removed) if lost == "reference" else integrate_lost_dna_once(records, s)

    if mode == "fasta":
        new = parsed  # (the reference stitches the file it was given, whatever the filters kept)
    elif mode == "singleton":
        new = remove_spurious_insertions(scaffolds)
    elif mode == "inversion":
        new = correct_spurious_inversions(scaffolds, criterion or "colinear")
    elif mode == "inversion2":
        new = reorient_consecutive_blocks(scaffolds, criterion or "blocks")
    elif mode == "rearrange":
        new = rearrange_intra_scaffolds(scaffolds)
    elif mode == "reincorporation":
        new = integrate(scaffolds)
    else:
        new = integrate(reorient_consecutive_blocks(rearrange_intra_scaffolds(scaffolds)))
    result["scaffolds"] = new
    if mode != "fasta":
        write_info_frags(new, os.path.join(output_dir, NEW_INFO_FRAGS_NAME))
        result["files"].append(NEW_INFO_FRAGS_NAME)
    if records is not None:
        result.update(coverage(records, new))
    lap("lists_s")
    if mode in ("fasta", "polishing"):
        plan = stitch_plan(records, new, junction=junction, width=width)
        path = os.path.join(output_dir, POLISHED_GENOME_NAME)
        with open(path, "wb") as fh:
            if device:
                from . import hip_lib

                ctx = hip_lib.Context(device_id)
                try:
                    comp_in, comp_out = stitch_device(ctx, records, plan, fh.write, window=window, times=times)
                finally:
                    ctx.close()
            else:
                image, comp_out = stitch(records, plan)
                fh.write(image.data)
                comp_in = composition(records)
        lap("stitch_s")
        stats = {"input": _stats_of(comp_in), "polished": _stats_of(comp_out)}
        label = "Assembly (%s mode)" % mode
        text = assembly_stats.format_assembly_stats(stats["polished"], label=label) + assembly_stats.format_comparison_table(stats)
        with open(os.path.join(output_dir, STATS_NAME), "w") as fh:
            fh.write(text)
        result.update(stats=stats, composition_input=comp_in, composition=comp_out, pieces_clipped=plan["pieces_clipped"], file_bytes=plan["file_bytes"], stats_text=text)
        result["files"] += [POLISHED_GENOME_NAME, STATS_NAME]
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m instagraal_amd.scaffold_polish", description="Polish and post-process an assembly (the reference's instagraal-polish).")
    ap.add_argument("-m", "--mode", default=None, type=str.lower, choices=MODES, help="default: the whole polishing (rearrange, inversion2, reincorporation, fasta)")
    ap.add_argument("-i", "--input", dest="info_frags", required=True, help="the info_frags.txt to process")
    ap.add_argument("-f", "--fasta", default=None, help="the FASTA the run started from (fasta, reincorporation, polishing)")
    ap.add_argument("-o", "--output-dir", default="out")
    ap.add_argument("-c", "--criterion", default=None, help="inversion: cis, colinear, contiguous; inversion2: blocks, sequences")
    ap.add_argument("-s", "--min-scaffold-size", type=int, default=0, help="scaffolds of more bins than this are kept")
    ap.add_argument("-l", "--min-scaffold-length", type=int, default=0, help="scaffolds of at least this many bp are kept")
    ap.add_argument("-j", "--junction", default="", help="the sequence put between two bins of different contigs")
    ap.add_argument("--lost", default="reference", choices=("reference", "once"), help="how the lost DNA goes back in")
    ap.add_argument("--host", action="store_true", help="stitch on the host, without the GPU")
    a = ap.parse_args(argv)
    if not os.path.isfile(a.info_frags):
        ap.error("no such file: %s" % a.info_frags)
    try:
        r = polish_assembly(a.info_frags, a.fasta, a.output_dir, mode=a.mode, criterion=a.criterion, min_scaffold_size=a.min_scaffold_size,
                            min_scaffold_length=a.min_scaffold_length, junction=a.junction, lost=a.lost, device=not a.host)
    except ValueError as e:
        ap.error(str(e))
    print(r["scaffolds_kept"], "of", r["scaffolds_in"], "scaffolds retained after filtering by bins [", a.min_scaffold_size, "] and length [", a.min_scaffold_length, "].")
    if "stats_text" in r:
        print(r["stats_text"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
