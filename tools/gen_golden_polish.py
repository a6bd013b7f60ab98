#!/usr/bin/env python3
"""Generate tests/golden/polish_tiny.npz by running the REFERENCE's own polish functions on a small genome and info_frags.txt.

Needs the reference checkout beside the repository, like tools/gen_golden_pre.py.  The reference's ``_scaffold_correct``, ``_scaffold_io``
and ``assembly_stats`` are imported unmodified; ``Bio`` is replaced by inert stand-ins in ``sys.modules`` where it is absent, and the two
places that read a FASTA through it (``_parse_fasta``, ``SeqIO.parse``) by the few-line reader below.  ``write_fasta`` needs Biopython's
``Seq`` and ``SeqIO.write`` themselves and is NOT run: the golden holds no FASTA bytes from the reference.

The genome is seeded: eight records, one of a single base, one that no bin touches, lower case, runs of N and ambiguity codes in it.
The info_frags holds twelve scaffolds: the three inversion kinds of the reference's docstring, singleton insertions at the first, a
middle and the last place, a contig split into three groups with a tie in size, blocks whose orientations sum to 0, bins with gaps
between them, a gap of exactly one base, bins that touch a record's last base, runs of consecutive fragment ids, scaffolds of one and
of two bins.

Only data is stored: the records, the info_frags text, every function's result as the text the reference's ``write_info_frags`` makes of
it, the lost stretches as arrays, the stats dict's values and the formatted strings.

usage:  python tools/gen_golden_polish.py [--out tests/golden] [--check]
"""
import argparse
import copy
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(1, "/root/reference/src")
from tools.gen_golden_pre import _StandIn  # noqa: E402

NAME = "polish_tiny"
SEED = 43
SIZES = (("contig1", 3200), ("contig2", 2000), ("ctgA", 400), ("ctgB", 900), ("ctgC", 1200), ("ctgD", 700), ("ctgOne", 1), ("ctgUntouched", 150))
SCAFFOLDS = {
    "inversions": [("contig1", 1, 100, 200, 1), ("contig1", 2, 200, 300, 1), ("contig1", 3, 300, 400, -1), ("contig1", 4, 400, 500, 1), ("contig1", 10, 1500, 1605, 1),
                   ("contig1", 12, 1750, 1850, -1), ("contig1", 23, 2100, 2499, 1), ("contig1", 28, 2850, 3000, 1), ("contig1", 0, 0, 100, -1), ("contig2", 554, 1850, 1900, -1)],
    "insertion_first": [("ctgB", 7, 0, 50, 1), ("ctgC", 1, 0, 100, 1), ("ctgC", 2, 100, 200, 1), ("ctgC", 3, 200, 300, -1)],
    "insertion_middle": [("ctgC", 4, 300, 400, 1), ("ctgC", 5, 400, 500, 1), ("ctgB", 8, 50, 120, -1), ("ctgC", 6, 500, 600, 1), ("contig2", 9, 0, 90, 1), ("ctgC", 7, 600, 700, 1)],
    "insertion_last": [("ctgC", 8, 700, 800, -1), ("ctgC", 9, 800, 900, -1), ("ctgB", 9, 120, 200, 1)],
    "three_groups": [("ctgD", 1, 0, 100, 1), ("ctgD", 2, 100, 200, 1), ("ctgB", 10, 200, 300, 1), ("ctgD", 4, 300, 400, -1), ("ctgD", 3, 200, 300, -1), ("contig2", 20, 100, 300, 1),
                     ("ctgD", 5, 400, 500, 1)],
    "orientation_tie": [("ctgB", 13, 400, 500, -1), ("ctgB", 12, 300, 400, 1), ("ctgC", 11, 1000, 1100, -1), ("ctgC", 10, 900, 1000, -1), ("ctgC", 12, 1100, 1200, 1)],
    "toy_gaps": [("ctgA", 0, 0, 100, 1), ("ctgA", 1, 100, 200, 1), ("ctgA", 3, 300, 400, 1)],
    "one_base_gap": [("ctgB", 14, 500, 600, 1), ("ctgB", 15, 601, 700, 1), ("ctgB", 17, 800, 900, -1)],
    "id_runs": [("contig2", 30, 400, 500, -1), ("contig2", 31, 500, 600, -1), ("contig2", 32, 600, 700, 1), ("contig2", 40, 900, 1000, 1), ("contig2", 39, 800, 900, 1),
                ("contig2", 38, 700, 800, 1), ("contig2", 50, 1200, 1300, -1), ("contig2", 60, 1400, 1500, 1)],
    "one_bin": [("ctgOne", 0, 0, 1, 1)],
    "two_bins": [("contig2", 70, 1600, 1700, -1), ("ctgD", 6, 600, 700, 1)],
    "reversed_end": [("ctgD", 7, 500, 590, -1), ("contig1", 29, 3000, 3200, -1), ("contig1", 5, 500, 640, 1)],
}
CRITERIA = ("cis", "colinear", "contiguous")


class _Record:
    def __init__(self, name, seq):
        self.id, self.seq = name, seq

    def __len__(self):
        return len(self.seq)


def _read(path_or_handle, fmt="fasta"):
    from instagraal_amd.pre import read_fasta

    path = path_or_handle if isinstance(path_or_handle, str) else path_or_handle.name
    return iter([_Record(n, s.decode()) for n, s in read_fasta(path)])


def import_reference():
    for name in ("Bio", "Bio.Seq", "Bio.SeqIO", "Bio.SeqRecord"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _StandIn(name)
    import importlib
    import types

    pkg = types.ModuleType("instagraal")  # (the package's own __init__ pulls in the whole program: only its directory is needed)
    pkg.__path__ = ["/root/reference/src/instagraal"]
    sys.modules.setdefault("instagraal", pkg)
    sio = importlib.import_module("instagraal._scaffold_io")
    cor = importlib.import_module("instagraal._scaffold_correct")
    ast = importlib.import_module("instagraal.assembly_stats")
    sio._parse_fasta = cor._parse_fasta = _read
    ast.SeqIO = types.SimpleNamespace(parse=_read)
    return sio, cor, ast


def make_genome(rng):
    records = []
    for name, n in SIZES:
        s = rng.choice(list("ACGT"), size=n, p=(0.3, 0.2, 0.2, 0.3))
        if n >= 150:
            low = rng.integers(0, n - 40)
            s[low:low + 40] = np.char.lower(s[low:low + 40])
            gap = rng.integers(0, n - 25)
            s[gap:gap + 25] = "N"
            for k, ch in enumerate("RYSWKMBDHVryswkmbdhvn"):
                s[(n // 3 + 7 * k) % n] = ch
        records.append((name, "".join(s).encode()))
    return records


def fasta_text(records, width=70):
    return "".join(">%s some description\n%s\n" % (n, "\n".join(s.decode()[i:i + width] for i in range(0, len(s), width))) for n, s in records)


def build():
    sio, cor, ast = import_reference()
    from instagraal_amd import scaffold_polish as sp

    rng = np.random.default_rng(SEED)
    records = make_genome(rng)
    out = {"names": np.array([n for n, _ in records]), "seq": np.frombuffer(b"\0".join(s for _, s in records), np.uint8)}
    with tempfile.TemporaryDirectory() as tmp:
        fa, frags = os.path.join(tmp, "genome.fa"), os.path.join(tmp, "info_frags.txt")
        with open(fa, "w") as fh:
            fh.write(fasta_text(records))
        with open(frags, "w") as fh:
            fh.write(sp.info_frags_text({k: [list(b) for b in v] for k, v in SCAFFOLDS.items()}))
        out["info_frags"] = np.frombuffer(open(frags, "rb").read(), np.uint8)
        parsed = sio.parse_info_frags(frags)

        def text(scaffolds):
            path = os.path.join(tmp, "out.txt")
            sio.write_info_frags(scaffolds, output=path)
            return np.frombuffer(open(path, "rb").read(), np.uint8)

        def lost_arrays(lost):
            rows = [(k, b[1], b[2], b[3], b[4]) for k, v in lost.items() for b in v]
            return np.array([r[0] for r in rows]), np.array([r[1:] for r in rows], np.int64).reshape(len(rows), 4)

        fresh = lambda: copy.deepcopy(parsed)  # noqa: E731  (the reference's reorient writes into the bins it is given)
        out["parsed"] = text(fresh())
        out["singleton"] = text(cor.remove_spurious_insertions(fresh()))
        for c in CRITERIA:
            out["inversion_" + c] = text(cor.correct_spurious_inversions(fresh(), c))
        out["rearrange"] = text(cor.rearrange_intra_scaffolds(fresh()))
        out["inversion2_blocks"] = text(cor.reorient_consecutive_blocks(fresh(), "blocks"))
        out["inversion2_sequences"] = text(cor.reorient_consecutive_blocks(fresh(), "sequences"))
        lost = cor.find_lost_dna(fa, fresh())
        out["lost_names"], out["lost_bins"] = lost_arrays(lost)
        lost_path = os.path.join(tmp, "lost.fa")
        cor.find_lost_dna(fa, fresh(), output_file=lost_path)
        out["lost_fasta"] = np.frombuffer(open(lost_path, "rb").read(), np.uint8)
        out["reincorporation"] = text(cor.integrate_lost_dna(fresh(), lost))
        arranged = cor.reorient_consecutive_blocks(cor.rearrange_intra_scaffolds(fresh()))
        lost2 = cor.find_lost_dna(fa, arranged)
        out["polishing_lost_names"], out["polishing_lost_bins"] = lost_arrays(lost2)
        out["polishing"] = text(cor.integrate_lost_dna(arranged, lost2))
        toy = {"toy": [["ctgA", 0, 0, 100, 1], ["ctgA", 1, 100, 200, 1], ["ctgA", 3, 300, 400, 1]]}
        toy_lost = cor.find_lost_dna(fa, toy)
        out["toy_lost_names"], out["toy_lost_bins"] = lost_arrays({"ctgA": toy_lost["ctgA"]})
        out["toy_integrated"] = text(cor.integrate_lost_dna(copy.deepcopy(toy), {"ctgA": toy_lost["ctgA"]}))
        stats = ast.compute_assembly_stats(fa)
        out["stats_keys"] = np.array(list(stats))
        out["stats_values"] = np.array([float(v) for v in stats.values()], np.float64)
        out["stats_text"] = np.array(ast.format_assembly_stats(stats, label="Assembly (polishing mode)"))
        out["stats_text_plain"] = np.array(ast.format_assembly_stats(stats))
        half = [(n, s[:len(s) // 2 + 1]) for n, s in records[:5]]
        with open(fa, "w") as fh:
            fh.write(fasta_text(half))
        stats2 = ast.compute_assembly_stats(fa)
        out["stats2_values"] = np.array([float(v) for v in stats2.values()], np.float64)
        out["stats2_records"] = np.int64(5)
        out["comparison"] = np.array(ast.format_comparison_table({"input": stats, "a rather long label": stats2}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true", help="compare with the file that is there and write nothing")
    a = ap.parse_args()
    data = build()
    path = os.path.join(a.out, NAME + ".npz")
    if a.check:
        have = np.load(path)
        bad = [k for k in data if k not in have.files or not np.array_equal(have[k], data[k])] + [k for k in have.files if k not in data]
        print("golden %s: %s" % (path, "differs in " + ", ".join(bad) if bad else "up to date"))
        return 1 if bad else 0
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(data)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
