#!/usr/bin/env python3
"""Generate tests/golden/pre_tiny.npz by running the REFERENCE's own ``pre`` functions on a small genome and pairs file.

Needs the reference checkout beside the repository, like tools/gen_golden_pairs.py.  The reference's ``instagraal.pre`` is imported
unmodified; the modules it wants and that may be absent (``Bio``, ``cooler``) are replaced by inert stand-ins in ``sys.modules``
(nothing of them is called by the functions used here: the digest itself, which is Biopython's, is NOT run -- the bins come from this
project's digest, ``instagraal_amd.pre.digest``).  The genome is seeded: a handful of records (one of a single base, one shorter than
a site), lower case and runs of N in it, planted sites at the records' first and last bases; the pairs file is a few thousand seeded
lines with position 0, positions beyond a record's end, an unknown record, a ``#columns:`` header in another order and a malformed line.
Then ``_build_bins_with_gc``, ``_pairs_to_pixels``, ``_write_fragments_list``, ``_write_info_contigs`` and ``_write_abs_contacts`` run
as they are; the fragment of single ends comes from ``_pairs_to_pixels`` on files of one line (the end paired with itself).

Only data is stored: the sequence bytes and the records' names, the enzymes' names (settings), the bins, the reference's G+C fractions,
the pairs file and its lines as integers, the reference's pixels and total, the fragments of the single ends, the bytes of the three files.

usage:  python tools/gen_golden_pre.py [--out tests/golden] [--check]
"""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(1, "/root/reference/src")

NAME = "pre_tiny"
SEED, N_RANDOM = 41, 3000
SIZES = (12000, 1, 9000, 300, 3, 15000)
ENZYMES = ("DpnII", "HinfI")
COLUMNS = ("readID", "strand1", "strand2", "chr1", "pos1", "chr2", "pos2")
UNKNOWN = "ctg_not_in_the_fasta"


class _StandIn(types.ModuleType):
    """an absent module: any attribute is another stand-in, a call returns its first argument"""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandIn(self.__name__ + "." + k)

    def __call__(self, *a, **k):
        return a[0] if a else None


def import_reference_pre():
    for name in ("cooler", "Bio", "Bio.Restriction", "Bio.Seq", "Bio.SeqIO", "Bio.SeqRecord"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _StandIn(name)
    import matplotlib

    matplotlib.use("Agg")
    from instagraal import pre

    return pre


def make_genome(rng):
    records = []
    for k, n in enumerate(SIZES):
        s = rng.choice(list("ACGT"), size=n, p=(0.3, 0.2, 0.2, 0.3))
        if n >= 300:
            low = rng.integers(0, n - 40)
            s[low:low + 40] = np.char.lower(s[low:low + 40])
            gap = rng.integers(0, n - 25)
            s[gap:gap + 25] = "N"
            s[n // 2] = "R"
            s[:4] = list("GATC")        # a site at the first base ...
            s[-5:] = list("GAnTC")      # ... and at the last, its N a lower-case n of the sequence
        records.append(("ctg%d" % (k + 1), "".join(s).encode()))
    return records


def write_pairs(path, records, dig, rng):
    """-> c1, p1, c2, p2 of the parsed lines (an unknown record is -1) and the malformed count"""
    R = len(records)
    lens = [len(s) for _, s in records]

    def anywhere(n):
        c = rng.choice(R, size=n, p=np.array(lens) / sum(lens))
        return c, np.array([rng.integers(1, lens[int(x)] + 1) for x in c], np.int64)

    c1, p1 = anywhere(N_RANDOM)
    c2, p2 = anywhere(N_RANDOM)
    near = rng.random(N_RANDOM) < 0.6   # most pairs are close: pixels with more than one pair, and the diagonal
    c2 = np.where(near, c1, c2)
    p2 = np.where(near, np.clip(p1 + rng.integers(-200, 201, N_RANDOM), 1, np.array(lens)[c1]), p2)
    special = [(0, 0, 0, 5), (0, 5, 0, 0), (2, lens[2] + 1, 2, 10), (3, 7, 3, lens[3] + 1000), (1, 1, 1, 1), (1, 2, 4, 3), (4, 1, 5, 1), (0, 0, 0, 0), (5, 10 ** 10, 0, 1)]
    for k, (a, b, c, d) in enumerate(special):
        c1[10 * k + 3], p1[10 * k + 3], c2[10 * k + 3], p2[10 * k + 3] = a, b, c, d
    col = {k: COLUMNS.index(k) for k in COLUMNS}
    rows, malformed = [], 0
    with open(path, "w") as f:
        f.write("## pairs format v1.0\n#sorted: chr1-chr2-pos1-pos2\n#shape: upper triangle\n")
        for (name, _), n in zip(records, lens):
            f.write("#chromsize: %s %d\n" % (name, n))
        f.write("#columns: " + " ".join(COLUMNS) + "\n")
        for k in range(N_RANDOM):
            parts = [""] * len(COLUMNS)
            n1, n2 = records[int(c1[k])][0], records[int(c2[k])][0]
            q1, q2 = str(int(p1[k])), str(int(p2[k]))
            a, b = int(c1[k]), int(c2[k])
            if k == 17:
                n2, b = UNKNOWN, -1
            if k == 29:
                n1, a = UNKNOWN, -1
            if k == 40:
                q1 = "12x"
            parts[col["readID"]], parts[col["chr1"]], parts[col["pos1"]], parts[col["chr2"]], parts[col["pos2"]] = "r%d" % k, n1, q1, n2, q2
            parts[col["strand1"]], parts[col["strand2"]] = "+", "-"
            f.write("\t".join(parts) + "\n")
            if k == 40:
                malformed += 1
                continue
            rows.append((a, int(p1[k]), b, int(p2[k])))
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], malformed


def single_ends(ref, tmp, bins, records, dig):
    """the fragment of single ends by the reference: every fragment's first and last base and the bases on either side, position 0, an
    unknown record -> (record, position, fragment or -1)"""
    recs, poss = [], []
    for f in range(dig["n_frags"]):
        r, s, e = int(dig["frag_rec"][f]), int(dig["start"][f]), int(dig["end"][f])
        for p in (s, s + 1, e, e + 1):
            recs.append(r)
            poss.append(p)
    recs += [-1, 0, 5]
    poss += [4, -3, 10 ** 9]
    out = []
    for r, p in zip(recs, poss):
        name = records[r][0] if r >= 0 else UNKNOWN
        path = tmp / "one.pairs"
        path.write_text("r\t%s\t%d\t%s\t%d\t+\t-\n" % (name, p, name, p))
        px, total = ref._pairs_to_pixels(path, bins)
        out.append(int(px["bin1_id"].iloc[0]) if total else -1)
    return np.array(recs, np.int64), np.array(poss, np.int64), np.array(out, np.int64)


def generate(outdir):
    import pandas as pd

    from instagraal_amd import pre

    ref = import_reference_pre()
    rng = np.random.default_rng(SEED)
    records = make_genome(rng)
    dig = pre.digest(records, list(ENZYMES))
    names = [n for n, _ in records]
    fasta_records = {n: s.decode() for n, s in records}
    bins = pd.DataFrame({"chrom": [names[r] for r in dig["frag_rec"]], "start": dig["start"], "end": dig["end"]})
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        bins_gc = ref._build_bins_with_gc(bins, fasta_records)
        c1, p1, c2, p2, malformed = write_pairs(tmp / "in.pairs", records, dig, rng)
        pixels, total = ref._pairs_to_pixels(tmp / "in.pairs", bins)
        ref._write_fragments_list(bins_gc, tmp / "fragments_list.txt")
        ref._write_info_contigs(bins_gc, fasta_records, tmp / "info_contigs.txt")
        ref._write_abs_contacts(pixels, len(bins), tmp / "abs_fragments_contacts_weighted.txt")
        end_rec, end_pos, end_frag = single_ends(ref, tmp, bins, records, dig)
        files = {k: np.frombuffer((tmp / (k + ".txt")).read_bytes(), np.uint8) for k in ("fragments_list", "info_contigs", "abs_fragments_contacts_weighted")}
        pairs_file = np.frombuffer((tmp / "in.pairs").read_bytes(), np.uint8)
    buf, offs, lens = pre.concatenate(records)
    out = os.path.join(outdir, NAME + ".npz")
    np.savez_compressed(
        out, seed=SEED, names=np.array(names), seq=buf, rec_off=offs, rec_len=lens, enzymes=np.array(ENZYMES), columns=np.array(COLUMNS),
        bins_rec=dig["frag_rec"].astype(np.int32), bins_start=dig["start"].astype(np.int64), bins_end=dig["end"].astype(np.int64),
        ref_gc=np.asarray(bins_gc["gc_content"], np.float64), pairs_file=pairs_file, c1=c1, p1=p1, c2=c2, p2=p2, malformed=malformed,
        ref_bin1=np.asarray(pixels["bin1_id"], np.int64), ref_bin2=np.asarray(pixels["bin2_id"], np.int64), ref_count=np.asarray(pixels["count"], np.int64),
        ref_total=total, end_rec=end_rec, end_pos=end_pos, ref_end_frag=end_frag, file_fragments_list=files["fragments_list"],
        file_info_contigs=files["info_contigs"], file_abs_contacts=files["abs_fragments_contacts_weighted"])
    print("wrote", out, os.path.getsize(out), "bytes:", len(records), "records,", dig["n_frags"], "fragments,", c1.size, "pairs,", total, "kept,", len(pixels), "pixels,",
          end_rec.size, "single ends")


def check(a):
    """regenerate into a temporary directory and compare with the committed file, array for array"""
    tmp = tempfile.mkdtemp(prefix="ig_golden_pre_check_")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--out", tmp], stdout=subprocess.DEVNULL)
    f = NAME + ".npz"
    if not os.path.exists(os.path.join(a.out, f)):
        print("MISSING in %s: %s" % (a.out, f))
        return 1
    new, old = np.load(os.path.join(tmp, f), allow_pickle=False), np.load(os.path.join(a.out, f), allow_pickle=False)
    bad = 0
    if sorted(new.files) != sorted(old.files):
        print("KEYS differ: %s" % sorted(set(new.files) ^ set(old.files)))
        bad += 1
    for k in sorted(set(new.files) & set(old.files)):
        x, y = new[k], old[k]
        if not (x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)):
            print("DIFFERS: %s:%s" % (f, k))
            bad += 1
    print("gen_golden_pre --check: %d arrays compared, %d differences" % (len(old.files), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true", help="regenerate into a temporary directory and compare with the committed file (--out), array for array")
    a = ap.parse_args()
    if a.check:
        sys.exit(check(a))
    os.makedirs(a.out, exist_ok=True)
    a.out = os.path.abspath(a.out)
    os.chdir(tempfile.mkdtemp())  # (the reference's modules may drop a log file in the CWD)
    generate(a.out)


if __name__ == "__main__":
    main()
