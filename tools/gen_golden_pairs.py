#!/usr/bin/env python3
"""Generate tests/golden/pairs_lift_tiny.npz by running the REFERENCE's own ``post`` functions on a small assembly and pairs file.

Needs the reference checkout beside the repository, like tools/gen_golden.py.  The reference's ``instagraal.post`` is
imported unmodified; the two modules it wants and that may be absent (``cooler``, ``Bio``) are then replaced by inert stand-ins in
``sys.modules`` (nothing of them is called by the functions used here).  The state is ``tiny``, bombed, behind seeded moves of the CPU oracle
that leave flipped bins and joined contigs, plus one scaffold with an inactive bin; ``io_frags.write_assembly`` writes its
``info_frags.txt``; the pairs file is a few thousand seeded lines that hit every interval's first and last base and the bases on
either side, name a contig the table does not have, hold a malformed line, carry a ``#columns:`` header in another order and use all
four strand combinations.  Then ``parse_info_frags``, ``_build_new_bins(junction_len=0)``, ``_build_liftover_index``,
``_pos_to_new_coords``, ``_pairs_to_lifted_pixels``, ``_pairs_to_fixed_bin_pixels`` over ``_binnify``, ``_write_lifted_pairs`` and
``_compute_ps`` run as they are.

Only data is stored: the state arrays, the input pairs as integers with the name list, the reference's lifted coordinates, its pixels,
its totals, its P(s) table and the break positions and bin widths it used (settings).

usage:  python tools/gen_golden_pairs.py [--out tests/golden] [--check]
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

NAME = "pairs_lift_tiny"
SEED, N_MOVES, N_RANDOM = 31, 150, 1500
BINSIZES = (1000, 7919)
COLUMNS = ("readID", "strand1", "strand2", "chr1", "pos1", "chr2", "pos2")


class _StandIn(types.ModuleType):
    """an absent module: any attribute is another stand-in, a call returns its first argument"""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandIn(self.__name__ + "." + k)

    def __call__(self, *a, **k):
        return a[0] if a else None


def import_reference_post():
    for name in ("cooler", "Bio", "Bio.Seq", "Bio.SeqIO", "Bio.SeqRecord"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _StandIn(name)
    import matplotlib

    matplotlib.use("Agg")
    from instagraal import post

    return post


def make_state():
    """tiny, bombed, behind seeded oracle moves; one bin of a scaffold of several bins made inactive -> (problem, state 17 x N)"""
    from instagraal_amd import synth
    from oracle import oracle_lib as ol
    from oracle.sampler_oracle import OracleSampler

    ol.build()
    prob = synth.make_problem(*synth.CONFIGS["tiny"])
    o = OracleSampler(**prob.sampler_kwargs(), mode=ol.MODE_DET)
    o.set_param_simu(prob.params)
    o.eval_likelihood_init()
    np.random.seed(SEED)
    o.bomb_the_genome()  # (every bin a contig of its own: what the moves then join is the assembly)
    frags = np.arange(prob.n_frags)
    np.random.shuffle(frags)
    for f in frags[:N_MOVES]:
        o.step_sampler(int(f), 5, o.dt)
    state = o.gpu_vect_frags.soa17().copy()
    id_c, ori = state[2], state[13]
    ids, sizes = np.unique(id_c, return_counts=True)
    assert (ori == -1).sum() >= 3, "the moves left no flipped bins"
    assert (sizes >= 2).sum() >= 3 and np.any(ori[np.isin(id_c, ids[sizes >= 2])] == -1), "the moves joined no contigs"
    victim = np.nonzero(id_c == ids[sizes >= 3][0])[0][1]
    state[15, victim] = 0
    return prob, state


def write_pairs(path, table, names, rng):
    """-> the parsed lines as integers: c1, p1, c2, p2, strands (what a reader makes of the file), and the malformed count"""
    iv = table["intervals"]
    ids = np.unique(iv["src_contig"])
    ends = {int(c): int(iv["src_end"][iv["src_contig"] == c].max()) for c in ids}

    def anywhere(n):
        c = rng.choice(ids, size=n)
        return c, np.array([rng.integers(1, ends[int(x)] + 1) for x in c], np.int64)

    edge_c = np.repeat(iv["src_contig"], 4)
    edge_p = np.stack([iv["src_start"], iv["src_start"] + 1, iv["src_end"], iv["src_end"] + 1], axis=1).ravel()
    oc, op = anywhere(edge_c.size)
    flip = rng.random(edge_c.size) < 0.5  # the edge is end 1 or end 2
    c1, p1 = np.where(flip, oc, edge_c), np.where(flip, op, edge_p)
    c2, p2 = np.where(flip, edge_c, oc), np.where(flip, edge_p, op)
    rc1, rp1 = anywhere(N_RANDOM)
    cis = rng.random(N_RANDOM) < 0.7
    rc2, rp2 = anywhere(N_RANDOM)
    rc2 = np.where(cis, rc1, rc2)
    rp2 = np.where(cis, np.array([rng.integers(1, ends[int(x)] + 1) for x in rc1], np.int64), rp2)
    c1, p1, c2, p2 = (np.concatenate(x) for x in ((c1, rc1), (p1, rp1), (c2, rc2), (p2, rp2)))
    by = rng.permutation(c1.size)
    c1, p1, c2, p2 = c1[by], p1[by], c2[by], p2[by]
    strands = rng.integers(0, 4, size=c1.size).astype(np.uint8)
    strands[:4] = (0, 1, 2, 3)
    name_of = {v: k for k, v in names.items()}
    col = {k: COLUMNS.index(k) for k in COLUMNS}
    rows, malformed = [], 0
    with open(path, "w") as f:
        f.write("## pairs format v1.0\n#sorted: chr1-chr2-pos1-pos2\n#shape: upper triangle\n#genome_assembly: synthetic tiny\n")
        for c in ids:
            f.write("#chromsize: %s %d\n" % (name_of[int(c)], ends[int(c)]))
        f.write("#columns: " + " ".join(COLUMNS) + "\n")
        for k in range(c1.size):
            parts = [""] * len(COLUMNS)
            n1, n2 = name_of[int(c1[k])], name_of[int(c2[k])]
            q1, q2 = str(int(p1[k])), str(int(p2[k]))
            unknown = k == 17
            if unknown:
                n2 = "ctg_not_in_the_table"
            if k == 40:
                q1 = "12x"
            parts[col["readID"]], parts[col["chr1"]], parts[col["pos1"]], parts[col["chr2"]], parts[col["pos2"]] = "r%d" % k, n1, q1, n2, q2
            parts[col["strand1"]], parts[col["strand2"]] = "+-"[strands[k] & 1], "+-"[(strands[k] >> 1) & 1]
            f.write("\t".join(parts) + "\n")
            if k == 40:
                malformed += 1
                continue
            rows.append((int(c1[k]), int(p1[k]), -1 if unknown else int(c2[k]), int(p2[k]), int(strands[k])))
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4].astype(np.uint8), malformed


def pixels_arrays(df):
    return (np.asarray(df["bin1_id"], np.int64), np.asarray(df["bin2_id"], np.int64), np.asarray(df["count"], np.int64))


def generate(outdir):
    from instagraal_amd import io_frags, pairs_lift as pl

    post = import_reference_post()
    prob, state = make_state()
    soa, sub = prob.S_o_A_frags, prob.S_o_A_sub_frags
    n_contigs = int(np.max(sub["id_c"]))
    names = {"ctg%d" % c: c for c in range(1, n_contigs + 1)}
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    table = pl.table_of_state(state, prob.np_sub_frags_id, parent, sub["id_c"], sub["len_bp"], names=names)
    rng = np.random.default_rng(SEED)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        # info_frags.txt of the state, through the project's own writer
        vect = types.SimpleNamespace(id_c=state[2], pos=state[0], ori=state[13], activ=state[15], id_d=state[16])
        init_names = ["ctg%d" % c for c in soa["id_c"]]
        start = np.asarray(soa["start_bp"], np.int64)
        end = start + np.asarray(soa["len_bp"], np.int64)
        seqs = {"ctg%d" % c: "A" * int(end[np.asarray(soa["id_c"]) == c].max()) for c in range(1, n_contigs + 1)}
        io_frags.write_assembly(vect, init_names, start.tolist(), end.tolist(), seqs, str(tmp / "genome.fasta"), str(tmp / "info_frags.txt"))
        c1, p1, c2, p2, strands, malformed = write_pairs(tmp / "in.pairs", table, names, rng)

        scaffolds = post.parse_info_frags(str(tmp / "info_frags.txt"))
        bins = post._build_new_bins(scaffolds, junction_len=0)
        index = post._build_liftover_index(bins)
        scaffold_rank = {name: k for k, name in enumerate(scaffolds)}
        name_of = {v: k for k, v in names.items()}
        ref = np.zeros((c1.size, 4), np.int64)
        for k in range(c1.size):
            for e, (c, p) in enumerate(((c1[k], p1[k]), (c2[k], p2[k]))):
                got = post._pos_to_new_coords(name_of.get(int(c), "ctg_not_in_the_table"), int(p), index)
                ref[k, 2 * e], ref[k, 2 * e + 1] = (-1, 0) if got is None else (scaffold_rank[got[0]], got[1])
        frag_px, frag_total = post._pairs_to_lifted_pixels(tmp / "in.pairs", index)
        chromsizes = {}
        for row in bins.itertuples(index=False):
            chromsizes[row.chrom] = max(chromsizes.get(row.chrom, 0), int(row.end))
        fixed = {}
        for B in BINSIZES:
            px, total = post._pairs_to_fixed_bin_pixels(tmp / "in.pairs", index, post._binnify(chromsizes, B))
            fixed[B] = pixels_arrays(px) + (total,)
        n_lines, n_remapped = post._write_lifted_pairs(tmp / "in.pairs", index, bins, tmp / "lifted.pairs.gz")
        ps = post._compute_ps(tmp / "lifted.pairs.gz")
        combos = {"++": 0, "+-": 1, "-+": 2, "--": 3}
        breaks = np.asarray(post._PS_BREAK_POS, np.int64)
        ps_combo = np.array([combos[s] for s in ps["strand_combo"]], np.int64)
        ps_bin = np.searchsorted(breaks, np.asarray(ps["binned_distance"], np.int64))
        assert np.array_equal(breaks[ps_bin], np.asarray(ps["binned_distance"], np.int64))

    out = os.path.join(outdir, NAME + ".npz")
    np.savez_compressed(
        out, config="tiny", seed=SEED, n_moves=N_MOVES, state=state.astype(np.int32),
        sub_ids=np.stack([prob.np_sub_frags_id[k] for k in "xyzw"]).astype(np.int32), parent=parent.astype(np.int32),
        sub_contig=np.asarray(sub["id_c"], np.int32), sub_len_bp=np.asarray(sub["len_bp"], np.int32),
        contig_names=np.array(sorted(names, key=names.get)), contig_ids=np.array(sorted(names.values()), np.int32),
        scaffold_names=np.array(list(scaffolds)), scaffold_sizes=np.array([chromsizes[s] for s in scaffolds], np.int64),
        c1=c1.astype(np.int32), p1=p1.astype(np.int32), c2=c2.astype(np.int32), p2=p2.astype(np.int32), strands=strands, malformed=malformed,
        columns=np.array(COLUMNS), ref_lifted=ref.astype(np.int32),
        frag_bin1=pixels_arrays(frag_px)[0], frag_bin2=pixels_arrays(frag_px)[1], frag_count=pixels_arrays(frag_px)[2], frag_total=frag_total,
        binsizes=np.array(BINSIZES, np.int64),
        **{"fixed%d_%s" % (i, k): v for i, B in enumerate(BINSIZES) for k, v in zip(("bin1", "bin2", "count", "total"), fixed[B])},
        lines=n_lines, remapped=n_remapped, ps_breaks=breaks, ps_binwidth=np.asarray(post._PS_BINWIDTH, np.int64), ps_combo=ps_combo, ps_bin=ps_bin,
        ps_norm_p=np.asarray(ps["norm_p"], np.float64))
    print("wrote", out, os.path.getsize(out), "bytes:", c1.size, "pairs,", n_remapped, "remapped,", len(scaffolds), "scaffolds,", int((state[13] == -1).sum()),
          "reversed bins,", ps_combo.size, "P(s) rows")


def check(a):
    """regenerate into a temporary directory and compare with the committed file, array for array"""
    tmp = tempfile.mkdtemp(prefix="ig_golden_pairs_check_")
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
    print("gen_golden_pairs --check: %d arrays compared, %d differences" % (len(old.files), bad))
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
