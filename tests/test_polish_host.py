"""The rule of the polish step (instagraal_amd/scaffold_polish.py, assembly_stats.py) on the host, no GPU: every
correction, the lost DNA and its integration and the statistics against tests/golden/polish_tiny.npz, which tools/gen_golden_polish.py
made with the reference's own functions; ``find_lost_dna`` against a per-base brute force; the ``once`` integration against its claim
(every input base exactly once); ``stitch`` against a per-bin string build; the reference's own expectations of ``write_fasta`` on the
parsed records; every refusal; the command line in a subprocess."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from instagraal_amd import assembly_stats as ast
from instagraal_amd import pre
from instagraal_amd import scaffold_polish as sp

GOLDEN = os.path.join(ROOT, "tests", "golden", "polish_tiny.npz")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    g["records"] = list(zip([str(n) for n in g["names"]], bytes(g["seq"]).split(b"\0")))
    return g


@pytest.fixture()
def folder(golden, tmp_path):
    fa, frags = tmp_path / "genome.fa", tmp_path / "info_frags.txt"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in golden["records"]))
    frags.write_bytes(bytes(golden["info_frags"]))
    return str(fa), str(frags)


def _text(g, key):
    return bytes(g[key]).decode()


def _lost(g, prefix):
    out = {}
    for name, b in zip(g[prefix + "_names"], g[prefix + "_bins"]):
        out.setdefault(str(name), []).append([str(name)] + [int(x) for x in b])
    return out


def naive_fasta(records, scaffolds, junction="", width=60):
    """the reference's write_fasta as strings: a slice per bin, Biopython's complement, lines of ``width``"""
    comp = {**pre.COMPLEMENT, **{k.lower(): v.lower() for k, v in pre.COMPLEMENT.items()}}
    seqs = {n: s.decode() for n, s in records}
    out = []
    for name, scaffold in scaffolds.items():
        body, previous = "", None
        for contig, _, a, b, ori in scaffold:
            if junction and previous not in {None, contig}:
                body += junction
            part = seqs[contig][a:b]
            body += part if ori == 1 else "".join(comp[ch] for ch in reversed(part))
            previous = contig
        out.append(">%s\n" % name + "".join(body[i:i + width] + "\n" for i in range(0, len(body), width)))
    return "".join(out).encode()


def parse_fasta_bytes(data):
    return {r.split(b"\n", 1)[0].decode(): r.split(b"\n", 1)[1].replace(b"\n", b"") for r in data.split(b">")[1:]}


# ---------------------------------------------------------------- against the reference's functions
def test_parse_and_write_reproduce_the_reference(golden, folder):
    parsed = sp.parse_info_frags(folder[1])
    assert sp.info_frags_text(parsed) == _text(golden, "parsed") == _text(golden, "info_frags")
    assert list(parsed)[0] == "inversions" and parsed["inversions"][2] == ["contig1", 3, 300, 400, -1]


@pytest.mark.parametrize("key,call", [
    ("singleton", lambda s: sp.remove_spurious_insertions(s)),
    ("inversion_cis", lambda s: sp.correct_spurious_inversions(s, "cis")),
    ("inversion_colinear", lambda s: sp.correct_spurious_inversions(s, "colinear")),
    ("inversion_contiguous", lambda s: sp.correct_spurious_inversions(s, "contiguous")),
    ("rearrange", lambda s: sp.rearrange_intra_scaffolds(s)),
    ("inversion2_blocks", lambda s: sp.reorient_consecutive_blocks(s, "blocks")),
    ("inversion2_sequences", lambda s: sp.reorient_consecutive_blocks(s, "sequences")),
])
def test_the_corrections_give_the_references_results(golden, folder, key, call):
    parsed = sp.parse_info_frags(folder[1])
    before = sp.info_frags_text(parsed)
    assert sp.info_frags_text(call(parsed)) == _text(golden, key)
    assert sp.info_frags_text(parsed) == before  # the input is left as it was
    assert _text(golden, key) != before or key == "inversion_contiguous"


def test_the_golden_holds_the_cases_it_is_there_for(golden):
    t = {k: _text(golden, k) for k in ("parsed", "singleton", "inversion_cis", "inversion_colinear", "inversion_contiguous", "rearrange", "inversion2_blocks")}
    assert len({t["inversion_cis"], t["inversion_colinear"], t["inversion_contiguous"]}) == 3  # the three criteria differ
    for gone in ("ctgB\t7\t", "ctgB\t8\t", "contig2\t9\t", "ctgB\t9\t"):  # the insertions at the first, a middle and the last place
        assert gone in t["parsed"] and gone not in t["singleton"]
    assert t["rearrange"].index("ctgD\t4\t") < t["rearrange"].index("ctgB\t10\t")  # the tie of two groups of two goes to the first
    assert "ctgB\t12\t1\t300\t400\nctgB\t13\t1\t400\t500\n" in t["inversion2_blocks"]  # a sum of 0 goes to +
    assert len(golden["records"]) == 8 and min(len(s) for _, s in golden["records"]) == 1


def test_find_lost_dna_against_the_reference_and_a_brute_force(golden, folder):
    records = golden["records"]
    parsed = sp.parse_info_frags(folder[1])
    lost = sp.find_lost_dna(records, parsed)
    assert lost == _lost(golden, "lost") and list(lost) == list(_lost(golden, "lost"))
    assert sp.lost_dna_text(records, lost) == _text(golden, "lost_fasta")
    brute = {}
    for name, seq in sorted(records, key=lambda r: len(r[1]), reverse=True):
        left = np.ones(len(seq), bool)
        for s in parsed.values():
            for contig, _, a, b, _ in s:
                if contig == name:
                    left[a:b + 1] = False
        edges = np.flatnonzero(np.diff(np.concatenate(([0], left.view(np.int8), [0]))))
        if edges.size:
            brute[name] = [[name, -1, int(a), int(b), 1] for a, b in edges.reshape(-1, 2)]
    assert lost == brute
    assert "ctgUntouched" in lost and lost["ctgUntouched"] == [["ctgUntouched", -1, 0, 150, 1]]
    # the toy of the issue: the base at a bin's end goes with the bin
    toy = {"toy": [["ctgA", 0, 0, 100, 1], ["ctgA", 1, 100, 200, 1], ["ctgA", 3, 300, 400, 1]]}
    toy_lost = {"ctgA": sp.find_lost_dna(records, toy)["ctgA"]}
    assert toy_lost == _lost(golden, "toy_lost") == {"ctgA": [["ctgA", -1, 201, 300, 1]]}
    assert sp.info_frags_text(sp.integrate_lost_dna(toy, toy_lost)) == _text(golden, "toy_integrated")
    assert "ctgA\t-1\t1\t200\t301\n" in _text(golden, "toy_integrated") and "ctgA\t-1\t1\t201\t300\n" in _text(golden, "toy_integrated")


def test_the_reference_integration_and_the_whole_polishing(golden, folder):
    records = golden["records"]
    parsed = sp.parse_info_frags(folder[1])
    assert sp.info_frags_text(sp.integrate_lost_dna(parsed, sp.find_lost_dna(records, parsed))) == _text(golden, "reincorporation")
    arranged = sp.reorient_consecutive_blocks(sp.rearrange_intra_scaffolds(parsed))
    lost = sp.find_lost_dna(records, arranged)
    assert lost == _lost(golden, "polishing_lost")
    assert sp.info_frags_text(sp.integrate_lost_dna(arranged, lost)) == _text(golden, "polishing")


def test_polish_assembly_writes_the_references_files(golden, folder, tmp_path):
    for mode, key in (("singleton", "singleton"), ("inversion", "inversion_colinear"), ("inversion2", "inversion2_blocks"), ("rearrange", "rearrange"),
                      ("reincorporation", "reincorporation"), ("polishing", "polishing")):
        out = tmp_path / mode
        r = sp.polish_assembly(folder[1], folder[0], str(out), mode=mode, device=False)
        assert (out / "new_info_frags.txt").read_text() == _text(golden, key), mode
        assert ("polished_genome.fa" in r["files"]) == (mode == "polishing") and ("lost_dna.fa" in r["files"]) == (mode in ("reincorporation", "polishing"))
    r = sp.polish_assembly(folder[1], folder[0], str(tmp_path / "c"), mode="inversion", criterion="cis", device=False)
    assert (tmp_path / "c" / "new_info_frags.txt").read_text() == _text(golden, "inversion_cis")
    out = tmp_path / "polishing"
    new = sp.parse_info_frags(str(out / "new_info_frags.txt"))
    got = parse_fasta_bytes((out / "polished_genome.fa").read_bytes())
    assert got == parse_fasta_bytes(naive_fasta(golden["records"], new))  # what the reference's write_fasta makes of that file, as parsed records
    r = sp.polish_assembly(folder[1], folder[0], str(out), mode="polishing", device=False)
    assert r["bases_duplicated"] > 0 and r["bases_input"] == sum(len(s) for _, s in golden["records"])  # the reference's integration puts bases in twice
    assert r["composition"][:, 7].sum() == sum(len(s) for s in got.values()) == r["bases_input"] - r["bases_lost"] + r["bases_duplicated"]
    assert "N50 (bp)" in (out / "assembly_stats.txt").read_text()
    # the fasta mode stitches the file it is given; the filters drop scaffolds
    r = sp.polish_assembly(folder[1], folder[0], str(tmp_path / "f"), mode="fasta", junction="NNNNNN", device=False)
    assert (tmp_path / "f" / "polished_genome.fa").read_bytes() == naive_fasta(golden["records"], sp.parse_info_frags(folder[1]), junction="NNNNNN")
    assert not (tmp_path / "f" / "new_info_frags.txt").exists()
    r = sp.polish_assembly(folder[1], None, str(tmp_path / "s"), mode="rearrange", min_scaffold_size=2, min_scaffold_length=400)
    assert (r["scaffolds_in"], r["scaffolds_kept"]) == (12, 6) and "one_bin" not in r["scaffolds"] and "two_bins" not in r["scaffolds"]


# ---------------------------------------------------------------- the once integration and the accounting
def test_once_puts_every_input_base_back_exactly_once(golden):
    records = golden["records"]
    rng = np.random.default_rng(5)
    scaffolds, k = {}, 0
    for name, seq in records:
        if name == "ctgUntouched":
            continue
        cuts = np.unique(np.concatenate(([0, len(seq)], rng.integers(0, len(seq) + 1, 9))))
        for a, b in zip(cuts[:-1], cuts[1:]):
            if rng.random() < 0.7:  # the other stretches are lost: at a record's first base, its last, between two bins, one base long
                scaffolds.setdefault("s%d" % (k % 5), []).append([name, k, int(a), int(b), 1 if rng.random() < 0.5 else -1])
                k += 1
    scaffolds["gap1"] = []
    before = sp.coverage(records, scaffolds)
    assert before["bases_lost"] > 150 and before["bases_duplicated"] == 0
    new = sp.integrate_lost_dna(scaffolds, None, mode="once", records=records)
    after = sp.coverage(records, new)
    assert after == dict(bases_input=before["bases_input"], bases_covered_once=before["bases_input"], bases_lost=0, bases_duplicated=0)
    assert "ctgUntouched_0_150" in new
    # the stitched genome, parsed back, holds every input record's bases exactly once: each base is marked where its bin says it came from
    image, counts = sp.stitch(records, sp.stitch_plan(records, new))
    got = parse_fasta_bytes(bytes(image))
    seen = {n: np.zeros(len(s), np.int64) for n, s in records}
    comp = bytes(sp.COMPLEMENT)
    for name, scaffold in new.items():
        at = 0
        for contig, _, a, b, ori in scaffold:
            piece = dict(records)[contig][a:b]
            assert got[name][at:at + b - a] == (piece if ori == 1 else piece[::-1].translate(comp))
            seen[contig][a:b] += 1
            at += b - a
        assert at == len(got[name])
    assert all((v == 1).all() for v in seen.values())
    assert np.array_equal(counts.sum(0)[4:], sp.composition(records).sum(0)[4:])  # N, other, lower and all bases survive a reverse complement
    # a stretch goes next to the bin it abuts, in that bin's orientation
    s = {"x": [["ctgA", 0, 100, 200, -1]]}
    assert sp.integrate_lost_dna_once([("ctgA", b"A" * 400)], s)["x"] == [["ctgA", -1, 200, 400, -1], ["ctgA", 0, 100, 200, -1], ["ctgA", -1, 0, 100, -1]]
    with pytest.raises(ValueError, match="records"):
        sp.integrate_lost_dna(scaffolds, None, mode="once")
    with pytest.raises(ValueError, match="neither"):
        sp.integrate_lost_dna(scaffolds, {}, mode="twice")


def test_coverage_counts_duplicates_and_losses():
    records = [("a", b"ACGTACGTAC"), ("b", b"GG")]
    s = {"s": [["a", 0, 0, 4, 1], ["a", 1, 2, 6, 1], ["a", 2, 2, 3, -1]]}
    assert sp.coverage(records, s) == dict(bases_input=12, bases_covered_once=4, bases_lost=6, bases_duplicated=3)


# ---------------------------------------------------------------- stitching
@pytest.mark.parametrize("width", [1, 59, 60, 61])
@pytest.mark.parametrize("junction", ["", "NNNNNN"])
def test_stitch_is_the_per_bin_string_build(golden, folder, width, junction):
    records = golden["records"]
    scaffolds = sp.parse_info_frags(folder[1])
    scaffolds["past_the_end"] = [["ctgA", 0, 390, 450, -1], ["ctgB", 1, 2000, 2100, 1], ["ctgA", 2, 0, 61, 1]]  # clipped as a slice clips, one of them to nothing
    scaffolds["empty"] = []
    plan = sp.stitch_plan(records, scaffolds, junction=junction, width=width)
    image, counts = sp.stitch(records, plan)
    want = naive_fasta(records, scaffolds, junction=junction, width=width)
    assert bytes(image) == want and plan["file_bytes"] == len(want) and plan["pieces_clipped"] == 2
    bodies = parse_fasta_bytes(want)
    assert [int(x) for x in plan["body_len"]] == [len(bodies[n]) for n in plan["names"]]
    for j, name in enumerate(plan["names"]):
        assert np.array_equal(counts[j], sp.composition([(name, bodies[name])])[0])
        at = int(plan["rec_off"][j]) + int(plan["hdr_len"][j])
        L = int(plan["body_len"][j])
        assert int(plan["rec_off"][j + 1]) - at == L + -(-L // width)
    assert plan["rec_off"].dtype == plan["body"].dtype == plan["start"].dtype == np.int64


def test_composition_and_complement_tables():
    comp = sp.composition([("r", b"ACGTNacgtnRYSWKMBDHVryswkmbdhv")])[0]
    assert dict(zip(sp.CLASSES, comp.tolist())) == dict(A=2, C=2, G=2, T=2, N=2, other=20, lower=15, bases=30)
    fwd = b"ABCDGHKMNRSTVWYabcdghkmnrstvwy"
    assert fwd.translate(bytes(sp.COMPLEMENT)) == b"TVGHCDMKNYSABWRtvghcdmknysabwr"
    assert fwd.translate(bytes(sp.COMPLEMENT)).translate(bytes(sp.COMPLEMENT)) == fwd


def test_the_references_expectations_of_write_fasta(tmp_path):
    simple = {"scaffold1": [["ctgA", 0, 0, 100, 1], ["ctgA", 1, 100, 200, 1], ["ctgA", 2, 200, 300, 1]], "scaffold2": [["ctgB", 0, 0, 150, 1], ["ctgB", 1, 150, 300, -1]]}
    records = [("ctgA", b"A" * 300), ("ctgB", b"C" * 300)]
    got = parse_fasta_bytes(bytes(sp.stitch(records, sp.stitch_plan(records, simple))[0]))
    assert len(got["scaffold1"]) == 300 and len(got["scaffold2"]) == 300 and got["scaffold2"] == b"C" * 150 + b"G" * 150
    records = [("ctgA", b"AAAA"), ("ctgB", b"CCCC")]
    got = parse_fasta_bytes(bytes(sp.stitch(records, sp.stitch_plan(records, {"s1": [["ctgA", 0, 0, 4, 1]], "s2": [["ctgB", 0, 0, 4, -1]]}))[0]))
    assert got == {"s1": b"AAAA", "s2": b"GGGG"}
    with gzip.open(tmp_path / "ref.fa.gz", "wt") as fh:
        fh.write(">ctgA\n" + "ACGT" * 25 + "\n")
    sp.write_info_frags({"s1": [["ctgA", 0, 0, 100, 1]]}, str(tmp_path / "info_frags.txt"))
    sp.polish_assembly(str(tmp_path / "info_frags.txt"), str(tmp_path / "ref.fa.gz"), str(tmp_path / "out"), mode="fasta", device=False)
    assert (tmp_path / "out" / "polished_genome.fa").read_bytes() == b">s1\n" + b"ACGT" * 15 + b"\n" + b"ACGT" * 10 + b"\n"


# ---------------------------------------------------------------- refusals
def test_every_refusal(golden, folder, tmp_path):
    def frags(text):
        p = tmp_path / "bad.txt"
        p.write_text(text)
        return str(p)

    head = ">s\ninit_contig\tid_frag\torientation\tstart\tend\nctgA\t0\t1\t0\t100\n"
    for line, what in (("ctgA\t1\t1\t100\t100\n", "line 4.*from 100 to 100"), ("ctgA\t1\t1\t-1\t100\n", "line 4.*from -1"), ("ctgA\t1\t0\t100\t200\n", "line 4.*orientation 0"),
                       ("ctgA\t1\t1\t100\n", "line 4.*not a bin"), ("ctgA\tx\t1\t100\t200\n", "line 4.*not a bin")):
        with pytest.raises(ValueError, match=what):
            sp.parse_info_frags(frags(head + line))
    with pytest.raises(ValueError, match="line 1"):
        sp.parse_info_frags(frags("ctgA\t1\t1\t100\t200\n"))
    records = golden["records"]
    with pytest.raises(ValueError, match="not in the FASTA"):
        sp.stitch_plan(records, {"s": [["nobody", 0, 0, 10, 1]]})
    with pytest.raises(ValueError, match="orientation"):
        sp.stitch_plan(records, {"s": [["ctgA", 0, 0, 10, 0]]})
    with pytest.raises(ValueError, match="from 10 to 10"):
        sp.stitch_plan(records, {"s": [["ctgA", 0, 10, 10, 1]]})
    with pytest.raises(ValueError, match="at least one base"):
        sp.stitch_plan(records, {}, width=0)
    with pytest.raises(ValueError, match="orientation"):
        sp.info_frags_text({"s": [["ctgA", 0, 0, 10, 2]]})
    with pytest.raises(ValueError, match="criterion"):
        sp.correct_spurious_inversions({"s": []}, "nearby")
    with pytest.raises(ValueError, match="neither"):
        sp.reorient_consecutive_blocks({"s": []}, "bins")
    for kw, what in ((dict(mode="shine"), "mode"), (dict(lost="twice"), "lost="), (dict(mode="polishing"), "FASTA"), (dict(mode="fasta"), "FASTA"), (dict(mode="reincorporation"), "FASTA")):
        with pytest.raises(ValueError, match=what):
            sp.polish_assembly(folder[1], None, str(tmp_path / "o"), **kw)
    bad = tmp_path / "bad.fa"
    bad.write_text(">r\nACGU\n")
    with pytest.raises(ValueError, match="not one of"):
        sp.polish_assembly(folder[1], str(bad), str(tmp_path / "o"), device=False)


# ---------------------------------------------------------------- the command line
def test_the_command_line_in_a_subprocess(golden, folder, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "instagraal_amd.scaffold_polish"]
    r = subprocess.run(cmd + ["-i", folder[1], "-f", folder[0], "-o", str(tmp_path / "cli"), "-j", "NNNNNN", "--lost", "once", "--host", "-s", "0", "-l", "0"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Assembly (polishing mode)" in r.stdout and "12 of 12 scaffolds" in r.stdout
    want = sp.polish_assembly(folder[1], folder[0], str(tmp_path / "api"), junction="NNNNNN", lost="once", device=False)
    for name in ("new_info_frags.txt", "polished_genome.fa", "lost_dna.fa", "assembly_stats.txt"):
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "api" / name).read_bytes(), name
    assert want["bases_lost"] == 0 and want["bases_duplicated"] == 0
    r = subprocess.run(cmd + ["-m", "INVERSION", "-c", "cis", "-i", folder[1], "-o", str(tmp_path / "cli2")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and (tmp_path / "cli2" / "new_info_frags.txt").read_text() == _text(golden, "inversion_cis")
    r = subprocess.run(cmd + ["-i", folder[1], "-o", str(tmp_path / "cli3")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "FASTA" in r.stderr
    r = subprocess.run(cmd + ["-i", str(tmp_path / "nothing.txt")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no such file" in r.stderr


# ---------------------------------------------------------------- statistics
def test_the_statistics_are_the_references(golden, folder, tmp_path):
    stats = ast.compute_assembly_stats(folder[0])
    assert list(stats) == [str(k) for k in golden["stats_keys"]] == list(ast.KEYS)
    assert [float(v) for v in stats.values()] == golden["stats_values"].tolist()
    assert isinstance(stats["n50"], int) and isinstance(stats["mean_length"], float)
    assert ast.format_assembly_stats(stats, label="Assembly (polishing mode)") == str(golden["stats_text"])
    assert ast.format_assembly_stats(stats) == str(golden["stats_text_plain"])
    comp = sp.composition(golden["records"])
    assert ast.compute_assembly_stats(comp[:, 7], comp[:, 1] + comp[:, 2]) == stats  # from lengths and G+C counts
    half = [(n, s[:len(s) // 2 + 1]) for n, s in golden["records"][:int(golden["stats2_records"])]]
    comp2 = sp.composition(half)
    stats2 = ast.compute_assembly_stats(comp2[:, 7], comp2[:, 1] + comp2[:, 2])
    assert [float(v) for v in stats2.values()] == golden["stats2_values"].tolist()
    assert ast.format_comparison_table({"input": stats, "a rather long label": stats2}) == str(golden["comparison"])
    (tmp_path / "e.fa").write_text(">a\n\n>b\n")
    empty = ast.compute_assembly_stats(str(tmp_path / "e.fa"))
    assert empty["n_contigs"] == 0 and empty["gc_content"] == 0.0 and ast.compute_assembly_stats([0], [0]) == empty
    with gzip.open(tmp_path / "g.fa.gz", "wt") as fh:
        fh.write(open(folder[0]).read())
    assert ast.compute_assembly_stats(str(tmp_path / "g.fa.gz")) == stats
