"""The rule of the input folder from a FASTA and read pairs (instagraal_amd/pre.py): the digest against an independent statement (Python
``re`` with a look-ahead per site, and a per-base brute force) and hand-written cases; the fragment of a position, the pixels and the
three writers against the golden made by the reference's own functions (tools/gen_golden_pre.py), byte for byte; ``display_matrix``
against a dense brute force; the folder ``run_pre(device=False)`` writes is one the pyramid takes.  No GPU."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from instagraal_amd import pre

GOLDEN = os.path.join(ROOT, "tests", "golden", "pre_tiny.npz")
CLASS = dict(A="A", C="C", G="G", T="T", R="[AG]", Y="[CT]", S="[CG]", W="[AT]", K="[GT]", M="[AC]", B="[CGT]", D="[AGT]", H="[ACT]", V="[ACG]", N=".")


def re_cuts(seq, enzymes):
    """Biopython's pattern restated with ``re``: a look-ahead so that matches overlap, ``.`` for N, a class of plain letters otherwise"""
    text = seq.decode().upper()
    cuts = {0, len(text)}
    for site, cut in enzymes:
        pat = re.compile("(?=(%s))" % "".join(CLASS[ch] for ch in site))
        cuts.update(m.start() + cut for m in pat.finditer(text))
    return sorted(cuts)


def brute_cuts(seq, enzymes):
    text = seq.decode().upper()
    plain = dict(A="A", C="C", G="G", T="T", R="AG", Y="CT", S="CG", W="AT", K="GT", M="AC", B="CGT", D="AGT", H="ACT", V="ACG")
    cuts = {0, len(text)}
    for site, cut in enzymes:
        for s in range(len(text) - len(site) + 1):
            if all(ch == "N" or text[s + j] in plain[ch] for j, ch in enumerate(site)):
                cuts.add(s + cut)
    return sorted(cuts)


def cuts_of(dig, r):
    a, b = int(dig["rec_first"][r]), int(dig["rec_first"][r + 1])
    assert np.array_equal(dig["start"][a + 1:b], dig["end"][a:b - 1]) and np.all(dig["frag_rec"][a:b] == r)
    return [int(x) for x in dig["start"][a:b]] + [int(dig["end"][b - 1])]


def seeded_records(seed, sizes, letters="ACGTacgtNnRY", p=None):
    rng = np.random.default_rng(seed)
    return [("rec%d" % k, "".join(rng.choice(list(letters), size=n, p=p)).encode()) for k, n in enumerate(sizes)]


@pytest.mark.parametrize("specs", [["DpnII"], ["Arima"], ["HinfI", "MseI"], ["G^ANTC", "NlaIII"], ["Csp6I", "DdeI", "EcoRI", "^NN"], ["RY^RY"], ["NNNNNNNN^NNNNNNNN"]])
def test_the_digest_is_the_regular_expression_and_the_brute_force(specs):
    enzymes = pre.expand_enzymes(specs)
    records = seeded_records(5, (1, 2, 3, 4, 5, 63, 64, 65, 300, 2000))
    dig = pre.digest(records, specs)
    for r, (_, seq) in enumerate(records):
        want = re_cuts(seq, enzymes)
        assert want == brute_cuts(seq, enzymes)
        assert cuts_of(dig, r) == want, (r, specs)
    assert dig["n_frags"] == dig["rec_first"][-1] == dig["start"].size and np.array_equal(dig["rec_len"], [len(s) for _, s in records])
    gc = pre.gc_counts(records, dig)
    for f in range(dig["n_frags"]):
        piece = records[dig["frag_rec"][f]][1][int(dig["start"][f]):int(dig["end"][f])].upper()
        assert gc[f] == piece.count(b"G") + piece.count(b"C")


def test_hand_written_digests():
    one = lambda seq, specs: cuts_of(pre.digest([("x", seq)], specs), 0)  # noqa: E731
    assert one(b"GANTCGAGTCGACTC", ["HinfI"]) == [0, 1, 6, 11, 15]  # N in the sequence under the site's N
    assert one(b"GAATCGRATC", ["HinfI"]) == [0, 1, 10]  # R in the sequence under a site's plain letter matches nothing ...
    assert one(b"GARTC", ["HinfI"]) == [0, 1, 5]  # ... under the site's N it does
    assert one(b"NNNN", ["N^N"]) == [0, 1, 2, 3, 4]  # overlapping matches through N
    assert one(b"ANNA", ["^NN"]) == [0, 1, 2, 4]
    assert one(b"GATCAAGATC", ["DpnII"]) == [0, 6, 10]  # a site at the first and at the last base
    assert one(b"AACATG", ["NlaIII"]) == [0, 6]  # a cut equal to the record's length
    assert one(b"CATGATC", ["NlaIII", "DpnII"]) == [0, 3, 4, 7]
    assert one(b"ACATGGATCA", ["NlaIII", "DpnII"]) == [0, 5, 10]  # two enzymes cutting at one position
    assert one(b"gatcGAtc", ["DpnII"]) == [0, 4, 8]  # lower case
    two = pre.digest([("a", b"AAGA"), ("b", b"TCAA")], ["DpnII"])  # a site that would span two records
    assert cuts_of(two, 0) == [0, 4] and cuts_of(two, 1) == [0, 4] and two["rec_first"].tolist() == [0, 1, 2]
    assert pre.gc_counts([("a", b"AAGA"), ("b", b"TCAA")], two).tolist() == [1, 1]
    assert one(b"A", ["DpnII"]) == [0, 1] and one(b"GAT", ["DpnII"]) == [0, 3]


def test_enzymes_and_their_refusals():
    assert pre.enzyme("DpnII") == ("GATC", 0) and pre.enzyme("HinfI") == ("GANTC", 1) and pre.enzyme("NlaIII") == ("CATG", 4) and pre.enzyme("g^antc") == ("GANTC", 1)
    for name in ("DpnII", "MboI", "Sau3AI", "HinfI", "DdeI", "MseI", "NlaIII", "HindIII", "EcoRI", "NcoI", "BglII", "Csp6I"):
        site, cut = pre.enzyme(name)
        assert 0 <= cut <= len(site) <= pre.MAX_SITE
    assert pre.expand_enzymes("Arima") == [("GATC", 0), ("GANTC", 1)] == pre.expand_enzymes(["DpnII", "HinfI"]) == pre.expand_enzymes("DpnII,HinfI")
    with pytest.raises(ValueError, match="Unknown restriction enzyme: 'XyzI'"):
        pre.enzyme("XyzI")
    with pytest.raises(ValueError, match="reverse complement"):
        pre.enzyme("GA^AGA")
    with pytest.raises(ValueError, match="one '\\^'"):
        pre.enzyme("G^AT^C")
    with pytest.raises(ValueError, match="1 .. 16 letters"):
        pre.enzyme("^" + "AT" * 9)
    with pytest.raises(ValueError, match="1 .. 16 letters"):
        pre.enzyme("^")
    with pytest.raises(ValueError, match="no IUPAC letter"):
        pre.enzyme("GA^XTC")
    with pytest.raises(ValueError, match="enzymes"):
        pre.expand_enzymes(["DpnII"] * 5)
    with pytest.raises(ValueError, match="enzymes"):
        pre.expand_enzymes([])
    with pytest.raises(ValueError, match="record 'b', position 3: the character 'X'"):
        pre.digest([("a", b"ACGT"), ("b", b"ACXT")], ["DpnII"])
    with pytest.raises(ValueError, match="record 'a', position 2"):
        pre.digest([("a", b"A-GT")], ["DpnII"])
    with pytest.raises(ValueError, match="empty"):
        pre.digest([("a", b"ACGT"), ("b", b"")], ["DpnII"])
    with pytest.raises(ValueError, match="repeated"):
        pre.digest([("a", b"ACGT"), ("a", b"AC")], ["DpnII"])
    assert pre.site_masks("GANTC").tolist()[:6] == [4, 1, 16, 8, 2, 0] and pre.site_masks("RYB")[:3].tolist() == [5, 10, 14]


def test_the_fasta_reader(tmp_path):
    text = b">one first record\nACGT\nacgt\n\n>two\tx\nNN\n>three\nGATC  \r\n"
    (tmp_path / "a.fa").write_bytes(text)
    with gzip.open(tmp_path / "a.fa.gz", "wb") as f:
        f.write(text)
    want = [("one", b"ACGTacgt"), ("two", b"NN"), ("three", b"GATC")]
    assert pre.read_fasta(tmp_path / "a.fa") == want == pre.read_fasta(str(tmp_path / "a.fa.gz"))
    buf, offs, lens = pre.concatenate(want)
    assert bytes(buf) == b"ACGTacgt\0NN\0GATC\0" and offs.tolist() == [0, 9, 12] and lens.tolist() == [8, 2, 4] and offs.dtype == np.int64


def test_fragment_of_a_position():
    dig = pre.digest([("a", b"AAGATCAAGATCAA"), ("b", b"CCCC")], ["DpnII"])  # a: [0, 2) [2, 8) [8, 14); b: [0, 4)
    rec = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, -1, 2, 0])
    pos = np.array([1, 2, 3, 8, 9, 14, 15, 10 ** 9, 1, 4, 5, 1, 1, 0])
    frag, beyond = pre.fragment_of(dig, rec, pos)
    assert frag.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, -1, -1, -1]
    assert beyond.tolist() == [False] * 6 + [True, True, False, False, True, False, False, False]
    assert pre.fragment_of(dig, [0, 1], [-5, -1])[0].tolist() == [-1, -1]
    px = pre.pixels_host(dig, rec, pos, rec[::-1].copy(), pos[::-1].copy())
    assert px["pairs_in"] == 14 == px["pairs_kept"] + px["end1_without_fragment"] + px["end2_without_fragment"]
    assert px["end1_without_fragment"] == 3 and px["end2_without_fragment"] == 3 and px["ends_beyond_record"] == 6 and px["pixels"] == px["col"].size
    assert int(px["count"].sum()) == px["pairs_kept"] and px["rowptr"][-1] == px["pixels"]


def brute_pixels(f1, f2, n):
    dense = np.zeros((n, n), np.int64)
    for a, b in zip(f1, f2):
        if a >= 0 and b >= 0:
            dense[min(a, b), max(a, b)] += 1
    return dense


def dense_of(px, n):
    dense = np.zeros((n, n), np.int64)
    rows = np.repeat(np.arange(n), np.diff(px["rowptr"]))
    dense[rows, px["col"]] = px["count"]
    return dense


def test_pixels_and_their_merge_against_a_dense_brute_force():
    records = seeded_records(9, (40, 700, 1, 333), "ACGT")
    dig = pre.digest(records, ["MseI", "DpnII"])
    rng = np.random.default_rng(2)
    n = 3000
    c1, c2 = rng.integers(-1, 5, n), rng.integers(-1, 5, n)
    p1, p2 = rng.integers(-2, 760, n), rng.integers(-2, 760, n)
    f1, f2 = pre.fragment_of(dig, c1, p1)[0], pre.fragment_of(dig, c2, p2)[0]
    px = pre.pixels_host(dig, c1, p1, c2, p2)
    want = brute_pixels(f1, f2, dig["n_frags"])
    assert np.array_equal(dense_of(px, dig["n_frags"]), want) and np.all(px["count"] > 0)
    rows = np.repeat(np.arange(dig["n_frags"]), np.diff(px["rowptr"]))
    assert np.all(np.diff(rows * dig["n_frags"] + px["col"]) > 0)  # sorted by (bin1, bin2), no pixel twice
    parts = [pre.pixels_host(dig, c1[a:b], p1[a:b], c2[a:b], p2[a:b]) for a, b in ((0, 1), (1, 1), (1, 2000), (2000, n))]
    merged = pre.merge_pixels(parts, dig["n_frags"])
    for k in ("rowptr", "col", "count"):
        assert np.array_equal(merged[k], px[k]), k
    assert all(merged[k] == px[k] for k in pre.SCALARS)
    empty = pre.merge_pixels([], 7)
    assert empty["rowptr"].tolist() == [0] * 8 and empty["pixels"] == 0


def test_display_matrix_against_a_dense_brute_force():
    rng = np.random.default_rng(4)
    n = 23
    dense = np.triu(rng.integers(0, 4, (n, n)))
    rows, cols = np.nonzero(dense)
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
    for max_bins in (1000, 23, 10, 5, 1):
        agg = max(1, (n + max_bins - 1) // max_bins)
        m = (n + agg - 1) // agg
        want = np.zeros((m, m), np.float32)
        for a in range(n):
            for b in range(a, n):
                v = np.float32(dense[a, b])
                want[a // agg, b // agg] += v
                if a // agg != b // agg:
                    want[b // agg, a // agg] += v
        got = pre.display_matrix(rowptr, cols, dense[rows, cols], max_display_bins=max_bins)
        assert got.dtype == np.float32 and got.shape == (m, m) and np.array_equal(got, np.log1p(want)) and np.array_equal(got, got.T)


# ---------------------------------------------------------------- the golden: the reference's own functions
@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN, allow_pickle=False)
    records = [(str(n), bytes(g["seq"][int(o):int(o) + int(ln)])) for n, o, ln in zip(g["names"], g["rec_off"], g["rec_len"])]
    return g, records, [str(e) for e in g["enzymes"]]


def test_the_golden_fragments_gc_and_pixels(golden):
    g, records, enzymes = golden
    dig = pre.digest(records, enzymes)
    assert np.array_equal(dig["frag_rec"], g["bins_rec"]) and np.array_equal(dig["start"], g["bins_start"]) and np.array_equal(dig["end"], g["bins_end"])
    gc = pre.gc_counts(records, dig)
    frac = np.array([pre.gc_fraction(a, b) for a, b in zip(gc, dig["end"] - dig["start"])], np.float64)
    assert frac.tobytes() == g["ref_gc"].tobytes()  # the reference's _build_bins_with_gc, bit for bit
    frag, beyond = pre.fragment_of(dig, g["end_rec"], g["end_pos"])  # single ends: every fragment's edges, position 0, an unknown record
    assert np.array_equal(frag, g["ref_end_frag"]) and np.any(frag < 0) and np.any(beyond)
    px = pre.pixels_host(dig, g["c1"], g["p1"], g["c2"], g["p2"])
    rows = np.repeat(np.arange(dig["n_frags"]), np.diff(px["rowptr"]))
    assert np.array_equal(rows, g["ref_bin1"]) and np.array_equal(px["col"], g["ref_bin2"]) and np.array_equal(px["count"], g["ref_count"])
    assert px["pairs_kept"] == int(g["ref_total"]) and px["pairs_in"] == g["c1"].size
    assert px["pairs_in"] == px["pairs_kept"] + px["end1_without_fragment"] + px["end2_without_fragment"]
    assert px["end1_without_fragment"] > 0 and px["end2_without_fragment"] > 0 and px["ends_beyond_record"] > 0 and np.any(rows == px["col"])


def test_the_golden_files_byte_for_byte(golden, tmp_path):
    g, records, enzymes = golden
    (tmp_path / "g.fa").write_bytes(b"".join(b">%s some text\n%s\n" % (n.encode(), b"\n".join(s[k:k + 60] for k in range(0, len(s), 60))) for n, s in records))
    (tmp_path / "in.pairs").write_bytes(bytes(g["pairs_file"]))
    sc = pre.run_pre(tmp_path / "g.fa", str(tmp_path / "in.pairs"), enzymes, str(tmp_path / "out"), device=False, chunk_pairs=1000)
    for name, key in (("fragments_list.txt", "file_fragments_list"), ("info_contigs.txt", "file_info_contigs"), ("abs_fragments_contacts_weighted.txt", "file_abs_contacts")):
        assert (tmp_path / "out" / name).read_bytes() == bytes(g[key]), name
    assert sc["malformed_lines"] == int(g["malformed"]) > 0 and sc["pairs_kept"] == int(g["ref_total"]) and sc["pixels"] == g["ref_count"].size
    assert sc["n_frags"] == g["bins_start"].size and sc["n_records"] == len(records)
    # ... and the folder is one the pyramid takes
    from instagraal_amd import pyramid

    pyr = pyramid.build_and_filter(str(tmp_path / "out"), 2, 3)
    assert pyr is not None and os.path.exists(os.path.join(str(tmp_path / "out"), "pyramids", "pyramid_2_thresh_auto"))


def test_run_pre_plots_the_map(golden, tmp_path):
    g, records, enzymes = golden
    (tmp_path / "g.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    with gzip.open(tmp_path / "reads.pairs.gz", "wb") as f:
        f.write(bytes(g["pairs_file"]))
    pre.run_pre(str(tmp_path / "g.fa"), str(tmp_path / "reads.pairs.gz"), enzymes, str(tmp_path / "out"), device=False, plot=True)
    assert os.path.getsize(tmp_path / "out" / "reads_hic_map.png") > 1000
    assert (tmp_path / "out" / "abs_fragments_contacts_weighted.txt").read_bytes() == bytes(g["file_abs_contacts"])


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/instagraal"), reason="the reference checkout is not beside the repository")
def test_the_generator_reproduces_the_golden():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_pre.py"), "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
