"""The rule of the read pairs lifted onto the current genome (instagraal_amd/pairs_lift.py) without a GPU: against the reference's own
``post`` functions (tests/golden/pairs_lift_tiny.npz, tools/gen_golden_pairs.py), against brute force in Python integers on a crafted
table, its identities and refusals, the 4DN reader and writer, and the chunking."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from instagraal_amd import assembly_contacts as ac, pairs_lift as pl

GOLDEN = os.path.join(ROOT, "tests", "golden", "pairs_lift_tiny.npz")


def golden_table(g):
    sub_ids = np.zeros(g["sub_ids"].shape[1], np.dtype([(k, np.int32) for k in "xyzw"]))
    for i, k in enumerate("xyzw"):
        sub_ids[k] = g["sub_ids"][i]
    names = {str(n): int(i) for n, i in zip(g["contig_names"], g["contig_ids"])}
    return pl.table_of_state(g["state"], sub_ids, g["parent"], g["sub_contig"], g["sub_len_bp"], names=names)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN, allow_pickle=False)
    table = golden_table(g)
    lifted = pl.lift_host(table, g["c1"], g["p1"], g["c2"], g["p2"])
    return g, table, lifted


def coo(res):
    return ac.rows_of(res["rowptr"]), res["col"].astype(np.int64), res["count"]


# ------------------------------------------------------------------ against the reference
def test_lifted_coordinates_and_statuses_equal_the_reference(gold):
    g, table, lifted = gold
    ref = g["ref_lifted"].astype(np.int64)
    assert np.array_equal(table["scaffold_len"], g["scaffold_sizes"])
    assert list(ac.scaffold_names(table["scaffold_ids"])) == [s.replace("|", "-") for s in g["scaffold_names"].tolist()]
    for e in (0, 1):
        ok = ref[:, 2 * e] >= 0
        # an end the reference lifts is lifted to the same place; one it does not is not covered, or lies on the unplaced scaffold
        assert np.array_equal(lifted["scaffold%d" % (e + 1)][ok], ref[ok, 2 * e]) and np.array_equal(lifted["pos%d" % (e + 1)][ok], ref[ok, 2 * e + 1])
        assert np.all(lifted["scaffold%d" % (e + 1)][~ok] == -1) and np.all(lifted["pos%d" % (e + 1)][~ok] == 0)
    kept_ref = (ref[:, 0] >= 0) & (ref[:, 2] >= 0)
    assert np.array_equal(lifted["status"] == pl.KEPT, kept_ref)
    assert lifted["pairs_kept"] == int(g["remapped"]) == int(kept_ref.sum()) and lifted["pairs_in"] + int(g["malformed"]) == int(g["lines"])
    assert lifted["unplaced"] > 0 and lifted["end1_not_covered"] > 0 and lifted["end2_not_covered"] > 0  # the golden has every status
    assert (lifted["rev1"][lifted["status"] == pl.KEPT] == 1).any() and set(np.unique(g["strands"])) == {0, 1, 2, 3}


def test_bin_pixels_equal_the_references_fragment_pixels(gold):
    g, table, lifted = gold
    r, c, n = coo(pl.pixels_host(lifted, table, "bin"))
    assert np.array_equal(r, g["frag_bin1"]) and np.array_equal(c, g["frag_bin2"]) and np.array_equal(n, g["frag_count"])
    assert int(n.sum()) == int(g["frag_total"]) == lifted["pairs_kept"]


@pytest.mark.parametrize("i", [0, 1])
def test_fixed_bin_pixels_equal_the_references(gold, i):
    g, table, lifted = gold
    res = pl.pixels_host(lifted, table, int(g["binsizes"][i]))
    r, c, n = coo(res)
    assert np.array_equal(r, g["fixed%d_bin1" % i]) and np.array_equal(c, g["fixed%d_bin2" % i]) and np.array_equal(n, g["fixed%d_count" % i])
    assert int(n.sum()) == int(g["fixed%d_total" % i]) == lifted["pairs_kept"]
    from instagraal_amd import zoom_levels as zl

    assert res["n_units"] == zl.binnify((table["scaffold_ids"], table["scaffold_len"]), int(g["binsizes"][i])).size


def test_the_law_as_read_equals_the_references_norm_p(gold):
    g, table, lifted = gold
    breaks = g["ps_breaks"]
    counts = pl.law_host(lifted, g["strands"], breaks[:pl.MAX_EDGES] if breaks.size > pl.MAX_EDGES else breaks, flip_strands=False)
    assert breaks.size <= pl.MAX_EDGES
    norm = pl.normalise(counts, breaks, widths=g["ps_binwidth"][:breaks.size - 1])
    seen = np.zeros(counts.shape, bool)
    seen[g["ps_combo"], g["ps_bin"]] = True
    assert np.array_equal(counts > 0, seen)  # the reference lists the bins that hold a pair, and only those
    np.testing.assert_allclose(norm[g["ps_combo"], g["ps_bin"]], g["ps_norm_p"], rtol=1e-12, atol=0)
    flipped = pl.law_host(lifted, g["strands"], breaks, flip_strands=True)
    assert flipped.sum() == counts.sum() and not np.array_equal(flipped, counts)
    assert np.array_equal(flipped.sum(axis=0), counts.sum(axis=0))  # a flip changes the combination, never the distance


def test_the_golden_regenerates_identically_from_the_reference():
    if not os.path.isdir("/root/reference/src/instagraal"):
        pytest.skip("the reference checkout is not here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_pairs.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 differences" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ against brute force
def crafted():
    """contig 0: [0, 10) placed, [10, 11) reversed of length 1, a gap, [15, 30) reversed; contig 2: [0, 7) unplaced, [7, 20); contig 1 has none"""
    sub_contig = np.array([0, 0, 0, 2, 2])
    len_bp = np.array([10, 1, 15, 7, 13])
    start = np.array([0, 10, 15, 0, 7])
    # bins: one per sub-fragment; scaffold 5 holds bins 4, 1 (reversed), 2 (reversed); scaffold 9 holds bin 0; bin 3 is not placed
    order = np.array([4, 1, 2, 0])
    contig_of_bin = np.array([9, 5, 5, 7, 5])
    ori = np.array([1, -1, -1, 1, 1])
    return pl.source_table(sub_contig, len_bp, order, np.arange(5), contig_of_bin, ori, start_bp=start, names=["a", "b", "c"])


def brute_end(table, c, p):
    """-> (hit, scaffold, 1-based position, unit, reversed) in Python integers, interval by interval"""
    iv = table["intervals"]
    pos0 = int(p) - 1
    for v in iv:
        if int(v["src_contig"]) == int(c) and int(v["src_start"]) <= pos0 < int(v["src_end"]):
            if int(v["scaffold"]) < 0:
                return True, -1, 0, -1, 0
            off = pos0 - int(v["src_start"])
            if v["reversed"]:
                off = int(v["src_end"]) - int(v["src_start"]) - 1 - off
            return True, int(v["scaffold"]), int(v["new_start"]) + off + 1, int(v["position"]), int(v["reversed"])
    return False, -1, 0, -1, 0


def test_the_rule_equals_brute_force_on_a_crafted_table():
    t = crafted()
    assert t["scaffold_len"].tolist() == [29, 10] and t["src_rowptr"].tolist() == [0, 3, 3, 5] and t["n_bin_units"] == 4
    cs, ps = [], []
    for c in (-1, 0, 1, 2, 3):
        for p in range(-1, 33):
            cs.append(c), ps.append(p)
    cs, ps = np.array(cs), np.array(ps)
    rng = np.random.default_rng(5)
    other = rng.permutation(cs.size)
    res = pl.lift_host(t, cs, ps, cs[other], ps[other])
    n_status = [0, 0, 0, 0]
    for k in range(cs.size):
        a, b = brute_end(t, cs[k], ps[k]), brute_end(t, cs[other[k]], ps[other[k]])
        status = 1 if not a[0] else 2 if not b[0] else 3 if a[1] < 0 or b[1] < 0 else 0
        n_status[status] += 1
        got = tuple(int(res[f][k]) for f in ("scaffold1", "pos1", "unit1", "rev1", "scaffold2", "pos2", "unit2", "rev2", "status"))
        assert got == a[1:] + b[1:] + (status,), (k, cs[k], ps[k], got)
    assert [res[k] for k in pl.SCALARS[1:5]] == n_status and min(n_status) > 0
    # the single cases the issue names: position 0, the reversed interval of length 1, adjacent intervals, the gap
    one = lambda c, p: brute_end(t, c, p)  # noqa: E731
    assert not one(0, 0)[0] and one(0, 11)[1:] == (0, t["intervals"][1]["new_start"] + 1, 1, 1)
    assert one(0, 10)[1] == 1 and one(0, 11)[1] == 0 and not one(0, 12)[0] and not one(0, 15)[0] and one(0, 16)[0] and one(0, 30)[0] and not one(0, 31)[0]
    assert one(0, 16)[2] == t["intervals"][2]["new_start"] + 15 and one(0, 30)[2] == t["intervals"][2]["new_start"] + 1  # mirrored


def brute_pixels(a, b, U):
    d = {}
    for x, y in zip(a.tolist(), b.tolist()):
        d[(min(x, y), max(x, y))] = d.get((min(x, y), max(x, y)), 0) + 1
    keys = sorted(d)
    return [k[0] for k in keys], [k[1] for k in keys], [d[k] for k in keys]


@pytest.mark.parametrize("units", ["sub", "bin", "scaffold", 1, 4, 1000])
def test_pixels_and_scalars_identities(units):
    t = crafted()
    rng = np.random.default_rng(7)
    n = 400
    c1, c2 = rng.choice([0, 2], n), rng.choice([0, 2, 1], n)
    p1, p2 = rng.integers(0, 32, n), rng.integers(0, 32, n)
    lifted = pl.lift_host(t, c1, p1, c2, p2)
    assert lifted["pairs_kept"] + lifted["end1_not_covered"] + lifted["end2_not_covered"] + lifted["unplaced"] == lifted["pairs_in"] == n
    res = pl.pixels_host(lifted, t, units)
    assert int(res["count"].sum()) == lifted["pairs_kept"] == res["entries_in"] and res["rowptr"][-1] == res["col"].size == res["entries_out"]
    a, b, U = pl.units_of(lifted, t, units)
    r, c, k = coo(res)
    assert (r.tolist(), c.tolist(), k.tolist()) == brute_pixels(a, b, U) and (r <= c).all() and (r == c).any()
    if units == 4:  # the fixed bins: scaffold 5 (29 bp) has 8, scaffold 9 (10 bp) has 3; a pair counts where it falls
        assert U == 11 and np.array_equal(a, np.where(lifted["scaffold1"][lifted["status"] == 0] == 0, 0, 8) + (lifted["pos1"][lifted["status"] == 0] - 1) // 4)


def test_law_brute_force_and_edges():
    t = crafted()
    rng = np.random.default_rng(9)
    n = 500
    c1 = rng.choice([0, 2], n)
    p1, p2 = rng.integers(1, 31, n), rng.integers(1, 31, n)
    strands = rng.integers(0, 4, n).astype(np.uint8)
    lifted = pl.lift_host(t, c1, p1, c1, p2)
    for edges in ([0, 40], [2, 5], [0, 1, 2, 3, 5, 8, 13, 21], list(range(0, 512))):
        for flip in (True, False):
            want = np.zeros((4, len(edges) - 1), np.int64)
            for k in range(n):
                if lifted["status"][k] or lifted["scaffold1"][k] != lifted["scaffold2"][k]:
                    continue
                d = abs(int(lifted["pos2"][k]) - int(lifted["pos1"][k]))
                idx = max(0, min(len(edges) - 2, sum(1 for e in edges if e <= d) - 1))
                s1, s2 = int(strands[k]) & 1, int(strands[k]) >> 1
                if flip:
                    s1, s2 = s1 ^ int(lifted["rev1"][k]), s2 ^ int(lifted["rev2"][k])
                want[2 * s1 + s2, idx] += 1
            assert np.array_equal(pl.law_host(lifted, strands, np.array(edges), flip), want)
    for bad in ([5], [3, 2], [-1, 4], list(range(513)), [0.5, 2.0]):
        with pytest.raises(ValueError):
            pl.law_host(lifted, strands, np.array(bad))
    norm = pl.normalise(np.array([[2, 2], [0, 0], [1, 3], [4, 0]]), np.array([0, 10, 30]))
    assert np.allclose(norm[0], [0.05, 0.025]) and np.isnan(norm[1]).all() and np.allclose(norm[2], [0.025, 0.0375])
    e = pl.default_edges_bp(1.8, 400.0)
    assert 2 <= e.size <= pl.MAX_EDGES and np.all(np.diff(e) > 0) and e[-1] >= 400_000 and e.dtype == np.int64


def test_source_table_running_sum_and_refusals():
    # no start_bp: the running sum of len_bp in sub-fragment id order inside each contig
    t = pl.source_table([3, 1, 3, 1], [5, 6, 7, 8], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [1, 1, 1, 1])
    iv = t["intervals"]
    assert iv["sub"].tolist() == [1, 3, 0, 2] and iv["src_start"].tolist() == [0, 6, 0, 5] and iv["src_end"].tolist() == [6, 14, 5, 12]
    assert t["src_rowptr"].tolist() == [0, 0, 2, 2, 4]
    with pytest.raises(ValueError, match="overlapping"):
        pl.source_table([0, 0], [10, 10], [0, 1], [0, 1], [0, 1], [1, 1], start_bp=[0, 9])
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        pl.source_table([0, 1], [1 << 30, 1 << 30], [0, 1], [0, 1], [4, 4], [1, 1])  # one scaffold of 2^31 bp
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        pl.source_table([0], [10], [0], [0], [0], [1], start_bp=[(1 << 31) - 5])
    with pytest.raises(ValueError):
        pl.source_table([0, -1], [10, 10], [0, 1], [0, 1], [0, 1], [1, 1])
    with pytest.raises(ValueError):
        pl.check_units(t, "fragments")
    with pytest.raises(ValueError):
        pl.contig_ids(t, ["a"])  # names, and the table has none
    ident = pl.identity_table([100, 50], names=["s0", "s1"])
    r = pl.lift_host(ident, pl.contig_ids(ident, ["s0", "s1", "nope"]), [100, 1, 1], [1, 0, 0], [50, 100, 1])
    assert r["scaffold1"].tolist() == [0, 1, -1] and r["pos1"].tolist() == [100, 1, 0] and r["pos2"].tolist() == [50, 100, 1] and r["status"].tolist() == [0, 0, 1]


# ------------------------------------------------------------------ the text side
HEADER = "## pairs format v1.0\n#sorted: chr1-chr2-pos1-pos2\n#shape: upper triangle\n#chromsize: a 30\n#chromsize: c 20\n#chromosomes: a c\n"
LINES = ["r0\ta\t5\tc\t9\t+\t-", "r1\ta\t11\ta\t16\t-\t-", "r2\tzz\t1\ta\t1\t+\t+", "r3\ta\tseven\ta\t1\t+\t+", "r4\tc\t3\ta\t2\t-\t+", "short", "r6\ta\t13\tc\t8\t+\t+",
         "r7\tc\t20\ta\t30\t-\t+\textra"]


def write_file(path, columns=None, gz=False):
    text = HEADER + ("#columns: %s\n" % " ".join(columns) if columns else "")
    cols = columns or pl.DEFAULT_COLUMNS
    for line in LINES:
        f = line.split("\t")
        if len(f) >= 7:
            d = dict(zip(pl.DEFAULT_COLUMNS, f))
            f = [d[k] for k in cols] + f[7:]
        text += "\t".join(f) + "\n"
    with (gzip.open if gz else open)(path, "wt") as h:
        h.write(text)


@pytest.mark.parametrize("columns", [None, ("readID", "strand2", "chr2", "pos2", "strand1", "chr1", "pos1")])
@pytest.mark.parametrize("gz", [False, True])
def test_reader_columns_malformed_unknown_and_chunking(tmp_path, columns, gz):
    path = str(tmp_path / ("in.pairs.gz" if gz else "in.pairs"))
    write_file(path, columns, gz)
    names = crafted()["names"]
    whole = None
    for chunk in (1, 7, 1 << 20):
        parts = list(pl.read_pairs(path, names, chunk))
        got = {k: np.concatenate([p[k] for p in parts]) for k in ("c1", "p1", "c2", "p2", "strands")}
        assert parts[-1]["malformed"] == 2 and all(p["c1"].size <= chunk for p in parts)
        if whole is None:
            whole = got
            assert got["c1"].tolist() == [0, 0, -1, 2, 0, 2] and got["p1"].tolist() == [5, 11, 1, 3, 13, 20] and got["c2"].tolist() == [2, 0, 0, 0, 2, 0]
            assert got["p2"].tolist() == [9, 16, 1, 2, 8, 30] and got["strands"].tolist() == [2, 3, 0, 1, 0, 1]
        for k in got:
            assert np.array_equal(got[k], whole[k]) and got[k].dtype == whole[k].dtype


def test_writer_header_order_and_kept_lines(tmp_path):
    t = crafted()
    src, out = str(tmp_path / "in.pairs"), str(tmp_path / "lifted.pairs.gz")
    cols = ("readID", "strand2", "chr2", "pos2", "strand1", "chr1", "pos1")
    write_file(src, cols)
    tot = pl.write_lifted_pairs(src, out, t, chunk_pairs=2)
    text = gzip.open(out, "rt").read().split("\n")
    assert text[:8] == ["## pairs format v1.0", "#sorted: none", "#shape: upper triangle", "#chromosomes: 3C-assembly-contig_5 3C-assembly-contig_9",
                        "#chromsize: 3C-assembly-contig_5 29", "#chromsize: 3C-assembly-contig_9 10", "#columns: " + " ".join(cols), text[7]]
    data = [ln.split("\t") for ln in text[7:] if ln]
    lifted = pl.lift_host(t, [0, 0, -1, 2, 0, 2], [5, 11, 1, 3, 13, 20], [2, 0, 0, 0, 2, 0], [9, 16, 1, 2, 8, 30])
    kept = np.nonzero(lifted["status"] == 0)[0]
    assert [d[0] for d in data] == [["r0", "r1", "r2", "r4", "r6", "r7"][k] for k in kept] and len(kept) >= 3  # input order
    names = ac.scaffold_names(t["scaffold_ids"])
    for d, k in zip(data, kept):
        assert (d[5], int(d[6]), d[2], int(d[3])) == (names[lifted["scaffold1"][k]], lifted["pos1"][k], names[lifted["scaffold2"][k]], lifted["pos2"][k])
    assert data[-1][-1] == "extra" and data[-1][1] == "+" and data[-1][4] == "-"  # the other fields as they were
    assert tot["pairs_in"] == 6 and tot["malformed"] == 2 and tot["lines"] == 8 and tot["pairs_kept"] == len(kept)
    # what was written lifts to itself under the identity table
    ident = pl.identity_table(t["scaffold_len"], names=list(names))
    again = pl.concat_lifted(pl.lift_host(ident, c["c1"], c["p1"], c["c2"], c["p2"]) for c in pl.read_pairs(out, ident["names"], 2))
    assert again["pairs_kept"] == len(kept) and np.array_equal(again["pos1"], lifted["pos1"][kept]) and np.array_equal(again["scaffold2"], lifted["scaffold2"][kept])


@pytest.mark.parametrize("chunk", [1, 7])
def test_chunked_lifts_concatenate_to_the_whole(gold, chunk):
    g, table, lifted = gold
    n = 300
    cut = lambda k, a: g[k][a:min(a + chunk, n)]  # noqa: E731
    parts = [pl.lift_host(table, cut("c1", a), cut("p1", a), cut("c2", a), cut("p2", a)) for a in range(0, n, chunk)]
    got = pl.concat_lifted(parts)
    whole = pl.lift_host(table, g["c1"][:n], g["p1"][:n], g["c2"][:n], g["p2"][:n])
    for k in whole:
        assert np.array_equal(got[k], whole[k]), k
