"""GPU tests of the read pairs lifted onto the current genome (ig_pairs_begin / _lift / _pixels_build / _law / _end, sampler.lift_pairs,
pairs_contacts, write_pairs_zoom_levels, pairs_distance_law, write_lifted_pairs) against the rule's host statement
(instagraal_amd.pairs_lift) over the table made from the same handle's genome, and against the reference's results
(tests/golden/pairs_lift_tiny.npz).  Every comparison is exact: the arrays' bytes."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LIFTED = ("scaffold1", "pos1", "unit1", "rev1", "scaffold2", "pos2", "unit2", "rev2", "status")
COUNTS = ("pairs_in", "pairs_kept", "end1_not_covered", "end2_not_covered", "unplaced")
ARRAYS = ("rowptr", "col", "count")
BINSIZES = (700, 4900)  # below and above the median sub-fragment of `tiny` (about 1 800 bp)
EDGES = ([0, 1 << 40], [0, 1, 10, 100, 1000, 10_000, 100_000, 1_000_000], (12 * np.arange(512, dtype=np.int64) ** 2).tolist())  # 2, 8 and 512 edges


def _sampler(cfg, seed=None, **extra):
    import test_hip_assembly_contacts as ta

    return ta._sampler(cfg, seed, **extra)


def _pairs(table, n, seed, covered=False):
    """n seeded pairs over the table's contigs: 70 % on one contig; unless ``covered``, some beyond the contig's end, at position 0, on an
    unknown contig; every strand combination"""
    rng = np.random.default_rng(seed)
    iv = table["intervals"]
    ids = np.unique(iv["src_contig"])
    end = np.zeros(int(ids.max()) + 2, np.int64)
    np.maximum.at(end, iv["src_contig"], iv["src_end"])
    c1 = rng.choice(ids, n)
    c2 = np.where(rng.random(n) < 0.7, c1, rng.choice(ids, n))
    if not covered:
        c2 = np.where(rng.random(n) < 0.02, int(ids.max()) + 1 + rng.integers(0, 3, n), c2)
        c1 = np.where(rng.random(n) < 0.01, -1, c1)
    slack = 0 if covered else 3
    p1 = rng.integers(1 - (slack > 0), end[np.maximum(c1, 0)] + 1 + slack)
    p2 = rng.integers(1 - (slack > 0), end[np.minimum(np.maximum(c2, 0), end.size - 1)] + 1 + slack)
    return c1.astype(np.int64), p1.astype(np.int64), c2.astype(np.int64), p2.astype(np.int64), rng.integers(0, 4, n).astype(np.uint8)


def _assert_lifted(got, want, what):
    for k in LIFTED:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS], (what, [got[k] for k in COUNTS], [want[k] for k in COUNTS])


def _pixels(s, units):
    from instagraal_amd import pairs_lift as pl

    kind, B, _, _ = pl.check_units(s._pairs, units)
    res = s.ctx.pairs_pixels(kind, B)
    res["col"], res["count"] = s.ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
    return res


def _assert_pixels(got, want, what):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["n_units"] == want["n_units"] and got["entries_out"] == want["entries_out"] and got["entries_kept"] == want["entries_in"] == got["contacts_kept"]


def _assert_session(s, prob, what, n=4097, seed=1, want_unplaced=False):
    """one session on the handle's genome: the lift, the four unit kinds, a zoom chain and the law against the rule"""
    from instagraal_amd import assembly_contacts as ac, pairs_lift as pl, zoom_levels as zl

    table = s.pairs_begin()
    # the table is the one the rule makes of the downloaded state
    host = pl.table_of_state(s.ctx.download_state(), prob.np_sub_frags_id, prob.np_sub_frags_2_frags["x"].astype(np.int64), prob.S_o_A_sub_frags["id_c"],
                             prob.S_o_A_sub_frags["len_bp"])
    assert host["intervals"].tobytes() == table["intervals"].tobytes() and np.array_equal(host["scaffold_len"], table["scaffold_len"])
    c1, p1, c2, p2, strands = _pairs(table, n, seed)
    want = pl.lift_host(table, c1, p1, c2, p2)
    got = s.lift_pairs(c1, p1, c2, p2, strands)
    _assert_lifted(got, want, what)
    assert got["pairs_stored"] == want["pairs_kept"] > 0 and (want["unplaced"] > 0) == want_unplaced and want["end1_not_covered"] > 0 and want["end2_not_covered"] > 0
    assert (want["rev1"][want["status"] == 0] == 1).any() or "fresh" in what
    for units in ("sub", "bin", "scaffold") + BINSIZES:
        _assert_pixels(_pixels(s, units), pl.pixels_host(want, table, units), (what, units))
    # a zoom chain by coarsening equals each level built from the store
    sizes = ac.chrom_sizes(table["table_sub"])
    B = BINSIZES[0]
    _pixels(s, B)
    for f in (2, 7):
        res = s.ctx.assembly_contacts_coarsen(*zl.coarse_map(sizes, B, f))
        res["col"], res["count"] = s.ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
        for k, w in zip(ARRAYS, (lambda r: (r["rowptr"], r["col"], r["count"]))(pl.pixels_host(want, table, B * f))):
            assert res[k].tobytes() == w.tobytes(), (what, "coarsened", B, f, k)
        B *= f
    res = s.ctx.assembly_contacts_coarsen(*zl.scaffold_map(sizes, B))
    res["col"], res["count"] = s.ctx.assembly_contacts_fetch(0, res.pop("n_entries"))
    for k in ARRAYS:
        assert res[k].tobytes() == pl.pixels_host(want, table, "scaffold")[k].tobytes(), (what, "to the scaffolds", k)
    s.ctx.assembly_contacts_release()
    for edges in EDGES:
        for flip in (True, False):
            counts, sc = s.ctx.pairs_law(np.array(edges, np.int64), flip)
            w = pl.law_host(want, strands, np.array(edges, np.int64), flip)
            assert counts.tobytes() == w.tobytes() and sc["pairs_cis"] == int(w.sum()) and sc["pairs_stored"] == want["pairs_kept"], (what, len(edges), flip)
    assert len(EDGES[0]) == 2 and len(EDGES[2]) == 512
    s.pairs_end()
    return want


def test_tiny_fresh_and_behind_moves_with_flips():
    prob, s = _sampler("tiny", seed=12)
    _assert_session(s, prob, "tiny fresh")
    s.bomb_the_genome()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:150], 5)
    g = s.gpu_vect_frags.copy_from_gpu()
    assert (g.ori == -1).sum() >= 3 and np.unique(g.id_c).size > 20
    _assert_session(s, prob, "tiny behind the bomb and moves", seed=2)
    s.free_gpu()


def test_a_state_with_a_ring_and_one_with_an_unplaced_contig():
    import test_hip_assembly_contacts as ta
    from instagraal_amd.hip_lib import FRAG_FIELDS

    prob, s = _sampler("tiny", seed=13)
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:60], 5)
    first, last = ta._first_and_last_of_a_contig(prob)
    s.test_copy_struct(first, last, 10)
    s.modify_gl_cuda_buffer()
    assert (s.gpu_vect_frags.copy_from_gpu().circ == 1).sum() >= 3
    _assert_session(s, prob, "tiny with a ring", seed=3)
    id_c = s.ctx.download_state()[FRAG_FIELDS.index("id_c")]
    ids, n = np.unique(id_c, return_counts=True)
    s.ctx.debug_set_bin_active(np.nonzero(id_c == ids[np.argmax(n >= 3)])[0][1], False)
    assert s.ctx.contact_map_order().size < prob.n_sub_frags
    _assert_session(s, prob, "tiny with an unplaced contig", seed=4, want_unplaced=True)
    s.free_gpu()


def test_the_golden_directly():
    """the reference's lifted coordinates, fragment pixels, fixed-bin pixels and P(s) from the device's own arrays"""
    from instagraal_amd import assembly_contacts as ac, pairs_lift as pl

    g = np.load(os.path.join(GOLDEN, "pairs_lift_tiny.npz"), allow_pickle=False)
    prob, s = _sampler(str(g["config"]), seed=11)
    state = g["state"].copy()
    victim = np.nonzero(state[15] == 0)[0]
    state[15] = 1
    s.ctx.upload_state(state)
    s.modify_gl_cuda_buffer()
    s.eval_likelihood_init()
    for b in victim:
        s.ctx.debug_set_bin_active(int(b), False)
    assert np.array_equal(s.ctx.download_state(), g["state"])
    s.contig_names = {str(n): int(i) for n, i in zip(g["contig_names"], g["contig_ids"])}
    got = s.lift_pairs(g["c1"], g["p1"], g["c2"], g["p2"], g["strands"])
    ref = g["ref_lifted"]
    kept = (ref[:, 0] >= 0) & (ref[:, 2] >= 0)
    assert np.array_equal(got["status"] == 0, kept) and got["pairs_kept"] == int(g["remapped"])
    for e in (0, 1):
        ok = ref[:, 2 * e] >= 0
        assert np.array_equal(got["scaffold%d" % (e + 1)][ok], ref[ok, 2 * e]) and np.array_equal(got["pos%d" % (e + 1)][ok], ref[ok, 2 * e + 1])
    res = _pixels(s, "bin")
    assert np.array_equal(ac.rows_of(res["rowptr"]), g["frag_bin1"]) and np.array_equal(res["col"], g["frag_bin2"]) and np.array_equal(res["count"], g["frag_count"])
    for i, B in enumerate(g["binsizes"].tolist()):
        res = _pixels(s, B)
        assert np.array_equal(ac.rows_of(res["rowptr"]), g["fixed%d_bin1" % i]) and np.array_equal(res["col"], g["fixed%d_bin2" % i])
        assert np.array_equal(res["count"], g["fixed%d_count" % i]) and int(res["count"].sum()) == int(g["fixed%d_total" % i])
    breaks = g["ps_breaks"]
    counts, _ = s.ctx.pairs_law(breaks, flip_strands=False)
    norm = pl.normalise(counts, breaks, widths=g["ps_binwidth"][:breaks.size - 1])
    seen = np.zeros(counts.shape, bool)
    seen[g["ps_combo"], g["ps_bin"]] = True
    assert np.array_equal(counts > 0, seen)
    np.testing.assert_allclose(norm[g["ps_combo"], g["ps_bin"]], g["ps_norm_p"], rtol=1e-12, atol=0)
    s.pairs_end()
    s.free_gpu()


@pytest.fixture(scope="module")
def moved():
    prob, s = _sampler("tiny", seed=21)
    s.bomb_the_genome()
    s.step_sampler_batch(np.random.permutation(prob.n_frags)[:150], 5)
    yield prob, s
    s.free_gpu()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_pair_counts_at_the_wave_and_workgroup_edges(moved, n):
    from instagraal_amd import pairs_lift as pl

    prob, s = moved
    table = s.pairs_begin()
    c1, p1, c2, p2, strands = _pairs(table, n, 100 + n, covered=n == 1)
    want = pl.lift_host(table, c1, p1, c2, p2)
    got = s.lift_pairs(c1, p1, c2, p2, strands)
    _assert_lifted(got, want, n)
    assert got["pairs_stored"] == want["pairs_kept"] and (n > 1 or want["pairs_kept"] == 1)
    _assert_pixels(_pixels(s, BINSIZES[0]), pl.pixels_host(want, table, BINSIZES[0]), n)
    _assert_pixels(_pixels(s, "sub"), pl.pixels_host(want, table, "sub"), n)
    counts, _ = s.ctx.pairs_law(np.array(EDGES[1]), True)
    assert counts.tobytes() == pl.law_host(want, strands, np.array(EDGES[1]), True).tobytes()
    s.ctx.assembly_contacts_release()
    s.pairs_end()


def test_chunks_of_64_and_1000_give_the_pixels_and_the_histogram_of_one_chunk(moved):
    from instagraal_amd import pairs_lift as pl

    prob, s = moved
    n = 4097
    results = []
    for chunk in (n, 64, 1000):
        table = s.pairs_begin(reserve_pairs=10 if chunk == 64 else 0)  # (a small reserve: the store grows across the chunks)
        c1, p1, c2, p2, strands = _pairs(table, n, 7)
        parts = [s.lift_pairs(c1[a:a + chunk], p1[a:a + chunk], c2[a:a + chunk], p2[a:a + chunk], strands[a:a + chunk]) for a in range(0, n, chunk)]
        whole = pl.concat_lifted(parts)
        _assert_lifted(whole, pl.lift_host(table, c1, p1, c2, p2), chunk)
        assert parts[-1]["pairs_stored"] == whole["pairs_kept"]
        px = [_pixels(s, u) for u in ("bin", BINSIZES[0])]
        law = s.ctx.pairs_law(np.array(EDGES[2]), True)[0]
        results.append([r[k].tobytes() for r in px for k in ARRAYS] + [law.tobytes()])
        s.ctx.pairs_clear()  # an emptied store builds no pixel
        assert _pixels(s, "bin")["entries_out"] == 0 and s.ctx.pairs_law(np.array(EDGES[1]))[0].sum() == 0
        s.pairs_end()
    assert results[0] == results[1] == results[2]
    s.ctx.assembly_contacts_release()


def test_a_session_across_a_committed_move_is_refused(moved):
    """the choice: refused, not rebuilt -- the caller's arrays were lifted under a table that no longer describes the genome"""
    from instagraal_amd import hip_lib

    prob, s = moved
    table = s.pairs_begin()
    c1, p1, c2, p2, strands = _pairs(table, 300, 9)
    s.lift_pairs(c1, p1, c2, p2, strands)
    before = s.ctx.contact_map_order()
    frags = np.random.permutation(prob.n_frags)
    for a in range(0, 200, 20):
        s.step_sampler_batch(frags[a:a + 20], 5)
        if not np.array_equal(s.ctx.contact_map_order(), before):
            break
    assert not np.array_equal(s.ctx.contact_map_order(), before)
    for call in (lambda: s.lift_pairs(c1, p1, c2, p2), lambda: s.ctx.pairs_pixels("bin"), lambda: s.ctx.pairs_law(np.array(EDGES[1])),
                 lambda: s.ctx.debug_pairs_time(c1, p1, c2, p2, strands, "bin", 0, EDGES[1])):
        with pytest.raises(hip_lib.HipError, match="the genome changed since ig_pairs_begin"):
            call()
    with pytest.raises(hip_lib.HipError, match="a session is open"):
        s.ctx.pairs_begin(table)
    s.pairs_end()
    with pytest.raises(hip_lib.HipError, match="no session"):
        s.ctx.pairs_law(np.array(EDGES[1]))
    with pytest.raises(hip_lib.HipError, match="no session"):
        s.ctx.pairs_end()
    got = s.lift_pairs(c1, p1, c2, p2, strands)  # a new session on the new genome works
    from instagraal_amd import pairs_lift as pl

    _assert_lifted(got, pl.lift_host(s._pairs, c1, p1, c2, p2), "behind the move")
    s.pairs_end()


def test_a_run_with_a_session_in_its_middle_is_the_run_without(tmp_path):
    outs = []
    for with_it in (False, True):
        prob, s = _sampler("tiny", seed=3)
        frags = np.random.permutation(prob.n_frags)[:150]
        res = [s.step_sampler_batch(frags[:75], 5)]
        if with_it:
            st = np.random.get_state()
            table = s.pairs_begin()
            pairs = _pairs(table, 2000, 5)
            s.pairs_end()
            assert s.pairs_contacts(pairs, binsize=2000)["count"].sum() > 0 and s.pairs_distance_law(pairs)["counts"].sum() > 0
            made = s.write_pairs_zoom_levels(str(tmp_path / "zoom"), pairs, resolutions=(1000, 5000))
            assert [m["made"] for m in made] == [("direct",), ("coarsen", 5), ("coarsen", "scaffolds")]
            after = np.random.get_state()
            assert np.array_equal(st[1], after[1]) and st[2] == after[2]
        res.append(s.step_sampler_batch(frags[75:], 5))
        sums, ints = s.ctx.debug_globals()
        outs.append((np.concatenate(res).tobytes(), s.gpu_vect_frags.copy_from_gpu().soa17(), sums.tolist(), ints.tolist(), np.random.get_state()[1].copy(),
                     np.random.get_state()[2]))
        s.free_gpu()
    a, b = outs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


def test_the_sampler_layer_an_open_session_is_kept_and_the_figure_is_written(moved, tmp_path):
    """pairs=None builds from the open session's store and leaves it; a call that brings its pairs is refused while a session is open
    (its store would be lost) and runs in a session of its own otherwise; display_pairs_distance_law writes the figure of the law"""
    from instagraal_amd import assembly_contacts as ac, pairs_lift as pl

    prob, s = moved
    table = s.pairs_begin()
    c1, p1, c2, p2, strands = _pairs(table, 3000, 41)
    s.pairs_end()
    half = 1500
    s.lift_pairs(c1[:half], p1[:half], c2[:half], p2[:half], strands[:half])  # (opens the session)
    got = s.lift_pairs(c1[half:], p1[half:], c2[half:], p2[half:], strands[half:])
    want = pl.lift_host(s._pairs, c1, p1, c2, p2)
    assert got["pairs_stored"] == want["pairs_kept"]
    for call in (lambda: s.pairs_contacts((c1, p1, c2, p2), binsize=BINSIZES[0]), lambda: s.pairs_distance_law((c1, p1, c2, p2, strands)),
                 lambda: s.write_pairs_zoom_levels(str(tmp_path / "z"), (c1, p1, c2, p2), (1000,)), lambda: s.write_lifted_pairs(str(tmp_path / "none.pairs"), str(tmp_path / "o.gz"))):
        with pytest.raises(ValueError, match="a session is open"):
            call()
    res = s.pairs_contacts(None, binsize=BINSIZES[0])  # the store is still whole
    w = pl.pixels_host(want, s._pairs, BINSIZES[0])
    assert all(res[k].tobytes() == w[k].tobytes() for k in ARRAYS) and res["binsize"] == BINSIZES[0] and res["bins"].size == w["n_units"]
    res = s.pairs_contacts(None, units="bin")
    assert all(res[k].tobytes() == pl.pixels_host(want, s._pairs, "bin")[k].tobytes() for k in ARRAYS) and res["bins"].size == s._pairs["n_bin_units"]
    edges = np.array(EDGES[1])
    png = str(tmp_path / "law.png")
    law = s.display_pairs_distance_law(png, None, edges, flip_strands=False)
    counts = pl.law_host(want, strands, edges, False)
    assert os.path.getsize(png) > 1000 and law["counts"].tobytes() == counts.tobytes() and law["flip_strands"] is False
    assert np.array_equal(law["norm_p"], pl.normalise(counts, edges), equal_nan=True) and law["pairs_stored"] == want["pairs_kept"]
    default = s.pairs_distance_law(None)  # the project's own edges, in bp
    assert default["counts"].sum() == counts.sum() and 2 <= default["edges_bp"].size <= pl.MAX_EDGES and s._pairs is not None
    s.pairs_end()
    with pytest.raises(ValueError, match="no session is open"):
        s.pairs_contacts(None, binsize=1000)
    own = s.pairs_contacts((c1, p1, c2, p2, strands), units="scaffold")  # a session of the call's own, ended behind it
    assert own["count"].sum() == want["pairs_kept"] == own["pairs_kept"] and s._pairs is None and np.array_equal(own["chrom_sizes"][1], ac.chrom_sizes(table["table_sub"])[1])
    with pytest.raises(NotImplementedError, match="balanc"):
        s.pairs_contacts((c1, p1, c2, p2), binsize=1000, balance=True)
    assert s._pairs is None


def test_sharded_and_in_flight_refusals_leave_the_handle_usable():
    from instagraal_amd import hip_lib, pairs_lift as pl
    from instagraal_amd.sampler import PARAM_NAMES

    prob, s = _sampler("tiny", seed=31)
    table = s.pairs_begin()
    c1, p1, c2, p2, strands = _pairs(table, 500, 11)
    want = pl.lift_host(table, c1, p1, c2, p2)
    s.pairs_end()
    s.ctx.set_shard(0, 2)
    with pytest.raises(hip_lib.HipError, match="ig_pairs_begin.*one handle"):
        s.ctx.pairs_begin(table)
    s.ctx.set_shard(0, 1)
    # between ig_nuis_begin and ig_nuis_end every call of the feature refuses, and the step ends as if nothing had happened
    s.pairs_begin()
    _assert_lifted(s.lift_pairs(c1, p1, c2, p2, strands), want, "before the step")
    cands = s.return_neighbours(3, 5)
    p8 = np.array([float(s.param_simu[k][0]) for k in PARAM_NAMES], np.float32)
    s.ctx.nuis_begin(3, sorted(int(x) for x in cands if x != 3), p8, s.mean_kb())
    for call in (lambda: s.ctx.pairs_lift(c1, p1, c2, p2), lambda: s.ctx.pairs_pixels("bin"), lambda: s.ctx.pairs_law(np.array(EDGES[1]))):
        with pytest.raises(hip_lib.HipError, match="ig_pairs_.*in flight"):
            call()
    s.ctx.nuis_end()
    s.pairs_end()  # (the step's move may have changed the genome: a new session)
    table = s.pairs_begin()
    want = pl.lift_host(table, c1, p1, c2, p2)
    _assert_lifted(s.lift_pairs(c1, p1, c2, p2, strands), want, "behind the step")
    _assert_pixels(_pixels(s, "scaffold"), pl.pixels_host(want, table, "scaffold"), "behind the step")
    # the refusals of the arguments leave the store as it was
    for kind, B, words in ((7, 0, "kind"), (2, 0, "bin size"), (2, 1 << 31, "bin size")):
        with pytest.raises(hip_lib.HipError, match=words):
            s.ctx.pairs_pixels(kind, B)
        with pytest.raises(hip_lib.HipError, match="nothing is built"):
            s.ctx.assembly_contacts_fetch(0, 1)
    for edges in ([5], [3, 2], list(range(513))):
        with pytest.raises(hip_lib.HipError, match="edges"):
            s.ctx.pairs_law(np.array(edges))
    _assert_pixels(_pixels(s, "scaffold"), pl.pixels_host(want, table, "scaffold"), "behind the refusals")
    ms, ck = s.ctx.debug_pairs_time(c1, p1, c2, p2, strands, "binsize", BINSIZES[0], EDGES[1], n=2)
    assert ms.shape == (2, len(hip_lib.PAIRS_PASSES)) and (ms[:, 0] > 0).all() and (ms[:, -1] > 0).all() and ck != 0
    _assert_pixels(dict(_pixels(s, BINSIZES[0])), pl.pixels_host(want, table, BINSIZES[0]), "behind the timed passes")  # the store holds the chunk once
    s.ctx.assembly_contacts_release()
    s.free_gpu()  # (a live session in front of ig_destroy)


def _contigs_of(data):
    rows = [ln.split("\t") for ln in open(os.path.join(data, "info_contigs.txt")).read().splitlines()[1:]]
    return [r[0] for r in rows], [int(r[1]) for r in rows]


def test_run_instagraal_pairs(tmp_path):
    from instagraal_amd import assembly_contacts as ac, pairs_lift as pl, synth, zoom_levels as zl
    from instagraal_amd.simulation import run_instagraal

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    names, lengths = _contigs_of(data)
    rng = np.random.default_rng(3)
    n = 3000
    k1 = rng.integers(0, len(names), n)
    k2 = np.where(rng.random(n) < 0.7, k1, rng.integers(0, len(names), n))
    src = str(tmp_path / "in.pairs")
    with open(src, "w") as f:
        f.write("## pairs format v1.0\n#shape: upper triangle\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n")
        for i in range(n):
            f.write("r%d\t%s\t%d\t%s\t%d\t%s\t%s\n" % (i, names[k1[i]], rng.integers(1, lengths[k1[i]] + 1), names[k2[i]], rng.integers(1, lengths[k2[i]] + 1),
                                                    "+-"[rng.integers(0, 2)], "+-"[rng.integers(0, 2)]))
        f.write("r_bad\tctg01\tx\tctg01\t5\t+\t+\nr_unknown\tnowhere\t5\tctg01\t5\t+\t+\n")
    np.random.seed(17)
    res = (2000, 10_000)
    p2 = run_instagraal(data, os.path.join(data, "genome.fa"), output_folder=str(tmp_path / "out"), level=2, cycles=1, bomb=True, save_resolutions=res, pairs=src,
                        save_lifted_pairs=True)
    s = p2.simulation.sampler
    out = p2.simulation.output_folder
    root = os.path.join(out, "pairs_zoom_levels")
    assert sorted(os.listdir(root)) == ["resolutions", "scaffolds"] and sorted(os.listdir(os.path.join(root, "resolutions")), key=int) == [str(b) for b in res]
    assert os.path.getsize(os.path.join(out, "pairs_law.txt")) > 0 and os.path.isdir(os.path.join(out, "zoom_levels"))
    # the files are the rule's: the table of the final genome, the file's pairs, the writers
    table = s.pairs_begin()
    chunks = list(pl.read_pairs(src, table["names"]))
    lifted = pl.concat_lifted(pl.lift_host(table, c["c1"], c["p1"], c["c2"], c["p2"]) for c in chunks)
    assert chunks[-1]["malformed"] == 1 and lifted["pairs_in"] == n + 1 and lifted["pairs_kept"] > n // 2
    for B in res:
        want = pl.pixels_host(lifted, table, B)
        px = zl.read_pixels(os.path.join(root, "resolutions", str(B), "pixels.tsv"))
        assert np.array_equal(px[0], ac.rows_of(want["rowptr"])) and np.array_equal(px[1], want["col"]) and np.array_equal(px[2], want["count"])
        assert zl.read_bins_bed(os.path.join(root, "resolutions", str(B), "bins.bed")).tobytes() == zl.binnify(ac.chrom_sizes(table["table_sub"]), B).tobytes()
    want = pl.pixels_host(lifted, table, "scaffold")
    px = zl.read_pixels(os.path.join(root, "scaffolds", "pixels.tsv"))
    assert np.array_equal(px[1], want["col"]) and np.array_equal(px[2], want["count"]) and px[2].sum() == lifted["pairs_kept"]
    # lifted.pairs.gz: the kept lines in input order, and read back it lifts to itself under the identity table
    scaffolds = list(ac.scaffold_names(table["scaffold_ids"]))
    head = [ln for ln in gzip.open(os.path.join(out, "lifted.pairs.gz"), "rt").read().split("\n") if ln.startswith("#")]
    assert head[1] == "#sorted: none" and head[3] == "#chromosomes: " + " ".join(scaffolds) and head[-1].startswith("#columns:")
    ident = pl.identity_table(table["scaffold_len"], names=scaffolds)
    back = list(pl.read_pairs(os.path.join(out, "lifted.pairs.gz"), ident["names"]))
    c1, p1, c2, p2 = (np.concatenate([c[k] for c in back]) for k in ("c1", "p1", "c2", "p2"))
    kept = lifted["status"] == 0
    assert np.array_equal(c1, lifted["scaffold1"][kept]) and np.array_equal(p1, lifted["pos1"][kept]) and np.array_equal(p2, lifted["pos2"][kept])
    s.pairs_end()
    s.ctx.pairs_begin(ident)  # (a device session under the identity table: a table is the caller's, whatever the genome)
    again = s.ctx.pairs_lift(c1, p1, c2, p2)
    s.ctx.pairs_end()
    assert again["pairs_kept"] == c1.size and np.array_equal(again["scaffold1"], c1) and np.array_equal(again["pos1"], p1) and np.array_equal(again["pos2"], p2)
    assert np.array_equal(again["scaffold2"], c2) and again["status"].sum() == 0
    s.free_gpu()
