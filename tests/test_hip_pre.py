"""GPU tests of the input folder from a FASTA and read pairs (ig_pre_begin / _digest / _fragments / _add_pairs / _pixels_build / _rows /
_fetch / _clear / _end, pre.run_pre, simulation.run_from_pairs) against the rule's host statement (instagraal_amd.pre) and the golden
made by the reference's functions (tests/golden/pre_tiny.npz).  Every comparison is exact: the arrays' bytes, the files' bytes."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pre_tiny.npz")
RUN, WORD, GROUP = 16, 64, 16 * 256  # PRE_RUN, a bitmap word, PRE_RUN * PRE_THREADS: bases of a thread, a word, a workgroup


def _scan_chunk():
    src = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_kernels_rows.cuh")).read()
    return int(re.search(r"#define SCAN_THREADS (\d+)", src).group(1)) * int(re.search(r"#define SCAN_ITEMS (\d+)", src).group(1))


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN, allow_pickle=False)
    records = [(str(n), bytes(g["seq"][int(o):int(o) + int(ln)])) for n, o, ln in zip(g["names"], g["rec_off"], g["rec_len"])]
    return g, records, [str(e) for e in g["enzymes"]]


def _concrete(site, rng):
    """letters that match the site: its plain letters as they are, any other by one of its set"""
    from instagraal_amd import pre

    return "".join(rng.choice(list(pre.IUPAC[ch])) for ch in site)


def edge_genome(enzymes, seed):
    """The first record starts the coordinate, so its positions are the device's: every site is planted across thread-run, bitmap-word
    and workgroup boundaries at every offset, and across the boundary of a scan chunk of bitmap words; behind it records of 1,
    L - 1, L bases, of 15 / 16 / 17, 63 / 64 / 65 and 4095 / 4096 / 4097 bases with a site at their first and last base."""
    rng = np.random.default_rng(seed)
    L = max(len(s) for s, _ in enzymes)
    n_big = WORD * _scan_chunk() + GROUP + 1
    big = rng.choice(list("ACGTacgtNR"), size=n_big, p=(0.22, 0.22, 0.22, 0.22, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02))

    def plant(arr, at, text):
        if 0 <= at and at + len(text) <= arr.size:
            arr[at:at + len(text)] = list(text)

    for site, _ in enzymes:
        for j in range(1, len(site)):
            plant(big, RUN * (10 + 3 * j) - j, _concrete(site, rng))
            plant(big, WORD * (60 + j) - j, _concrete(site, rng))
            plant(big, GROUP * (1 + j) - j, _concrete(site, rng))
        plant(big, WORD * _scan_chunk() - len(site) // 2, _concrete(site, rng))
        plant(big, 0, _concrete(site, rng))
        plant(big, n_big - len(site), _concrete(site, rng))
    records = [("big", "".join(big).encode())]
    for n in (1, L - 1, L, RUN - 1, RUN, RUN + 1, WORD - 1, WORD, WORD + 1, GROUP - 1, GROUP, GROUP + 1, 777):
        if n < 1:
            continue
        s = rng.choice(list("ACGTn"), size=n)
        for site, _ in enzymes:
            plant(s, 0, _concrete(site, rng))
            plant(s, n - len(site), _concrete(site, rng).lower())
        records.append(("r%d_%d" % (len(records), n), "".join(s).encode()))
    return records


def _assert_digest(got, records, want, what):
    from instagraal_amd import pre

    assert got["n_frags"] == want["n_frags"], what
    for k in ("rec_first", "frag_rec", "start", "end", "rec_len"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["gc_count"].tobytes() == pre.gc_counts(records, want).tobytes(), (what, "gc")


@pytest.mark.parametrize("specs", [["DpnII"], ["Arima"], ["GATCNNNNNNNNGATC^"], ["^GATCGATCGATCGATC", "HinfI", "MseI", "NlaIII"], ["N^N"]])
def test_the_digest_and_gc_are_the_rules_at_every_boundary(ctx, specs):
    from instagraal_amd import pre

    enzymes = pre.expand_enzymes(specs)
    records = edge_genome(enzymes, 3)
    want = pre.digest(records, enzymes)
    buf, offs, lens = pre.concatenate(records)
    assert (buf.size + 63) // 64 > _scan_chunk()  # more than one scan chunk of bitmap words
    ctx.pre_begin(buf, offs, lens)
    try:
        got = ctx.pre_digest(enzymes, piece=1000)
        _assert_digest(got, records, want, specs)
        if specs == ["DpnII"]:  # a second digest of the session, under other enzymes
            _assert_digest(ctx.pre_digest("HinfI"), records, pre.digest(records, "HinfI"), "second digest")
    finally:
        ctx.pre_end()
    assert want["n_frags"] > 2 * len(records)


def test_the_golden_digest_and_pixels(ctx, golden):
    from instagraal_amd import pre

    g, records, enzymes = golden
    want = pre.digest(records, enzymes)
    ctx.pre_begin(g["seq"], g["rec_off"], g["rec_len"])
    try:
        got = ctx.pre_digest(enzymes)
        _assert_digest(got, records, want, "golden")
        assert np.array_equal(got["start"], g["bins_start"]) and np.array_equal(got["end"], g["bins_end"])
        frac = np.array([pre.gc_fraction(a, b) for a, b in zip(got["gc_count"], got["end"] - got["start"])], np.float64)
        assert frac.tobytes() == g["ref_gc"].tobytes()
        p1, p2 = pre._clip32(g["p1"]), pre._clip32(g["p2"])
        sc = ctx.pre_add_pairs(g["c1"], p1, g["c2"], p2)
        px = ctx.pre_pixels(piece=500)
        rows = np.repeat(np.arange(want["n_frags"]), np.diff(px["rowptr"]))
        assert np.array_equal(rows, g["ref_bin1"]) and np.array_equal(px["col"], g["ref_bin2"]) and np.array_equal(px["count"], g["ref_count"])
        assert px["pairs_kept"] == int(g["ref_total"]) == sc["pairs_kept"] == sc["pairs_stored"]
        host = pre.pixels_host(want, g["c1"], g["p1"], g["c2"], g["p2"])
        assert [px[k] for k in pre.SCALARS] == [host[k] for k in pre.SCALARS]
        # the single ends, each paired with itself: the diagonal pixel is the fragment
        ctx.pre_clear()
        ctx.pre_add_pairs(g["end_rec"], pre._clip32(g["end_pos"]), g["end_rec"], pre._clip32(g["end_pos"]))
        one = ctx.pre_pixels()
        hit = g["ref_end_frag"][g["ref_end_frag"] >= 0]
        assert np.array_equal(np.diff(one["rowptr"]), np.bincount(hit, minlength=want["n_frags"]) > 0) and one["count"].sum() == hit.size
        assert one["end1_without_fragment"] == int((g["ref_end_frag"] < 0).sum()) and one["end2_without_fragment"] == 0
    finally:
        ctx.pre_end()


def _assert_pixels(got, want, what):
    from instagraal_amd import pre

    for k in ("rowptr", "col", "count"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert [got[k] for k in pre.SCALARS] == [want[k] for k in pre.SCALARS], what
    assert got["pairs_in"] == got["pairs_kept"] + got["end1_without_fragment"] + got["end2_without_fragment"], what


def _seeded_pairs(dig, n, seed):
    rng = np.random.default_rng(seed)
    R = len(dig["rec_len"])
    c1 = rng.integers(-1, R + 1, n)
    c2 = np.where(rng.random(n) < 0.7, c1, rng.integers(-1, R + 1, n))
    ln = np.concatenate((dig["rec_len"], [50, 50]))
    p1 = rng.integers(-1, ln[c1] + 4)
    p2 = np.where(rng.random(n) < 0.5, np.maximum(p1 + rng.integers(-300, 300, n), 0), rng.integers(-1, ln[c2] + 4))
    return c1.astype(np.int64), p1.astype(np.int64), c2.astype(np.int64), p2.astype(np.int64)


def test_pairs_in_one_chunk_and_in_several(ctx, golden):
    from instagraal_amd import pre

    g, records, enzymes = golden
    dig = pre.digest(records, enzymes)
    ctx.pre_begin(g["seq"], g["rec_off"], g["rec_len"])
    try:
        ctx.pre_digest(enzymes)
        for n in (0, 1, 4097):
            pairs = _seeded_pairs(dig, n, 11 + n)
            want = pre.pixels_host(dig, *pairs)
            ctx.pre_clear()
            ctx.pre_add_pairs(*pairs)
            _assert_pixels(ctx.pre_pixels(), want, ("one chunk", n))
            ctx.pre_clear()
            stored = 0
            for a, b in ((0, n // 3), (n // 3, n // 3), (n // 3, n - 1), (max(n - 1, 0), n)):  # the store grows; an empty chunk between
                sc = ctx.pre_add_pairs(*(x[a:b] for x in pairs))
                stored += sc["pairs_kept"]
                assert sc["pairs_stored"] == stored and sc["pairs_in"] == max(b - a, 0)
            _assert_pixels(ctx.pre_pixels(piece=97), want, ("several chunks", n))
            _assert_pixels(ctx.pre_pixels(), want, ("built twice", n))
        # all pairs on one pixel, and on the diagonal
        f = dig["n_frags"] - 2
        r, s = int(dig["frag_rec"][f]), int(dig["start"][f])
        n = 5000
        ctx.pre_clear()
        ctx.pre_add_pairs(np.full(n, r), np.full(n, s + 1), np.full(n, r), np.full(n, int(dig["end"][f])))
        px = ctx.pre_pixels()
        assert px["pixels"] == 1 and px["col"].tolist() == [f] and px["count"].tolist() == [n] and px["rowptr"].tolist() == [0] * (f + 1) + [1, 1]
    finally:
        ctx.pre_end()


def test_rows_longer_than_every_limit_of_a_sort_form(ctx, golden):
    """a row of about a hundred distinct columns under the limits (4, 16), (8, 64) and the defaults: the wave, the workgroup and the merge form"""
    from instagraal_amd import pre

    g, records, enzymes = golden
    dig = pre.digest(records, enzymes)
    rng = np.random.default_rng(8)
    n = 6000
    big = int(np.argmax(dig["rec_len"]))
    a, b = int(dig["rec_first"][big]), int(dig["rec_first"][big + 1])
    assert b - a > 80
    f1 = np.where(rng.random(n) < 0.5, a, rng.integers(a, b, n))  # half of the pairs in the row of the record's first fragment
    f2 = rng.integers(a, b, n)
    pairs = (np.full(n, big), dig["start"][f1] + 1, np.full(n, big), dig["end"][f2])
    want = pre.pixels_host(dig, *pairs)
    assert np.diff(want["rowptr"]).max() > 64
    ctx.pre_begin(g["seq"], g["rec_off"], g["rec_len"])
    try:
        ctx.pre_digest(enzymes)
        ctx.pre_add_pairs(*pairs)
        for limits in ((4, 16), (8, 64), (0, 0)):
            ctx.debug_assembly_contacts_limits(*limits)
            _assert_pixels(ctx.pre_pixels(), want, limits)
    finally:
        ctx.debug_assembly_contacts_limits(0, 0)
        ctx.pre_end()


def test_refusals_name_the_entry_and_leave_the_handle_right(ctx, golden):
    from instagraal_amd import hip_lib, pre

    g, records, enzymes = golden
    buf, offs, lens = pre.concatenate([("a", b"ACGTGATCAA"), ("b", b"GATC")])
    for call, who in ((ctx.pre_end, "ig_pre_end"), (ctx.pre_clear, "ig_pre_clear"), (ctx.pre_pixels, "ig_pre_pixels_build")):
        with pytest.raises(hip_lib.HipError, match=who + ": no session"):
            call()
    bad = buf.copy()
    bad[12] = ord("X")
    with pytest.raises(hip_lib.HipError, match="ig_pre_begin: record 1, position 2: the character 0x58"):
        ctx.pre_begin(bad, offs, lens)
    bad = buf.copy()
    bad[10] = ord("A")
    with pytest.raises(hip_lib.HipError, match="ig_pre_begin: the byte behind record 0"):
        ctx.pre_begin(bad, offs, lens)
    with pytest.raises(hip_lib.HipError, match="ig_pre_begin: record 1 starts at 10"):
        ctx.pre_begin(buf, offs - np.array([0, 1]), lens)
    with pytest.raises(hip_lib.HipError, match="ig_pre_begin: record 1 is empty"):
        ctx.pre_begin(buf, offs, lens * np.array([1, 0]))
    ctx.pre_begin(buf, offs, lens)
    try:
        with pytest.raises(hip_lib.HipError, match="ig_pre_begin: a session is open"):
            ctx.pre_begin(buf, offs, lens)
        with pytest.raises(hip_lib.HipError, match="ig_pre_add_pairs: nothing is digested"):
            ctx.pre_add_pairs([0], [1], [0], [2])
        with pytest.raises(hip_lib.HipError, match="ig_pre_pixels_build: nothing is digested"):
            ctx.pre_pixels()
        with pytest.raises(hip_lib.HipError, match="enzyme 0, letter 1: the mask 0x11"):
            _bad_masks(ctx)
        got = ctx.pre_digest("DpnII")
        assert got["start"].tolist() == [0, 4, 0] and got["end"].tolist() == [4, 10, 4] and got["gc_count"].tolist() == [2, 2, 2]
        import ctypes as C

        lib = hip_lib.lib()
        assert lib.ig_pre_fragments(ctx._h, C.c_int64(2), C.c_int64(2), None, None, None, None) != 0 and b"fragments 2 .. 4 of 3" in lib.ig_last_error()
        with pytest.raises(hip_lib.HipError, match="ig_pre_pixels_rows: nothing is built"):
            lib_rows = np.zeros(4, np.int64)
            hip_lib._ck(lib.ig_pre_pixels_rows(ctx._h, hip_lib._p(lib_rows), C.c_int64(4)))
        ctx.pre_add_pairs([0, 1, 5], [1, 4, 1], [1, 0, 0], [9, 10, 1])
        px = ctx.pre_pixels()
        assert px["rowptr"].tolist() == [0, 1, 2, 2] and px["col"].tolist() == [2, 2] and px["count"].tolist() == [1, 1] and px["ends_beyond_record"] == 1
        assert lib.ig_pre_pixels_fetch(ctx._h, C.c_int64(1), C.c_int64(2), None, None) != 0 and b"pixels 1 .. 3 of 2" in lib.ig_last_error()
    finally:
        ctx.pre_end()
    with pytest.raises(hip_lib.HipError, match="ig_pre_digest: no session"):
        ctx.pre_digest("DpnII")


def _bad_masks(ctx):
    """ig_pre_digest with a mask that is neither a set of plain letters nor the valid bit"""
    import ctypes as C

    from instagraal_amd import hip_lib

    ln, cut = np.array([2], np.int32), np.array([1], np.int32)
    masks = np.zeros((1, 16), np.uint8)
    masks[0, :2] = (4, 17)
    per, nf = np.zeros(2, np.int64), C.c_int64()
    hip_lib._ck(hip_lib.lib().ig_pre_digest(ctx._h, C.c_int32(1), hip_lib._p(ln), hip_lib._p(cut), hip_lib._p(masks), hip_lib._p(per), C.byref(nf), None))


def _write_inputs(tmp_path, g, records):
    (tmp_path / "g.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    (tmp_path / "in.pairs").write_bytes(bytes(g["pairs_file"]))
    return str(tmp_path / "g.fa"), str(tmp_path / "in.pairs")


def test_run_pre_writes_the_same_folder_on_the_device_and_on_the_host(ctx, golden, tmp_path):
    from instagraal_amd import pre

    g, records, enzymes = golden
    fasta, pairs = _write_inputs(tmp_path, g, records)
    host = pre.run_pre(fasta, pairs, enzymes, str(tmp_path / "host"), device=False)
    dev = pre.run_pre(fasta, pairs, enzymes, str(tmp_path / "dev"), device=ctx, chunk_pairs=700)
    own = pre.run_pre(fasta, pairs, enzymes, str(tmp_path / "own"), device=True)
    assert host == dev == own and host["malformed_lines"] == 1
    for name, key in (("fragments_list.txt", "file_fragments_list"), ("info_contigs.txt", "file_info_contigs"), ("abs_fragments_contacts_weighted.txt", "file_abs_contacts")):
        want = bytes(g[key])
        for folder in ("host", "dev", "own"):
            assert (tmp_path / folder / name).read_bytes() == want, (folder, name)


def seeded_assembly_inputs(tmp_path, n_contigs=8, contig_bp=30_000, pairs_per_kb=150, seed=5):
    """a seeded genome and pairs file the pyramid's filters keep: contigs of about a hundred DpnII fragments, pairs that decay with distance"""
    rng = np.random.default_rng(seed)
    records = [("ctg%02d" % (k + 1), "".join(rng.choice(list("ACGT"), size=contig_bp + 1000 * k)).encode()) for k in range(n_contigs)]
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    lens = np.array([len(s) for _, s in records])
    n = int(lens.sum() // 1000 * pairs_per_kb)
    c1 = rng.choice(n_contigs, n, p=lens / lens.sum())
    p1 = rng.integers(1, lens[c1] + 1)
    cis = rng.random(n) < 0.9
    c2 = np.where(cis, c1, rng.choice(n_contigs, n))
    off = (np.exp(rng.uniform(np.log(50), np.log(20_000), n)) * rng.choice((-1, 1), n)).astype(np.int64)
    p2 = np.where(cis, np.clip(p1 + off, 1, lens[c1]), rng.integers(1, lens[c2] + 1))
    with open(tmp_path / "reads.pairs", "w") as f:
        f.write("## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n")
        f.write("".join("r%d\t%s\t%d\t%s\t%d\t+\t-\n" % (k, records[c1[k]][0], p1[k], records[c2[k]][0], p2[k]) for k in range(n)))
    return str(fasta), str(tmp_path / "reads.pairs"), n


def test_run_from_pairs_goes_through_the_pyramid_and_a_cycle(tmp_path):
    from instagraal_amd.simulation import run_from_pairs

    fasta, pairs, n = seeded_assembly_inputs(tmp_path)
    np.random.seed(17)
    p2 = run_from_pairs(fasta, pairs, "DpnII", str(tmp_path / "out"), level=2, cycles=1, bomb=True)
    contacts = open(tmp_path / "out" / "pre" / "abs_fragments_contacts_weighted.txt").read().splitlines()
    assert sum(int(ln.split("\t")[2]) for ln in contacts[1:]) == n and int(contacts[0].split("\t")[2]) == len(contacts) - 1  # every pair is in a pixel
    assert len(open(tmp_path / "out" / "pre" / "info_contigs.txt").read().splitlines()) == 1 + 8
    assert sorted(os.listdir(tmp_path / "out" / "pre"))[:3] == ["abs_fragments_contacts_weighted.txt", "fragments_list.txt", "info_contigs.txt"]
    out = p2.simulation.output_folder
    assert os.path.getsize(os.path.join(out, "genome.fasta")) > 0 and os.path.getsize(os.path.join(out, "info_frags.txt")) > 0
