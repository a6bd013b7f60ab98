"""GPU tests of the polished FASTA of the polish step (ig_seq_begin / _composition / _plan / _window / _out_composition / _end,
scaffold_polish.stitch_device, polish_assembly) against the rule's host statement (scaffold_polish.stitch, composition).  Every
comparison is exact: the file's bytes, the counts."""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "polish_tiny.npz")
RUN, WAVE, GROUP_SPAN = 16, 1024, 4 * 16 * 1024  # a thread's bytes, a wave's per turn, a workgroup's: 4 waves of SEQ_WAVE_TURNS turns
LETTERS = "ACGTNRYSWKMBDHVacgtnryswkmbdhv"


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


def device_file(ctx, records, plan, window):
    from instagraal_amd import scaffold_polish as sp

    parts = []
    comp_in, comp_out = sp.stitch_device(ctx, records, plan, lambda v: parts.append(bytes(v)), window=window)
    return b"".join(parts), comp_in, comp_out


def check(ctx, records, scaffolds, junction="", width=60, windows=(4096, 1 << 28)):
    from instagraal_amd import scaffold_polish as sp

    plan = sp.stitch_plan(records, scaffolds, junction=junction, width=width)
    want, counts = sp.stitch(records, plan)
    for window in windows:
        got, comp_in, comp_out = device_file(ctx, records, plan, window)
        assert len(got) == plan["file_bytes"]
        bad = np.flatnonzero(np.frombuffer(got, np.uint8) != want)
        assert bad.size == 0, "window %d: %d bytes differ, the first at %d: %r, the rule has %r" % (window, bad.size, bad[0], got[bad[0] - 8:bad[0] + 8], bytes(want[bad[0] - 8:bad[0] + 8]))
        assert np.array_equal(comp_out, counts) and np.array_equal(comp_in, sp.composition(records))
    return plan


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(11)
    sizes = (150000, 1, 15, 16, 17, 4095, 4096, 4097, 300, 70001)
    p = np.array([20.0] * 4 + [1.0] * (len(LETTERS) - 4))
    return [("r%d" % k, "".join(rng.choice(list(LETTERS), size=n, p=p / p.sum())).encode()) for k, n in enumerate(sizes)]


def test_composition_has_every_class_in_every_size(ctx, genome):
    from instagraal_amd import pre, scaffold_polish as sp

    buf, offs, lens = pre.concatenate(genome)
    ctx.seq_begin(buf, offs, lens)
    try:
        got = ctx.seq_composition()
    finally:
        ctx.seq_end()
    want = sp.composition(genome)
    assert np.array_equal(got, want) and got.dtype == np.int64
    assert [int(x) for x in want[:, 7]] == [len(s) for _, s in genome]
    assert (want[5:8] > 0).all() and (want[0] > 0).all()  # all eight classes in the records of 4 095 .. 4 097 bases and in the first
    one = [("a", b"n"), ("b", b"GATTACAgattacaRN" * 3), ("c", b"c")]  # records of one base in front of and behind the buffer's other bytes
    buf, offs, lens = pre.concatenate(one)
    ctx.seq_begin(buf, offs, lens)
    try:
        assert np.array_equal(ctx.seq_composition(), sp.composition(one))
    finally:
        ctx.seq_end()


def test_pieces_of_every_length_alignment_and_orientation(ctx, genome):
    """forward and reversed pieces at every source alignment against every destination alignment, of every length around a run, a line
    and two lines; pieces that begin at a record's first base and end at its last, the buffer's first and last record included"""
    scaffolds, k = {}, 0
    for ori in (1, -1):
        s, at, base0 = [], 0, len(">align%+d\n" % ori)  # (the first output record: its header starts the file)
        for d in range(16):
            for a in range(16):
                fill = next(f for f in range(1, 40) if (base0 + at + f + (at + f) // 60) % 16 == d)  # a filler brings the piece to the destination d
                s.append(["r0", k, 120000 + a, 120000 + a + fill, 1])
                s.append(["r0", k, 1000 + 16 * k + a, 1000 + 16 * k + a + 45, ori])
                at += fill + 45
                k += 1
        scaffolds["align%+d" % ori] = s
    lengths = (1, 15, 16, 17, 59, 60, 61, 119, 120, 121, 122)
    for ori in (1, -1):
        at, s = 40000, []
        for n in lengths * 3:
            s.append(["r0", k, at, at + n, ori])
            at += n + 3
            k += 1
        scaffolds["lengths%+d" % ori] = s
    last = len(genome) - 1
    n_last = len(genome[last][1])
    scaffolds["ends"] = [["r0", 0, 0, 200, -1], ["r0", 1, 150000 - 200, 150000, 1], ["r0", 2, 0, 33, 1], ["r0", 3, 150000 - 33, 150000, -1],
                         ["r%d" % last, 4, n_last - 100, n_last, -1], ["r%d" % last, 5, n_last - 16, n_last, 1], ["r%d" % last, 6, 0, 50, -1], ["r1", 7, 0, 1, -1],
                         ["r2", 8, 0, 15, -1], ["r3", 9, 0, 16, -1], ["r4", 10, 0, 17, -1], ["r5", 11, 0, 4095, -1], ["r6", 12, 0, 4096, 1], ["r7", 13, 0, 4097, -1]]
    plan = check(ctx, genome, scaffolds)
    # the claim of the docstring, from the plan: reversed and forward pieces long enough for the 16-byte path at all 256 pairs of alignments
    from instagraal_amd import pre

    offs = pre.concatenate(genome)[1]
    for ori in (1, -1):
        pairs = set()
        j = plan["names"].index("align%+d" % ori)
        for p in range(int(plan["piece_first"][j]) + 1, int(plan["piece_first"][j + 1]), 2):  # (every other piece is a filler)
            b = int(plan["body"][p])
            pairs.add(((int(offs[plan["src"][p]]) + int(plan["start"][p])) % 16, (int(plan["rec_off"][j]) + int(plan["hdr_len"][j]) + b + b // 60) % 16))
        assert len(pairs) == 256 and plan["ori"][int(plan["piece_first"][j]) + 1] == ori and plan["length"][int(plan["piece_first"][j]) + 1] == 45


@pytest.mark.parametrize("width", [1, 60])
def test_bodies_headers_junctions_and_windows(ctx, genome, width):
    """bodies of 1, 60 and 61 bases, a header longer than 16 bytes and one longer than a line, junctions of 1, 6 and 130 bytes, pieces
    across a wave's 1 024 bytes, a workgroup's span and the windows' boundaries; windows of 4 096 bytes and a last partial one"""
    long_piece = 3 * GROUP_SPAN // (2 if width == 60 else 64)
    scaffolds = {
        "b1": [["r1", 0, 0, 1, 1]],
        "a_name_longer_than_sixteen_bytes": [["r0", 1, 10, 70, -1]],
        "b61": [["r0", 2, 100, 161, 1]],
        "n" * 75: [["r0", 3, 200, 230, 1], ["r8", 4, 0, 300, -1], ["r0", 5, 230, 260, 1]],
        "straddle": [["r0", 6, 300, 300 + WAVE - 37, 1], ["r0", 7, 20000, 20000 + long_piece, -1], ["r0", 8, 5000, 5000 + long_piece, 1], ["r9", 9, 69000, 70001, -1]],
        "empty": [],
        "tail": [["r7", 10, 4000, 4097, -1]],
    }
    for junction in ("", "N", "NNNNNN", "nacgtRYKM" * 14 + "NNNN"):
        plan = check(ctx, genome, scaffolds, junction=junction, width=width, windows=(4096,) if junction else (4096, 1 << 28, 16))
        assert (len(junction) == 0) == (-1 not in plan["src"]) and plan["file_bytes"] % 4096 != 0
    assert plan["file_bytes"] > 2 * GROUP_SPAN // (1 if width == 60 else 16)


def test_the_session_refuses_what_the_rule_cannot_mean(ctx, genome):
    from instagraal_amd import hip_lib, pre, scaffold_polish as sp

    buf, offs, lens = pre.concatenate(genome)
    plan = sp.stitch_plan(genome, {"s": [["r0", 0, 0, 100, 1], ["r9", 1, 0, 100, -1]]})
    out = np.zeros(plan["file_bytes"], np.uint8)
    with pytest.raises(hip_lib.HipError, match="no session"):
        ctx.seq_plan(plan)
    ctx.seq_begin(buf, offs, lens)
    try:
        with pytest.raises(hip_lib.HipError, match="a session is open"):
            ctx.seq_begin(buf, offs, lens)
        with pytest.raises(hip_lib.HipError, match="no plan"):
            ctx.seq_window(0, out)
        for key, value, what in (("body", [0, 101], "a gap or an overlap"), ("body", [0, 99], "a gap or an overlap"), ("start", [0, 70000], "piece 1 is 70000 .. 70100 of record 9"),
                                 ("length", [100, 0], "piece 1 has 0 bases"), ("src", [0, 10], "record 10 of 10"), ("ori", [1, 0], "orientation 0"),
                                 ("rec_off", [0, plan["file_bytes"] + 1], "not monotone"), ("piece_first", [0, 1], "hold 100 bases"), ("hdr_lit", [4], "header of record 0")):
            bad = dict(plan)
            bad[key] = np.array(value, plan[key].dtype)
            with pytest.raises(hip_lib.HipError, match=what):
                ctx.seq_plan(bad)
            with pytest.raises(hip_lib.HipError, match="no plan"):  # a refused plan leaves none behind
                ctx.seq_window(0, out)
        ctx.seq_plan(plan)
        with pytest.raises(hip_lib.HipError, match="multiple of 16"):
            ctx.seq_window(8, out[8:])
        with pytest.raises(hip_lib.HipError, match="multiple of 16"):
            ctx.seq_window(0, out[:40])
        with pytest.raises(hip_lib.HipError, match="of a file of"):
            ctx.seq_window(16, out)
        with pytest.raises(hip_lib.HipError, match="up to the file's end first"):
            ctx.seq_out_composition(1)
        ctx.seq_window(0, out[:64])
        ctx.seq_window(64, out[64:])
        ctx.seq_window(0, out[:32])  # stitched again: not counted again
        want, counts = sp.stitch(genome, plan)
        assert np.array_equal(out, want) and np.array_equal(ctx.seq_out_composition(1), counts)
    finally:
        ctx.seq_end()
    with pytest.raises(hip_lib.HipError, match="no session"):
        ctx.seq_end()


def test_polish_assembly_writes_the_same_folder_with_and_without_the_device(tmp_path):
    from instagraal_amd import scaffold_polish as sp

    g = np.load(GOLDEN)
    records = list(zip([str(n) for n in g["names"]], bytes(g["seq"]).split(b"\0")))
    (tmp_path / "genome.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    (tmp_path / "info_frags.txt").write_bytes(bytes(g["info_frags"]))
    for k, kw in enumerate((dict(), dict(lost="once", junction="NNNNNN"), dict(mode="fasta", width=61, window=1024))):
        a = sp.polish_assembly(str(tmp_path / "info_frags.txt"), str(tmp_path / "genome.fa"), str(tmp_path / ("dev%d" % k)), device=True, **kw)
        b = sp.polish_assembly(str(tmp_path / "info_frags.txt"), str(tmp_path / "genome.fa"), str(tmp_path / ("host%d" % k)), device=False, **kw)
        assert sorted(os.listdir(tmp_path / ("dev%d" % k))) == sorted(os.listdir(tmp_path / ("host%d" % k))) == sorted(a["files"])
        for name in a["files"]:
            assert (tmp_path / ("dev%d" % k) / name).read_bytes() == (tmp_path / ("host%d" % k) / name).read_bytes(), (kw, name)
        assert np.array_equal(a["composition"], b["composition"]) and np.array_equal(a["composition_input"], b["composition_input"]) and a["stats"] == b["stats"]


def test_run_and_polish_behind_a_run(tmp_path, capsys):
    """a small run with both switches on: ``<run folder>/polished/`` is what ``polish_assembly`` makes of the run's final info_frags.txt on the
    host alone, every input base is in the polished genome exactly once under ``lost="once"``, and the comparison table is written and printed"""
    from instagraal_amd import assembly_stats, pre, scaffold_polish as sp, synth
    from instagraal_amd.simulation import run_and_polish

    data = str(tmp_path / "data")
    synth.write_text_dataset(data, n_contigs=10, mean_frags=110, seed=7, contacts_per_frag=40)
    fasta = os.path.join(data, "genome.fa")
    np.random.seed(17)
    p2 = run_and_polish(data, fasta, output_folder=str(tmp_path / "out"), post_polish=True, stats=True, lost="once", level=2, cycles=1, bomb=True)
    out = p2.simulation.output_folder
    host = sp.polish_assembly(os.path.join(out, "info_frags.txt"), fasta, str(tmp_path / "host"), lost="once", device=False)
    assert sorted(os.listdir(os.path.join(out, "polished"))) == sorted(host["files"]) == sorted(["new_info_frags.txt", "polished_genome.fa", "lost_dna.fa", "assembly_stats.txt"])
    for name in host["files"]:
        assert open(os.path.join(out, "polished", name), "rb").read() == open(os.path.join(str(tmp_path / "host"), name), "rb").read(), name
    r = p2.polish_result
    records = pre.read_fasta(fasta)
    assert r["bases_lost"] == 0 and r["bases_duplicated"] == 0 and r["bases_input"] == sum(len(s) for _, s in records)
    assert int(r["composition"][:, 7].sum()) == r["bases_input"] and np.array_equal(r["composition_input"], sp.composition(records))
    table = open(os.path.join(out, "assembly_stats_comparison.txt")).read()
    assert table == assembly_stats.format_comparison_table({"input": assembly_stats.compute_assembly_stats(fasta),
                                                            "genome.fasta": assembly_stats.compute_assembly_stats(os.path.join(out, "genome.fasta")),
                                                            "polished": assembly_stats.compute_assembly_stats(os.path.join(out, "polished", "polished_genome.fa"))})
    assert table in capsys.readouterr().out
