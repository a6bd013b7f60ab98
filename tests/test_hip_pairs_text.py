"""GPU tests of the reader of 4DN pairs text on the device (ig_text_begin / _parse / _fetch / _feed_pre / _feed_pairs / _end,
pairs_lift.read_pairs_device, run_pre_reader(reader="device"), the sampler's pairs_reader = "device") against the rule on bytes
(instagraal_amd/pairs_text.py), array for array, and against the Python reader."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _pairs_text_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pre_tiny.npz")
KEYS = ("status", "line_start", "c1", "p1", "c2", "p2", "strands", "deferred")


def _span():
    src = open(os.path.join(ROOT, "instagraal_amd", "csrc", "ig_kernels_text.cuh")).read()
    return int(re.search(r"#define TEXT_LDS_SPAN (\d+)", src).group(1)), int(re.search(r"#define TEXT_LINES (\d+)", src).group(1))


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.text_end()
    c.close()


def _assert_chunk(ctx, text, cols, names, what):
    """one chunk on an open session against the rule -> the rule's result"""
    from instagraal_amd import pairs_text as pt

    want = pt.parse_chunk(text, cols, names)
    got = ctx.text_fetch(ctx.text_parse(text, cols))
    assert got["to_host"] == want["to_host"], what
    if want["to_host"]:
        return want
    assert got["counts"] == want["counts"] and got["first_columns_line"] == want["first_columns_line"], (what, got["counts"], want["counts"], got["first_columns_line"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)
    for k, t in pt.ARRAYS:
        assert got[k].dtype == t, (what, k)
    return want


def test_the_clean_and_the_planted_families_against_the_rule(ctx):
    from instagraal_amd import pairs_text as pt

    for n_lines, n_names, strands, trailing in ((300, 1, True, True), (777, 2, False, True), (2000, 1000, True, False)):
        text, names = cases.clean(n_lines, n_names, strands, trailing, seed=n_lines)
        ctx.text_begin(names)
        head = _assert_chunk(ctx, text, pt.DEFAULT_COLS, names, ("clean, the header", n_lines))
        body = text[head["line_start"][head["first_columns_line"] + 1]:]
        res = _assert_chunk(ctx, body, pt.DEFAULT_COLS, names, ("clean", n_lines))
        assert res["counts"] == dict(lines=n_lines, data=n_lines, comment=0, malformed=0, deferred=0) and (res["c1"] >= 0).all()
        ctx.text_end()
    text, names, where = cases.planted()
    ctx.text_begin(names)
    res = _assert_chunk(ctx, text, pt.DEFAULT_COLS, names, "planted")
    assert res["counts"]["deferred"] == sum(s == "deferred" for _, _, s in where) and res["counts"]["malformed"] == 2
    text, names = cases.with_columns()
    assert _assert_chunk(ctx, text[len(cases.HEADER):], pt.DEFAULT_COLS, names, "columns")["first_columns_line"] == 30
    _assert_chunk(ctx, text[len(cases.HEADER):], (2, 0, 3, 1, 5, 6), names, "reordered")
    for what, bad in (("crlf", text.replace(b"\n", b"\r\n")), ("a lone cr at the end", text + b"\r"), ("utf-8", text + "é".encode())):
        assert _assert_chunk(ctx, bad, pt.DEFAULT_COLS, names, what)["to_host"]
        with pytest.raises(Exception, match="to_host"):
            ctx.text_fetch(dict(ctx.text_parse(bad), to_host=False))
    ctx.text_end()


def test_chunk_sizes_and_both_forms_of_the_parse(ctx):
    from instagraal_amd import pairs_text as pt

    span, per = _span()
    rng = np.random.default_rng(3)
    names = cases.vocabulary(1000)
    ctx.text_begin(names)
    line = cases.data_line(rng, names)
    chunks = [("0 bytes", b""), ("1 line without a newline", line[:-1]), ("only comments", b"#a\n##b\n#c"), ("a newline at byte 0", b"\n" + line), ("only newlines", b"\n" * 700)]
    for n in (15, 16, 17, 8193):  # the last 16-byte run partly, wholly and just beyond filled; two workgroups of the mark and a byte
        body = b"".join(cases.data_line(rng, names) for _ in range(n // 30 + 2))
        chunks.append(("%d bytes" % n, body[:n]))
    chunks.append(("about 20 KB", b"".join(cases.data_line(rng, names) for _ in range(400))))  # five workgroups of the mark: the scan's bases
    # the same lines on both sides of the span threshold, padded by the readID: 256 lines of just under and just over span / 256 bytes
    short = [cases.data_line(rng, names, read_id="r%05d" % k) for k in range(3 * per)]
    for what, width in (("staged", span // per - 1), ("direct", span // per + 1), ("the threshold itself", span // per)):
        padded = [ln.replace(b"r", b"r" + b"x" * (width - len(ln)), 1) for ln in short]
        assert all(len(ln) == width for ln in padded)
        chunks.append((what, b"".join(padded)))
    # a workgroup whose lines force the direct form next to one that is staged
    chunks.append(("direct next to staged", b"".join(short[:per]) + cases.data_line(rng, names, read_id="L" * (span + 5)) + b"".join(short[per:2 * per + 7])))
    results = {}
    for what, text in chunks:
        results[what] = _assert_chunk(ctx, text, pt.DEFAULT_COLS, names, what)
    assert results["0 bytes"]["counts"]["lines"] == 0 and results["1 line without a newline"]["counts"]["data"] == 1 and results["only comments"]["counts"]["comment"] == 3
    assert results["only newlines"]["counts"] == dict(lines=700, data=0, comment=0, malformed=700, deferred=0)
    for k in ("c1", "p1", "c2", "p2", "strands"):  # both forms return the same fields of the same lines
        assert np.array_equal(results["staged"][k], results["direct"][k]) and np.array_equal(results["staged"][k], results["the threshold itself"][k]), k
    assert results["staged"]["counts"]["data"] == 3 * per
    ctx.text_end()


def test_refusals(ctx):
    from instagraal_amd import hip_lib, pairs_text as pt

    lib, h = hip_lib.lib(), ctx._h
    sc, cols = np.zeros(8, np.int64), np.array(pt.DEFAULT_COLS, np.int32)
    one = np.frombuffer(b"x", np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    err = lambda: lib.ig_last_error().decode()  # noqa: E731
    assert lib.ig_text_end(h) == 0  # without a session: harmless
    assert lib.ig_text_parse(h, p(one), 1, p(cols), p(sc), None) != 0 and "no session" in err()
    assert lib.ig_text_feed_pre(h, p(sc), None) != 0 and "no session" in err()
    ctx.text_begin({"chr1": 0})
    with pytest.raises(hip_lib.HipError, match="a session is open"):
        ctx.text_begin({"chr1": 0})
    free0 = __import__("torch").cuda.mem_get_info()[0]
    assert lib.ig_text_parse(h, p(one), (1 << 30) + 1, p(cols), p(sc), None) != 0 and "2^30" in err()  # on the argument: the one byte is never read
    assert __import__("torch").cuda.mem_get_info()[0] == free0  # ... and nothing of that size was allocated
    assert lib.ig_text_parse(h, p(one), -1, p(cols), p(sc), None) != 0 and lib.ig_text_parse(h, None, 1, p(cols), p(sc), None) != 0 and "NULL" in err()
    with pytest.raises(hip_lib.HipError, match="nothing is parsed"):
        ctx.text_feed_pre()
    ctx.text_parse(b"r\tchr1\t5\tchr1\t9\n")
    with pytest.raises(hip_lib.HipError, match="ig_pre_begin first"):
        ctx.text_feed_pre()
    with pytest.raises(hip_lib.HipError, match="ig_pairs_begin first"):
        ctx.text_feed_pairs()
    with pytest.raises(hip_lib.HipError, match="column 1 is -1"):
        ctx.text_parse(b"x\n", (1, -1, 3, 4, 5, 6))
    ctx.text_end()


def test_read_pairs_device_equals_read_pairs(ctx, tmp_path):
    from instagraal_amd import pairs_lift as pl

    files = [cases.planted()[:2], cases.with_columns(), cases.clean(500, 1000, trailing=False, seed=9)]
    text, names = cases.clean(300, 2, seed=5)
    files.append((text.replace(b"\n", b"\r\n", 40), names))
    for k, (text, names) in enumerate(files):
        path = tmp_path / ("f%d.pairs" % k)
        path.write_bytes(text)
        want = list(pl.read_pairs(str(path), names))
        for chunk_bytes in (4096, None):
            got = list(pl.read_pairs_device(str(path), names, ctx, chunk_bytes))
            cases.assert_same_reading(got, want, (k, chunk_bytes))
        assert len(got) == len(want)  # one block: the flushes are those at the #columns: lines


def test_run_pre_with_the_device_reader_gives_the_golden_files(ctx, tmp_path):
    from instagraal_amd import pre

    g = np.load(GOLDEN, allow_pickle=False)
    records = [(str(n), bytes(g["seq"][int(o):int(o) + int(ln)])) for n, o, ln in zip(g["names"], g["rec_off"], g["rec_len"])]
    (tmp_path / "g.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    (tmp_path / "in.pairs").write_bytes(bytes(g["pairs_file"]))
    enzymes = [str(e) for e in g["enzymes"]]
    sc = pre.run_pre_reader(str(tmp_path / "g.fa"), str(tmp_path / "in.pairs"), enzymes, str(tmp_path / "out"), device=ctx, reader="device")
    for name, key in (("fragments_list.txt", "file_fragments_list"), ("info_contigs.txt", "file_info_contigs"), ("abs_fragments_contacts_weighted.txt", "file_abs_contacts")):
        assert (tmp_path / "out" / name).read_bytes() == bytes(g[key]), name
    assert sc == pre.run_pre(str(tmp_path / "g.fa"), str(tmp_path / "in.pairs"), enzymes, str(tmp_path / "host"), device=ctx) and sc["malformed_lines"] == int(g["malformed"]) > 0
    # a clean file: nothing deferred, so nothing but scalars comes back from the device (no line_start, no indices)
    rng = np.random.default_rng(8)
    names = {n: k for k, (n, _) in enumerate(records)}
    lines = []
    for _ in range(700):
        a, b = (records[int(rng.integers(len(records)))] for _ in range(2))
        lines.append(b"r\t%s\t%d\t%s\t%d\t+\t-\n" % (a[0].encode(), rng.integers(1, len(a[1]) + 1), b[0].encode(), rng.integers(1, len(b[1]) + 1)))
    (tmp_path / "clean.pairs").write_bytes(b"".join(lines))
    dev = pre.run_pre_reader(str(tmp_path / "g.fa"), str(tmp_path / "clean.pairs"), enzymes, str(tmp_path / "clean_dev"), device=ctx, reader="device")
    assert dev == pre.run_pre(str(tmp_path / "g.fa"), str(tmp_path / "clean.pairs"), enzymes, str(tmp_path / "clean_host"), device=ctx)
    assert dev["malformed_lines"] == 0 and dev["pairs_in"] == 700 and len(names) == len(records)
    assert (tmp_path / "clean_dev" / "abs_fragments_contacts_weighted.txt").read_bytes() == (tmp_path / "clean_host" / "abs_fragments_contacts_weighted.txt").read_bytes()


def _pairs_file(path, table, n, seed):
    """a pairs file over the table's contigs under their names, with what Python has to decide in it: a deferred line that parses, one
    that does not, a malformed line, an unknown contig"""
    import test_hip_pairs_lift as tp

    c1, p1, c2, p2, strands = tp._pairs(table, n, seed)
    name = {v: k for k, v in table["names"].items()}
    lines = [cases.HEADER]
    for k in range(n):
        lines.append(b"\t".join([b"r%d" % k, name.get(int(c1[k]), "nowhere").encode(), b"%d" % p1[k], name.get(int(c2[k]), "nowhere").encode(), b"%d" % p2[k],
                                 b"-" if strands[k] & 1 else b"+", b"-" if strands[k] & 2 else b"+"]) + b"\n")
    first = name[int(c1[np.flatnonzero(c1 >= 0)[0]])].encode()
    lines += [b"r\t" + first + b"\t 7\t" + first + b"\t1_1\t-\t+\n", b"r\t" + first + b"\t7x\t" + first + b"\t11\t-\t+\n", b"short\tline\n"]
    with open(path, "wb") as f:
        f.write(b"".join(lines))


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_the_sampler_reads_a_file_on_the_device_as_on_the_host(cfg, tmp_path):
    import test_hip_pairs_lift as tp

    prob, s = tp._sampler(cfg, seed=4)
    try:
        if s.contig_names is None:
            s.contig_names = {"contig_%d" % k: k for k in range(int(np.max(s.S_o_A_sub_frags["id_c"])) + 1)}
        table = s.pairs_begin()
        s.pairs_end()
        path = str(tmp_path / "reads.pairs")
        _pairs_file(path, table, 3000, 11)
        assert s.pairs_reader == "host"
        host, law_host = s.pairs_contacts(path, binsize=1000), s.pairs_distance_law(path)
        s.pairs_reader = "device"
        dev, law_dev = s.pairs_contacts(path, binsize=1000), s.pairs_distance_law(path)
        for k in ("rowptr", "col", "count"):
            assert host[k].tobytes() == dev[k].tobytes(), k
        for k in ("pairs_in", "pairs_kept", "end1_not_covered", "end2_not_covered", "unplaced", "malformed"):
            assert host[k] == dev[k], (k, host[k], dev[k])
        assert host["malformed"] == 2 and host["pairs_in"] == 3001 and host["pairs_kept"] > 0
        a, b = law_host, law_dev
        assert a["counts"].tobytes() == b["counts"].tobytes() and a["counts"].sum() > 0 and a["malformed"] == b["malformed"] == 2
        with pytest.raises(ValueError, match="reader"):
            s.pairs_reader = "gpu"
            s.pairs_contacts(path, binsize=1000)
    finally:
        s.pairs_end()
