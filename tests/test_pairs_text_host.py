"""The reader of 4DN pairs text as a rule on bytes (instagraal_amd/pairs_text.py) against the Python line loop it restates
(``pairs_lift.read_pairs``): the concatenated arrays, the malformed count and the flushes at ``#columns:`` on seeded files
(tests/_pairs_text_cases.py), the status of every planted line, the chunk sizes, ``.gz``, and ``run_pre_reader(reader="device", device=False)``
on the golden.  No GPU."""
import gzip
import os

import numpy as np
import pytest

from conftest import ROOT

import _pairs_text_cases as cases
from instagraal_amd import pairs_lift as pl, pairs_text as pt, pre

GOLDEN = os.path.join(ROOT, "tests", "golden", "pre_tiny.npz")
CODE = dict(data=pt.DATA, comment=pt.COMMENT, malformed=pt.MALFORMED, deferred=pt.DEFERRED)


def _write(tmp_path, text, name="in.pairs"):
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


def _counting_parse(names, seen):
    def parse(seg, cols):
        res = pt.parse_chunk(seg, cols, names)
        seen.append(res)
        return res
    return parse


@pytest.mark.parametrize("n_lines,n_names,strands,trailing", [(300, 1, True, True), (777, 2, False, True), (2000, 1000, True, False), (1024, 1000, False, False)])
def test_clean_files_equal_read_pairs_and_nothing_is_deferred(tmp_path, n_lines, n_names, strands, trailing):
    text, names = cases.clean(n_lines, n_names, strands, trailing, seed=n_lines)
    path = _write(tmp_path, text)
    seen = []
    got = list(pt.read_pairs_bytes(path, names, _counting_parse(names, seen)))
    want = list(pl.read_pairs(path, names))
    cases.assert_same_reading(got, want, "clean")
    assert len(got) == len(want) == 1 and got[0]["c1"].size == n_lines and got[0]["malformed"] == 0 and got[0]["c1"].dtype == want[0]["c1"].dtype
    # what keeps a reader that defers everything, or hands everything back, from passing
    assert not any(r["to_host"] for r in seen) and sum(r["counts"]["deferred"] for r in seen) == 0
    assert sum(r["counts"]["data"] for r in seen) == n_lines and (got[0]["c1"] >= 0).all()
    assert (got[0]["strands"].max() == 3) == strands
    # the header's #columns: line was found and the rest parsed again behind it
    assert seen[0]["first_columns_line"] == text.split(b"\n").index(next(x for x in text.split(b"\n") if x.startswith(b"#columns:"))) and len(seen) == 2


def test_the_status_of_every_planted_line(tmp_path):
    text, names, where = cases.planted()
    res = pt.parse_chunk(text, pt.DEFAULT_COLS, names)
    assert not res["to_host"] and res["first_columns_line"] == -1
    for j, what, status in where:
        assert res["status"][j] == CODE[status], (what, int(res["status"][j]))
    planted = {j for j, _, _ in where}
    assert all(res["status"][j] == pt.DATA for j in range(res["status"].size) if j not in planted)
    assert res["deferred"].tolist() == [j for j, _, s in where if s == "deferred"]
    assert res["counts"] == dict(lines=res["status"].size, data=int((res["status"] == 0).sum()), comment=1, malformed=2, deferred=len(res["deferred"]))
    assert np.array_equal(res["line_start"], pt.line_starts(text)) and res["line_start"][-1] == len(text)
    # the fields of the planted DATA lines
    rank = {int(j): k for k, j in enumerate(np.flatnonzero(res["status"] == pt.DATA))}
    field = lambda what, k: res[k][rank[next(j for j, w, _ in where if w == what)]]  # noqa: E731
    assert (field("+5", "p1"), field("-3", "p2"), field("007", "p1"), field("18 digits", "p1")) == (5, -3, 7, 123456789012345678)
    assert (field("an unknown contig", "c1"), field("an empty name", "c1"), field("a name that is a prefix", "c1"), field("a name that is a prefix", "c2")) == (-1, -1, -1, 2)
    assert [field(w, "strands") for w in ("strands - +", "strands . -", "strands -- and none", "no strand columns", "a readID of 5 000 bytes")] == [1, 2, 0, 0, 3]
    # ... and the whole file through complete equals the line loop: 12x and a sign alone are malformed, the blank, 1_0 and 19 digits parse
    path = _write(tmp_path, text)
    got, want = list(pt.read_pairs_bytes(path, names)), list(pl.read_pairs(path, names))
    cases.assert_same_reading(got, want, "planted")
    assert want[-1]["malformed"] == 2 + 3 and 1234567890123456789 in want[0]["p1"] and 10 in want[0]["p1"]


def test_columns_lines_in_the_body_flush_and_change_the_columns(tmp_path):
    text, names = cases.with_columns()
    path = _write(tmp_path, text)
    got, want = list(pt.read_pairs_bytes(path, names)), list(pl.read_pairs(path, names))
    assert len(got) == len(want) == 4  # a flush at every #columns: line behind the first
    for a, b in zip(got, want):
        cases.assert_same_reading([a], [b], "columns")
    assert [g["c1"].size for g in got] == [30, 25, 10, 20] and got[-1]["malformed"] == 1
    res = pt.parse_chunk(text[len(cases.HEADER):], pt.DEFAULT_COLS, names)
    assert res["first_columns_line"] == 30 and res["counts"] == dict(lines=30 + 1 + 25 + 1 + 1 + 10 + 1 + 20, data=30, comment=0, malformed=0, deferred=0)
    assert (res["status"][30:] == pt.COMMENT).all() and res["c1"].size == 30


@pytest.mark.parametrize("what,mutate", [("crlf", lambda t: t.replace(b"\n", b"\r\n")), ("a lone cr", lambda t: t.replace(b"\n", b"\r", 3)),
                                         ("a utf-8 readID", lambda t: t.replace(b"read", "réad٣".encode(), 5))])
def test_chunks_with_cr_or_bytes_beyond_ascii_go_to_the_line_loop(tmp_path, what, mutate):
    text, names = cases.clean(300, 2, seed=5)
    text = mutate(text[len(cases.HEADER):])
    assert pt.parse_chunk(text, pt.DEFAULT_COLS, names)["to_host"]
    path = _write(tmp_path, cases.HEADER + text)
    for chunk_bytes in (256, pt.DEFAULT_CHUNK_BYTES):
        seen = []
        got = list(pt.read_pairs_bytes(path, names, _counting_parse(names, seen), chunk_bytes))
        assert any(r["to_host"] for r in seen)
        cases.assert_same_reading(got, pl.read_pairs(path, names), what)
    assert sum(g["c1"].size for g in got) == 300


def test_chunk_sizes_give_the_same_arrays(tmp_path):
    files = [cases.planted()[:2], cases.with_columns(), cases.clean(500, 1000, trailing=False, seed=9), (b"", {}), (b"\n", {}), (b"#only\n#comments", {})]
    line = cases.clean(1, 1, seed=3)[0][len(cases.HEADER):]
    files.append((line * 3 + line[:-1] + b"\n" * (256 - len(line) % 256), {"chr1": 0}))  # a cut exactly at a line's end, empty lines behind it
    for k, (text, names) in enumerate(files):
        path = _write(tmp_path, text, "f%d.pairs" % k)
        want = list(pl.read_pairs(path, names))
        for chunk_bytes in (64, 256, 4096, pt.DEFAULT_CHUNK_BYTES):  # 64: lines longer than the chunk (the 5 000-byte readID: the carry grows)
            cases.assert_same_reading(pt.read_pairs_bytes(path, names, None, chunk_bytes), want, (k, chunk_bytes))
        assert [len(b) for b in pt.blocks(path, 64)] and sum(len(b) for b in pt.blocks(path, 64)) == len(text) or not text
        assert all(b.endswith(b"\n") for b in list(pt.blocks(path, 64))[:-1])


def test_a_result_without_deferred_lines_needs_no_line_starts():
    # what a chunk fed on the device brings back where nothing is deferred: the scalars alone
    assert list(pt.deferred_lines(dict(deferred=()), b"r\tchr1\t1\tchr1\t2\n")) == []
    res = pt.parse_chunk(b"r\tchr1\t 1\tchr1\t2\n", pt.DEFAULT_COLS, {"chr1": 0})
    assert list(pt.deferred_lines(res, b"r\tchr1\t 1\tchr1\t2\n")) == [["r", "chr1", " 1", "chr1", "2"]]


def test_gz_equals_plain(tmp_path):
    text, names, _ = cases.planted()
    plain = _write(tmp_path, text)
    with gzip.open(tmp_path / "in.pairs.gz", "wb") as f:
        f.write(text)
    cases.assert_same_reading(pt.read_pairs_bytes(str(tmp_path / "in.pairs.gz"), names, None, 1000), pl.read_pairs(plain, names), "gz")


def test_duplicate_and_odd_names():
    names = {"a": 0, "b": 5, "a\tb": 7, "é": 8}
    text = b"r\ta\t1\tb\t2\nr\ta\tb\t3\t4\n"
    res = pt.parse_chunk(text, pt.DEFAULT_COLS, names)
    assert res["c1"].tolist() == [0] and res["c2"].tolist() == [5] and res["status"].tolist() == [pt.DATA, pt.DEFERRED]
    b, off, ids = pt.vocabulary(names)
    assert off.tolist() == [0, 1, 2, 5, 7] and ids.tolist() == [0, 5, 7, 8] and bytes(b) == b"aba\tb\xc3\xa9"


def test_run_pre_with_the_rule_as_reader_gives_the_golden_files(tmp_path):
    g = np.load(GOLDEN, allow_pickle=False)
    records = [(str(n), bytes(g["seq"][int(o):int(o) + int(ln)])) for n, o, ln in zip(g["names"], g["rec_off"], g["rec_len"])]
    (tmp_path / "g.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in records))
    (tmp_path / "in.pairs").write_bytes(bytes(g["pairs_file"]))
    sc = pre.run_pre_reader(str(tmp_path / "g.fa"), str(tmp_path / "in.pairs"), [str(e) for e in g["enzymes"]], str(tmp_path / "out"), device=False, reader="device")
    for name, key in (("fragments_list.txt", "file_fragments_list"), ("info_contigs.txt", "file_info_contigs"), ("abs_fragments_contacts_weighted.txt", "file_abs_contacts")):
        assert (tmp_path / "out" / name).read_bytes() == bytes(g[key]), name
    assert sc["malformed_lines"] == int(g["malformed"]) > 0 and sc["pairs_kept"] == int(g["ref_total"])
    with pytest.raises(ValueError, match="reader"):
        pre.run_pre_reader(str(tmp_path / "g.fa"), str(tmp_path / "in.pairs"), [str(e) for e in g["enzymes"]], str(tmp_path / "out2"), device=False, reader="gpu")
