"""Seeded 4DN pairs text for the tests of the reader on bytes (instagraal_amd/pairs_text.py) and of its device form: the CLEAN family
(nothing deferred, nothing for the host) and the PLANTED family (lines whose status the rule names).  A helper, not a test module."""
import numpy as np

HEADER = b"## pairs format v1.0\n#shape: upper triangle\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
HEADER_NO_STRANDS = b"## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2\n"


def vocabulary(n_names):
    """{name: id}: 1 name; 2 names, one a prefix of the other; 1 000 names -- prefixes of one another (ctg1, ctg10, ctg100) and, in a
    table of 2 048 slots, probes longer than one"""
    if n_names == 1:
        return {"chr1": 0}
    if n_names == 2:
        return {"ab": 0, "a": 1}
    return {"ctg%d" % k: k for k in range(n_names)}


def data_line(rng, names, strands=True, read_id=None, extra=False):
    keys = list(names)
    a, b = keys[int(rng.integers(len(keys)))], keys[int(rng.integers(len(keys)))]
    f = [read_id or "read%d" % int(rng.integers(1 << 30)), a, str(int(rng.integers(1, 250_000_000))), b, str(int(rng.integers(1, 250_000_000)))]
    if strands:
        f += ["+-"[int(rng.integers(2))], "+-"[int(rng.integers(2))]]
        if extra:
            f += ["UU", "60"]
    return "\t".join(f).encode() + b"\n"


def clean(n_lines, n_names, strands=True, trailing=True, seed=0, read_id=None):
    """-> (text, names): a header with its #columns: line, then n_lines data lines"""
    rng = np.random.default_rng(seed)
    names = vocabulary(n_names)
    text = (HEADER if strands else HEADER_NO_STRANDS) + b"".join(data_line(rng, names, strands, read_id, extra=k % 3 == 0) for k in range(n_lines))
    return (text if trailing else text[:-1]), names


# (what the line shows, the line, the status the rule names): positions in a body of good lines with the default columns
PLANTED = (
    ("an empty line", b"\n", "malformed"),
    ("too few fields", b"r\tchr1\t5\tchr1\n", "malformed"),
    ("12x", b"r\tchr1\t12x\tchr1\t7\t+\t-\n", "deferred"),
    ("a blank in front", b"r\tchr1\t 12\tchr1\t7\t+\t-\n", "deferred"),
    ("+5", b"r\tchr1\t+5\tchr1\t7\t+\t-\n", "data"),
    ("-3", b"r\tchr1\t9\tchr1\t-3\t+\t-\n", "data"),
    ("1_0", b"r\tchr1\t1_0\tchr1\t7\t+\t-\n", "deferred"),
    ("007", b"r\tchr1\t007\tchr1\t7\t+\t-\n", "data"),
    ("18 digits", b"r\tchr1\t123456789012345678\tchr1\t7\t+\t-\n", "data"),
    ("19 digits", b"r\tchr1\t1234567890123456789\tchr1\t7\t+\t-\n", "deferred"),
    ("an empty position", b"r\tchr1\t\tchr1\t7\t+\t-\n", "deferred"),
    ("a sign alone", b"r\tchr1\t-\tchr1\t7\t+\t-\n", "deferred"),
    ("an unknown contig", b"r\tchrUn\t5\tchr1\t7\t+\t-\n", "data"),
    ("an empty name", b"r\t\t5\tchr1\t7\t+\t-\n", "data"),
    ("strands - +", b"r\tchr1\t5\tchr1\t7\t-\t+\n", "data"),
    ("strands . -", b"r\tchr1\t5\tchr1\t7\t.\t-\n", "data"),
    ("strands -- and none", b"r\tchr1\t5\tchr1\t7\t--\n", "data"),
    ("no strand columns", b"r\tchr1\t5\tchr1\t7\n", "data"),
    ("a comment in the body", b"#a comment\tchr1\t5\tchr1\t7\n", "comment"),
    ("a readID of 5 000 bytes", b"R" * 5000 + b"\tchr1\t5\tchr1\t7\t-\t-\n", "data"),
    ("a name that is a prefix", b"r\tchr\t5\tchr11\t7\t+\t+\n", "data"),
)


def planted(seed=1, good=40):
    """-> (text, names, [(line index, what, status)]): no header (line indices are the file's), `good` clean lines around each planted one"""
    rng = np.random.default_rng(seed)
    names = {"chr1": 0, "chr2": 1, "chr11": 2}
    lines, where = [], []
    for what, line, status in PLANTED:
        lines += [data_line(rng, names) for _ in range(int(rng.integers(1, good)))]
        where.append((len(lines), what, status))
        lines.append(line)
    lines += [data_line(rng, names) for _ in range(good)]
    return b"".join(lines), names, where


def with_columns(seed=2):
    """#columns: in the body: reordered (the positions in front, no strands named: the old strand columns stay), then with unknown
    columns only (nothing changes), then reordered again with strands"""
    rng = np.random.default_rng(seed)
    names = {"chr1": 0, "chr2": 1}
    out = [HEADER] + [data_line(rng, names) for _ in range(30)]
    out.append(b"#columns: pos1 pos2 chr1 chr2 readID\n")
    for _ in range(25):
        f = data_line(rng, names).rstrip(b"\n").split(b"\t")
        out.append(b"\t".join([f[2], f[4], f[1], f[3], f[0], f[5], f[6]]) + b"\n")
    out.append(b"bad\tline\n")
    out.append(b"#columns: foo bar baz\n")
    for _ in range(10):
        f = data_line(rng, names).rstrip(b"\n").split(b"\t")
        out.append(b"\t".join([f[2], f[4], f[1], f[3], f[0], f[5], f[6]]) + b"\n")
    out.append(b"#columns: strand2 strand1 chr2 pos2 chr1 pos1\n")
    for _ in range(20):
        f = data_line(rng, names).rstrip(b"\n").split(b"\t")
        out.append(b"\t".join([f[6], f[5], f[3], f[4], f[1], f[2]]) + b"\n")
    return b"".join(out), names


def concat(chunks):
    """the yields of a reader as one: (c1, p1, c2, p2, strands, the last malformed count)"""
    chunks = list(chunks)
    cat = lambda k, t: np.concatenate([c[k] for c in chunks]).astype(t) if chunks else np.zeros(0, t)  # noqa: E731
    return [cat("c1", np.int64), cat("p1", np.int64), cat("c2", np.int64), cat("p2", np.int64), cat("strands", np.uint8)], (chunks[-1]["malformed"] if chunks else 0)


def assert_same_reading(got, want, what):
    (a, ma), (b, mb) = concat(got), concat(want)
    for x, y, k in zip(a, b, ("c1", "p1", "c2", "p2", "strands")):
        assert x.tobytes() == y.tobytes(), (what, k)
    assert ma == mb, (what, ma, mb)
