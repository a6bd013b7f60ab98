"""4DN pairs text as a rule on bytes: lines, fields, integers, contig names (numpy and plain Python, no GPU).  The device
(``hip_lib.Context.text_*``, csrc/ig_kernels_text.cuh) reproduces the arrays of ``parse_chunk`` byte for byte; ``read_pairs_bytes`` with
either of them yields what ``pairs_lift.read_pairs`` yields, on any input whatever.

A CHUNK is a run of whole lines: every line ends in ``\\n`` except possibly the last of the file.  Line ``j`` starts behind the ``j``-th
``\\n`` (line 0 at byte 0), a final stretch without ``\\n`` is a line, a chunk of 0 bytes has none.

* **Whole-chunk refusal.**  A chunk that holds a byte ``\\r`` or a byte >= 0x80 is not parsed (``to_host``): Python's text mode translates
  ``\\r\\n`` and a lone ``\\r`` and decodes UTF-8, and ``int()`` accepts digits beyond ASCII.  Such a chunk goes to the line loop of
  ``read_pairs`` whole.
* **Status of a line.**  ``COMMENT``: its first byte is ``#``.  ``MALFORMED``: fewer than ``max(cols[0..3]) + 1`` fields (split at ``\\t``
  only; an empty line is one empty field).  ``DEFERRED``: enough fields, but a position is not exactly ``[+-]?[0-9]{1,18}`` -- blanks
  around it, ``_``, 19 digits or more: whatever ``int()`` may still accept or refuse is left to Python (``complete``).  ``DATA``: the rest.
  Up to 18 digits fit an int64 without a check (10^18 < 2^63).
* **Fields of a DATA line.**  The two positions as int64; a strand bit where the column exists and the field is exactly ``-``; a contig
  id by the exact bytes of the field, -1 for an unknown name (the empty one included).
* **``#columns:``.**  The index of the first line that starts with ``#columns:`` is returned (or -1); the lines from it on are not
  parsed under the old columns (their status is ``COMMENT``, they are in none of the counts but ``lines``).  The caller applies
  ``pairs_lift._columns`` and parses the rest of the chunk again from that line's end."""
import gzip
import io
import re

import numpy as np

from . import pairs_lift

DATA, COMMENT, MALFORMED, DEFERRED = range(4)
STATUS = ("data", "comment", "malformed", "deferred")
# the order of ig_text_parse's scalars[8]
SCALARS = ("lines", "data", "comment", "malformed", "deferred", "first_columns_line", "to_host", "reserved7")
DEFAULT_CHUNK_BYTES = 64 << 20  # a starting value, not a measurement (tools/pairs_text_bench.py records what it costs)
MAX_CHUNK_BYTES = 1 << 30       # offsets inside a chunk are 32-bit on the device
DEFAULT_COLS = (1, 2, 3, 4, 5, 6)
_INT = re.compile(rb"[+-]?[0-9]{1,18}\Z")
_REFUSED = re.compile(rb"[\r\x80-\xff]")
ARRAYS = (("c1", np.int32), ("p1", np.int64), ("c2", np.int32), ("p2", np.int64), ("strands", np.uint8))


def names_bytes(names):
    """{name: id} -> {the name's bytes: id}; a name that has no UTF-8 form matches no field"""
    out = {}
    for k, v in names.items():
        try:
            out[k if isinstance(k, bytes) else str(k).encode()] = int(v)
        except UnicodeEncodeError:
            pass
    return out


def vocabulary(names):
    """the arrays ``ig_text_begin`` takes: (name_bytes uint8, name_off int64 [n + 1], name_id int32 [n]); an id outside 32 bits is -1, as
    ``Context.pairs_lift`` maps it"""
    items = list(names_bytes(names).items())
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k, _ in items])
    ids = np.array([v if 0 <= v < 1 << 31 else -1 for _, v in items], np.int64).astype(np.int32)
    return np.frombuffer(b"".join(k for k, _ in items), np.uint8), off, ids


def line_starts(buf):
    """int64 [n_lines + 1]: the start of every line and the chunk's length"""
    a = np.frombuffer(buf, np.uint8)
    if a.size == 0:
        return np.zeros(1, np.int64)
    nl = np.flatnonzero(a == 10).astype(np.int64) + 1
    if nl.size == 0 or nl[-1] != a.size:
        nl = np.concatenate((nl, [a.size]))
    return np.concatenate(([0], nl)).astype(np.int64)


def _result(n_lines, status, line_start, rows, deferred, first_columns, to_host):
    a = np.array(rows, np.int64).reshape(-1, 5)
    out = {k: a[:, i].astype(t) for i, (k, t) in enumerate(ARRAYS)}
    counts = np.bincount(status[:first_columns] if first_columns >= 0 else status, minlength=4)
    out.update(status=status, line_start=line_start, deferred=np.array(deferred, np.int64), first_columns_line=first_columns, to_host=to_host,
               counts=dict(lines=n_lines, data=int(counts[DATA]), comment=int(counts[COMMENT]), malformed=int(counts[MALFORMED]), deferred=int(counts[DEFERRED])))
    return out


def parse_chunk(buf, cols=DEFAULT_COLS, names=None):
    """The rule.  buf: bytes or uint8; cols: the six column indices of ``read_pairs``; names: {name: id}.  -> dict: ``status`` (uint8
    [n_lines]), ``line_start`` (int64 [n_lines + 1]), ``c1``, ``p1``, ``c2``, ``p2``, ``strands`` of the DATA lines in input order (int32, int64,
    int32, int64, uint8), ``deferred`` (the indices of the DEFERRED lines), ``first_columns_line``, ``to_host`` and ``counts``.  With
    ``to_host`` nothing else of the result is defined."""
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    if _REFUSED.search(buf):
        return _result(0, np.zeros(0, np.uint8), np.zeros(1, np.int64), [], [], -1, True)
    ids = names_bytes(names or {})
    ls = line_starts(buf)
    n = ls.size - 1
    status = np.full(n, COMMENT, np.uint8)
    need = max(cols[:4]) + 1
    rows, deferred, first_columns = [], [], -1
    for j in range(n):
        line = buf[ls[j]:ls[j + 1]]
        if line.endswith(b"\n"):
            line = line[:-1]
        if line.startswith(b"#"):
            if line.startswith(b"#columns:"):
                first_columns = j
                break
            continue
        f = line.split(b"\t")
        if len(f) < need:
            status[j] = MALFORMED
        elif not (_INT.match(f[cols[1]]) and _INT.match(f[cols[3]])):
            status[j] = DEFERRED
            deferred.append(j)
        else:
            status[j] = DATA
            s = (1 if cols[4] < len(f) and f[cols[4]] == b"-" else 0) | (2 if cols[5] < len(f) and f[cols[5]] == b"-" else 0)
            rows.append((ids.get(f[cols[0]], -1), int(f[cols[1]]), ids.get(f[cols[2]], -1), int(f[cols[3]]), s))
    return _result(n, status, ls, rows, deferred, first_columns, False)


def deferred_lines(res, buf):
    """the DEFERRED lines of a parsed chunk as the fields ``read_pairs`` would split them into, in input order"""
    if len(res["deferred"]) == 0:  # (a result fed on the device brings line_start only where a line is deferred)
        return
    ls = res["line_start"]
    for j in np.asarray(res["deferred"]).tolist():
        yield bytes(buf[int(ls[j]):int(ls[j + 1])]).decode("ascii").rstrip("\n").split("\t")


def complete(res, buf, cols, names):
    """``pairs_lift._parse`` on every DEFERRED line; what parses is merged into the arrays at its place in input order, the rest is
    counted as malformed -> dict: ``c1``, ``p1``, ``c2``, ``p2`` (int64), ``strands`` (uint8), ``malformed`` (of this chunk)"""
    malformed = res["counts"]["malformed"]
    late, at = [], []
    for j, parts in zip(np.asarray(res["deferred"]).tolist(), deferred_lines(res, buf)):
        rec = pairs_lift._parse(parts, cols, names)
        if rec is None:
            malformed += 1
        else:
            late.append(rec)
            at.append(j)
    out = {k: np.asarray(res[k]).astype(np.int64 if k != "strands" else np.uint8) for k, _ in ARRAYS}
    if late:
        a = np.array(late, np.int64).reshape(-1, 5)
        st = np.asarray(res["status"])
        where = np.flatnonzero(st[:res["first_columns_line"]] == DATA if res["first_columns_line"] >= 0 else st == DATA)
        order = np.argsort(np.concatenate((where, np.array(at, np.int64))), kind="stable")
        for i, (k, _) in enumerate(ARRAYS):
            out[k] = np.concatenate((out[k], a[:, i].astype(out[k].dtype)))[order]
    out["malformed"] = malformed
    return out


def blocks(path, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """the raw bytes of a pairs file (``.gz`` / ``.bgz`` by extension) in blocks of whole lines: each is cut at its last ``\\n`` and the
    rest is carried; a block grows where one line is longer than ``chunk_bytes``"""
    chunk_bytes = max(int(chunk_bytes), 1)
    opener = gzip.open if str(path).endswith((".gz", ".bgz")) else open
    with opener(path, "rb") as fh:
        carry, data = b"", fh.read(chunk_bytes)
        while data:
            ahead = fh.read(chunk_bytes)
            data = carry + data
            if not ahead:  # the file's last bytes, with or without a newline behind them
                yield data
                return
            cut = data.rfind(b"\n") + 1
            if cut:
                yield data[:cut]
            carry, data = data[cut:], ahead


def walk(path, names, parse, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The events of a pairs file, in order: ``("block",)`` in front of every block, ``("parsed", res, seg, cols)`` for a stretch of whole
    lines ``seg`` that ``parse(seg, cols)`` took under the columns ``cols``, ``("rows", rows, malformed)`` for the lines of a refused
    (``to_host``) block that the line loop of ``read_pairs`` parsed, ``("columns",)`` at every ``#columns:`` line."""
    cols = list(DEFAULT_COLS)
    for block in blocks(path, chunk_bytes):
        yield ("block",)
        seg = block
        while seg:
            res = parse(seg, cols)
            if res["to_host"]:
                rows, malformed = [], 0
                for line in io.TextIOWrapper(io.BytesIO(seg)):
                    if line.startswith("#"):
                        if line.startswith("#columns:"):
                            yield ("rows", rows, malformed)
                            yield ("columns",)
                            rows, malformed = [], 0
                            cols = pairs_lift._columns(line, cols)
                        continue
                    rec = pairs_lift._parse(line.rstrip("\n").split("\t"), cols, names)
                    if rec is None:
                        malformed += 1
                    else:
                        rows.append(rec)
                yield ("rows", rows, malformed)
                break
            yield ("parsed", res, seg, list(cols))
            j = res["first_columns_line"]
            if j < 0:
                break
            a, b = int(res["line_start"][j]), int(res["line_start"][j + 1])
            yield ("columns",)
            cols = pairs_lift._columns(seg[a:b].decode("ascii"), cols)
            seg = seg[b:]


def read_pairs_bytes(path, names, parse=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """``pairs_lift.read_pairs`` (without ``with_lines``) over raw bytes.  parse: ``(seg, cols) -> `` the dict of ``parse_chunk`` (None: the
    rule itself).  Yields dicts ``c1``, ``p1``, ``c2``, ``p2`` (int64), ``strands`` (uint8), ``malformed`` (the running count): their
    concatenation is that of ``read_pairs``' yields; a flush happens at every ``#columns:`` line and between blocks."""
    if parse is None:
        parse = lambda seg, cols: parse_chunk(seg, cols, names)  # noqa: E731
    parts, malformed = [], 0

    def flush():
        out = {k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, np.int64 if k != "strands" else np.uint8) for k, _ in ARRAYS}
        out["malformed"] = malformed
        parts.clear()
        return out

    def held():
        return any(p["c1"].size for p in parts)

    for ev in walk(path, names, parse, chunk_bytes):
        if ev[0] == "parsed":
            got = complete(ev[1], ev[2], ev[3], names)
            malformed += got.pop("malformed")
            parts.append(got)
        elif ev[0] == "rows":
            a = np.array(ev[1], np.int64).reshape(-1, 5)
            parts.append({k: a[:, i].astype(np.int64 if k != "strands" else np.uint8) for i, (k, _) in enumerate(ARRAYS)})
            malformed += ev[2]
        elif held():  # a block's start or a #columns: line
            yield flush()
    if held() or malformed:
        yield flush()
