"""The rule of the two layers every report on the current genome shares -- the 64-bit scan and the row builder (ig_kernels_rows.cuh,
ig_host_rows.inc) -- in a few lines of numpy, the inputs the direct GPU tests (test_hip_rows_direct.py) drive the layers with, and,
here, without a GPU: both rules against a pure-Python brute force, and every property of the inputs that the GPU tests depend on,
so that a generator cannot quietly stop producing the hard case."""
import ctypes as C
import os

import numpy as np
import pytest

SHORT_CAP, LDS_CAP = 64, 1024      # LIFT_SHORT_CAP, LIFT_LDS_CAP
SCAN_THREADS, SCAN_ITEMS = 256, 8  # a workgroup of the scan, the words of a thread
SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS
MAX_COUNT = 2**31 - 1
FILLER = np.uint64(0x7FFFFFFF7FFFFFFF)  # the word of a lane without an entry (lo = -1): it must never reach a result


# ---------------------------------------------------------------- the rules

def scan_rule(words_2d, n):
    """the inclusive prefix sums, modulo 2^64, of the first n words of every array -> uint64 [n_arrays, n]"""
    return np.cumsum(np.asarray(words_2d, np.uint64)[:, :n], axis=1, dtype=np.uint64)


def rows_rule(lo, word, n_rows, reduce):
    """entry k belongs to row lo[k] (negative: no entry) and is the word column << 32 | count; every row sorted by its words as
    unsigned integers; reduce: the runs of one column inside a row become one entry, their counts summed as int64.
    -> dict: rowptr, n_entries, n_out, lengths (the rows' lengths BEFORE the reduction), and word, or col and count"""
    lo, word = np.asarray(lo, np.int64), np.asarray(word, np.uint64)
    keep = lo >= 0
    lo, word = lo[keep], word[keep]
    lengths = np.bincount(lo, minlength=n_rows).astype(np.int64)
    by = np.lexsort((word, lo))
    lo, word = lo[by], word[by]
    out = dict(n_entries=int(lo.size), lengths=lengths)
    if not reduce:
        out.update(rowptr=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), word=word, n_out=int(lo.size))
        return out
    col, cnt = (word >> np.uint64(32)).astype(np.int64), (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
    head = np.ones(lo.size, bool)
    head[1:] = (lo[1:] != lo[:-1]) | (col[1:] != col[:-1])
    first = np.nonzero(head)[0]
    count = np.add.reduceat(cnt, first) if first.size else np.zeros(0, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(lo[first], minlength=n_rows))]).astype(np.int64)
    out.update(rowptr=rowptr, col=col[first].astype(np.int32), count=count.astype(np.int64), n_out=int(first.size))
    return out


def effective_limits(limits):
    """the limits as the library applies them: 0 is the default, a value above a form's capacity counts as the capacity"""
    short_max, lds_max = limits
    return min(short_max or SHORT_CAP, SHORT_CAP), min(lds_max or LDS_CAP, LDS_CAP)


def forms_rule(lengths, limits):
    """the work lists of the three sort forms from the rows' lengths, as ``Context.debug_assembly_contacts_forms`` reports them"""
    short_max, lds_max = effective_limits(limits)
    n = np.asarray(lengths, np.int64)
    rows = dict(short=(n >= 2) & (n <= short_max), lds=(n >= 2) & (n > short_max) & (n <= lds_max), long=(n >= 2) & (n > short_max) & (n > lds_max))
    out = {k: (int(rows[k].sum()), int(n[rows[k]].sum())) for k in rows}
    out["runs"] = int(((n[rows["long"]] + lds_max - 1) // lds_max).sum()) if lds_max > 1 else 0
    out["longest"] = int(n[rows["long"]].max()) if rows["long"].any() else 0
    return out


def merge_passes(lengths, limits):
    """(merge steps of the long form, whether a copy-back step follows them): the widths double from the lds limit while they are
    below the longest long row; an odd number of steps leaves the rows in the scratch buffer"""
    longest, width, passes = forms_rule(lengths, limits)["longest"], effective_limits(limits)[1], 0
    while width < longest:
        width, passes = 2 * width, passes + 1
    return passes, passes % 2 == 1


def scan_chunks(n):
    return (n + SCAN_CHUNK - 1) // SCAN_CHUNK


# ---------------------------------------------------------------- the inputs of the scan tests

SCAN_N = (1, 7, 8, 9, 2047, 2048, 2049, 4097, 524_287, 524_288, 524_289, 1_100_000)
SCAN_FAMILIES = ("random", "ones", "signed", "top_first", "top_chunk_end")
TOP = np.uint64(1 << 63)


def scan_layouts(n):
    return ((1, n), (3, n + 5))


def top_chunk_end_index(n):
    """the last word of the last whole chunk (of the only, partial one where n is below a chunk)"""
    return n // SCAN_CHUNK * SCAN_CHUNK - 1 if n >= SCAN_CHUNK else n - 1


def scan_input(family, n, n_arrays, stride, seed=0):
    """uint64 [n_arrays, stride]; the stride - n words behind every array hold noise the scan must not read into its sums"""
    rng = np.random.default_rng([seed, SCAN_FAMILIES.index(family), n, n_arrays])
    w = rng.integers(0, 2**64, size=(n_arrays, stride), dtype=np.uint64)
    if family == "ones":
        w[:, :n] = 1
    elif family == "signed":  # small signed values as two's complement: what the junction profile's difference arrays hold
        w[:, :n] = rng.integers(-5, 6, size=(n_arrays, n)).astype(np.int64).view(np.uint64)
    elif family in ("top_first", "top_chunk_end"):
        w[:, :n] = 0
        w[:, 0 if family == "top_first" else top_chunk_end_index(n)] = TOP
    return w


# ---------------------------------------------------------------- the inputs of the row builder's tests

COMMON_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3071, 3072, 3073)
BUILD_LENGTHS = dict(A=COMMON_LENGTHS + (4095, 4096, 4097, 5000), B=COMMON_LENGTHS + (4095, 4096), C=tuple(n for n in COMMON_LENGTHS if n <= 2048))
LIMITS = ((0, 0), (64, 65), (4, 16), (3, 5), (1, 1))  # (3, 5): runs whose length is no power of two
# the merge steps of the long form per build under each of LIMITS (the widths double from the lds limit up to the longest row: 5 000,
# 4 096, 2 048); an odd number leaves the rows in the scratch buffer, and a copy-back step follows
BUILD_PASSES = dict(A=(3, 7, 9, 10, 13), B=(2, 6, 8, 10, 12), C=(1, 5, 7, 9, 11))
FAMILIES = ("random", "equal", "descending", "ascending", "two_columns", "five_columns", "extreme_columns", "max_counts")


def pack(col, cnt):
    return (np.asarray(col, np.uint64) << np.uint64(32)) | np.asarray(cnt, np.uint64)


def family_words(family, n, rng):
    """n words of one row; columns in [0, 2^31), counts in [0, 2^31)"""
    k = np.arange(n, dtype=np.int64)
    if family == "random":
        return pack(rng.integers(0, 2**31, n), rng.integers(0, 2**31, n))
    if family == "equal":
        return np.full(n, pack(rng.integers(0, 2**31), rng.integers(0, 2**31)), np.uint64)
    if family == "descending":  # strictly, as words: the columns fall, the counts rise
        return pack(10_000 - k, k)
    if family == "ascending":
        return pack(7 + k // 3, 5 * k)
    if family == "two_columns":  # ties on the column, broken by counts that all differ
        return pack(np.where(k % 2 == 0, 11, 12), (n - k) * 3 + k % 2)
    if family == "five_columns":
        return pack(rng.choice(np.array([0, 1, 1000, 2**30, 2**31 - 1]), n), rng.integers(0, 100, n))
    if family == "extreme_columns":
        return pack(np.where(rng.integers(0, 2, n) == 0, 0, 2**31 - 1), rng.integers(0, 2**31, n))
    assert family == "max_counts"  # one column, every count 2^31 - 1: 5 000 of them reduce to about 1.07e13
    return np.full(n, pack(77, MAX_COUNT), np.uint64)


def build_rows(name):
    """the rows of build A, B or C -> list of (length, family): every length of the build once, the lengths up to 129 eight times and
    those between the lds limit and 4 000 three times, the families cycled over them; the 5 000 of build A has one column and counts of
    2^31 - 1.  An empty row follows every third row, and the last row is empty."""
    lengths = list(BUILD_LENGTHS[name]) + [n for rep in range(len(FAMILIES) - 1) for n in COMMON_LENGTHS if n <= 129]
    lengths += [n for rep in range(2) for n in BUILD_LENGTHS[name] if 1024 < n < 4000]
    shift = "ABC".index(name) * 3
    rows = []
    for i, n in enumerate(lengths):
        rows.append((n, "max_counts" if n == 5000 else FAMILIES[(i + shift) % len(FAMILIES)]))
        if i % 3 == 2:
            rows.append((0, "random"))
    order = np.random.default_rng(["ABC".index(name), 1]).permutation(len(rows))
    return [rows[i] for i in order] + [(0, "random")]


_BUILDS = {}


def build_input(name):
    """-> (lo int32 [n], word uint64 [n], n_rows): the entries grouped by row, inside a row as the family gives them.  Computed once."""
    if name not in _BUILDS:
        rng = np.random.default_rng(["ABC".index(name), 2])
        rows = build_rows(name)
        lo = np.repeat(np.arange(len(rows), dtype=np.int32), [n for n, _ in rows])
        word = np.concatenate([family_words(f, n, rng) for n, f in rows])
        lo.setflags(write=False)
        word.setflags(write=False)
        _BUILDS[name] = (lo, word, len(rows))
    return _BUILDS[name]


ORDERS = ("grouped", "permuted", "crafted")


def presented(order):
    """build A's entries in another order of presentation -> (lo, word, n_rows).  "crafted": the first two waves hold 60 lanes of
    different rows, then one row over lanes 60 .. 63 and lanes 0 .. 3 of the next wave, then another row up to lane 63; a whole wave
    without an entry; the bulk grouped by row with every third lane empty (lo = -1 inside the runs); two more empty waves; and a
    ragged last wave"""
    lo, word, n_rows = build_input("A")
    if order == "grouped":
        return lo, word, n_rows
    if order == "permuted":
        by = np.random.default_rng(5).permutation(lo.size)
        return lo[by], word[by], n_rows
    lengths = np.bincount(lo, minlength=n_rows)
    start = np.concatenate([[0], np.cumsum(lengths)])
    big, other = int(np.argmax(lengths)), int(np.nonzero(lengths == 4097)[0][0])
    singles = np.nonzero((lengths >= 1) & (np.arange(n_rows) != big) & (np.arange(n_rows) != other))[0][:60]
    head = np.concatenate([start[singles], start[big] + np.arange(8), start[other] + np.arange(60)])  # two waves
    assert head.size == 128 and np.unique(head).size == 128
    rest = np.setdiff1d(np.arange(lo.size), head)
    tail, bulk = rest[-37:], rest[:-37]
    third = np.full(bulk.size + (bulk.size + 1) // 2, -1, np.int64)  # two entries, then a lane without one
    third[np.arange(bulk.size) + np.arange(bulk.size) // 2] = bulk
    third = np.concatenate([third, np.full(-third.size % 64, -1, np.int64)])
    empty = np.full(64, -1, np.int64)
    src = np.concatenate([head, empty, third, empty, empty, tail])
    out_lo = np.where(src >= 0, lo[np.maximum(src, 0)], -1).astype(np.int32)
    out_word = np.where(src >= 0, word[np.maximum(src, 0)], FILLER).astype(np.uint64)
    return out_lo, out_word, n_rows


SCALE_ROWS = 600_000
SCALE_CHAIN = 60_000  # the first rows: row r holds 1 .. 3 entries of column r and 1 .. 4 of column r + 1, so that column r + 1 closes row r and opens row r + 1
SCALE_LIMITS = ((0, 0), (2, 4))
_SCALE = []


def scale_input():
    """-> (lo, word, n_rows): 600 000 rows and about 1.2 M entries -- the chain of equal columns across the rows' ends, three longer
    rows, and rows of 0 .. 3 entries with columns from a few values; the entries grouped by row, shuffled inside a row"""
    if not _SCALE:
        rng = np.random.default_rng(11)
        r = np.arange(SCALE_CHAIN, dtype=np.int64)
        k1, k2 = 1 + r % 3, 1 + (r // 3) % 4
        chain_lo = np.concatenate([np.repeat(r, k1), np.repeat(r, k2)])
        chain_col = np.concatenate([np.repeat(r, k1), np.repeat(r + 1, k2)])
        lengths = rng.choice(4, SCALE_ROWS - SCALE_CHAIN, p=[0.15, 0.2, 0.25, 0.4])
        for row, n in ((100, 3000), (200_000, 1500), (SCALE_ROWS - SCALE_CHAIN - 2, 70)):
            lengths[row] = n
        rest_lo = np.repeat(np.arange(SCALE_CHAIN, SCALE_ROWS, dtype=np.int64), lengths)
        rest_col = rng.integers(0, 6, rest_lo.size)
        lo, col = np.concatenate([chain_lo, rest_lo]), np.concatenate([chain_col, rest_col])
        cnt = rng.integers(0, 2**31, lo.size)
        cnt[rng.random(lo.size) < 0.3] = MAX_COUNT
        by = np.lexsort((rng.random(lo.size), lo))
        lo, word = lo[by].astype(np.int32), pack(col[by], cnt[by])
        lo.setflags(write=False)
        word.setflags(write=False)
        _SCALE.append((lo, word, SCALE_ROWS))
    return _SCALE[0]


def equal_column_runs(lo, word):
    """of the sorted entries: first and last index of every run of one (row, column) -> (first, last)"""
    lo, word = np.asarray(lo, np.int64), np.asarray(word, np.uint64)
    keep = lo >= 0
    lo, word = lo[keep], word[keep]
    by = np.lexsort((word, lo))
    lo, col = lo[by], (word[by] >> np.uint64(32)).astype(np.int64)
    head = np.ones(lo.size, bool)
    head[1:] = (lo[1:] != lo[:-1]) | (col[1:] != col[:-1])
    first = np.nonzero(head)[0]
    return first, np.concatenate([first[1:], [lo.size]]) - 1


# ---------------------------------------------------------------- the CPU tests

def _brute_rows(lo, word, n_rows, reduce):
    rows = [[] for _ in range(n_rows)]
    for r, w in zip(lo.tolist(), word.tolist()):
        if r >= 0:
            rows[r].append(w)
    rowptr, words, cols, counts = [0], [], [], []
    for entries in rows:
        entries.sort()
        if reduce:
            sums = {}
            for w in entries:
                sums[w >> 32] = sums.get(w >> 32, 0) + (w & 0xFFFFFFFF)
            cols += sorted(sums)
            counts += [sums[c] for c in sorted(sums)]
            rowptr.append(len(cols))
        else:
            words += entries
            rowptr.append(len(words))
    return rowptr, words, cols, counts


def test_the_rules_equal_a_brute_force():
    rng = np.random.default_rng(3)
    for n, n_rows in ((0, 0), (0, 5), (1, 1), (300, 7), (400, 90), (257, 1)):
        lo = rng.integers(-1, max(n_rows, 1), n) if n_rows else np.full(n, -1)
        word = pack(rng.integers(0, 4, n) * (2**31 - 1) // 3, rng.integers(0, 2**31, n))
        word[rng.random(n) < 0.3] = pack(2**31 - 1, MAX_COUNT)  # equal words, and sums above 2^32
        for reduce in (False, True):
            got = rows_rule(lo, word, n_rows, reduce)
            rowptr, words, cols, counts = _brute_rows(lo, word, n_rows, reduce)
            assert got["rowptr"].tolist() == rowptr and got["lengths"].tolist() == [int((lo == r).sum()) for r in range(n_rows)]
            assert got["n_entries"] == int((lo >= 0).sum()) and got["n_out"] == (len(cols) if reduce else len(words))
            if reduce:
                assert got["col"].tolist() == cols and got["count"].tolist() == counts and got["col"].dtype == np.int32 and got["count"].dtype == np.int64
            else:
                assert got["word"].tolist() == words and got["word"].dtype == np.uint64
    for n_arrays, stride, n in ((1, 1, 1), (3, 300, 295), (2, 64, 64)):
        w = rng.integers(0, 2**64, size=(n_arrays, stride), dtype=np.uint64)
        got = scan_rule(w, n)
        assert got.shape == (n_arrays, n) and got.dtype == np.uint64
        for a in range(n_arrays):
            run, want = 0, []
            for v in w[a, :n].tolist():
                run = (run + v) % 2**64
                want.append(run)
            assert got[a].tolist() == want
    # the forms, by hand: rows of 1, 2, 5, 6, 17 entries under the limits (2, 5) and (1, 1), and the defaults' capacities
    n = np.array([0, 1, 2, 5, 6, 17])
    assert forms_rule(n, (2, 5)) == dict(short=(1, 2), lds=(1, 5), long=(2, 23), runs=2 + 4, longest=17) and merge_passes(n, (2, 5)) == (2, False)
    assert forms_rule(n, (1, 1)) == dict(short=(0, 0), lds=(0, 0), long=(4, 30), runs=0, longest=17) and merge_passes(n, (1, 1)) == (5, True)
    assert effective_limits((0, 0)) == effective_limits((100, 5000)) == (SHORT_CAP, LDS_CAP)
    assert forms_rule([64, 65, 1024, 1025], (0, 0)) == dict(short=(1, 64), lds=(2, 1089), long=(1, 1025), runs=2, longest=1025)


def test_the_inputs_hold_every_case_the_gpu_tests_depend_on():
    # ---- the scan: the chunk counts around the carry loop's second turn (above SCAN_THREADS chunks), 64-bit prefixes, negatives
    assert [scan_chunks(n) for n in SCAN_N] == [1, 1, 1, 1, 1, 1, 2, 3, 256, 256, 257, 538]
    assert sum(scan_chunks(n) > SCAN_THREADS for n in SCAN_N) == 2 and SCAN_ITEMS in SCAN_N and SCAN_CHUNK in SCAN_N
    for n in (9, 4097, 524_289):
        for n_arrays, stride in scan_layouts(n):
            assert (n_arrays == 1 and stride == n) or (n_arrays > 1 and stride > n)
            w = scan_input("random", n, n_arrays, stride)
            assert (scan_rule(w, n) > np.uint64(2**32)).any() and len({w[a, :n].tobytes() for a in range(n_arrays)}) == n_arrays
            s = scan_input("signed", n, n_arrays, stride).view(np.int64)[:, :n]
            assert (s < 0).any() and (s > 0).any() and np.abs(s).max() <= 5
            assert (scan_rule(scan_input("signed", n, n_arrays, stride), n).view(np.int64) < 0).any()
            assert np.array_equal(scan_rule(scan_input("ones", n, n_arrays, stride), n)[0], np.arange(1, n + 1, dtype=np.uint64))
            for family in ("top_first", "top_chunk_end"):
                t = scan_input(family, n, n_arrays, stride)[:, :n]
                at = 0 if family == "top_first" else top_chunk_end_index(n)
                assert (t[:, at] == TOP).all() and np.count_nonzero(t) == n_arrays and (at == n - 1 or (at + 1) % SCAN_CHUNK == 0 or at == 0)
    assert top_chunk_end_index(524_289) == 524_287 and top_chunk_end_index(2047) == 2046 and top_chunk_end_index(2048) == 2047
    # ---- the three builds: the lengths, the forms and the merge steps at the default caps and under every limit
    for name in "ABC":
        lo, word, n_rows = build_input(name)
        want = rows_rule(lo, word, n_rows, True)
        n = want["lengths"]
        assert set(n.tolist()) == set(BUILD_LENGTHS[name]) and 25_000 < lo.size < 80_000 and n[-1] == 0
        assert np.any((n[1:-1] == 0) & (n[:-2] > 0) & (n[2:] > 0))  # an empty row between two that are not
        assert (word >> np.uint64(63)).max() == 0 and (word & np.uint64(1 << 31)).max() == 0  # columns and counts below 2^31
        assert [merge_passes(n, limits) for limits in LIMITS] == [(p, p % 2 == 1) for p in BUILD_PASSES[name]]
        forms = forms_rule(n, (0, 0))
        assert forms["long"][0] > 0 and forms["lds"][0] > 0 and forms["short"][0] > 0 and forms["longest"] == max(BUILD_LENGTHS[name])
        assert forms["runs"] == int(((n[n > LDS_CAP] + LDS_CAP - 1) // LDS_CAP).sum()) and LDS_CAP in n and 2 * LDS_CAP in n  # whole runs without a padding lane
        assert want["n_out"] < want["n_entries"] and want["count"].max() > 2**32
        # every family meets the short, the lds and the long form
        met = {(f, "short" if m <= SHORT_CAP else "lds" if m <= LDS_CAP else "long") for m, f in build_rows(name) if m >= 2}
        assert {f for f, _ in met} == set(FAMILIES) and sum(1 for f, k in met if k == "long") >= 6 and sum(1 for f, k in met if k == "short") == len(FAMILIES)
    lo, word, n_rows = build_input("A")
    want = rows_rule(lo, word, n_rows, True)
    big = int(np.argmax(want["lengths"]))
    assert want["lengths"][big] == 5000 and want["rowptr"][big + 1] - want["rowptr"][big] == 1 and want["count"][want["rowptr"][big]] == 5000 * MAX_COUNT > 10**13
    # ties: rows whose words are all equal, and rows whose equal columns differ only in count, in the long form
    start = np.concatenate([[0], np.cumsum(want["lengths"])])
    tied = [(int(m), np.unique(word[start[r]:start[r] + m]).size, np.unique(word[start[r]:start[r] + m] >> np.uint64(32)).size)
            for r, m in enumerate(want["lengths"]) if m > LDS_CAP]
    assert any(words == 1 for _, words, _ in tied) and any(words == m and cols == 2 for m, words, cols in tied)
    # ---- the orders of presentation
    ref = rows_rule(lo, word, n_rows, False)
    for order in ORDERS:
        o_lo, o_word, o_rows = presented(order)
        got = rows_rule(o_lo, o_word, o_rows, False)
        assert got["word"].tobytes() == ref["word"].tobytes() and got["rowptr"].tobytes() == ref["rowptr"].tobytes()
    p_lo = presented("permuted")[0].astype(np.int64)
    assert np.mean(p_lo[1:] != p_lo[:-1]) > 0.8  # nearly every lane is a head
    c_lo = presented("crafted")[0].astype(np.int64)
    assert c_lo.size % 64 != 0 and c_lo[-1] >= 0 and np.unique(c_lo[:60]).size == 60 and c_lo[:60].min() >= 0
    assert np.unique(c_lo[60:68]).size == 1 and c_lo[60] >= 0 and c_lo[59] != c_lo[60] != c_lo[68]  # a run over the last four lanes of a wave and the first four of the next
    assert np.unique(c_lo[68:128]).size == 1 and c_lo[127] >= 0 and c_lo[128] == -1  # a run that ends at lane 63
    waves = c_lo[:c_lo.size // 64 * 64].reshape(-1, 64)
    bulk = c_lo[3 * 64:3 * 64 + 90_000]  # behind the two waves and the empty one: two entries, then a lane without one
    assert (waves == -1).all(axis=1).sum() >= 3 and (bulk[2::3] == -1).all() and (bulk[0::3] >= 0).all() and (bulk[1::3] >= 0).all()
    inside = (c_lo[1:-1] == -1) & (c_lo[:-2] >= 0) & (c_lo[:-2] == c_lo[2:])
    assert inside.sum() > 1000  # lanes without an entry inside a run of one row
    assert ((waves[:-1, 63] >= 0) & (waves[:-1, 63] == waves[1:, 0])).sum() > 100  # runs that go on in the next wave
    # ---- the scale input
    lo, word, n_rows = scale_input()
    assert n_rows == SCALE_ROWS and scan_chunks(n_rows) > SCAN_THREADS and scan_chunks(lo.size) > 2 * SCAN_THREADS and 1_100_000 < lo.size < 1_400_000
    want = rows_rule(lo, word, n_rows, True)
    n = want["lengths"]
    assert np.mean(n <= 3) > 0.9 and set(range(4)) <= set(n.tolist()) and n.max() == 3000 and want["count"].max() > 2**32
    for limits in SCALE_LIMITS:
        forms = forms_rule(n, limits)
        assert forms["long"][0] > 0 and forms["short"][0] > 0 and forms["lds"][0] > 0
    first, last = equal_column_runs(lo, word)
    assert np.any(first // SCAN_CHUNK != last // SCAN_CHUNK) and np.any(first // SCAN_ITEMS != last // SCAN_ITEMS)  # runs across a chunk's and a thread's end
    # the same column closes one row and opens the next: only the row's bit splits the two runs
    s_lo = np.sort(lo.astype(np.int64))
    s_col = (word[np.lexsort((word, lo))] >> np.uint64(32)).astype(np.int64)
    seam = (s_lo[1:] != s_lo[:-1]) & (s_col[1:] == s_col[:-1])
    assert seam.sum() > SCALE_CHAIN // 2 and np.any(seam[SCAN_CHUNK - 1::SCAN_CHUNK]) and np.any(seam[SCAN_ITEMS - 1::SCAN_ITEMS])  # also where a chunk / a thread ends


def test_the_debug_symbols_exist_in_the_built_library():
    from instagraal_amd import hip_lib

    if not os.path.exists(hip_lib.LIB_PATH):
        pytest.fail("libinstagraal_hip.so is not built: run __graft_entry__.build()")
    lib = C.CDLL(hip_lib.LIB_PATH)
    for name in ("ig_debug_scan64", "ig_debug_rows_build", "ig_debug_rows_fetch"):
        assert hasattr(lib, name), name
    header = open(os.path.join(hip_lib.ROOT, "include", "instagraal_hip.h")).read()
    for name in ("int ig_debug_scan64(ig_ctx* ctx, uint64_t* in, int32_t n, int32_t n_arrays, int64_t stride, uint64_t* out);",
                 "int ig_debug_rows_build(ig_ctx* ctx, const int32_t* lo, const uint64_t* word, int64_t n, int32_t n_rows, int32_t reduce, int32_t combine,",
                 "int ig_debug_rows_fetch(ig_ctx* ctx, int64_t* rowptr, int64_t n_rowptr, uint64_t* word, int32_t* col, int64_t* count, int64_t capacity);"):
        assert name in header, name
