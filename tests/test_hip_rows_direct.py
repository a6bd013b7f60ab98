"""GPU tests of the two layers every report on the current genome shares, driven directly with chosen data (ig_debug_scan64,
ig_debug_rows_build): the 64-bit scan and the row builder at the library's default caps, held to the numpy rules of
test_rows_rule_host.py.  What the reports' own tests cannot reach on their natural data: whole runs of 1 024 entries and merge widths
from 1 024 up with the copy-back step, the scan's carry loop above 256 chunks, sums above 2^32, the scan over several arrays, the
lane patterns of the run-head ballot, ties in the merge.  Every comparison is exact equality of bytes; a bare handle is enough."""
import numpy as np
import pytest

import test_rows_rule_host as rule

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3C3C3C3C3C3C3C3


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


_WANT = {}


def _want(key, lo, word, n_rows, reduce):
    """the rule's result, computed once per input and shared"""
    if (key, reduce) not in _WANT:
        _WANT[key, reduce] = rule.rows_rule(lo, word, n_rows, reduce)
    return _WANT[key, reduce]


def _blob(got, reduce):
    return b"".join(got[k].tobytes() for k in (("rowptr", "col", "count") if reduce else ("rowptr", "word")))


def _assert_rows(got, want, reduce, what):
    assert (got["n_entries"], got["n_out"]) == (want["n_entries"], want["n_out"]), what
    for k in ("rowptr", "col", "count") if reduce else ("rowptr", "word"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("n", rule.SCAN_N)
def test_the_scan_equals_the_rule(ctx, n):
    for n_arrays, stride in rule.scan_layouts(n):
        for family in rule.SCAN_FAMILIES:
            words = rule.scan_input(family, n, n_arrays, stride)
            out, after = ctx.debug_scan64(words, n, sentinel=SENTINEL)
            what = (n, n_arrays, stride, family)
            assert out[:, :n].tobytes() == rule.scan_rule(words, n).tobytes(), what
            assert after.tobytes() == words.tobytes(), what  # the input is left alone
            assert (out[:, n:] == np.uint64(SENTINEL)).all(), what  # and so is the output between the arrays


@pytest.mark.parametrize("name", "ABC")
def test_every_length_around_the_caps_under_every_limit(ctx, name):
    lo, word, n_rows = rule.build_input(name)
    lengths = _want(name, lo, word, n_rows, False)["lengths"]
    try:
        for reduce in (False, True):
            want = _want(name, lo, word, n_rows, reduce)
            first = None
            for limits in rule.LIMITS:
                ctx.debug_assembly_contacts_limits(*limits)
                for combine in (True, False):
                    what = (name, reduce, limits, combine)
                    got = ctx.debug_rows_build(lo, word, n_rows, reduce=reduce, combine=combine)
                    _assert_rows(got, want, reduce, what)
                    assert got["forms"] == rule.forms_rule(lengths, limits), what
                    if limits == (0, 0):
                        print(name, "reduce" if reduce else "sorted", "combine" if combine else "one atomic per entry", got["forms"], "merge steps, copy-back:",
                              rule.merge_passes(lengths, limits))
                        assert got["forms"]["long"][0] > 0 and got["forms"]["longest"] == max(rule.BUILD_LENGTHS[name])
                    first = _blob(got, reduce) if first is None else first
                    assert _blob(got, reduce) == first, what
    finally:
        ctx.debug_assembly_contacts_limits(0, 0)


@pytest.mark.parametrize("order", rule.ORDERS)
def test_every_order_of_presentation(ctx, order):
    lo, word, n_rows = rule.presented(order)
    a_lo, a_word, _ = rule.build_input("A")
    for reduce in (False, True):
        want = _want("A", a_lo, a_word, n_rows, reduce)
        for combine in (True, False):
            _assert_rows(ctx.debug_rows_build(lo, word, n_rows, reduce=reduce, combine=combine), want, reduce, (order, reduce, combine))


def test_more_rows_and_more_chunks_than_one_turn_of_the_carry_loop(ctx):
    lo, word, n_rows = rule.scale_input()
    lengths = _want("scale", lo, word, n_rows, False)["lengths"]
    try:
        for limits in rule.SCALE_LIMITS:
            ctx.debug_assembly_contacts_limits(*limits)
            for reduce in (False, True):
                got = ctx.debug_rows_build(lo, word, n_rows, reduce=reduce)
                _assert_rows(got, _want("scale", lo, word, n_rows, reduce), reduce, (limits, reduce))
                assert got["forms"] == rule.forms_rule(lengths, limits), (limits, reduce)
    finally:
        ctx.debug_assembly_contacts_limits(0, 0)


def test_refusals_name_the_entry_and_leave_the_handle_right(ctx):
    from instagraal_amd import hip_lib

    lo, word, n_rows = rule.build_input("C")
    want = _want("C", lo, word, n_rows, True)

    def ok(what):
        _assert_rows(ctx.debug_rows_build(lo, word, n_rows, reduce=True), want, True, what)

    small_lo, small_word = np.array([0, 2, -1, 1], np.int32), rule.pack([5, 6, 7, 8], [1, 2, 3, 4])
    with pytest.raises(hip_lib.HipError, match="ig_debug_rows_build.*negative"):
        ctx.debug_rows_build(small_lo, small_word, -1)
    ok("behind negative rows")
    with pytest.raises(hip_lib.HipError, match="ig_debug_rows_build.*entry 1 is of row 2, there are 2 rows"):
        ctx.debug_rows_build(small_lo, small_word, 2)
    ok("behind a row out of range")
    bad = small_word.copy()
    bad[3] |= np.uint64(1 << 63)
    with pytest.raises(hip_lib.HipError, match="ig_debug_rows_build.*entry 3 has a column of 2\\^31 or more"):
        ctx.debug_rows_build(small_lo, bad, 3)
    ok("behind a column out of range")
    lib = hip_lib.lib()
    import ctypes as C

    out = np.zeros(10, np.int64)
    assert lib.ig_debug_rows_build(ctx._h, C.c_void_p(small_lo.ctypes.data), C.c_void_p(small_word.ctypes.data), C.c_int64(-1), C.c_int32(3), C.c_int32(0), C.c_int32(1),
                                   C.c_void_p(out[0:].ctypes.data), C.c_void_p(out[1:].ctypes.data), C.c_void_p(out[2:].ctypes.data)) != 0
    assert b"ig_debug_rows_build" in lib.ig_last_error() and b"negative" in lib.ig_last_error()
    rowptr = np.zeros(4, np.int64)
    assert lib.ig_debug_rows_fetch(ctx._h, C.c_void_p(rowptr.ctypes.data), C.c_int64(4), None, None, None, C.c_int64(0)) != 0  # (a refused build leaves no stale result)
    assert b"ig_debug_rows_fetch: nothing is built" in lib.ig_last_error()
    ok("behind a negative number of entries")
    # the small input itself, and no input at all
    got = ctx.debug_rows_build(small_lo, small_word, 3)
    _assert_rows(got, rule.rows_rule(small_lo, small_word, 3, False), False, "small")
    none = ctx.debug_rows_build(np.zeros(0, np.int32), np.zeros(0, np.uint64), 4, reduce=True)
    assert none["n_entries"] == none["n_out"] == 0 and none["rowptr"].tolist() == [0] * 5 and none["col"].size == 0
    nothing_kept = ctx.debug_rows_build(np.full(100, -1, np.int32), np.full(100, rule.FILLER), 0)
    assert nothing_kept["n_entries"] == 0 and nothing_kept["rowptr"].tolist() == [0] and nothing_kept["word"].size == 0
    words = np.ones((2, 8), np.uint64)
    for n in (0, 9):
        with pytest.raises(hip_lib.HipError, match="ig_debug_scan64"):
            ctx.debug_scan64(words, n)
    ok("behind refused scans")
