"""GPU tests of the ordered sum of the balancing (ig_debug_lane_sums: k_bal_marginals over caller data on a bare handle) against the
rule (instagraal_amd.balance.lane_sum), byte for byte, in every form of the kernel.

The values are order-sensitive mixtures -- mostly ones and a few 1e16, where 1e16 + 1 == 1e16 but 1e16 + 2 != 1e16 -- so another order
of the additions gives other bytes (tests/test_balance_host.py shows that for np.sum and for the reversed row): equality here says the
device adds in the rule's order.  No -0.0 among them, and none can arise (every term the product adds is a count times a
non-negative b): the packed form serves a short row with 16 lanes and relies on x + 0.0 == x for the accumulators it leaves out,
which holds for every x but -0.0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = ("default", "wave", "packed")
ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 4097, 70000)
VEC_LENGTHS = (1, 64, 65, 50001)


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


def _mixture(n, seed):
    """ones, small fractions and a few 1e16: sums that depend on the order of the additions; non-negative, no -0.0"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 0.02, 1e16, np.where(rng.random(n) < 0.5, 1.0, rng.random(n)))
    if n:
        v[0] = 1e16
    assert not np.signbit(v).any()
    return v


@pytest.fixture(scope="module")
def rows_case():
    """every length of ROW_LENGTHS, twice and shuffled, with empty rows in between: the packed form's four rows of a wave mix short,
    long and empty ones; the rule's sums are computed once"""
    from instagraal_amd import balance as bal

    rng = np.random.default_rng(5)
    lens = np.array(ROW_LENGTHS + ROW_LENGTHS[:-1] + (3, 16, 16, 16, 16, 1, 0, 0, 0, 0, 5), np.int64)
    lens = lens[rng.permutation(lens.size)]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values = _mixture(int(rowptr[-1]), 6)
    return lens, rowptr, values, bal.lane_sum(values, rowptr)


@pytest.mark.parametrize("form", FORMS)
def test_rows_of_every_length_equal_the_rule(ctx, rows_case, form):
    lens, rowptr, values, want = rows_case
    assert set(ROW_LENGTHS) <= set(lens.tolist())
    ctx.debug_balance_form(form)
    got = ctx.debug_lane_sums(values, rowptr)
    ctx.debug_balance_form("default")
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, (form, lens[bad].tolist(), got[bad], want[bad])
    # (and the order matters on this input: numpy's pairwise sum differs on some row)
    plain = np.array([values[a:b].sum() for a, b in zip(rowptr[:-1], rowptr[1:])])
    assert np.any(plain != want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", VEC_LENGTHS)
def test_the_vector_form_equals_the_rule(ctx, form, n):
    from instagraal_amd import balance as bal

    x = _mixture(n, 100 + n)
    ctx.debug_balance_form(form)
    got = ctx.debug_lane_sums(x, np.array([0, n], np.int64))
    ctx.debug_balance_form("default")
    assert got.view(np.uint64)[0] == np.float64(bal.vec_sum(x)).view(np.uint64), (form, n)


def test_bad_arguments_are_refused(ctx):
    import ctypes as C

    from instagraal_amd import hip_lib

    with pytest.raises(hip_lib.HipError, match="rowptr"):
        ctx.debug_lane_sums(np.ones(3), np.array([0, 2, 1, 3], np.int64))
    v, rp, out = np.ones(3), np.array([1, 3], np.int64), np.zeros(1)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert hip_lib.lib().ig_debug_lane_sums(ctx._h, p(v), p(rp), C.c_int64(1), p(out)) != 0 and b"starts at 0" in hip_lib.lib().ig_last_error()
    with pytest.raises(hip_lib.HipError, match="form"):
        hip_lib._ck(hip_lib.lib().ig_debug_balance_form(ctx._h, C.c_int32(3)))
    assert ctx.debug_lane_sums(np.ones(3), np.array([0, 3], np.int64))[0] == 3.0
