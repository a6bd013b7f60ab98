"""GPU test of the combining idiom every combined pass over the contacts shares (wave_runs / wave_run_sum, ig_kernels_wave.cuh), driven
directly with chosen data (ig_debug_wave_runs) and held to the numpy rule of test_wave_runs_rule_host.py.  What the reports' own
tests cannot reach on their natural data: a run across a wave's and a workgroup's end, a run that ends and one that starts at lane
63, lanes without a key inside a run, whole waves without one, the wave that skips the scan next to one that runs it, sums that
cancel, the largest sums either width holds.  Every comparison is equality of integers; a bare handle is enough."""
import ctypes as C

import numpy as np
import pytest

import test_wave_runs_rule_host as rule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from instagraal_amd import hip_lib

    c = hip_lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(rule.CASES))
def test_the_sums_and_the_atomics_equal_the_rule(ctx, name):
    keys, values, n_dest, wides = rule.CASES[name]
    want_out, want_atomics = rule.want(name)
    for wide in wides:
        out, atomics = ctx.debug_wave_runs(keys, values, n_dest, wide=bool(wide))
        assert out.dtype == want_out.dtype and out.tobytes() == want_out.tobytes(), (name, wide)
        assert atomics == want_atomics, (name, wide)


def test_no_entry_is_no_launch(ctx):
    out, atomics = ctx.debug_wave_runs(np.zeros(0, np.int32), np.zeros(0, np.int64), 3)
    assert out.tolist() == [0, 0, 0] and atomics == 0


def test_bad_arguments_are_refused_loudly(ctx):
    from instagraal_amd import hip_lib

    keys, values = np.array([0, 1, 2, -1], np.int32), np.array([1, 2, 3, 4], np.int64)
    with pytest.raises(hip_lib.HipError, match="ig_debug_wave_runs.*entry 2 has the key 2, there are 2 words"):
        ctx.debug_wave_runs(keys, values, 2)
    lib, out, n_at = hip_lib.lib(), np.zeros(3, np.int64), C.c_int64()
    p = lambda a: C.c_void_p(a.ctypes.data)
    args = lambda k, v, n, o, a: (ctx._h, k, v, C.c_int64(n), C.c_int32(3), C.c_int32(1), o, a)
    assert lib.ig_debug_wave_runs(*args(p(keys), p(values), -1, p(out), C.byref(n_at))) != 0
    assert b"ig_debug_wave_runs" in lib.ig_last_error() and b"negative" in lib.ig_last_error()
    assert lib.ig_debug_wave_runs(ctx._h, p(keys), p(values), C.c_int64(4), C.c_int32(-1), C.c_int32(1), p(out), C.byref(n_at)) != 0
    assert b"ig_debug_wave_runs" in lib.ig_last_error() and b"negative" in lib.ig_last_error()  # (n_dest < 0)
    for bad in (args(None, p(values), 4, p(out), C.byref(n_at)), args(p(keys), None, 4, p(out), C.byref(n_at)),
                args(p(keys), p(values), 4, None, C.byref(n_at)), args(p(keys), p(values), 4, p(out), None)):
        assert lib.ig_debug_wave_runs(*bad) != 0
        assert b"ig_debug_wave_runs: NULL argument" in lib.ig_last_error()
    out, atomics = ctx.debug_wave_runs(keys, values, 3)  # the handle is as good as before
    assert out.tolist() == [1, 2, 3] and atomics == 3
