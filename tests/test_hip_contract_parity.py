"""The device's compilation of the arithmetic contract (include/ig_detmath.h: the inline-asm fma with a scalar constant, the
frexp / ldexp builtins, the double-to-float conversion under the kernel's denormal mode, the log-factorial table k_lgf_table builds,
the P_z table k_build_pz builds) against the host's, bit for bit, where the two could part and the shipped parameter sets never go:
the parameter families and operands of tests/_contract_cases.py through the probe k_debug_terms, and the P_z table itself.
tests/test_contract_precision_host.py holds the host side to mpmath at 200 bits, so this holds the kernels' arithmetic to it too."""
import numpy as np
import pytest

import _contract_cases as cc

pytestmark = pytest.mark.gpu

BASE = cc.base_params()
FAMILIES = cc.families(BASE) + cc.gpu_extra_families(BASE)


@pytest.fixture(scope="module")
def tiny():
    from instagraal_amd import synth

    return synth.make_problem(*synth.CONFIGS["tiny"])


@pytest.fixture(scope="module")
def mean_kb(tiny):
    return np.float32(tiny.S_o_A_sub_frags["len_bp"].mean() / 1000.0)


@pytest.fixture(scope="module")
def ctx(tiny):
    from instagraal_amd.sampler import problem_to_context

    c = problem_to_context(tiny)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ol(oracle_lib):
    oracle_lib.set_mode(oracle_lib.MODE_DET)
    return oracle_lib


def _p8(p):
    return [np.float32(p[k]) for k in cc.NAMES]


def _same_bits(name, what, host, dev, s, s_tot, ob):
    view = {4: np.uint32, 8: np.uint64}[host.dtype.itemsize]
    diff = np.nonzero(host.view(view) != dev.view(view))[0]
    assert diff.size == 0, "%s: %s differs at %d of %d operands; first (s, s_tot, ob, host, device): %s" % (
        name, what, diff.size, host.size, [(float(s[i]), float(s_tot[i]), int(ob[i]), host[i], dev[i], hex(int(host.view(view)[i])), hex(int(dev.view(view)[i])))
                                          for i in diff[:6]])


def test_the_base_set_is_tinys(tiny):
    assert all(np.float32(tiny.params[k]) == BASE[k] for k in cc.NAMES)


@pytest.mark.parametrize("fam", range(len(FAMILIES)), ids=[f[0] for f in FAMILIES])
def test_terms_bit_exact_over_the_families(ctx, mean_kb, ol, fam):
    """ex, exc, term and q of the device probe equal the host contract's as bits on every operand: the edges of s (zeros, -1, the
    smallest subnormal, FLT_MIN, 1, d_max, each with both neighbours, FLT_MAX, inf, NaN) against the edge counts, 60 000 random
    positive finite bit patterns and 60 000 values log-uniform in [1e-3, 1e5] against 0 .. 2048, 2^k - 1, 2^k, 2^k + 1 up to 2^31 - 1 and
    counts below 40; s_tot in {0, s, 2 s, 3 s}."""
    name, p, fast = FAMILIES[fam]
    assert cc.expect_fast(p) == fast
    s, s_tot, ob = cc.operands(p["d_max"], 60000, 60000)
    assert s.size > 120000
    ex, exc, term, q = ol.eval_terms(s, s_tot, ob, cc.param_record(ol, p))
    if name == "subnormal ex":  # expectations in the float subnormals occur, and the host keeps them: the device must not flush them
        sub = (ex > 0) & (ex < cc.FLT_MIN)
        assert sub.mean() > 0.2, float(sub.mean())
    ctx.set_params(_p8(p), mean_kb, 0)
    gex, gexc, gterm, gq = ctx.debug_eval_terms(s, s_tot, ob)
    _same_bits(name, "ex", ex, gex, s, s_tot, ob)
    _same_bits(name, "exc", exc, gexc, s, s_tot, ob)
    _same_bits(name, "q", q, gq, s, s_tot, ob)
    _same_bits(name, "term", term, gterm, s, s_tot, ob)


PZ_CASES = [
    # name, overrides, mean_kb (None: tiny's), which
    ("ends inside the table", {}, None, 0),
    ("hits the cap", {"d_max": 1.0e5}, None, 0),
    ("settled set: the cap", "settled", None, 0),
    ("fractional mean_kb", {}, 0.37, 0),
    ("one entry short of the cap", {"d_max": 4093.5 * 0.37}, 0.37, 0),
    ("d 3, the second set", {"d": 3.0, "d_max": 600.0}, None, 1),
    ("second set at the cap", {"d_max": 2.0e4, "slope": -0.9}, 1.25, 1),
    ("d_max 0", {"d_max": 0.0}, None, 1),
]


@pytest.mark.parametrize("case", range(len(PZ_CASES)), ids=[c[0] for c in PZ_CASES])
def test_pz_table_is_the_host_contracts(ctx, tiny, mean_kb, ol, case):
    """the P_z table k_build_pz leaves behind ig_set_params: its length is what ig_set_params documents (the first rank distance whose
    s_z reaches d_max, plus one, at most 4096: (int)(d_max / mean_kb + 2) in double), and pz[d] is, as bits, the host contract's
    ig_rippe(fl(d mean_kb)) for every d below it (beyond d_max that is v_inter)."""
    from instagraal_amd import synth

    name, over, mk, which = PZ_CASES[case]
    p = dict(BASE)
    if over == "settled":
        p.update({k: np.float32(v) for k, v in synth.settled_params(tiny.params).items()})
    else:
        p.update({k: np.float32(v) for k, v in over.items()})
    mk = mean_kb if mk is None else np.float32(mk)
    ctx.set_params(_p8(p), mk, which)
    pz = ctx.debug_pz_table(which)
    need = float(p["d_max"]) / float(mk) + 2.0
    want_n = min(int(need), 4096)
    assert pz.size == want_n, (name, pz.size, want_n)
    if "cap" in name and "short" not in name:
        assert want_n == 4096
    elif "short" in name:
        assert want_n == 4095
    else:
        assert 0 < want_n < 4096
    d = np.arange(want_n, dtype=np.int32)
    s_z = (d.astype(np.float32) * mk).astype(np.float32)
    ex = ol.eval_terms(s_z, np.zeros(want_n, np.float32), np.zeros(want_n, np.int32), cc.param_record(ol, p))[0]
    beyond = s_z >= p["d_max"]
    assert np.all(ex[beyond] == p["v_inter"]) and (want_n == 4096 or beyond[-1])  # a table that ends below the cap ends beyond d_max
    _same_bits(name, "pz", ex, pz, s_z, np.zeros(want_n, np.float32), d)
    if which == 0:
        ctx.set_params(_p8(BASE), mean_kb, 0)
