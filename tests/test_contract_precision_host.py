"""The arithmetic contract (include/ig_detmath.h) as gcc compiles it -- oracle_lib.eval_terms in MODE_DET -- against mpmath at
200 bits: ig_powf and ig_expf to the header's "within 1 ulp of the correctly rounded value", the per-contact term to a multiple
of 2^-53 of the magnitudes of its parts that is derived from the header's stated bounds (K_DERIVATION below), over the parameter
families and operands of tests/_contract_cases.py.  tests/test_hip_contract_parity.py holds the device to the host contract bit
for bit on the same families, which ties the kernels' arithmetic to this reference.

The mpmath side restates the formulas of the header's comment block; where the contract rounds to float the step is reproduced
in np.float32 arithmetic.  It never calls the contract."""
import hashlib

import mpmath
import numpy as np
import pytest

import _contract_cases as cc

mp, mpf = mpmath.mp, mpmath.mpf

PREC = 200
U = 2.0 ** -53            # unit roundoff of a double
EPS_L = 1e-15             # the header's bound on ig_log2_pos, absolute (before the integer exponent is added: see K_DERIVATION)
CLAMP = 1048576.0
QSCALE = 4294967296.0
LOG_E_F = float(np.float32(0.43429448190325182))  # the float literal of KA:4462

# ---------------------------------------------------------------------------------------------------------------------------
K_DERIVATION = """
    TERM_K: how many units of 2^-53 S the contract's term may be away from the exact one, S = ob |log10 P| + P + |lgf| + |P_z| log10 e.
    Derived from the header's statements about its two double functions, not from what the code gives (u = 2^-53):

     eps_L = 1e-15 = 9.0 u: ig_log2_pos, absolute, apart from the rounding of its last sum with the integer exponent (one of the
     roundings counted below: a double near 2^7 cannot be 1e-15 from anything).  The degree-5 Taylor polynomial of log2(1 + u) on
     |u| <= 2^-8 leaves log2(e) u^6 / 6 / (1 - |u|) = 8.6e-16 at the ends of an interval, the table entry and the last fma half an
     ulp of a number below 1 each (5.6e-17), the roundings inside the polynomial 1e-18.  test_log2_and_exp2_hold_their_bounds holds
     the function to it directly.
     eps_E = 13.2 u: ig_exp2_core, relative.  The degree-4 Taylor polynomial of 2^t - 1 on |t| <= 2^-8 leaves (ln 2 * 2^-8)^5 / 5! =
     1.21e-15 = 11.1 u (with the tail of the series), the table entry and the last fma one rounding each, the four roundings inside
     the polynomial 0.02 u together.  Held directly by the same test.

     lgf, the log10(ob!) part (reference: exact product below 10, the contract's own float-Stirling table for 10 .. 14, the double
     Stirling formula from 15 on).  ig_log10(x) = fl(log2(x) fl(log10 2)): 0.301 eps_L = 2.71 u absolute, and three roundings
     (log2's own sum, the constant, the product) relative to |log10 x|.  From 15 on o log10(o) adds a product rounding
     (4 u o log10 o + 2.71 u o), the subtraction of o one of |o log10 o - o|, the half-log of 2 pi o 1.36 u + 1.5 u log10(2 pi o) +
     0.87 u (two roundings in its argument), the last sum one of |lgf|.  Over |lgf| that is largest at o = 15: 131 u / 12.1 =
     10.8, and tends to 6.  K_LGF = 10.9.

     S >= 0.797 + lgf(ob) for ob >= 1 (ob |log10 P| + P is smallest at P = min(1, ob / ln 10)), so ob <= R S, R = max ob / (0.797 +
     lgf(ob)) = 1.687 at ob = 3.  An ABSOLUTE error e in log2 P costs ob log10(2) e <= 0.301 R e in the term.

     generic path (ig_pixel_term on the float ex): ob ig_log10(ex) - ex - lgf + P_z c.  ig_log10: 2.71 u R = 4.6 absolute, 3
     relative; the product with ob 1; the two subtractions and the addition 3 (each result is at most S); ex and P_z c are exact
     (P_z c is a product of two 24-bit significands).  K_GENERIC = 4.6 + 3 + 1 + 3 + K_LGF = 22.5.

     fast path (ig_term_hot): y = fma(slope, log2 s, log2 amp) carries (|slope| + 1) eps_L <= 7.5 eps_L = 67.6 u absolute and
     one rounding u |y|.
       ob log10 P = ob fl(y fl(log10 2)): the absolute part 0.301 * 67.6 u * R = 34.3; relative to ob |log10 P| the roundings of y,
       of the constant and of the product: 3.
       P = ig_exp2_core(y): relative ln 2 * 67.6 u = 46.8 u from y's absolute error; |ln P| u from y's rounding; eps_E = 13.2 u.
       P |ln P| <= 24 S inside the clamp: for P <= 1 it is 2.31 P |log10 P| <= 2.31 ob |log10 P|; for 1 < P <= 2^20 |ln P| <= 13.9;
       for P > 2^20 a term above -2^20 needs ob log10 P >= P - 2^20, so S >= P, and ob < 2^31 bounds P by 2.2e10: |ln P| <= 24.
       Together 46.8 + 13.2 + 24 = 84.0.
       the fma with ob, the subtraction of lgf and the addition of P_z c: 3.
     K_FAST = 34.3 + 3 + 84.0 + 3 + K_LGF = 135.2.
"""
EPS_L_U = EPS_L / U
EPS_E_U = 13.2
R_OB = 1.687
K_LGF = 10.9
K_GENERIC = 0.30103 * EPS_L_U * R_OB + 3 + 1 + 3 + K_LGF
K_FAST = 0.30103 * 7.5 * EPS_L_U * R_OB + 3 + (0.69315 * 7.5 * EPS_L_U + EPS_E_U + 24) + 3 + K_LGF
assert 22.4 < K_GENERIC < 22.6 and 135.0 < K_FAST < 135.4


@pytest.fixture(scope="module")
def ol(oracle_lib):
    oracle_lib.set_mode(oracle_lib.MODE_DET)
    return oracle_lib


@pytest.fixture(autouse=True)
def _precision():
    old = mp.prec
    mp.prec = PREC
    yield
    mp.prec = old


BASE = cc.base_params()
FAMILIES = cc.families(BASE)


def _ulp32_unit(t):
    """the float ulp at the (positive, float64) value t: 2^(floor(log2 t) - 23), 2^-149 below 2^-126"""
    _, e = np.frexp(t)  # t = m 2^e, m in [1/2, 1)
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def _alone(ol, s, **over):
    p = dict(BASE, c1=1.0, fact=1.0, d=2.0, d_max=np.inf, v_inter=0.0)
    p.update(over)
    z = np.zeros(s.size, np.float32)
    return ol.eval_terms(s, z, np.zeros(s.size, np.int32), cc.param_record(ol, p))[0]


def _pow_operands():
    rng = np.random.default_rng(11)
    return np.concatenate([cc.s_edges(37.5), cc.s_edges(np.inf), cc.random_positive_floats(rng, 20000)]).astype(np.float32)


def _check_ulps(got32, true64, what):
    """got within 1 ulp of the exact value (float64 holds it to 2^-29 of a float ulp); +inf where it exceeds FLT_MAX by more than
    half an ulp, 0 where it is below 2^-150.  Returns the largest error in ulps."""
    got = got32.astype(np.float64)
    got[np.isinf(got)] = 2.0 ** 128
    err = np.abs(got - true64) / _ulp32_unit(np.maximum(true64, 2.0 ** -149))
    over = true64 > float(cc.FLT_MAX) + 2.0 ** 103
    under = true64 < 2.0 ** -150
    assert np.all(np.isinf(got32[over])), what
    assert np.all(got32[under] == 0), what
    fin = ~over & ~under
    assert fin.any()
    assert err[fin].max() <= 1.0, (what, float(err[fin].max()))
    return float(err[fin].max()), int(over.sum()), int(under.sum()), int(((true64 < 2.0 ** -126) & ~under).sum())


def test_powf_within_one_ulp_of_mpmath(ol):
    """c1 = fact = 1, d = 2, d_max = inf, v_inter = 0: ex IS ig_powf(s, slope) for every s in (0, inf), and 0 elsewhere.  The
    header's statement, for results in the subnormal range as well (unit 2^-149), with +inf / 0 beyond the float range."""
    s = _pow_operands()
    inr = (s > 0) & np.isfinite(s)
    log2s = [mp.log(mpf(float(x))) / mp.ln2 for x in s[inr]]
    worst = {}
    for slope in cc.POW_SLOPES:
        sl = np.float32(slope)
        ex = _alone(ol, s, slope=sl)
        assert np.all(ex[~inr] == 0)  # -1, +-0, NaN, +inf: outside (0, d_max)
        true = np.array([float(mp.power(2, mpf(float(sl)) * l)) for l in log2s])
        worst[slope] = _check_ulps(ex[inr], true, "slope %g" % slope)
    for slope, (e, over, under, sub) in worst.items():
        print("ig_powf slope %5.2f: largest error %.5f ulp (%d operands; %d overflow to +inf, %d underflow to 0, %d subnormal results)"
              % (slope, e, int(inr.sum()), over, under, sub))
    assert sum(w[3] for w in worst.values()) > 100  # results in the subnormal range did occur
    # the two exponents ig_powf answers without a logarithm
    assert np.all(_alone(ol, s, slope=0.0)[inr] == 1.0)
    with np.errstate(all="ignore"):
        sq = (s * s).astype(np.float32)
    assert np.array_equal(_alone(ol, s, slope=2.0)[inr].view(np.uint32), sq[inr].view(np.uint32))


def test_expf_within_one_ulp_of_mpmath(ol):
    """slope = 0 makes pw exactly 1: ex = ig_expf(a), a = fl((d - 2) / fl(fl(t t) + d)), t = fl(fl(s lm) / kuhn) (KA:159)"""
    rng = np.random.default_rng(12)
    s = np.concatenate([_pow_operands(), np.exp(rng.uniform(np.log(1e-3), np.log(1e5), 20000)).astype(np.float32)])
    inr = (s > 0) & np.isfinite(s)
    lm, kuhn = np.float32(BASE["lm"]), np.float32(BASE["kuhn"])
    for d in cc.EXP_D:
        d32 = np.float32(d)
        ex = _alone(ol, s, slope=0.0, d=d32)
        assert np.all(ex[~inr] == 0)
        with np.errstate(all="ignore"):
            t = ((s[inr] * lm).astype(np.float32) / kuhn).astype(np.float32)
            a = ((d32 - np.float32(2.0)) / ((t * t).astype(np.float32) + d32).astype(np.float32)).astype(np.float32)
        assert a.dtype == np.float32 and np.unique(a).size > 1000
        cache = {}
        for v in np.unique(a):
            cache[float(v)] = float(mp.exp(mpf(float(v))))
        true = np.array([cache[float(v)] for v in a])
        e = _check_ulps(ex[inr], true, "d %g" % d)[0]
        print("ig_expf d %.1f: largest error %.5f ulp (%d operands, a in [%.3g, %.3g])" % (d, e, int(inr.sum()), float(a.min()), float(a.max())))


def test_log2_and_exp2_hold_their_bounds(ol):
    """ig_log2_pos within 1e-15 + 2^-53 |log2 x| of log2 x (the header's bound on the table-and-polynomial part, and the rounding of
    its sum with the integer exponent) on the doubles the contract feeds it: every kind of positive float (subnormal floats are
    normal doubles), the two ends and the middle of each of the 128 intervals in several binades (the polynomial's remainder is
    largest at the ends), products c1 fact.  ig_exp2 within 13.2 x 2^-53 of 2^y, relative, over |y| <= 1000."""
    rng = np.random.default_rng(13)
    j = np.arange(128, dtype=np.float64)
    m = np.concatenate([0.5 + j / 256, np.nextafter(0.5 + (j + 1) / 256, 0), 0.5 + (j + 0.5) / 256, rng.uniform(0.5, 1.0, 4000)])
    x = np.concatenate([np.ldexp(m, e) for e in (-148, -126, -30, -1, 0, 1, 2, 30, 128)]
                       + [cc.random_positive_floats(rng, 20000).astype(np.float64),
                          np.exp(rng.uniform(np.log(1e-3), np.log(1e5), 20000)).astype(np.float32).astype(np.float64),
                          rng.uniform(1, 2, 4000).astype(np.float32).astype(np.float64) * rng.uniform(1, 2, 4000).astype(np.float32).astype(np.float64)])
    got = ol.detmath_probe(0, x)
    worst, where = 0.0, 0.0
    for xi, gi in zip(x, got):
        true = mp.log(mpf(float(xi))) / mp.ln2
        excess = float(abs(mpf(float(gi)) - true)) - U * abs(float(true))
        if excess > worst:
            worst, where = excess, float(xi)
    print("ig_log2_pos: largest |error| - 2^-53 |log2 x| = %.3g at x = %r (%d operands; bound %.1g)" % (worst, where, x.size, EPS_L))
    assert worst <= EPS_L, (worst, where)
    y = np.concatenate([rng.uniform(-1000, 1000, 20000), rng.uniform(-2, 2, 10000), (np.arange(-1280, 1281) + 0.5) / 128.0, [-1000.0, 1000.0, 0.0]])
    got = ol.detmath_probe(1, y)
    rel = max(float(abs(mpf(float(g)) / mp.power(2, mpf(float(v))) - 1)) for v, g in zip(y, got))
    print("ig_exp2: largest relative error %.2f x 2^-53 (%d operands; bound %.1f)" % (rel / U, y.size, EPS_E_U))
    assert rel <= EPS_E_U * U, rel / U
    assert ol.detmath_probe(1, np.array([1000.5, -1000.5, np.inf, -np.inf])).tolist() == [np.inf, 0.0, np.inf, 0.0]
    assert np.isnan(ol.detmath_probe(1, np.array([np.nan])))[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the term

def _lgf_ref(ob, lgf15, cache):
    """log10(ob!) as KA:111-124 / 251-270 define it: exact product below 10, the float Stirling value for 10 .. 14 (the
    contract's table: its five floats are held to the formula by test_float_stirling_table), the double Stirling formula from 15"""
    v = cache.get(ob)
    if v is None:
        if ob < 10:
            v = mp.log10(mp.factorial(ob))
        elif ob < 15:
            v = mpf(float(lgf15[ob]))
        else:
            o = mpf(ob)
            v = o * mp.log10(o) - o + mp.log10(mp.sqrt(2 * mp.pi * o))
        cache[ob] = v
    return v


def _reference(p, fast, s, ob, ex, exc, term, q, lgf15):
    """per operand: class (0 inside the clamp, 1 beyond, 2 the reference is inf - inf), |term - ref| and |q - ref 2^32| (inside), S"""
    amp = mpf(float(p["c1"])) * mpf(float(p["fact"]))
    slope, v_inter, d_max = mpf(float(p["slope"])) if fast else None, mpf(float(p["v_inter"])), float(p["d_max"])
    c_f = mpf(LOG_E_F)
    n = s.size
    cls = np.zeros(n, np.int8)
    sign = np.zeros(n, np.int8)
    err_t, err_q, S = np.zeros(n), np.zeros(n), np.zeros(n)
    lcache, fcache = {}, {}
    inf = float("inf")
    for i in range(n):
        o, si, pz = int(ob[i]), float(s[i]), float(exc[i])
        assert pz == pz
        if fast and o > 0:
            if si > 0 and si < d_max:  # (false for a NaN)
                l2 = lcache.get(si)
                if l2 is None:
                    l2 = lcache[si] = mp.log(mpf(si)) / mp.ln2
                P = amp * mp.power(2, slope * l2)
                if P < v_inter:
                    P = v_inter
            else:
                P = v_inter
            lgf = _lgf_ref(o, lgf15, fcache)
            a, b = o * mp.log10(P), P
            val, parts = a - b - lgf, abs(a) + b + abs(lgf)
        else:
            e = float(ex[i])
            assert e == e and e >= 0
            if e == 0:
                val, parts = mpf(0), mpf(0)
            elif e == inf:
                val, parts = (None if o > 0 else -inf), inf  # ob log10(inf) - inf
            elif o > 0:
                lgf = _lgf_ref(o, lgf15, fcache)
                a, b = o * mp.log10(mpf(e)), mpf(e)
                val, parts = a - b - lgf, abs(a) + b + abs(lgf)
            else:
                val, parts = -mpf(e), mpf(e)
        if pz == inf:
            val = None if (val is None or val == -inf) else inf
        elif val is not None and val != -inf:
            val = val + mpf(pz) * c_f
            parts = parts + abs(mpf(pz)) * c_f
        if val is None:
            cls[i] = 2
            continue
        if val == inf or val == -inf or abs(val) >= CLAMP * (1 + 1e-6):
            cls[i], sign[i] = 1, (1 if val > 0 else -1)
            continue
        # (a reference within 1e-6 of the clamp from either side is held to the tolerance against the clamped value)
        vc = min(max(val, -CLAMP), CLAMP)
        S[i] = float(parts)
        err_t[i] = float(abs(mpf(float(term[i])) - val)) if abs(val) < CLAMP else 0.0
        err_q[i] = float(abs(mpf(int(q[i])) - vc * QSCALE))
    return cls, sign, err_t, err_q, S


def test_float_stirling_table(ol):
    """the five float values factorial() takes from Stirling's formula (KA:121, counts 10 .. 14), recovered from the contract's
    table of their log10, lie within 2 float ulps of n^n e^-n sqrt(2 pi n); below 10 the table is the log10 of the exact product"""
    t = ol.lgf_table()
    for n in range(10):
        assert abs(mpf(float(t[n])) - mp.log10(mp.factorial(n))) <= 0.30103 * EPS_L + 3 * U * float(mp.log10(mp.factorial(n)))
    for n in range(10, 15):
        f = np.float32(float(mp.power(10, mpf(float(t[n])))))  # the float itself: the table holds its log10 to ~1e-15
        true = mpf(n) ** n * mp.exp(-n) * mp.sqrt(2 * mp.pi * n)
        err = float(abs(mpf(float(f)) - true)) / float(_ulp32_unit(np.float64(float(true))))
        print("factorial(%d) in float: %.9g, %.3f ulp from Stirling's formula" % (n, float(f), err))
        assert err <= 2.0, (n, err)


@pytest.mark.parametrize("fam", range(len(FAMILIES)), ids=[f[0] for f in FAMILIES])
def test_term_against_mpmath(ol, fam):
    """Every operand falls in exactly one class and none is skipped.  Beyond the clamp (|reference| >= 2^20 (1 + 1e-6), infinite
    ones included): q is exactly +-2^20 2^32.  Inside (a reference within 1e-6 of +-2^20 counts as inside and is compared clamped:
    there the rounding of the term decides on which side of the clamp it falls): |term - ref| <= k 2^-53 S and |q - ref 2^32| <= 1/2 + k 2^-53 S 2^32, k = K_FAST
    for what ig_term_hot evaluates (a fast family, count above zero) and K_GENERIC for what ig_pixel_term does.  Where the
    reference itself is inf - inf (an infinite expectation against a count, or against an infinite P_z) the term is a NaN and
    joins the sums as 0, as ig_quantize states.

    At least half of a family's operands lie inside the clamp -- except where quirk Q6 alone decides: P_z is at least d_max, so
    with d_max log10(e) >= 2^20 (d_max = inf, the settled set's 2.93e6) the term is beyond the clamp whatever the contact, and so
    it is under an infinite v_inter, which no expectation lies below; there at least half lie beyond or are inf - inf."""
    name, p, fast = FAMILIES[fam]
    assert cc.expect_fast(p) == fast, name
    s, s_tot, ob = cc.operands(p["d_max"], 2500, 2500)
    ex, exc, term, q = ol.eval_terms(s, s_tot, ob, cc.param_record(ol, p))
    cls, sign, err_t, err_q, S = _reference(p, fast, s, ob, ex, exc, term, q, ol.lgf_table())
    inside, beyond, undef = cls == 0, cls == 1, cls == 2
    assert np.all(q[beyond] == sign[beyond].astype(np.int64) * np.int64(CLAMP * QSCALE)), name
    assert np.all(np.isnan(term[undef])) and np.all(q[undef] == 0), name
    k = np.where(fast & (ob > 0), K_FAST, K_GENERIC)
    tol = k * U * S
    with np.errstate(all="ignore"):
        mult = np.where(S > 0, np.maximum(err_t, np.maximum(err_q - 0.5, 0) / QSCALE) / (U * S), 0.0)[inside]
    print("%-22s %s: %5.1f %% inside the clamp, %4.1f %% beyond; largest error %.2f x 2^-53 S (k = %.1f%s); largest |q - ref 2^32| %.2f"
          % (name, "fast   " if fast else "generic", 100 * inside.mean(), 100 * beyond.mean(), mult.max() if mult.size else 0.0,
             K_FAST if fast else K_GENERIC, ", %.1f at a count of 0" % K_GENERIC if fast else "", float(err_q[inside].max()) if inside.any() else 0.0))
    bad = inside & ((err_t > tol) | (err_q > 0.5 + tol * QSCALE))
    assert not bad.any(), (name, [(float(s[i]), int(ob[i]), float(term[i]), err_t[i], tol[i]) for i in np.nonzero(bad)[0][:5]])
    assert np.all(err_t[inside & (S == 0)] == 0)
    forced = float(p["d_max"]) * LOG_E_F >= CLAMP or float(p["v_inter"]) == np.inf
    if forced:
        assert (beyond | undef).mean() >= 0.5, name
    else:
        assert inside.mean() >= 0.5, (name, float(inside.mean()))
    if name == "subnormal ex":  # the family is there for expectations in the float subnormals: they occur, and not as zeros
        sub = (ex > 0) & (ex < cc.FLT_MIN)
        assert sub.mean() > 0.2, float(sub.mean())


test_term_against_mpmath.__doc__ += "\n" + K_DERIVATION


def test_contract_bits_are_pinned(ol):
    """The contract is a definition of bits: a change to a coefficient, a table entry or the order of two operations changes
    results somewhere in the last place, far below any tolerance above.  One digest of (ex, exc, term, q) over a fixed lattice of
    operands under the shipped set and the d = 3 set (ig_expf), and of ig_log2_pos and ig_exp2 on their own, says that nothing has moved.  Whoever changes the contract on
    purpose regenerates the goldens of tests/golden and this digest with them."""
    i = np.arange(200000, dtype=np.uint64)
    s = ((i * np.uint64(2654435761)) % np.uint64(0x7F7FFFFF) + np.uint64(1)).astype(np.uint32).view(np.float32)
    j = i[::2]  # every other one in [2^-10, 2^17): (1 + k / 1024) 2^e, exact operations only
    s[::2] = np.ldexp(np.float32(1.0) + (j % np.uint64(1021)).astype(np.float32) / np.float32(1024.0), ((j * np.uint64(7)) % np.uint64(27)).astype(np.int32) - 10).astype(np.float32)
    ob = ((i * np.uint64(40503)) % np.uint64(3000)).astype(np.int32)
    with np.errstate(over="ignore"):
        s_tot = (s * (i % np.uint64(4)).astype(np.float32)).astype(np.float32)
    h = hashlib.sha256()
    h.update(s.tobytes())
    for p in (BASE, dict(BASE, d=np.float32(3.0))):
        for a in ol.eval_terms(s, s_tot, ob, cc.param_record(ol, p)):
            h.update(a.tobytes())
    # ... and the two double functions on their own: a last-place change of a log2 is often absorbed by the roundings behind it
    h.update(ol.detmath_probe(0, s.astype(np.float64)).tobytes())
    h.update(ol.detmath_probe(1, ((i * np.uint64(7919)) % np.uint64(2000001)).astype(np.float64) / 1000.0 - 1000.0).tobytes())
    assert h.hexdigest() == PINNED_DIGEST, h.hexdigest()


PINNED_DIGEST = "27aa4bdaf5c94292891cf4c90429c52689ee82b3e7646b4641f02ae53eba3dbe"
