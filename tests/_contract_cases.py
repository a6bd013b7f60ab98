"""Parameter families and operands shared by tests/test_contract_precision_host.py (the contract as gcc compiles it against
mpmath) and tests/test_hip_contract_parity.py (the device against the host contract, bit for bit): the places where the two
compilations of include/ig_detmath.h could part, and where the shipped parameter sets never go.

A family is (name, overrides of tiny's parameter set, fast): `fast` is what ig_hot_make must decide for it (the one-log
evaluation of ig_term_hot for counts above zero).  Everything here is seeded and pure."""
import numpy as np

FLT_MIN = np.float32(2.0 ** -126)
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(2.0 ** -149)
INF = np.float32(np.inf)
NAMES = ("kuhn", "lm", "c1", "slope", "d", "d_max", "fact", "v_inter")

# what ig_powf's own test runs through (ten slopes) and the values of d of ig_expf's
POW_SLOPES = (-6.5, -6.4, -3.0, -1.5, -1.0, -0.53, 0.3, 1.0, 6.4, 6.5)
EXP_D = (2.5, 3.0, 7.0)


def _up(x):
    return np.nextafter(np.float32(x), INF)


def _down(x):
    return np.nextafter(np.float32(x), -INF)


def base_params():
    """tiny's parameter set as eight float32 values"""
    from instagraal_amd import synth

    p = synth.rippe_params(1.8)  # (what make_problem hands every configuration: test_hip_contract_parity checks it against tiny's)
    return {k: np.float32(p[k]) for k in NAMES}


def _family(base, name, fast, **over):
    p = dict(base)
    p.update({k: np.float32(v) for k, v in over.items()})
    return name, p, fast


def families(base):
    """[(name, parameters, fast)].  Where a family's operands would mostly lie beyond the clamp of ig_quantize under tiny's d_max
    (an amplitude of 2^30 puts P(s) above 2^20 for every s below 100 kb) its d_max is lowered, and the same set under tiny's d_max
    follows in gpu_extra_families(): bit parity has no use for the clamp."""
    from instagraal_amd import synth

    def fam(name, fast, **over):
        return _family(base, name, fast, **over)

    settled = {k: np.float32(v) for k, v in synth.settled_params({k: float(v) for k, v in base.items()}).items()}
    out = [
        fam("shipped", True),
        ("settled", settled, True),  # d_max 2.93e6: quirk Q6 puts P_z log10(e) = 1.27e6 beyond the clamp on its own
        ("settled, d_max 2e6", dict(settled, d_max=np.float32(2.0e6)), True),
        fam("slope -6.4", True, slope=-6.4),
        fam("slope 6.4", True, slope=6.4),
        fam("slope -6.5", False, slope=-6.5),
        fam("slope 6.5", False, slope=6.5),
        fam("slope 0", False, slope=0.0),
        fam("slope 2", False, slope=2.0),
        fam("slope 1", True, slope=1.0),
        fam("d 3", False, d=3.0),
        fam("v_inter 0", False, v_inter=0.0),
        fam("v_inter 1e-45", True, v_inter=DENORM_MIN),
        fam("v_inter FLT_MIN", True, v_inter=FLT_MIN),
        fam("v_inter inf", False, v_inter=INF),
        fam("amp 2^-30", False, c1=2.0 ** -30, fact=1.0),
        fam("amp 2^-30 inner", True, c1=_up(2.0 ** -30), fact=1.0),
        fam("amp 2^30", False, c1=2.0 ** 30, fact=1.0, d_max=1.0),
        fam("amp 2^30 inner", True, c1=_down(2.0 ** 30), fact=1.0, d_max=1.0),
        fam("amp 2^-31", False, c1=2.0 ** -31, fact=1.0),
        fam("subnormal ex", False, c1=1e-38, fact=1.0, v_inter=0.0, d_max=3.0e4),
        fam("d_max 0", True, d_max=0.0),
        fam("d_max inf", True, d_max=INF),
        fam("d_max 37.5", True, d_max=37.5),
        fam("slope nan", False, slope=np.nan),
    ]
    return out


def gpu_extra_families(base):
    return [_family(base, "amp 2^30, tiny's d_max", False, c1=2.0 ** 30, fact=1.0),
            _family(base, "amp 2^30 inner, tiny's d_max", True, c1=_down(2.0 ** 30), fact=1.0)]


def expect_fast(p):
    """ig_hot_make's domain, restated"""
    amp = float(p["c1"]) * float(p["fact"])
    sl, v = float(p["slope"]), float(p["v_inter"])
    return bool(float(p["d"]) == 2.0 and sl != 0.0 and sl != 2.0 and -6.5 < sl < 6.5 and 0.0 < v < np.inf and 2.0 ** -30 < amp < 2.0 ** 30)


def s_edges(d_max):
    e = [0.0, -0.0, -1.0, DENORM_MIN, _down(FLT_MIN), FLT_MIN, _up(FLT_MIN), _down(1.0), 1.0, _up(1.0), FLT_MAX, INF, np.nan]
    d_max = np.float32(d_max)
    e += [_down(d_max), d_max, _up(d_max)]
    return np.array(e, np.float32)


def random_positive_floats(rng, n):
    """bit patterns drawn from all positive finite floats, subnormals included"""
    return rng.integers(1, 0x7F800000, n, dtype=np.uint32).view(np.float32)


OB_EDGE = np.array([0, 1, 9, 10, 14, 15, 1023, 1024, 2 ** 24, 2 ** 31 - 1], np.int64)


def ob_special():
    """0, every count 1 .. 2048 (the factorial changes form at 9|10 and 14|15, the device's table ends at 1023|1024) and
    2^k - 1, 2^k, 2^k + 1 up to 2^31 - 1"""
    pw = np.array([min(max(2 ** k + j, 0), 2 ** 31 - 1) for k in range(32) for j in (-1, 0, 1)], np.int64)
    return np.concatenate([np.arange(0, 2049, dtype=np.int64), pw])


def operands(d_max, n_bits, n_log, seed=20):
    """(s, s_tot, ob): every edge of s against every edge count; then n_bits random positive finite bit patterns and n_log values
    log-uniform in [1e-3, 1e5], shuffled together, the special counts on the first of them and counts below 40 on the rest;
    s_tot cycles through {0, s, 2 s, 3 s} (every sign of the circular n)."""
    rng = np.random.default_rng(seed)
    e = s_edges(d_max)
    s_e = np.repeat(e, OB_EDGE.size)
    ob_e = np.tile(OB_EDGE, e.size)
    s_r = np.concatenate([random_positive_floats(rng, n_bits), np.exp(rng.uniform(np.log(1e-3), np.log(1e5), n_log)).astype(np.float32)])
    s_r = s_r[rng.permutation(s_r.size)]
    ob_r = rng.integers(0, 40, s_r.size).astype(np.int64)
    sp = ob_special()
    assert sp.size <= ob_r.size
    ob_r[: sp.size] = sp
    s = np.concatenate([s_e, s_r]).astype(np.float32)
    ob = np.concatenate([ob_e, ob_r])
    assert ob.min() >= 0 and ob.max() == 2 ** 31 - 1  # no negative counts: the host table has no entry for them
    with np.errstate(all="ignore"):
        s_tot = (s * (np.arange(s.size) % 4).astype(np.float32)).astype(np.float32)
    return s, s_tot, ob.astype(np.int32)


def param_record(ol, p):
    r = np.zeros(1, ol.PARAM_DTYPE)
    for k in NAMES:
        r[k] = np.float32(p[k])
    return r
