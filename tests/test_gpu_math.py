"""GPU (-m gpu): the elementary functions of is3d_amd/csrc/cf_math.h against numpy long double, through is3d_math_probe.  The accuracy
figures quoted in DESIGN.md and in the kernels' comments are the assertions here.  Besides random arguments: the arguments where a
reduction or a seed is worst (half-integer multiples of ln2, domain edges, powers of two), against mpmath, and the helpers the p.dsigma
clamp rests on -- the clamped add / fma bit for bit against an exactly rounded a b + c, exp_p9_scaled at every exponent phase 2e of
cf_prep_feqmod can produce, rcp_batch at the four sizes the kernels instantiate.  Measured on an MI355X: structured arguments 4.6e-16
(exp_full) and 3.3e-14 (exp_p9); exp_p9_scaled 6.4e-14 and the bits of ldexp(exp_p9, e); rcp_batch 2.0e-15 .. 2.2e-15."""
import numpy as np
import pytest

from is3d_amd import api

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(got.astype(LD) - ref) / np.abs(ref)))


def test_exponentials():
    rng = np.random.default_rng(1)
    x = np.concatenate([-rng.random(200000) * 700.0, -rng.random(50000) * 2.0, rng.random(20000) * 20.0, [0.0, -1e-300, -0.5 * np.log(2), -708.0]])
    ref = np.exp(x.astype(LD))
    assert _rel(api.math_probe("exp_full", x), ref) < 2.5e-15          # Cody-Waite + degree 10: 1.4e-15 on the reduced interval, + the reduction
    assert _rel(api.math_probe("exp_full_sat", x), ref) < 2.5e-15
    e9 = _rel(api.math_probe("exp_p9", x), ref)
    assert e9 < 7e-14, e9                                              # one-fma reduction (|n| 2.3e-17) + degree 9 (4.5e-14)
    assert _rel(api.math_probe("exp_p9_sat", x), ref) < 7e-14
    assert np.array_equal(api.math_probe("exp_p9", x), api.math_probe("exp_p9_sat", x))   # the two conversions agree wherever both are defined
    # a power-of-two factor through the shift constant (cf_main_feqmod: the cell's p.dsigma scale): 2^5 e^x, the bits of 32 * exp_p9(x)
    norm = x[x > -700.0]
    assert np.array_equal(api.math_probe("exp_p9_x32", norm), 32.0 * api.math_probe("exp_p9", norm))
    # the exact-zero rule of the row culls: e^v is exactly +0 for v < -745.2 in every variant, and the saturating forms take any argument
    far = np.array([-745.25, -746.0, -1000.0, -1.0e6, -1.3e9])
    for f in ("exp_full", "exp_p9", "exp_full_sat", "exp_p9_sat"):
        assert not api.math_probe(f, far).any(), f
    # the saturating forms: exactly +0 for arguments far beyond the shift trick's domain -- up to ~1e45, where the reduced argument's
    # polynomial overflows; what this test found: they are NOT defined for every double (e^-1e300 came out inf, e^-inf nan), so the prep
    # kernels bound the argument of every per-evaluation exponential instead (status[7]: IS3D_EDOMAIN) and the main kernels use exp_p9
    huge = np.array([-1.0e12, -1.0e20, -1.0e30, -1.0e40])
    for f in ("exp_full_sat", "exp_p9_sat"):
        assert not api.math_probe(f, huge).any(), f
    # denormal results stay within a few ulps of the denormal grid
    den = np.array([-709.0, -720.0, -740.0, -744.0])
    got = api.math_probe("exp_p9", den)
    assert np.all(np.abs(got - np.exp(den)) <= 4 * 4.9406564584124654e-324 + 1e-13 * np.exp(den))


def test_square_roots_and_reciprocals():
    rng = np.random.default_rng(2)
    x = np.exp(rng.uniform(np.log(1e-200), np.log(1e200), 200000))
    assert _rel(api.math_probe("sqrt_g1", x), np.sqrt(x.astype(LD))) < 4e-15     # v_rsq_f64 (4.5e-8) + one Goldschmidt step: 1.5 e0^2
    assert _rel(api.math_probe("sqrt_nr", x), np.sqrt(x.astype(LD))) < 3e-16
    d = np.concatenate([x[:100000], -x[100000:]])
    assert _rel(api.math_probe("rcp_nr1", d), 1 / d.astype(LD)) < 4e-15           # v_rcp_f64 + one Newton step
    assert _rel(api.math_probe("rcp_nr", d), 1 / d.astype(LD)) < 3e-16
    api.math_probe("rcp_nr", d[:1])                                                 # sets the argument types
    assert api.load().is3d_math_probe(17, 0, None, None, -1) == api.IS3D_EINVAL      # an unknown function is refused
    assert api.load().is3d_math_probe(-1, 0, None, None, -1) == api.IS3D_EINVAL
    assert max(api.MATH_FUNCS.values()) == 16


def test_square_roots_and_reciprocals_at_the_domain_edges():
    """the documented domain of the square roots, [1e-280, 1e280], and every even power of two inside it (an exact root); the reciprocals at
    +-2^k for |k| <= 1000 (an exact quotient, and a seed at both ends of v_rcp_f64's range) -- at the bounds asserted above"""
    x = np.concatenate([[1e-280, 1e280], np.ldexp(1.0, 2 * np.arange(-465, 466))])
    assert x.min() >= 1e-280 and x.max() <= 1e280
    ref = np.sqrt(x.astype(LD))
    assert _rel(api.math_probe("sqrt_g1", x), ref) < 4e-15
    assert _rel(api.math_probe("sqrt_nr", x), ref) < 3e-16
    p = np.ldexp(1.0, np.arange(-1000, 1001))
    d = np.concatenate([p, -p])
    assert _rel(api.math_probe("rcp_nr1", d), 1 / d.astype(LD)) < 4e-15
    assert _rel(api.math_probe("rcp_nr", d), 1 / d.astype(LD)) < 3e-16


def _steps(x, k):
    """x moved by k ulps"""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _mp_exp(v, e=None):
    """2^e exp(v) with mpmath's exponential at 120 bits"""
    import mpmath
    with mpmath.workprec(120):
        return [mpmath.ldexp(mpmath.exp(mpmath.mpf(float(v[i]))), int(e[i]) if e is not None else 0) for i in range(len(v))]


def _rel_mp(got, v, e=None, refs=None):
    """max |got - ref| / ref against _mp_exp(v, e) (or the refs computed before)"""
    import mpmath
    refs = refs if refs is not None else _mp_exp(v, e)
    with mpmath.workprec(120):
        return float(max(abs(mpmath.mpf(float(g)) - r) / r for g, r in zip(got, refs)))


def test_exponentials_at_structured_arguments():
    """Where the reduction is worst, not where a uniform draw lands: v = (n + 1/2) ln2 moved by 0, +-1, +-2 ulp (the reduced argument at
    +-ln2/2, on either side of the rounding of n) and v = n ln2 moved by 0, +-1 ulp (r = 0), for every n in [-1020, 1021]: 16 336 points, all
    inside (-708, 709.7).  An fp64 emulation of both polynomials on exactly this set gives 4.6e-16 (exp_full) and 3.3e-14 (exp_p9), |r| up
    to 1.000000000001 ln2/2: the bounds asserted for random arguments hold with room.  Then the overflow edge and the stated domain edge of the
    shift trick."""
    n = np.arange(-1020, 1022, dtype=np.float64)
    ln2 = np.log(2.0)
    x = np.concatenate([_steps((n + 0.5) * ln2, k) for k in (0, 1, -1, 2, -2)] + [_steps(n * ln2, k) for k in (0, 1, -1)])
    assert x.size == 16336 and x.min() > -708.0 and x.max() < 709.7
    refs = _mp_exp(x)
    for f, bound in (("exp_full", 2.5e-15), ("exp_full_sat", 2.5e-15), ("exp_p9", 7e-14), ("exp_p9_sat", 7e-14)):
        err = _rel_mp(api.math_probe(f, x), x, refs=refs)
        print("%s on the structured set: %.3e" % (f, err))
        assert err < bound, f
    # up to the largest finite result; past it +inf
    top = np.linspace(709.0, 709.78, 157)
    over = np.array([709.79, 709.8, 710.0, 745.2, 1.0e3, 1.0e6])
    for f, bound in (("exp_full", 2.5e-15), ("exp_full_sat", 2.5e-15), ("exp_p9", 7e-14), ("exp_p9_sat", 7e-14)):
        got = api.math_probe(f, top)
        assert np.isfinite(got).all(), f
        assert _rel_mp(got, top) < bound, f
        assert np.array_equal(api.math_probe(f, over), np.full(over.size, np.inf)), f
    # the stated domain edge of the shift trick, |v| < 1.4e9 (n still inside the low dword): exactly +0 and +inf
    for f in ("exp_full", "exp_p9"):
        got = api.math_probe(f, np.array([-1.4e9, 1.4e9]))
        assert got[0] == 0.0 and not np.signbit(got[0]) and got[1] == np.inf, f


SCALE_E = [-20, -1, 0, 1, 5, 12, 64, 300, 997]   # phase 2e of cf_prep_feqmod produces up to ~997 (a bound below 1e300)


def test_exp_p9_scaled_at_every_exponent():
    """exp_p9_scaled(v, kExpShift + e) is ldexp(exp_p9(v), e) bit for bit wherever both are normal and finite, and within exp_p9's 7e-14 of
    2^e e^v: the shift constant carries e into the low word next to n and the reduced argument does not see it"""
    rng = np.random.default_rng(12)
    ln2 = np.log(2.0)
    for e in SCALE_E:
        lo, hi = max(-1020.0, -1020.0 - e), min(1022.0, 1022.0 - e)          # n and n + e both inside the normal exponents
        v = np.concatenate([rng.uniform(lo, hi, 3000) * ln2, (np.arange(np.ceil(lo), np.floor(hi)) + 0.5) * ln2])
        got = api.math_probe("exp_p9_scaled", np.column_stack([v, np.full(v.size, float(e))]))
        base = api.math_probe("exp_p9", v)
        want = np.ldexp(base, e)
        tiny = np.finfo(np.float64).tiny
        ok = np.isfinite(want) & (want >= tiny) & (base >= tiny) & np.isfinite(got) & (got >= tiny)
        assert ok.mean() > 0.99, e
        assert np.array_equal(got[ok], want[ok]), e
        sub = slice(None, None, 7)
        err = _rel_mp(got[ok][sub], v[ok][sub], np.full(v.size, e)[ok][sub])
        print("exp_p9_scaled e = %d: %d points bit for bit, %.3e against mpmath" % (e, int(ok.sum()), err))
        assert err < 7e-14, e
    if "exp_p9_x32" in api.MATH_FUNCS:
        v = rng.uniform(-700.0, 700.0, 1000)
        assert np.array_equal(api.math_probe("exp_p9_x32", v), api.math_probe("exp_p9_scaled", np.column_stack([v, np.full(v.size, 5.0)])))


def _clamp_reference(a, b, c):
    """min(max(fl(a b + c), 0), 1) with the fma rounded once (exact rational arithmetic, then one rounding to double), NaN -> 0"""
    from fractions import Fraction
    out = np.empty(len(a))
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        if np.isfinite([x, y, z]).all():
            try:
                r = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
            except OverflowError:
                r = np.inf if (x > 0) == (y > 0) else -np.inf
        elif np.isfinite(x) and np.isfinite(y):
            r = float(z)                                                   # a finite product, however large, plus inf or NaN
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                r = float(np.float64(x) * np.float64(y) + np.float64(z))   # an inf or a NaN factor decides: no rounding to get wrong
        out[i] = 0.0 if np.isnan(r) else min(max(r, 0.0), 1.0)
    return out


def _clamp_inputs():
    rng = np.random.default_rng(13)
    recs = []
    # results within +-2 ulp of 0 and of 1, where the single rounding of the fma decides: c = t - fl(a b), moved by j ulp
    a, b = rng.uniform(0.5, 2.0, 400), rng.uniform(0.5, 2.0, 400) * rng.choice([-1.0, 1.0], 400)
    for t in (0.0, 1.0):
        for j in (-2, -1, 0, 1, 2):
            recs.append(np.column_stack([a, b, _steps(t - a * b, j)]))
    one = np.array([_steps(1.0, j) for j in (-2, -1, 0, 1, 2)])
    zero = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-323, -1e-323, 2.2250738585072014e-308, -2.2250738585072014e-308])
    edge = np.concatenate([one, zero])
    recs.append(np.column_stack([np.ones(edge.size), np.ones(edge.size), edge]))            # 1 * 1 + c
    recs.append(np.column_stack([edge, np.ones(edge.size), np.zeros(edge.size)]))           # a * 1 + 0
    recs.append(np.column_stack([edge, -np.ones(edge.size), -np.zeros(edge.size)]))         # -a - 0: -0 results
    # inside, negative, above 1, huge
    m = rng.uniform(-3.0, 3.0, (2000, 3)) * np.ldexp(1.0, rng.integers(-60, 60, (2000, 3)))
    recs.append(m)
    recs.append(rng.uniform(-1.0, 1.0, (1000, 3)))
    # denormal results: products of two small normals, sums of denormals
    d = np.column_stack([rng.uniform(1.0, 2.0, 500) * 2.0 ** -540, rng.uniform(-2.0, 2.0, 500) * 2.0 ** -530, rng.uniform(-1.0, 1.0, 500) * 2.0 ** -1070])
    recs.append(d)
    # infinities and NaN in every slot, inf * 0, inf - inf, overflowing products
    s = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0, 0.5, 1e308, -1e308]
    recs.append(np.array([[x, y, z] for x in s for y in s for z in s]))
    return np.ascontiguousarray(np.concatenate(recs))


def test_clamped_add_and_fma():
    """The helpers that form max(p.dsigma 2^-e, 0): v_add_f64 / v_fma_f64 with the VOP3 clamp modifier are min(max(fl(a b + c), 0), 1) bit
    for bit -- around 0 and 1 to the ulp, for negative values, values above 1, infinities, denormal results and signed zeros -- and a NaN
    gives 0 (DX10_CLAMP), never a NaN that the accumulators would keep.  Zeros are compared by value, not by sign."""
    r = _clamp_inputs()
    a, b, c = r[:, 0], r[:, 1], r[:, 2]
    got = api.math_probe("fma_clamp01", r)
    assert got.shape == (len(r),)
    ref = _clamp_reference(a, b, c)
    assert not np.isnan(got).any()
    assert np.array_equal(got, ref), int(np.argmax(got != ref))
    assert ((ref > 0) & (ref < 1)).sum() > 500 and (ref == 0).sum() > 500 and (ref == 1).sum() > 500
    # a * b + 0.5
    got = api.math_probe("fma_clamp01_half", np.ascontiguousarray(r[:, :2]))
    assert np.array_equal(got, _clamp_reference(a, b, np.full(len(r), 0.5)))
    ha = np.random.default_rng(14).uniform(0.5, 1.0, 300)
    for s in (0.5, -0.5):                                                       # a b within 2 ulp of +-1/2: results around 1 and 0
        x = np.ascontiguousarray(np.concatenate([np.column_stack([ha, _steps(s / ha, j)]) for j in (-2, -1, 0, 1, 2)]))
        assert np.array_equal(api.math_probe("fma_clamp01_half", x), _clamp_reference(x[:, 0], x[:, 1], np.full(len(x), 0.5)))
    # a + b: records (a b, c) of the same set, rounded once by the sum itself
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.concatenate([np.column_stack([a * b, c]), np.column_stack([a, c]), np.column_stack([b, -b]), np.column_stack([_steps(1.0 - c, 1), c])])
    p = np.ascontiguousarray(p)
    got = api.math_probe("add_clamp01", p)
    assert np.array_equal(got, _clamp_reference(p[:, 0], np.ones(len(p)), p[:, 1]))
    # every slot of a record carries the value, and a length that is no multiple of the arity is refused
    L = api.load()
    x = np.ascontiguousarray(r[:8]).reshape(-1)
    y = np.zeros_like(x)
    assert L.is3d_math_probe(api.MATH_FUNCS["fma_clamp01"], x.size, x.ctypes.data_as(api._dp), y.ctypes.data_as(api._dp), -1) == 0
    assert np.array_equal(y.reshape(-1, 3), np.repeat(_clamp_reference(r[:8, 0], r[:8, 1], r[:8, 2])[:, None], 3, axis=1))
    for name, arity in api.MATH_ARITY.items():
        assert L.is3d_math_probe(api.MATH_FUNCS[name], arity + 1, x.ctypes.data_as(api._dp), y.ctypes.data_as(api._dp), -1) == api.IS3D_EINVAL, name


@pytest.mark.parametrize("RB", [2, 3, 4, 8])
def test_rcp_batch(RB):
    """one v_rcp_f64 for RB quotients (the kernels instantiate 2, 3, 4 and 8; 3 takes the prefix-product branch): records log-uniform in
    [2^-100, 2^100] with mixed signs -- the product of eight stays below 2^800, inside the caller's contract -- and every quotient within
    4e-15 + (RB + 2) 2^-53 of 1 / q_i: rcp_nr1's asserted bound plus the roundings the comment in cf_math.h counts"""
    rng = np.random.default_rng(100 + RB)
    q = np.exp2(rng.uniform(-100.0, 100.0, (20000, RB))) * rng.choice([-1.0, 1.0], (20000, RB))
    q[:RB] = np.ldexp(1.0, 100) * np.where(np.eye(RB) > 0, -1.0, 1.0)          # the largest product, every sign pattern of one negative
    q[RB:2 * RB] = np.ldexp(1.0, -100)
    with np.errstate(over="raise", under="raise"):
        assert np.isfinite(np.prod(q, axis=1)).all()
    got = api.math_probe("rcp_batch%d" % RB, np.ascontiguousarray(q))
    assert got.shape == q.shape
    err = float(np.max(np.abs(got.astype(LD) * q.astype(LD) - 1)))
    print("rcp_batch<%d>: worst quotient error %.3e (bound %.3e)" % (RB, err, 4e-15 + (RB + 2) * 2.0 ** -53))
    assert err < 4e-15 + (RB + 2) * 2.0 ** -53
