"""The arithmetic helpers of the throughput kernels (sipnet_amd/csrc/fast_math.h) on the device, on their own, through
sipnet_debug_fast_math (csrc/fast_math_probe.hip: compiled with the flags of step_fast.o): fexp2 bit for bit against the
emulation of tests/fast_math_reference.py and within the header's bound of the true 2^x, fdiv's error exact through
rationals and its range of validity, the float overloads against correctly rounded floats, the clamps, recR, and the hook's
refusals.  The yardsticks are held on the CPU by tests/test_fast_math_reference.py.  Every figure is printed before it is
asserted (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import fast_math_reference as fm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261020
F32_MAX = float(np.finfo(np.float32).max)
F64_MAX = float(np.finfo(np.float64).max)


def run(op, x, y=None, prec=sa.F64):
    """numpy in, numpy out"""
    tx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV)
    ty = None if y is None else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(DEV)
    return sa.debug_fast_math(op, tx, ty, prec).cpu().numpy()


def library_info():
    info = []
    sa.debug_fast_math(_lib.FM_EXP2, torch.empty(0, dtype=torch.float64, device=DEV), info=info)
    return tuple(info)


@pytest.fixture(scope="module")
def build():
    degree, newton = library_info()
    assert degree in fm.DEGREES and newton >= 0, (degree, newton)
    return degree, newton


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, x):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]]


# ---- a. fexp2, double, bit for bit -----------------------------------------------------------------------------------------

# The arguments the step kernels give fexp2 (fast_body.inc, coop_wave_light / _factor / _water.inc), with the parameter ranges
# of tests/golden/smoke/niwot/sipnet.param and forcings to +-60 C:
CALL_SITE_RANGES = {
    # Q10 factors: t10 * log2(Q10), t10 = T / 10 in [-6, 6], Q10 in [1.4, 5]: |x| <= 6 log2(5)
    "q10": (-14.0, 14.0),
    # canopy attenuation K_attl * lai = -attenuation / 6 * log2(e) * lai, attenuation in [0.38, 0.62], lai to 30
    "canopy_r1": (-4.5, 0.0),
    # light saturation q * r^k, q = -par / halfSatPar (par to 100 a day step, halfSatPar from 4; down to 1e-4 / 27), 0 < r <= 1
    "canopy_q": (-100.0, 0.0),
    # soil resistance K_c1l - K_c2l * wf = (rSoilConst1 - rSoilConst2 * wf) log2(e), constants in [0, 16.4] and [0, 8.6], wf in [0, 1]
    "rsoil": (-12.5, 23.7),
    # VPD term K_vexp * log2vpd, dVpdExp in [1, 3], log2vpd from log2(1e-6) (the plan's floor of a zero VPD) to log2(1e4)
    "vpd": (-59.8, 39.9),
}


def crafted_points():
    pts = [x for x, _ in fm.crafted_exp2_points()]
    pts += [k * 0.5 for k in range(-2160, 2061)]                   # every integer and half-integer of [-1080, 1030]
    ks = list(range(-8, 12)) + [-1075, -1074, -1073, -1023, -1022, -1021, -512, -100, -53, -52, 52, 53, 100, 511, 1000, 1021,
                                1022, 1023, 1024, 1029]
    assert len(ks) == 40
    for k in ks:                                                    # both neighbours of k +- 0.5
        for h in (k - 0.5, k + 0.5):
            pts += [math.nextafter(h, -math.inf), math.nextafter(h, math.inf)]
    return np.array(pts)


_emulated = {}


def emulated(name, x, degree):
    """exp2_emulated over x, once per point set"""
    if (name, degree) not in _emulated:
        _emulated[(name, degree)] = np.array([fm.exp2_emulated(v, degree) for v in x])
    return _emulated[(name, degree)]


def test_exp2_bits_on_the_crafted_points_the_integers_the_ties_and_their_neighbours(build):
    degree, _ = build
    x = crafted_points()
    got = run(_lib.FM_EXP2, x)
    assert_bits(got, emulated("crafted", x, degree), x)
    for (v, want), g in zip(fm.crafted_exp2_points(), got):
        if want is not None:
            assert g == want, (v, g, want)


def test_exp2_bits_on_uniform_points_of_the_whole_range(build):
    degree, _ = build
    x = np.random.default_rng(SEED).uniform(-1080.0, 1030.0, 20000)
    assert_bits(run(_lib.FM_EXP2, x), emulated("uniform", x, degree), x)


@pytest.mark.parametrize("site", list(CALL_SITE_RANGES))
def test_exp2_bits_on_the_ranges_of_the_call_sites(build, site):
    degree, _ = build
    lo, hi = CALL_SITE_RANGES[site]
    rng = np.random.default_rng(SEED + 1 + list(CALL_SITE_RANGES).index(site))
    x = rng.uniform(lo, hi, 5000)
    if site == "canopy_q":                                          # half of them log-uniform down to -1e-12: the deep layers
        x[::2] = -np.exp(rng.uniform(math.log(1e-12), math.log(100.0), x[::2].size))
    x[:2] = lo, hi
    got = run(_lib.FM_EXP2, x)
    assert_bits(got, emulated(site, x, degree), x)
    worst = max(fm.exp2_rel_err(g, v) for g, v in zip(got[::10], x[::10]))
    print(f"fexp2 {site} [{lo}, {hi}]: worst |rel err| on {x[::10].size} points = {worst:.4e}")
    assert worst <= fm.exp2_bound(degree)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_exp2_bits_at_the_probes_own_tail(build, length):
    """lengths around the wavefront and the 256-thread workgroup; the elements past n stay as they were"""
    degree, _ = build
    x = np.random.default_rng(SEED).uniform(-1080.0, 1030.0, 20000)[:length]
    want = emulated("uniform", np.random.default_rng(SEED).uniform(-1080.0, 1030.0, 20000), degree)[:length]
    pad = 300
    tx = torch.from_numpy(np.concatenate([x, np.full(pad, 3.0)])).to(DEV)
    out = torch.full((length + pad,), -7.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    assert sa.lib().sipnet_debug_fast_math(_lib.FM_EXP2, sa.F64, length, _lib.ptr(tx), None, _lib.ptr(out), None) == _lib.OK
    got = out.cpu().numpy()
    assert_bits(got[:length], want, x)
    assert (got[length:] == -7.0).all()


# ---- b. fexp2, double, against the truth -----------------------------------------------------------------------------------

def test_exp2_against_numpy_and_the_50_digit_truth(build):
    degree, _ = build
    rng = np.random.default_rng(SEED + 10)
    x = rng.uniform(-60.0, 20.0, 1 << 20)
    x[:4] = -60.0, 20.0, -59.5, 19.5
    got = run(_lib.FM_EXP2, x)
    ref = np.exp2(x)
    rel = np.abs(got - ref) / ref
    bound = fm.exp2_bound(degree)
    print(f"fexp2 degree {degree}: worst |rel err| against np.exp2 on 2^20 points of [-60, 20] = {rel.max():.4e} "
          f"(bound {bound + 2.0 ** -52:.4e})")
    assert rel.max() <= bound + 2.0 ** -52
    # the sharp check: the 10 000 worst of the sweep and 10 000 random ones of the rest against 2^x to 50 digits
    order = np.argsort(rel)
    pick = np.unique(np.concatenate([order[-10000:], rng.choice(order[:-10000], 10000, replace=False), np.arange(4)]))
    assert pick.size >= 20000
    worst = max(fm.exp2_rel_err(got[i], x[i]) for i in pick)
    print(f"fexp2 degree {degree}: worst |rel err| against the 50-digit 2^x on {pick.size} points = {worst:.4e} "
          f"= {worst / bound:.4f} of the bound {bound:.4e}")
    assert worst <= bound


# ---- c. fexp2 outside the polynomial's range -------------------------------------------------------------------------------

# fast_math.h: fexp2's domain is the finite doubles.  Past +-2^31 the conversion (int)n saturates and v_ldexp_f64 clamps, which
# gives 0 and +inf as exp2 does.  -inf gives NaN (-inf - rint(-inf)), +inf gives NaN too.  No caller leaves the domain: every
# argument is a product of a finite parameter-derived constant and a finite record field or a clamped state
# (CALL_SITE_RANGES; log2vpd is floored at log2(1e-6) by the plan, plan.cpp).
OUTSIDE_ZERO = [-1100.0, -1200.5, -4096.0, -2.0 ** 31 + 1.0, -2.0 ** 31, -2.0 ** 31 - 1.0, -2.0 ** 40, -1e300, -F64_MAX]
OUTSIDE_INF = [1024.0, 1024.5, 1100.0, 4096.0, 2.0 ** 31 - 1.0, 2.0 ** 31, 2.0 ** 31 + 1.0, 2.0 ** 40, 1e300, F64_MAX]
NO_CALLER = ("fexp2's domain is the finite doubles (fast_math.h): x - rint(x) is NaN for an infinite x, and no caller can pass "
             "one -- every argument is a finite parameter-derived constant times a finite record field or a clamped state")


@pytest.mark.parametrize("x", OUTSIDE_ZERO)
def test_exp2_far_below_the_range_is_zero(x):
    got = run(_lib.FM_EXP2, np.array([x]))[0]
    print(f"fexp2({x!r}) = {got!r}")
    assert got == 0.0


@pytest.mark.parametrize("x", OUTSIDE_INF)
def test_exp2_above_the_range_is_inf(x):
    got = run(_lib.FM_EXP2, np.array([x]))[0]
    print(f"fexp2({x!r}) = {got!r}")
    assert got == math.inf


@pytest.mark.xfail(strict=True, reason=NO_CALLER)
def test_exp2_of_minus_infinity_is_zero():
    got = run(_lib.FM_EXP2, np.array([-math.inf]))[0]
    print(f"fexp2(-inf) = {got!r}")
    assert got == 0.0


@pytest.mark.xfail(strict=True, reason=NO_CALLER)
def test_exp2_of_plus_infinity_is_infinity():
    got = run(_lib.FM_EXP2, np.array([math.inf]))[0]
    print(f"fexp2(+inf) = {got!r}")
    assert got == math.inf


# ---- d. fdiv, double -------------------------------------------------------------------------------------------------------

def mantissas(rng, n):
    """[1, 2): a third uniform, a third within 8 ulp above 1, a third within 8 ulp below 2"""
    m = rng.uniform(1.0, 2.0, n)
    kind = rng.integers(0, 3, n)
    near = rng.integers(0, 9, n) * 2.0 ** -52
    return np.where(kind == 0, m, np.where(kind == 1, 1.0 + near, 2.0 - 2.0 ** -52 - near))


def pairs(rng, n):
    """(a, b): b = m 2^eb, eb in [-1021, 1021]; the quotient m' 2^eq, eq in [-1020, 1020]; every pairing of the two binades for
    which a = fl(quotient b) is a normal double (drawn by rejection), signs of a mixed"""
    eb = rng.integers(-1021, 1022, 3 * n)
    eq = rng.integers(-1020, 1021, 3 * n)
    ok = (eb + eq >= -1021) & (eb + eq <= 1021)
    eb, eq = eb[ok][:n], eq[ok][:n]
    assert eb.size == n
    b = np.ldexp(mantissas(rng, n), eb)
    a = np.ldexp(mantissas(rng, n), eq) * b
    a = np.where(rng.random(n) < 0.25, -a, a)
    assert np.isfinite(a).all() and (np.abs(a) >= 2.0 ** -1022).all()
    return a, b


def crafted_pairs():
    a, b = [], []
    for eb in (-1021, -1000, -512, -1, 0, 1, 512, 1000, 1021):
        for mb in (1.0, 1.0 + 2.0 ** -52, 1.5, 2.0 - 2.0 ** -52):
            bb = math.ldexp(mb, eb)
            for eq in (-1020, -600, -1, 0, 1, 600, 1020):
                if not -1021 <= eb + eq <= 1021:
                    continue
                exact = math.ldexp(bb, eq)                          # quotient 2^eq exactly, then one ulp of a off it
                for aa in (exact, math.nextafter(exact, math.inf), math.nextafter(exact, 0.0), -exact):
                    a.append(aa)
                    b.append(bb)
            a += [0.0, -0.0, bb, -bb, 3.0 * bb, bb / 3.0]           # a = +-0, a = b, an exact and an inexact quotient
            b += [bb] * 6
    return np.array(a), np.array(b)


def worst_ulps(a, b, q):
    u = np.array([fm.div_ulps(x, y, z) for x, y, z in zip(a, b, q)])
    return u


def test_fdiv_error_is_at_most_one_ulp_exactly(build):
    """1 ulp is derived (u = 2^-53): after the Newton steps r is within a few u of 1 / b for any v_rcp_f64 seed of 2^-14 relative
    or better, q = a r is then within a few ulp, and the residual step fma(fma(-b, q, a), r, q) leaves 0.5 ulp plus a term of
    order u^2; 1 ulp leaves room without admitting a missing Newton or residual step"""
    rng = np.random.default_rng(SEED + 20)
    ca, cb = crafted_pairs()
    ra, rb = pairs(rng, 20000)
    # the same pairings with a in its lowest binades, 2^-1021 .. 2^-960, where the residual a - b q falls among the denormals
    ta, tb = pairs(rng, 400000)
    tiny = np.abs(ta) < 2.0 ** -960
    ta, tb = ta[tiny][:4000], tb[tiny][:4000]
    assert ta.size >= 2000
    for name, a, b in (("crafted", ca, cb), ("random", ra, rb), ("random, a below 2^-960", ta, tb)):
        q = run(_lib.FM_DIV, a, b)
        assert np.isfinite(q).all(), name
        u = worst_ulps(a, b, q)
        exact = np.abs(bits(q) - bits(a / b)) == 0
        zero = a == 0.0
        assert (q[zero] == 0.0).all()
        k = int(np.argmax(u))
        print(f"fdiv {name}: {a.size} pairs, worst {u.max():.4f} ulp at a = {float(a[k]).hex()}, b = {float(b[k]).hex()}; "
              f"correctly rounded {100.0 * exact.mean():.3f} %")
        assert u.max() <= 1.0, (name, float(a[k]).hex(), float(b[k]).hex(), float(q[k]).hex())


def test_fdiv_sweep_against_the_ieee_quotient():
    rng = np.random.default_rng(SEED + 21)
    a, b = pairs(rng, 1 << 20)
    q = run(_lib.FM_DIV, a, b)
    d = fm.ulp_distance(q, a / b)
    print(f"fdiv sweep: 2^20 pairs, {int((d > 0).sum())} results differ from the IEEE quotient, by at most {int(d.max())} unit(s) "
          f"in the last place; correctly rounded {100.0 * (d == 0).mean():.4f} %")
    assert d.max() <= 1.0


# The contract of fdiv(double), as fast_math.h states it: 2^-1021 <= b < 2^1022 (1 / b and its Newton steps stay normal) and
# a = 0 or a / b a normal double: at most 1 ulp.
CONTRACT_B = (-1021, 1021)


def ladder(mode):
    """per binade e: the worst error in ulp (inf: a non-finite result) over four mantissas of b and four of the quotient.
    "b, a of order 1": b = m 2^e, quotients of order 1 / b;  "b, a of order b": b = m 2^e, quotients of order 1;
    "a": a = m 2^e against b of order 1.  Only pairs whose exact quotient is a normal double."""
    es, a, b = [], [], []
    for e in range(-1074, 1024):
        for mb in (1.0, 1.0 + 2.0 ** -52, 1.5, 2.0 - 2.0 ** -52):
            for mq in (1.0, 1.3, 0.7, 2.0 - 2.0 ** -52):
                if mode == "a":
                    aa, bb = math.ldexp(mq, e), mb
                else:
                    bb = math.ldexp(mb, e)
                    aa = mq * bb if mode == "b, a of order b" else mq
                if aa == 0.0 or bb == 0.0 or math.isinf(aa) or math.isinf(bb):
                    continue
                if not fm.Fraction(2) ** -1022 <= fm.Fraction(aa) / fm.Fraction(bb) < fm.Fraction(2) ** 1024:
                    continue                                         # (the quotient itself leaves the normal doubles)
                es.append(e)
                a.append(aa)
                b.append(bb)
    a, b = np.array(a), np.array(b)
    q = run(_lib.FM_DIV, a, b)
    worst = {}
    for e, x, y, z in zip(es, a, b, q):
        worst[e] = max(worst.get(e, 0.0), fm.div_ulps(x, y, z) if math.isfinite(z) else math.inf)
    return worst


@pytest.mark.parametrize("mode", ["b, a of order 1", "b, a of order b", "a"])
def test_fdiv_range_over_the_binade_ladder(mode):
    """the smallest and the largest binade, walking out from 2^0, down to and up to which the error stays within 1 ulp: what
    fast_math.h states as the contract (CONTRACT_B for b, a margin inside what is measured; any a whose quotient is normal: the
    residual a - b q of a below 2^-969 falls among the denormals, and the error there still measured 0.70 ulp at the most)"""
    worst = ladder(mode)
    lo = hi = 0
    while lo - 1 in worst and worst[lo - 1] <= 1.0:
        lo -= 1
    while hi + 1 in worst and worst[hi + 1] <= 1.0:
        hi += 1
    below = {e: round(worst[e], 3) for e in sorted(e for e in worst if e < lo)[-3:]}
    above = {e: round(worst[e], 3) for e in sorted(e for e in worst if e > hi)[:3]}
    beyond = [v for e, v in worst.items() if not lo <= e <= hi]
    print(f"fdiv ladder ({mode}): <= 1 ulp (worst {max(worst[e] for e in range(lo, hi + 1)):.4f}) for binades 2^{lo} .. 2^{hi} of "
          f"{min(worst)} .. {max(worst)} tested; just below: {below}; just above: {above}; worst beyond: {max(beyond, default=0.0)}")
    if mode == "a":                                                  # every binade of a whose quotient is normal
        assert lo == min(worst) <= -1022 and hi == max(worst) >= 1022, (lo, hi)
    else:
        assert lo <= CONTRACT_B[0] and hi >= CONTRACT_B[1], (lo, hi)


EDGES = [
    ("b denormal (2^-1030)", 1.0, 2.0 ** -1030), ("b the largest denormal", 1.0, 2.0 ** -1022 - 2.0 ** -1074),
    ("b = 2^-1022", 1.0, 2.0 ** -1022), ("b = 2^-1074, a = 2^-1070", 2.0 ** -1070, 2.0 ** -1074),
    ("b = 2^1022", 2.0 ** 1022, 2.0 ** 1022), ("b = 1.5 2^1022", 3.0, 1.5 * 2.0 ** 1022), ("b = 2^1023", 2.0 ** 1023, 2.0 ** 1023),
    ("b = DBL_MAX", 1.0, F64_MAX), ("b = +inf", 1.0, math.inf), ("b = 0", 1.0, 0.0), ("0 / 0", 0.0, 0.0),
    ("a = +inf", math.inf, 2.0), ("inf / inf", math.inf, math.inf),
    ("a / b overflows", 2.0 ** 1000, 2.0 ** -100), ("a / b just overflows", F64_MAX, 0.5),
    ("a / b denormal", 2.0 ** -1000, 2.0 ** 50), ("a / b = 2^-1074", 2.0 ** -1000, 2.0 ** 74), ("a / b underflows to 0", 2.0 ** -1000, 2.0 ** 200),
    ("a tiny, quotient normal", 3.0 * 2.0 ** -1022, 7.0 * 2.0 ** -1000),
]


def test_fdiv_at_the_edges_of_well_scaled():
    """recorded, next to the IEEE quotient (fast_math.h and NOTES.md quote this table); asserted: inside CONTRACT_B with a
    normal quotient the result is within 1 ulp, and b = 0, b = +inf and a denormal b below 2^-1024 do NOT give the IEEE quotient
    (which is why every caller guards or discards them)"""
    a = np.array([e[1] for e in EDGES])
    b = np.array([e[2] for e in EDGES])
    q = run(_lib.FM_DIV, a, b)
    with np.errstate(all="ignore"):
        ieee = a / b
    got = {}
    for (name, x, y), g, w in zip(EDGES, q, ieee):
        off = f"   {fm.div_ulps(x, y, g):.3f} ulp" if math.isfinite(g) and math.isfinite(x) and math.isfinite(y) and y != 0.0 else ""
        print(f"fdiv edge: {name:28s} a = {float(x).hex():>24s} b = {float(y).hex():>24s} -> {float(g)!r:>24s}   IEEE {float(w)!r}{off}")
        got[name] = float(g)
    for name in ("b = +inf", "b = 0", "b denormal (2^-1030)"):
        assert math.isnan(got[name]) or got[name] != dict(zip([e[0] for e in EDGES], ieee))[name], name


# ---- e. the float overloads and the small helpers --------------------------------------------------------------------------

def test_exp2_float_is_within_one_ulp():
    """v_exp_f32 is specified to 1 ulp; the yardstick is float64 exp2 of the float argument (its own error, 2^-52, is 2^-29 float ulp)"""
    rng = np.random.default_rng(SEED + 30)
    x = rng.uniform(-125.0, 127.0, 1 << 20).astype(np.float32)
    grid = np.arange(-125.0, 127.5, 0.5)                            # every integer and half-integer, both ends
    x[:grid.size] = grid
    x = x.astype(np.float64)
    got = run(_lib.FM_EXP2, x, prec=sa.F32_MIXED)
    assert (got == got.astype(np.float32)).all()
    truth = np.exp2(x)
    u = fm.ulps32(got, truth)
    rounded = (got == truth.astype(np.float32)).mean()
    k = int(np.argmax(u))
    print(f"fexp2(float): 2^20 floats of [-125, 127], worst {u.max():.4f} ulp at x = {x[k]!r}; correctly rounded {100.0 * rounded:.3f} %")
    assert u.max() <= 1.0


def test_exp2_float_outside_the_normal_range():
    lo = np.array([-126.5, -127.0, -130.0, -140.0, -149.0, -149.5, -151.0, -200.0, -1e30, -F32_MAX])
    hi = np.array([128.0, 128.5, 200.0, 1e30, F32_MAX])
    got_lo = run(_lib.FM_EXP2, lo, prec=sa.F32_MIXED)
    got_hi = run(_lib.FM_EXP2, hi, prec=sa.F32_MIXED)
    for x, g in zip(np.concatenate([lo, hi]), np.concatenate([got_lo, got_hi])):
        print(f"fexp2(float {x!r}) = {float(g)!r}")
    flushed = not (got_lo[:5] > 0.0).any()
    print("fexp2(float): results below 2^-126 are " + ("flushed to 0" if flushed else "denormal floats"))
    assert ((got_lo >= 0.0) & (got_lo <= 2.0 ** -126)).all()
    assert (got_hi == math.inf).all()


def test_fdiv_float_is_within_two_ulp():
    """a * v_rcp_f32(b): 1 ulp from the reciprocal, 0.5 from the product, and room for how they combine: 2 ulp; b and the quotient
    within 2^[-120, 120] and a normal, so that 1 / b, a and a / b are normal floats"""
    rng = np.random.default_rng(SEED + 31)
    n = 1 << 20
    eb = rng.integers(-120, 121, 3 * n)
    eq = rng.integers(-120, 121, 3 * n)
    ok = np.abs(eb + eq) <= 120
    eb, eq = eb[ok][:n], eq[ok][:n]
    m1 = (1.0 + rng.integers(0, 1 << 23, n) * 2.0 ** -23)
    m2 = (1.0 + rng.integers(0, 1 << 23, n) * 2.0 ** -23)
    edge = rng.integers(0, 4, n)
    m1 = np.where(edge == 0, 1.0 + rng.integers(0, 4, n) * 2.0 ** -23, np.where(edge == 1, 2.0 - (1 + rng.integers(0, 4, n)) * 2.0 ** -23, m1))
    b = np.ldexp(m1, eb).astype(np.float32).astype(np.float64)
    a = (np.ldexp(m2, eq) * b).astype(np.float32).astype(np.float64)
    a = np.where(rng.random(n) < 0.25, -a, a)
    a[:4], b[:4] = [1.0, 6.0, 0.0, -0.0], [3.0, 3.0, 5.0, 5.0]
    got = run(_lib.FM_DIV, a, b, prec=sa.F32_MIXED)
    assert (got == got.astype(np.float32)).all() and (got[2:4] == 0.0).all()
    u = fm.ulps32(got[4:], a[4:] / b[4:])                            # (the double quotient of two floats: 2^-29 float ulp from exact)
    u = np.concatenate([[fm.div_ulps_f32(a[i], b[i], got[i]) for i in range(2)], u])
    rounded = (got == (a / b).astype(np.float32)).mean()
    k = int(np.argmax(u))
    print(f"fdiv(float): 2^20 pairs, worst {u.max():.4f} ulp at a = {a[k]!r}, b = {b[k]!r}; correctly rounded {100.0 * rounded:.3f} %")
    worst = np.argsort(u)[-200:]
    exact = max(fm.div_ulps_f32(a[i], b[i], got[i]) for i in worst)
    assert exact <= 2.0 and u.max() <= 2.0 + 1e-6


def test_fdiv_float_outside_its_range_is_recorded():
    """what a * v_rcp_f32(b) returns outside 2^[-120, 120], next to the correctly rounded float quotient (fast_math.h quotes it);
    asserted: a zero, denormal or infinite b does not crash the probe and a = 0 over a normal b is 0"""
    f = np.float32
    cases = [("b = 0", 1.0, 0.0), ("0 / 0", 0.0, 0.0), ("b = 2^-149", 1.0, 2.0 ** -149), ("b = 2^-127", 2.0 ** -100, 2.0 ** -127),
             ("0 / 2^-130", 0.0, 2.0 ** -130), ("b = 2^-126", 1.0, 2.0 ** -126), ("b = 2^126", 1.0, 2.0 ** 126), ("b = 2^127", 1.0, 2.0 ** 127),
             ("b = 1.5 2^127", 2.0 ** 120, 1.5 * 2.0 ** 127), ("b = +inf", 1.0, math.inf), ("a = +inf", math.inf, 2.0),
             ("quotient denormal", 2.0 ** -100, 2.0 ** 40), ("quotient overflows", 2.0 ** 100, 2.0 ** -100), ("0 / 3", 0.0, 3.0)]
    a = np.array([c[1] for c in cases])
    b = np.array([c[2] for c in cases])
    got = run(_lib.FM_DIV, a, b, prec=sa.F32_MIXED)
    with np.errstate(all="ignore"):
        ieee = (a.astype(f) / b.astype(f)).astype(np.float64)
    for (name, x, y), g, w in zip(cases, got, ieee):
        print(f"fdiv(float) edge: {name:20s} a = {x!r:>24} b = {y!r:>24} -> {float(g)!r:>24}   IEEE float {float(w)!r}")
    assert got[-1] == 0.0 and abs(got[5] / 2.0 ** 126 - 1.0) <= 2.0 ** -22            # (the last normal b: still within 2 ulp)


SMALL64 = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, -(2.0 ** -1022), 1e-310, 0.25, 1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, -1.0, 2.5,
           -3.75, 1e300, -1e300, math.inf, -math.inf]
SMALL32 = [0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126), 2.0 ** -130, 0.25, 1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, -1.0,
           2.5, -3.75, F32_MAX, -F32_MAX, math.inf, -math.inf]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_the_clamps_are_min_and_max(prec):
    vals = np.array(SMALL64 if prec == sa.F64 else SMALL32)
    x, y = [v.ravel() for v in np.meshgrid(vals, vals)]
    for name, op, got, want in (("rminv", _lib.FM_RMINV, run(_lib.FM_RMINV, x, y, prec), np.minimum(x, y)),
                                ("rmax0", _lib.FM_RMAX0, run(_lib.FM_RMAX0, vals, None, prec), np.maximum(vals, 0.0)),
                                ("clip01", _lib.FM_CLIP01, run(_lib.FM_CLIP01, vals, None, prec), np.minimum(np.maximum(vals, 0.0), 1.0))):
        bad = np.nonzero(~(got == want))[0]                          # (== : +0 and -0 are one value; no NaN in, none out)
        assert bad.size == 0, (name, [(float(got[i]), float(want[i])) for i in bad[:6]])
        nz = want != 0.0
        assert (bits(got)[nz] == bits(want)[nz]).all(), name


def slot_of(f32):
    """plan.h's narrow slot: the float in the low word, the quiet-NaN tag 0x7FF80000 above"""
    lo = np.asarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (np.uint64(0x7FF8000000000000) | lo).view(np.float64)


def test_recr_reads_the_low_word_of_a_narrow_slot_and_leaves_a_double_alone():
    f = np.array([0.0, -0.0, 1.0, -1.5, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, 2.0 ** -126, F32_MAX, -F32_MAX, math.inf, -math.inf,
                  0.1, 287.15, -40.0], dtype=np.float32)
    got = run(_lib.FM_RECR, slot_of(f), prec=sa.F32_MIXED)
    assert (got.astype(np.float32).view(np.uint32) == f.view(np.uint32)).all(), got
    assert (bits(got) == bits(f.astype(np.float64))).all()           # (widened exactly: denormal floats and -0.0 kept)
    d = np.array(SMALL64 + [0.1, 287.15, -40.0, F64_MAX])
    assert (bits(run(_lib.FM_RECR, d, prec=sa.F64)) == bits(d)).all()


# ---- f. refusals -----------------------------------------------------------------------------------------------------------

def test_the_hook_refuses_bad_arguments():
    L = sa.lib()
    x = torch.ones(8, dtype=torch.float64, device=DEV)
    out = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    px, po = _lib.ptr(x), _lib.ptr(out)
    info = (C.c_int32 * 2)(-1, -1)
    bad = _lib.ERR_BAD_ARGUMENT
    assert L.sipnet_debug_fast_math(-1, sa.F64, 8, px, px, po, info) == bad
    assert L.sipnet_debug_fast_math(6, sa.F64, 8, px, px, po, info) == bad
    assert b"sipnet_debug_fast_math" in L.sipnet_last_error()
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, 2, 8, px, px, po, info) == bad
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, -1, 8, px, px, po, info) == bad
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, sa.F64, -1, px, px, po, info) == bad
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, sa.F64, (1 << 31) + 1, px, px, po, info) == bad      # (refused before anything is read)
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, sa.F64, 8, None, px, po, info) == bad
    assert L.sipnet_debug_fast_math(_lib.FM_EXP2, sa.F64, 8, px, px, None, info) == bad
    for op in (_lib.FM_DIV, _lib.FM_RMINV):
        assert L.sipnet_debug_fast_math(op, sa.F64, 8, px, None, po, info) == bad
        assert L.sipnet_debug_fast_math(op, sa.F32_MIXED, 8, px, None, po, info) == bad
    assert list(info) == [-1, -1]
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()                         # nothing was launched
    # what is allowed: no second operand where none is read, NULL arrays with n = 0, no info
    for op in (_lib.FM_EXP2, _lib.FM_RMAX0, _lib.FM_CLIP01, _lib.FM_RECR):
        assert L.sipnet_debug_fast_math(op, sa.F64, 8, px, None, po, None) == _lib.OK
    assert L.sipnet_debug_fast_math(_lib.FM_DIV, sa.F64, 0, None, None, None, info) == _lib.OK
    assert tuple(info) == library_info()
    assert sa.debug_fast_math(_lib.FM_DIV, torch.empty(0, dtype=torch.float64, device=DEV), torch.empty(0, dtype=torch.float64, device=DEV)).numel() == 0
