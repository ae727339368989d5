"""Yardsticks of the throughput kernels' arithmetic helpers (sipnet_amd/csrc/fast_math.h); no tests in here, the standard
library and numpy only.

  exp2_emulated(x, degree)   the exact bits fexp2 must return for a double x: n = rint(x) (ties to even), f = x - n (exact),
                             the Horner chain of fused multiply-adds over the coefficients of tools/fit_exp2.fit(degree),
                             each rounded ONCE from the exact rational, and one last rounding of p 2^n from the exact
                             rational: the single rounding of ldexp into the denormals, 0 below 2^-1075, inf from 2^1024
  exp2_true(x)               2^x as a 50-digit Decimal, the way tools/fit_exp2.py computes it
  exp2_bound(degree)         the header's relative-error figure of the degree plus 2^-52 (the fused chain against the
                             tool's multiply + add)
  div_ulps(a, b, q)          |q - a/b| in units of ulp(a/b), exact; div_ulps_f32: the same for floats
  ulp_distance(p, q)         how many doubles lie between two arrays' elements (0: the same value; +0 and -0 are one)
"""
import importlib.util
import math
import os
import re
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "sipnet_amd", "csrc", "fast_math.h")

_spec = importlib.util.spec_from_file_location("fit_exp2", os.path.join(REPO, "tools", "fit_exp2.py"))
fit_exp2 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fit_exp2)        # (sets the Decimal context to 50 digits)

DEGREES = (8, 9, 11)
HEADER_FIGURES = {11: 1.7e-16, 9: 3.7e-14, 8: 2.2e-12}    # fast_math.h's comment; test_fast_math_reference holds them
_coef = {}


def coefficients(degree):
    """c1 .. cN of tools/fit_exp2.fit(degree), computed once"""
    if degree not in _coef:
        _coef[degree] = tuple(fit_exp2.fit(degree))
    return _coef[degree]


def header_coefficients(degree):
    """the literals of loadExp2Coef()'s branch for `degree`, as the doubles the compiler reads"""
    text = open(HEADER).read()
    m = re.search(r"SIPNET_EXP2_DEGREE == %d\s*\n\s*Exp2Coef k = \{(.*?)\};" % degree, text, re.S)
    return tuple(float(t) for t in m.group(1).replace("\n", " ").split(","))


def header_figures():
    """degree -> the |rel err| figure quoted in fast_math.h's comment"""
    text = open(HEADER).read()
    return {int(d): float(v) for d, v in re.findall(r"degree (\d+): (?:\|rel err\| <= )?([0-9.]+e-[0-9]+)", text)}


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # one rounding, to nearest even


def _round_scaled(p, n):
    """p 2^n rounded once to a double: denormals by the same single rounding, 0 below 2^-1075, inf from 2^1024"""
    n = max(-2200, min(2200, n))
    try:
        return float(Fraction(p) * Fraction(2) ** n)
    except OverflowError:
        return math.inf if p > 0 else -math.inf


def exp2_emulated(x, degree, coef=None):
    """the bits fexp2(double) must produce for a finite double |x| < 2^31"""
    x = float(x)
    assert math.isfinite(x) and abs(x) < 2.0 ** 31
    c = coefficients(degree) if coef is None else coef
    n = round(x)                                   # ties to even, an int
    f = x - float(n)
    assert Fraction(f) == Fraction(x) - n, "x - rint(x) is exact"
    p = c[-1]
    for ck in reversed(c[:-1]):
        p = _fma(p, f, ck)
    p = _fma(p, f, 1.0)
    return _round_scaled(p, n)


def exp2_emulated_parts(x):
    """(n, f) of the range reduction"""
    n = round(float(x))
    return n, float(x) - float(n)


def exp2_true(x):
    """2^x to 50 digits"""
    getcontext().prec = 50
    return (Decimal(float(x)) * fit_exp2.LN2).exp()


def exp2_rel_err(value, x):
    """|value - 2^x| / 2^x as a float"""
    t = exp2_true(x)
    return abs(float((Decimal(float(value)) - t) / t))


def exp2_bound(degree):
    return HEADER_FIGURES[degree] + 2.0 ** -52


def _floor_log2(q):
    """floor(log2 q) of a positive Fraction"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    return e


def ulp_of(exact, mant_bits=52, emin=-1022):
    """the unit in the last place of the binade a Fraction lies in (denormal spacing below 2^emin)"""
    if exact == 0:
        return Fraction(2) ** (emin - mant_bits)
    return Fraction(2) ** (max(_floor_log2(abs(exact)), emin) - mant_bits)


def div_ulps(a, b, q):
    """|q - a/b| / ulp(a/b) for doubles a, b (b != 0) and a finite double q"""
    exact = Fraction(float(a)) / Fraction(float(b))
    return float(abs(Fraction(float(q)) - exact) / ulp_of(exact))


def div_ulps_f32(a, b, q):
    """the same for floats: a, b, q are float32 values (given as anything float() reads), the ulp is float's"""
    for v in (a, b, q):
        assert float(np.float32(v)) == float(v), "not a float32 value"
    exact = Fraction(float(a)) / Fraction(float(b))
    return float(abs(Fraction(float(q)) - exact) / ulp_of(exact, 23, -126))


def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i, i)          # (monotone in the value; -0.0 -> 0 like +0.0)


def ulp_distance(p, q):
    """number of representable doubles from p to q, elementwise (finite or infinite values, no NaN), as float64"""
    a, b = _ordered(p), _ordered(q)
    far = np.abs(a.astype(np.float64) - b.astype(np.float64))            # (rounded: right for distances past 2^62 ...)
    with np.errstate(over="ignore"):
        near = np.abs(a - b).astype(np.float64)                           # (... exact where the difference fits an int64)
    return np.where(far > 2.0 ** 62, far, near)


def ulps32(value, truth):
    """|value - truth| in float32 ulps of truth's binade, elementwise in float64 (truth: the float64 yardstick, normal floats)"""
    truth = np.asarray(truth, dtype=np.float64)
    e = np.floor(np.log2(np.abs(truth)))
    e = np.where(np.abs(truth) < 2.0 ** e, e - 1, e)            # (a log2 rounded up at a binade's edge)
    return np.abs(np.asarray(value, dtype=np.float64) - truth) / 2.0 ** (np.maximum(e, -126) - 23)


def crafted_exp2_points():
    """the edge cases of the emulation and of the device alike: (x, what 2^x must emulate to, or None where only the bits count)"""
    return [(0.0, 1.0), (-0.0, 1.0), (1.0, 2.0), (-1.0, 0.5), (10.0, 1024.0), (-1022.0, 2.0 ** -1022), (-1074.0, 2.0 ** -1074),
            (0.5, None), (1.5, None), (2.5, None), (-0.5, None), (-1074.5, 2.0 ** -1074), (-1075.0, 0.0), (1023.999, None),
            (1024.0, math.inf)]


def exp2_grid(n=20000):
    """at least n points of [-0.5, 0.5]: evenly spaced with both ends, and 0, +-2^-60 and both neighbours of +-0.5 (the ones
    outside the interval reduce to the other end's side: x = 0.5 + ulp gives n = 1, f just above -0.5)"""
    pts = [-0.5 + i / float(n) for i in range(n + 1)]
    pts += [0.0, 2.0 ** -60, -2.0 ** -60, 0.5, -0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0),
            math.nextafter(-0.5, 0.0), math.nextafter(-0.5, -1.0)]
    return pts
