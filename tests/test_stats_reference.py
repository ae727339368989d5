"""tests/stats_reference.py against fractions.Fraction, and its bounds against sums that are wrong and sums that are merely
rounded: the yardstick of tests/test_gpu_stats_edges.py must itself be exact, refuse a dropped or doubled element and a plane
read at the wrong pitch, and accept a correct double-precision sum in whatever order it was added."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import stats_reference as sr


def fraction_stats(v):
    fr = [Fraction(float(e)) for e in v]
    return sum(fr, Fraction(0)), sum((f * f for f in fr), Fraction(0))


def rounded(f):
    try:
        return float(f)
    except OverflowError:
        return math.inf if f > 0 else -math.inf


def inputs():
    rng = np.random.default_rng(20)
    out = {}
    for n in (1, 2, 3, 17, 64, 65, 257):
        out[f"normal{n}"] = rng.standard_normal(n) * 3.0 - 1.0
    big = rng.standard_normal(40) * 1e15
    out["cancelling"] = np.concatenate([big, -big, [1.0, 2.0 ** -40, -3.0]])
    out["cancelling_squares"] = np.array([2.0 ** 27 + 1.0, -(2.0 ** 27 + 1.0), 1.0 + 2.0 ** -30, 3.0])
    out["spread"] = 1e6 + 1e-3 * rng.standard_normal(129)
    out["denormals"] = 5e-324 * np.arange(1, 70)
    out["denormals_and_ones"] = np.concatenate([5e-324 * np.arange(1, 9), [1.0, -1.0], 2.0 ** -1040 * np.arange(1, 5)])
    out["float_denormals"] = (np.float32(2.0 ** -149) * np.arange(1, 50, dtype=np.float32)).astype(np.float64)
    out["near_underflow"] = 2.0 ** -537 * (1.0 + rng.random(33))        # squares around the smallest normal double
    out["huge"] = np.array([1e160, -1e160, 1e160, 3.0])
    out["near_overflow"] = np.array([1.5e308, 1.5e308, -1.5e308, 1e300])
    out["zeros"] = np.array([0.0, -0.0, 0.0])
    out["floats"] = rng.standard_normal(100).astype(np.float32).astype(np.float64)
    return out


INPUTS = inputs()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_reference_is_the_exact_sum_rounded_once(name):
    v = INPUTS[name]
    f1, f2 = fraction_stats(v)
    s1, s2 = sr.cell_stats(v)
    assert (s1, s2) == (rounded(f1), rounded(f2)), name
    # ... and the measured error of a value is its exact distance from the exact sum, rounded once
    for g1, g2 in ((s1, s2), (0.0, 0.0), (1.0, 2.5)):
        if not (math.isfinite(s1) and math.isfinite(s2)):
            continue
        e1, e2 = sr.cell_errors(g1, g2, v)
        assert (e1, e2) == (rounded(abs(Fraction(g1) - f1)), rounded(abs(Fraction(g2) - f2))), name
    # the split squares are exact where the fast path takes them
    if sr._safe(v):
        for x, t in zip(v, sr.square_terms(v)):
            assert sum((Fraction(float(e)) for e in t), Fraction(0)) == Fraction(float(x)) ** 2


def test_the_conventions_for_nan_infinities_and_overflow():
    nan, inf = math.nan, math.inf
    s = sr.plane_stats(np.array([[1.0, nan, 2.0, 3.0], [inf, 1.0, inf, -inf], [-inf, 0.0, 1e160, -1e160]]), 2, 2)
    assert np.isnan(s[0, 0]).all() and tuple(s[0, 1]) == (5.0, 13.0)
    assert tuple(s[1, 0]) == (inf, inf) and np.isnan(s[1, 1, 0]) and s[1, 1, 1] == inf
    assert tuple(s[2, 0]) == (-inf, inf) and tuple(s[2, 1]) == (0.0, inf)
    x = np.array([[1.0, nan, 2.0, 3.0], [inf, 1.0, inf, -inf], [-inf, 0.0, 1e160, -1e160]])
    r = sr.ratios(s, x, 2, 2)
    assert (r == 0.0).all()                                           # the same values: NaN equals NaN
    wrong = s.copy()
    wrong[0, 0, 0] = 3.0                                              # a NaN lost
    wrong[1, 1, 0] = inf                                              # inf - inf taken for inf
    wrong[2, 1, 1] = 1.7e308                                          # an overflow missed
    wrong[0, 1, 1] = nan                                              # a NaN that leaked into a neighbour
    r = sr.ratios(wrong, x, 2, 2)
    assert r[0, 0, 0] == inf and r[1, 1, 0] == inf and r[2, 1, 1] == inf and r[0, 1, 1] == inf
    assert (np.delete(r.reshape(-1), [0, 3, 6, 11]) == 0.0).all()
    # a cell of zeros has a zero bound on its sum: only zeros pass
    z = np.zeros((1, 4))
    assert (sr.ratios(np.zeros((1, 1, 2)), z, 1, 4) == 0.0).all()
    assert sr.ratios(np.array([[[5e-324, 0.0]]]), z, 1, 4)[0, 0, 0] == inf


def forward(v):
    s = np.float64(0.0)
    for e in v:
        s = s + e
    return float(s)


def pairwise(v):
    v = [np.float64(e) for e in v]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return float(v[0])


def lanes_then_butterfly(v):
    lanes = [np.float64(0.0)] * 64
    for i, e in enumerate(v):
        lanes[i % 64] = lanes[i % 64] + e
    off = 32
    while off:
        lanes = [lanes[i] + lanes[i ^ off] for i in range(64)]
        off >>= 1
    return float(lanes[0])


ORDERS = [forward, pairwise, lanes_then_butterfly]


@pytest.mark.parametrize("order", ORDERS, ids=[f.__name__ for f in ORDERS])
def test_a_correct_double_sum_in_any_order_is_inside_the_bounds(order):
    rng = np.random.default_rng(7)
    worst = 0.0
    cases = [INPUTS[k] for k in sorted(INPUTS) if k not in ("huge", "near_overflow")]
    cases += [rng.standard_normal(n) * 3.0 - 1.0 for n in (386, 1025, 4097)] + [1e6 + 1e-3 * rng.standard_normal(4097)]
    for v in cases:
        with np.errstate(under="ignore"):
            sq = np.asarray(v, dtype=np.float64) * np.asarray(v, dtype=np.float64)        # every square rounded once
        got = np.array([[[order(v), order(sq)]]])
        r = sr.ratios(got, np.asarray(v)[None, :], 1, len(v))
        worst = max(worst, float(r.max()))
    print(f"{order.__name__}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_a_wrong_sum_is_outside_the_bounds():
    rng = np.random.default_rng(11)
    for n in (2, 3, 65, 386, 4097):
        for v in (rng.standard_normal(n) * 3.0 - 1.0, 1e6 + 1e-3 * rng.standard_normal(n)):
            x = v[None, :]
            s1, s2 = sr.cell_stats(v)
            k = int(np.argmin(np.abs(v)))                             # the element whose loss shows least
            dropped = np.delete(v, k)
            r = sr.ratios(np.array([[sr.cell_stats(dropped)]]), x, 1, n)
            assert r[0, 0, 0] > 1.0 and r[0, 0, 1] > 1.0, (n, r)
            twice = np.append(v, v[k])
            r = sr.ratios(np.array([[sr.cell_stats(twice)]]), x, 1, n)
            assert r[0, 0, 0] > 1.0 and r[0, 0, 1] > 1.0, (n, r)
            assert (sr.ratios(np.array([[[s1, s2]]]), x, 1, n) <= 1.0 / n).all()       # the rounded sum itself: half an ulp <= u |sum|


def test_a_float_plane_read_at_the_pitch_of_doubles_is_outside_the_bounds():
    rng = np.random.default_rng(13)
    rows, n_sites, M = 4, 3, 21
    ld = n_sites * M + 1
    plane = (rng.standard_normal((2 * rows, ld)) * 3.0 - 1.0).astype(np.float32)
    flat = plane.reshape(-1)
    # row r read at element offset 2 r ld: the byte pitch of a plane of doubles
    misread = np.stack([flat[2 * r * ld:2 * r * ld + ld] for r in range(rows)])
    got = sr.plane_stats(misread, n_sites, M)
    r = sr.ratios(got, plane[:rows], n_sites, M)
    assert (r[0] <= 1.0).all()                                         # row 0 lies where it should
    assert (r[1:] > 1.0).all(), r
