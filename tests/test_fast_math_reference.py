"""The yardsticks of tests/test_gpu_fast_math.py, held on the CPU: the coefficient literals of fast_math.h are the fit's,
the emulation of fexp2 stays within the header's figures of a 50-digit 2^x, its edge cases are what exp2 and a single
rounding give, a coefficient one ulp off changes its bits (so the device's bit comparison sees a wrong literal that the
error bound cannot), and div_ulps agrees with hand cases."""
import math

import numpy as np
import pytest

from tests import fast_math_reference as fm

_grid_err = {}


def grid_errors(degree):
    """(worst relative error of the emulation on the grid, the emulated values), once per degree"""
    if degree not in _grid_err:
        pts = fm.exp2_grid()
        vals = [fm.exp2_emulated(x, degree) for x in pts]
        _grid_err[degree] = (max(fm.exp2_rel_err(v, x) for v, x in zip(vals, pts)), pts, vals)
    return _grid_err[degree]


@pytest.mark.parametrize("degree", fm.DEGREES)
def test_the_header_literals_are_the_fit_to_the_bit(degree):
    lit = fm.header_coefficients(degree)
    fit = fm.coefficients(degree)
    assert len(fit) == degree and lit[:degree] == fit
    assert all(v == 0.0 for v in lit[degree:]) and len(lit) == 11


def test_the_figures_table_is_the_header_comment():
    assert fm.header_figures() == fm.HEADER_FIGURES


@pytest.mark.parametrize("degree", fm.DEGREES)
def test_the_emulation_is_within_the_bound_and_the_header_figure_is_not_smaller_than_the_grid(degree):
    worst, pts, _ = grid_errors(degree)
    assert len(pts) >= 20000
    for must in (0.5, -0.5, 0.0, 2.0 ** -60, -2.0 ** -60, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0),
                 math.nextafter(-0.5, 0.0), math.nextafter(-0.5, -1.0)):
        assert must in pts
    print(f"degree {degree}: worst |rel err| of the emulation on {len(pts)} points = {worst:.4e}, "
          f"bound {fm.exp2_bound(degree):.4e}, header {fm.HEADER_FIGURES[degree]:.1e}")
    assert worst <= fm.exp2_bound(degree)
    # the header's figure (plain Horner, two digits) is not smaller than what the grid gives, the fused chain's 2^-52 apart
    assert fm.HEADER_FIGURES[degree] + 2.0 ** -52 >= worst
    plain = fm.fit_exp2.max_rel_err(list(fm.coefficients(degree)))
    assert fm.HEADER_FIGURES[degree] >= plain, (degree, plain)


@pytest.mark.parametrize("degree", fm.DEGREES)
def test_the_edge_cases_of_the_emulation(degree):
    for k in list(range(-1074, 1024, 37)) + [-1074, -1022, -1, 0, 1, 1023]:
        assert fm.exp2_emulated(float(k), degree) == math.ldexp(1.0, k)            # integers: exact powers of two
    assert fm.exp2_emulated(0.0, degree) == 1.0 and fm.exp2_emulated(-0.0, degree) == 1.0
    assert fm.exp2_emulated_parts(0.5) == (0, 0.5)                                  # ties to even
    assert fm.exp2_emulated_parts(1.5) == (2, -0.5)
    assert fm.exp2_emulated_parts(2.5) == (2, 0.5)
    assert fm.exp2_emulated_parts(-0.5) == (0, -0.5) and fm.exp2_emulated_parts(-1.5) == (-2, 0.5)
    for x in (0.5, 1.5, 2.5):
        assert fm.exp2_rel_err(fm.exp2_emulated(x, degree), x) <= fm.exp2_bound(degree)
    assert fm.exp2_emulated(-1074.5, degree) == 2.0 ** -1074                        # 2^-1074.5 = 0.707 of the last denormal
    assert fm.exp2_emulated(-1075.0, degree) == 0.0                                 # the tie to even
    assert fm.exp2_emulated(math.nextafter(-1075.0, 0.0), degree) == 2.0 ** -1074   # just above the tie
    assert fm.exp2_emulated(-1080.0, degree) == 0.0
    top = fm.exp2_emulated(1023.999, degree)
    assert math.isfinite(top) and fm.exp2_rel_err(top, 1023.999) <= fm.exp2_bound(degree)
    assert fm.exp2_emulated(1024.0, degree) == math.inf and fm.exp2_emulated(1030.0, degree) == math.inf
    # one rounding into the denormals: 2^-1073.4 is 1.52 denormal units -> 2 of them
    assert fm.exp2_emulated(-1073.4, degree) == 2 * 2.0 ** -1074
    for x, want in fm.crafted_exp2_points():
        if want is not None:
            assert fm.exp2_emulated(x, degree) == want, x


@pytest.mark.parametrize("degree", fm.DEGREES)
def test_a_coefficient_moved_by_an_eighth_of_an_ulp_of_the_result_changes_the_emulated_bits(degree):
    """What the 3.7e-14 bound cannot see and the bit comparison on the device can.  Moving c_k by d moves the polynomial by
    d f^k, at most d 2^-k.  A move of ONE ULP of c_k is visible in the result's bits for c1 .. c3 only: for degree 9 it changes
    3709, 334, 25, 3, 1, 0, 0, 0, 0 of the grid's 20 010 values (k = 1 .. 9, measured with this emulation), because from c5 on
    ulp(c_k) 2^-k is below 2^-74, a millionth of the result's ulp -- no test of the results can see such a literal, the
    comparison of the literals with the fit (above) does.  So: one ulp for c1 .. c3, and for every coefficient the move that
    shifts the polynomial by 2^-56 at f = +-0.5 (an eighth of the result's ulp there; 2^(k-56), never less than one ulp)."""
    _, pts, vals = grid_errors(degree)
    sub = [i for i in range(len(pts)) if abs(pts[i]) >= 0.4][::2] + list(range(len(pts) - 9, len(pts)))
    c = fm.coefficients(degree)
    for k in range(degree):
        for sign in (1.0, -1.0):
            steps = [2.0 ** (k + 1 - 56)]
            if k < 3:
                steps.append(0.0)                       # (0: one ulp)
            for d in steps:
                moved = list(c)
                moved[k] = c[k] + sign * d
                if moved[k] == c[k]:
                    moved[k] = math.nextafter(c[k], sign * math.inf)
                changed = sum(fm.exp2_emulated(pts[i], degree, coef=moved) != vals[i] for i in sub)
                assert changed > 0, (degree, k + 1, sign, d)


def test_div_ulps_hand_cases():
    assert fm.div_ulps(6.0, 3.0, 2.0) == 0.0 and fm.div_ulps(-1.0, 4.0, -0.25) == 0.0 and fm.div_ulps(0.0, 7.0, 0.0) == 0.0
    assert fm.div_ulps(0.0, 7.0, -0.0) == 0.0
    # 1/3 = 0.0101..b: the correctly rounded double is below it by a third of an ulp
    third = 1.0 / 3.0
    assert fm.div_ulps(1.0, 3.0, third) == pytest.approx(1.0 / 3.0, rel=1e-15)
    assert fm.div_ulps(1.0, 3.0, math.nextafter(third, 1.0)) == pytest.approx(2.0 / 3.0, rel=1e-15)
    assert fm.div_ulps(1.0, 3.0, math.nextafter(third, 0.0)) == pytest.approx(4.0 / 3.0, rel=1e-15)
    assert fm.div_ulps(-1.0, 3.0, -third) == pytest.approx(1.0 / 3.0, rel=1e-15)
    # next to a power of two: the quotient 1 - 2^-53 exactly (a = 2^53 - 1, b = 2^53) lies in [0.5, 1), ulp 2^-53 ...
    a, b = 2.0 ** 53 - 1.0, 2.0 ** 53
    assert fm.div_ulps(a, b, 1.0 - 2.0 ** -53) == 0.0
    assert fm.div_ulps(a, b, 1.0) == 1.0                                 # ... so 1.0 is one (small) ulp off
    assert fm.div_ulps(a, b, 1.0 + 2.0 ** -52) == 3.0                    # and the next double up three
    # just above 1 the ulp is 2^-52: (1 + 2^-52) / 1
    assert fm.div_ulps(1.0 + 2.0 ** -52, 1.0, 1.0) == 1.0 and fm.div_ulps(1.0 + 2.0 ** -52, 1.0, 1.0 - 2.0 ** -53) == 1.5
    # a quotient in the denormals is measured in denormal units
    assert fm.div_ulps(2.0 ** -1060, 2.0 ** 10, 2.0 ** -1070) == 0.0 and fm.div_ulps(2.0 ** -1060, 2.0 ** 10, 0.0) == 16.0
    # floats
    t32 = float(np.float32(1.0) / np.float32(3.0))
    assert fm.div_ulps_f32(1.0, 3.0, t32) == pytest.approx(1.0 / 3.0, rel=1e-6)
    assert fm.div_ulps_f32(6.0, 3.0, 2.0) == 0.0
    assert fm.div_ulps_f32(2.0 ** 24 - 1.0, 2.0 ** 24, 1.0) == 1.0
    with pytest.raises(AssertionError):
        fm.div_ulps_f32(1.0, 3.0, third)                                  # not a float32 value


def test_ulp_distance_and_float_ulps():
    a = np.array([1.0, 1.0, 0.0, -0.0, 2.0 ** -1074, math.inf, -1.0])
    b = np.array([1.0, 1.0 + 2.0 ** -52, -0.0, 2.0 ** -1074, -(2.0 ** -1074), 1.7976931348623157e308, -1.0 - 2.0 ** -52])
    assert fm.ulp_distance(a, b).tolist() == [0.0, 1.0, 0.0, 1.0, 2.0, 1.0, 1.0]
    assert fm.ulps32(np.array([1.0 + 2.0 ** -23, 0.5, 2.0 ** -127 + 2.0 ** -149, 2.0]),
                     np.array([1.0, 0.5 + 2.0 ** -24, 2.0 ** -127, 2.0 - 2.0 ** -23])).tolist() == [1.0, 1.0, 1.0, 1.0]
