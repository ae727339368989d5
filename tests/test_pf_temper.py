"""tests/pf_temper_reference.py pinned on the CPU: the search of sipnet_batch_pf_temper_sites over a longdouble ESS of real
weights.  The bracket it returns contains the root that 200 plain bisections find, is as narrow as sixteen sections in eight
rounds make it, every code has its conditions, and the candidates are exactly the stated double expressions."""
from fractions import Fraction

import numpy as np
import pytest

from tests import pf_temper_reference as tr

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit significand on this machine")


def chi2_loglik(M, scale, seed):
    """-0.5 chi^2-like log-likelihoods: the root of ESS(d) = M / 2 sits near 1 / scale^2 .. 1 / scale"""
    rng = np.random.default_rng(seed)
    ll = -0.5 * scale * rng.chisquare(3, M)
    ll[::17] = -np.inf
    ll[5::29] = np.nan
    return ll


def bisect(ess, delta_max, target, n=200):
    """-> (a, b): ESS(a) >= target > ESS(b) after n plain bisections of [0, delta_max]"""
    a, b = 0.0, float(delta_max)
    for _ in range(n):
        mid = 0.5 * (a + b)
        if mid == a or mid == b:
            break
        if ess(np.array([mid]))[0] >= target:
            a = mid
        else:
            b = mid
    return a, b


@pytest.mark.parametrize("delta_max", [1.0, 0.25, 2.0 ** -40])
@pytest.mark.parametrize("scale", [1.0, 30.0, 3000.0])
@pytest.mark.parametrize("M", [255, 1000])
def test_the_bracket_contains_the_root_and_is_narrow(M, scale, delta_max):
    ll = chi2_loglik(M, scale, seed=M)
    ess = tr.ess_real_of(ll)
    live = float(np.isfinite(ll).sum())
    target = 0.5 * live
    trace = []
    code, lo, hi, e = tr.search(ess, delta_max, target, trace)
    e_max = ess(np.array([delta_max]))[0]
    if e_max >= target:
        assert (code, lo, hi, e) == (tr.END, delta_max, delta_max, e_max) and not trace
        return
    assert code == tr.FOUND and len(trace) == tr.ROUNDS
    assert 0.0 <= lo < hi <= delta_max
    assert e == ess(np.array([lo]))[0] >= target > ess(np.array([hi]))[0]
    assert hi - lo <= delta_max * 16.0 ** -8 * (1 + 2.0 ** -40)
    a, b = bisect(ess, delta_max, target)           # (ESS falls with d: one root)
    assert lo <= b and a <= hi, (lo, hi, a, b)


def test_the_codes_and_their_conditions():
    ll = chi2_loglik(300, 30.0, seed=2)
    ess = tr.ess_real_of(ll)
    live = float(np.isfinite(ll).sum())
    assert ess(np.array([0.0]))[0] == live
    assert tr.search(ess, 1.0, np.nextafter(live, np.inf)) == (tr.UNREACHABLE, 0.0, 0.0, live)
    assert tr.search(ess, 1.0, live)[0] == tr.FOUND
    e_max = ess(np.array([1.0]))[0]
    assert tr.search(ess, 1.0, e_max) == (tr.END, 1.0, 1.0, e_max)
    assert tr.search(ess, 1.0, np.nextafter(e_max, np.inf))[0] == tr.FOUND
    dead = tr.ess_real_of(np.full(40, -np.inf))
    assert tr.search(dead, 1.0, 3.0) == (tr.NO_WEIGHT, 0.0, 0.0, 0.0)
    for dm, tg in ((0.0, 3.0), (-1.0, 3.0), (np.inf, 3.0), (np.nan, 3.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.nan)):
        assert tr.search(ess, dm, tg) == (tr.BAD_INPUT, 0.0, 0.0, 0.0), (dm, tg)
    assert tr.search(ess, 1.0, np.inf)[0] == tr.UNREACHABLE


def test_with_carried_weights_the_search_runs_over_their_sum():
    ll = chi2_loglik(500, 30.0, seed=3)
    base = 0.01 * np.where(np.isfinite(ll), ll, 0.0)
    ess = tr.ess_real_of(ll, base)
    e0 = ess(np.array([0.0]))[0]
    assert e0 < float(np.isfinite(ll).sum())           # (the carried weights alone are uneven already)
    code, lo, hi, e = tr.search(ess, 0.99, 0.5 * e0)
    assert code == tr.FOUND and e >= 0.5 * e0 > ess(np.array([hi]))[0]
    a, b = bisect(ess, 0.99, 0.5 * e0)
    assert lo <= b and a <= hi


def rounded(x):
    """the double nearest a rational (ties to even)"""
    return float(x)


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (0.0, 0.25), (0.0, 2.0 ** -40), (0.1, 0.7), (1.0 / 3.0, 1.0 / 3.0 + 2.0 ** -30),
                                   (0.3, np.nextafter(0.3, 1.0)), (0.3, 0.3), (5e-324, 1.5e-323)])
def test_the_candidates_are_the_stated_double_expressions(lo, hi):
    b = tr.candidates(lo, hi)
    assert b.dtype == np.float64 and len(b) == tr.SECTIONS - 1
    width = rounded(Fraction(hi) - Fraction(lo))                      # each operation rounded on its own ...
    for i in range(1, tr.SECTIONS):
        prod = rounded(Fraction(width) * Fraction(i, 16))
        want = rounded(Fraction(lo) + Fraction(prod))
        assert b[i - 1] == want and b[i - 1] == lo + (hi - lo) * (i * 0.0625), (lo, hi, i)
    assert (np.diff(b) >= 0).all() and lo <= b[0] and b[-1] <= hi
    if (lo, hi) == (0.0, 1.0):                                        # ... which a fused multiply-add would not be
        assert list(b) == [i / 16.0 for i in range(1, 16)]
