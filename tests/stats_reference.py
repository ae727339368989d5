"""The ensemble statistics of sipnet_batch_reduce_plane / sipnet_batch_run_stats, exactly: per (row, site) the sum and the
sum of squares over the site's members, each the exact real number rounded ONCE to a double (tests/test_stats_reference.py,
tests/test_gpu_stats_edges.py).  numpy, math.fsum and fractions.Fraction only; numpy.sum is not used (it rounds as it goes).

Exactness.  math.fsum returns the correctly rounded sum of its arguments.  A square is split into terms that are doubles
exactly: Veltkamp's split x = hi + lo (26 bits each) gives x^2 = hi hi + 2 hi lo + lo lo with every product exact as long as
nothing overflows or underflows, which holds for 2^-400 <= |x| <= 2^400 (the lowest bit of lo lo then lies above 2^-906);
a cell with a value outside that range, or whose sums overflow on the way, is summed in fractions.Fraction, whose float()
rounds correctly and raises past the largest double.

Conventions.  A cell with a NaN among its values has NaN in both sums.  Infinities follow IEEE: the sum is +inf, -inf, or
NaN when both signs occur; the sum of squares is +inf.  A finite cell whose exact sum (of squares) rounds past the largest
double has +inf / -inf there -- what a device sum gives too, since its partial sums of squares only grow.

Bounds (stats_bounds): what ANY order of double additions of the n = M values stays within, measured from the EXACT sum.
With u = 2^-53, n - 1 rounded additions in any order (a forward loop, a tree, lanes and a butterfly) satisfy (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2)
    |fl(sum x) - sum x| <= gamma_(n-1) sum |x|,   gamma_k = k u / (1 - k u),
and gamma_(n-1) <= n u whenever n (n - 1) u <= 1, that is for every n < 2^26: the bound on a sum is n 2^-53 sum |x|.
A sum of squares rounds each square once (relative u, or at most 2^-1075 absolutely when it underflows) -- or fuses it into
the addition, one rounding instead of two -- and then adds: every term passes through at most n roundings, so
    |fl(sum x^2) - sum x^2| <= gamma_n sum x^2 + n 2^-1074,   gamma_n <= (n + 1) u  for n (n + 1) u <= 1 (n < 2^26):
(n + 1) 2^-53 sum x^2 + n 2^-1074.  The slack between gamma and the round figure (u sum |x| at least) is far more than the
rounding of the bound's own few operations.  stats_errors measures the distance to the EXACT sum, not to its rounding:
fsum over (-got, the terms) rounds that difference once.  Narrowing of a float plane to doubles is exact, so the same
reference and bounds serve both element types."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
_SAFE_LO, _SAFE_HI = 2.0 ** -400, 2.0 ** 400


def square_terms(v):
    """doubles v, each zero or 2^-400 <= |v| <= 2^400 -> [len(v)][3]: hi hi, 2 hi lo, lo lo, whose exact sum is v^2"""
    v = np.asarray(v, dtype=np.float64)
    c = 134217729.0 * v                                  # 2^27 + 1
    hi = c - (c - v)
    lo = v - hi
    return np.stack([hi * hi, 2.0 * (hi * lo), lo * lo], axis=-1)


def _safe(v):
    a = np.abs(v)
    return bool(np.all((a == 0.0) | ((a >= _SAFE_LO) & (a <= _SAFE_HI))))


def _round(f):
    """the Fraction f rounded to a double; past the largest one: the infinity of its sign"""
    try:
        return float(f)
    except OverflowError:
        return math.inf if f > 0 else -math.inf


def _exact(v):
    """finite doubles -> (sum, sum of squares) as Fractions"""
    fr = [Fraction(float(e)) for e in v]
    return sum(fr, Fraction(0)), sum((f * f for f in fr), Fraction(0))


def _special(v):
    """a cell with a NaN or an infinity -> (sum, sum of squares), else None"""
    if np.isnan(v).any():
        return math.nan, math.nan
    inf = np.isinf(v)
    if inf.any():
        pos, neg = bool((v[inf] > 0).any()), bool((v[inf] < 0).any())
        return (math.nan if pos and neg else math.inf if pos else -math.inf), math.inf
    return None


def cell_stats(v):
    """one cell's values (doubles) -> (sum, sum of squares), each the exact value rounded once"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    sp = _special(v)
    if sp is not None:
        return sp
    if _safe(v):
        try:
            return math.fsum(v.tolist()), math.fsum(square_terms(v).reshape(-1).tolist())
        except OverflowError:                            # (cannot happen below 2^400 with n < 2^26; kept for safety)
            pass
    s1, s2 = _exact(v)
    return _round(s1), _round(s2)


def cell_errors(got1, got2, v):
    """|got1 - sum v| and |got2 - sum v^2| against the EXACT sums, rounded once.  Where the reference is not finite (NaN,
    infinities, overflow): 0 when got equals it as a value (NaN equals NaN), else inf; a got that is not finite where the
    reference is: inf"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    got1, got2 = float(got1), float(got2)
    want = cell_stats(v)
    out = []
    fast = _special(v) is None and _safe(v)
    exact = None
    for k, (g, w) in enumerate(((got1, want[0]), (got2, want[1]))):
        if not math.isfinite(w):
            out.append(0.0 if (g == w or (math.isnan(g) and math.isnan(w))) else math.inf)
        elif not math.isfinite(g):
            out.append(math.inf)
        elif fast:
            terms = v.tolist() if k == 0 else square_terms(v).reshape(-1).tolist()
            out.append(abs(math.fsum([-g] + terms)))
        else:
            if exact is None:
                exact = _exact(v)
            out.append(_round(abs(Fraction(g) - exact[k])))
    return out[0], out[1]


def cell_bounds(v):
    """(n u sum |v|, (n + 1) u sum v^2 + n 2^-1074) for one cell; NaN where the reference is not finite (no bound there:
    the value itself is compared)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    n = v.size
    w1, w2 = cell_stats(v)
    a1, a2 = cell_stats(np.abs(v)) if math.isfinite(w1) or math.isfinite(w2) else (math.nan, math.nan)
    b1 = n * U * a1 if math.isfinite(w1) and math.isfinite(a1) else math.nan
    b2 = (n + 1) * U * a2 + n * TINY if math.isfinite(w2) else math.nan
    return b1, b2


def _cells(x, n_sites, M):
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[1] >= n_sites * M, (x.shape, n_sites, M)
    x = x.astype(np.float64)
    for r in range(x.shape[0]):
        for s in range(n_sites):
            yield r, s, x[r, s * M:(s + 1) * M]


def plane_stats(x, n_sites, M):
    """x [rows][>= n_sites M] -> [rows][n_sites][2]: the exactly rounded sum and sum of squares of every cell"""
    out = np.zeros((np.asarray(x).shape[0], n_sites, 2))
    for r, s, v in _cells(x, n_sites, M):
        out[r, s] = cell_stats(v)
    return out


def stats_bounds(x, n_sites, M):
    """-> [rows][n_sites][2]: what a device sum may differ from the exact one by (cell_bounds)"""
    out = np.zeros((np.asarray(x).shape[0], n_sites, 2))
    for r, s, v in _cells(x, n_sites, M):
        out[r, s] = cell_bounds(v)
    return out


def stats_errors(got, x, n_sites, M):
    """got [rows][n_sites][2] -> [rows][n_sites][2]: its distance from the exact sums (cell_errors)"""
    got = np.asarray(got, dtype=np.float64)
    out = np.zeros((np.asarray(x).shape[0], n_sites, 2))
    assert got.shape == out.shape, (got.shape, out.shape)
    for r, s, v in _cells(x, n_sites, M):
        out[r, s] = cell_errors(got[r, s, 0], got[r, s, 1], v)
    return out


def ratios(got, x, n_sites, M, bounds=None):
    """-> [rows][n_sites][2]: stats_errors / stats_bounds; where the reference is not finite 0 for the same value and inf
    otherwise; 0 / 0 = 0 (a cell of zeros must give zeros).  Inside the bounds: every entry <= 1.  bounds: stats_bounds(x,
    n_sites, M) where the caller has them already"""
    err, bnd = stats_errors(got, x, n_sites, M), stats_bounds(x, n_sites, M) if bounds is None else bounds
    out = np.zeros_like(err)
    for i in np.ndindex(err.shape):
        e, b = err[i], bnd[i]
        out[i] = e if (math.isnan(b) or e == 0.0) else math.inf if b == 0.0 else e / b
    return out
