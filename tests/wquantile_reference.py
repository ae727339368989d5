"""The weighted order statistics of sipnet_batch_plane_quantiles_weighted, written plainly (include/sipnet_amd.h;
tests/test_wquantiles.py pins this file; tests/test_gpu_wquantiles.py and tests/test_gpu_wquantiles_edges.py hold the kernels
to it through tests/wquantile_gpu_common.py).  numpy only.  At its end: the inputs of the edge tests' special-value and
observation rows, which the CPU pins and the GPU tests share.

Everything here takes GIVEN integer weights w (int64, 0: the member is not in the sample): the sample of a cell is the values
with w > 0, n their number, S = sum w.  Quantile q: sort by value, cumulative weights C in int64, T = max(1, ceil(q S)) with
the product rounded once in float64, Q = the first sorted value whose C >= T (np.searchsorted on integers).  rank = {sum of w
over x < y, sum of w over x == y}.  The moments and the CRPS are the definitions in np.longdouble: mean = sum p x, m2 =
sum p (x - mean)^2, crps = sum p |x - y| - (1/2) sum sum p_i p_j |x_i - x_j|, p = w / S.  weights_of gives the integers a site's
log-weights stand for, from tests/pf_edges_reference.py's exponential of higher precision (the device may differ by one unit
where the exact value is next to a half: the GPU tests take the device's integers and check them against these)."""
import numpy as np

from tests import pf_edges_reference as er

U = 2.0 ** -53


def target(S, q):
    """T of the contract: max(1, (int64) ceil(q * (double) S)), one rounded product"""
    return max(1, int(np.ceil(np.float64(q) * np.float64(S))))


def site_code(logw, used=None):
    """0 analysed (S is looked at by the caller), -2: a +inf log-weight among the used members"""
    lw = np.asarray(logw, dtype=np.float64)
    if used is not None:
        lw = lw[np.asarray(used, dtype=bool)]
    return -2 if np.isposinf(lw).any() else 0


def weights_of(logw, used=None):
    """the integers of ONE site's log-weights: rint(2^30 e^(lw - m)), m the maximum of the used members' log-weights that are
    not NaN; 0 for a member that is not used, for NaN and -inf, and for everybody when a used log-weight is +inf
    -> (w int64 [M], d, tol): where d > tol the device's integer must be w, else it may be the neighbour"""
    lw = np.asarray(logw, dtype=np.float64)
    use = np.ones(lw.size, bool) if used is None else np.asarray(used, dtype=bool)
    ok = use & ~np.isnan(lw)
    zero = np.zeros(lw.size, np.int64), np.full(lw.size, np.inf), np.zeros(lw.size)
    if not ok.any() or site_code(lw, use) == -2:
        return zero
    m = lw[ok].max()
    if np.isneginf(m):
        return zero
    w, d, tol = er.fixed_weight_exact(np.where(ok, lw, -np.inf), m)
    return w, d, tol


def quantiles(x, w, q):
    """the weighted quantiles of the sample (x, w > 0; no NaN among its values; may be empty) -> float64 [n_q]"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.int64)
    keep = w > 0
    x, w = x[keep], w[keep]
    out = np.full(q.size, np.nan)
    if x.size == 0:
        return out
    order = np.argsort(x, kind="stable")
    xs, C = x[order], np.cumsum(w[order], dtype=np.int64)
    for i in range(q.size):
        out[i] = xs[np.searchsorted(C, target(int(C[-1]), q[i]), side="left")]
    return out


def moments(x, w):
    """(mean, centred second moment) of the sample in np.longdouble"""
    L = np.longdouble
    keep = np.asarray(w) > 0
    xl, wl = np.asarray(x, dtype=np.float64)[keep].astype(L), np.asarray(w, dtype=np.int64)[keep].astype(L)
    S = wl.sum()
    mean = (wl * xl).sum() / S
    return mean, (wl * (xl - mean) ** 2).sum() / S


def moments_bounds(x, w):
    """what a fixed-order double evaluation of the contract's two expressions stays within, p = w / S:
        mean: (n + 16) 2^-53 sum p |x|                 (a rounded product and at most n - 1 additions a term, one division)
        m2:   (n + 16) 2^-53 sum p (x - mean)^2 + 2 (the mean's bound)^2
    The second: with the computed mean off by e, sum p (x - mean - e)^2 = m2 + e^2 exactly (the cross term is sum p (x - mean)
    = 0), and each term carries four roundings (the difference, its square, the product with w) before the n - 1 additions."""
    L = np.longdouble
    keep = np.asarray(w) > 0
    xl, wl = np.asarray(x, dtype=np.float64)[keep].astype(L), np.asarray(w, dtype=np.int64)[keep].astype(L)
    n, p = xl.size, wl / wl.sum()
    mean, m2 = moments(x, w)
    b_mean = (n + 16) * U * float((p * np.abs(xl)).sum())
    return b_mean, (n + 16) * U * float(m2) + 2.0 * b_mean * b_mean


def crps_pairwise(x, w, y):
    """sum p |x - y| - (1/2) sum sum p_i p_j |x_i - x_j| in np.longdouble"""
    L = np.longdouble
    keep = np.asarray(w) > 0
    xl, wl = np.asarray(x, dtype=np.float64)[keep].astype(L), np.asarray(w, dtype=np.int64)[keep].astype(L)
    S = wl.sum()
    pair = L(0.0)
    for i0 in range(0, xl.size, 256):                    # (blocks of rows: n^2 longdoubles need not exist at once)
        pair += (wl[i0:i0 + 256, None] * wl[None, :] * np.abs(xl[i0:i0 + 256, None] - xl[None, :])).sum()
    return (wl * np.abs(xl - L(y))).sum() / S - pair / (2 * S * S)


def crps_bound(x, w, y):
    """4 (n + 2) 2^-53 sum p |x - y|: the unweighted bound with the mean weighted.  Both sums of the sorted form have terms
    of at most p |d| (the coefficient (C_(i-1) + C_i - S) / S lies in [-1, 1]); a term carries at most three roundings (d, the
    coefficient's product, the product with d), a sum n - 1 additions, the two quotients three more: (2 n + 6) 2^-53 sum p |d|
    to first order, under the 4 (n + 2) the unweighted call is held to."""
    L = np.longdouble
    keep = np.asarray(w) > 0
    xl, wl = np.asarray(x, dtype=np.float64)[keep].astype(L), np.asarray(w, dtype=np.int64)[keep].astype(L)
    return 4.0 * (xl.size + 2) * U * float((wl * np.abs(xl - L(y))).sum() / wl.sum())


def cell(x, w, q, y=None, code=0):
    """one cell: values x, integer weights w, the quantiles q, the observation y (None: no scores), the site's code
    -> (quant [n_q], rank (2,) int64 or None, nan: every floating-point output of the cell is NaN)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.int64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    nan = np.full(q.size, np.nan)
    two = lambda v: None if y is None else np.array([v, v], np.int64)
    if code == -2:
        return nan, two(-2), True
    if w.sum() == 0:
        return nan, two(0), True
    if y is not None and np.isinf(y):
        return nan, two(-2), True
    if np.isnan(x[w > 0]).any():
        return nan, two(-1), True
    quant = quantiles(x, w, q)
    if y is None:
        return quant, None, False
    if np.isnan(y):
        return quant, two(-1), False
    return quant, np.array([w[(x < y) & (w > 0)].sum(), w[(x == y) & (w > 0)].sum()], np.int64), False


# ---- the inputs of the edge tests (tests/test_gpu_wquantiles_edges.py; pinned without a device in tests/test_wquantiles.py) --
TINY = 2.0 ** -1074                                                      # the spacing of the denormal doubles
SPECIAL_ROWS = ("zeros", "zeros among others", "infinities", "denormals", "float denormals", "large mean", "large magnitude",
                "equal values", "nan")
DENORMAL_ROWS = (3, 4)
OBS_KINDS = ("below", "above", "tied", "ties weight 0 only", "+0 against -0", "nan", "+inf", "-inf", "inside", "inside, mean 1e6")


def denormal_allowance(n):
    """what the two denormal rows add to the mean's and the CRPS's bounds: the relative bounds count roundings of 2^-53 of
    the result, but a result (or a partial sum) below 2^-1022 is rounded to a multiple of 2^-1074 instead: half a spacing for
    each of the at most 2 n + 6 roundings of a sum of n terms and its quotients -- (2 n + 8) 2^-1074 with the margin"""
    return (2 * n + 8) * TINY


def special_rows(rng, n_sites, M, f32, weighs):
    """the rows of SPECIAL_ROWS over n_sites x M members, weighs [n_sites M] bool: the members that will weigh something (every
    site needs two) -> (x [9][n_sites M] as the device reads it through the element type, y [9][n_sites])"""
    n = n_sites * M
    first = [np.flatnonzero(weighs[s * M:(s + 1) * M])[:2] + s * M for s in range(n_sites)]
    nobody = [np.flatnonzero(~weighs[s * M:(s + 1) * M])[:1] + s * M for s in range(n_sites)]
    x = np.zeros((len(SPECIAL_ROWS), n))
    y = np.zeros((len(SPECIAL_ROWS), n_sites))
    x[0] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    x[1] = np.round(rng.normal(size=n) * 2.0)
    x[1, ::5], x[1, 1::5] = -0.0, 0.0
    x[2] = rng.normal(size=n)
    x[2, rng.random(n) < 0.02] = np.inf                                  # (site 0 has both for sure, and both with weight)
    x[2, rng.random(n) < 0.02] = -np.inf
    x[2, first[0]] = [np.inf, -np.inf]
    for s in range(1, n_sites):                                          # the last site: infinities under weight 0 only;
        inf_here = np.flatnonzero(np.isinf(x[2, s * M:(s + 1) * M])) + s * M                   # those between: only +inf under weight
        if s == n_sites - 1:
            x[2, inf_here[weighs[inf_here]]] = 0.5
            x[2, nobody[s]] = -np.inf
        else:
            x[2, inf_here[weighs[inf_here] & (x[2, inf_here] < 0)]] = 0.5
            x[2, first[s][0]] = np.inf
    x[3] = rng.integers(1, 2 ** 39, n) * 5e-324
    x[4] = rng.integers(1, 2 ** 22, n) * 2.0 ** -149
    x[5] = 1e8 + 1e-3 * rng.normal(size=n)
    x[6] = (1e30 if f32 else 1e140) * rng.normal(size=n)                 # (1e140 is no float)
    x[7] = 0.1
    x[8] = rng.normal(size=n)
    x[8, first[1][0]] = np.nan                                           # under weight, in site 1 only
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    for r in (3, 4, 7):
        y[r] = [x[r, first[s][1]] for s in range(n_sites)]               # a member's value
    y[2], y[5], y[8] = 0.3, 1e8, 0.1
    return x, y


def score_rows(rng, M, weighs):
    """ONE site's rows of OBS_KINDS: weighs [M] bool, the members that will weigh something (at least one; the rows that need
    a member without weight are plain rows when there is none) -> (x [10][M], y [10])"""
    pos, zero = np.flatnonzero(weighs), np.flatnonzero(~weighs)
    x = np.round(rng.normal(size=(len(OBS_KINDS), M)) * 2.0, 1)
    y = np.zeros(len(OBS_KINDS))
    x[9] = 1e6 + rng.normal(size=M)
    if zero.size:
        x[0, zero[0]] = x[0, pos].min() - 5.0                            # below y, and weighs nothing
        x[1, zero[0]] = x[1, pos].max() + 5.0
        x[3, zero[0]] = 7.25                                             # (no multiple of 0.1: nobody else has it)
    y[0], y[1] = x[0, pos].min() - 1.0, x[1, pos].max() + 1.0
    y[2] = x[2, pos[0]]
    y[3] = 7.25
    x[4, pos[0]] = -0.0
    x[4, pos[-1]] = -0.0
    y[4] = 0.0
    y[5], y[6], y[7] = np.nan, np.inf, -np.inf
    y[8] = float(np.median(x[8, pos])) + 0.013
    y[9] = 1e6 + 0.1
    return x, y


def plane(series, n_sites, M, w, q, obs=None, codes=None):
    """every cell of series [rows][>= n_sites M] (any float dtype; widened) under the integers w [n_sites M]; codes
    [n_sites] or None (-2 where a used log-weight was +inf) -> (quant [n_q][rows][n_sites], site [n_sites][3] int64 =
    {S, n, code}, rank [rows][n_sites][2] int64 or None, nan [rows][n_sites] bool)"""
    series = np.asarray(series)
    w = np.asarray(w, dtype=np.int64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    rows = series.shape[0]
    quant = np.zeros((q.size, rows, n_sites))
    site = np.zeros((n_sites, 3), np.int64)
    rank = np.zeros((rows, n_sites, 2), np.int64) if obs is not None else None
    nan = np.zeros((rows, n_sites), bool)
    for s in range(n_sites):
        ws = w[s * M:(s + 1) * M]
        code = -2 if codes is not None and codes[s] == -2 else 0
        if code == -2:
            ws = np.zeros(M, np.int64)
        S = int(ws.sum())
        site[s] = [S, int((ws > 0).sum()), code if code else (1 if S == 0 else 0)]
        for r in range(rows):
            x = series[r, s * M:(s + 1) * M].astype(np.float64)
            got = cell(x, ws, q, None if obs is None else float(obs[r, s]), code)
            quant[:, r, s], nan[r, s] = got[0], got[2]
            if obs is not None:
                rank[r, s] = got[1]
    return quant, site, rank, nan
