"""The order statistics of sipnet_batch_plane_quantiles, written plainly (include/sipnet_amd.h; tests/test_quantiles.py,
tests/test_gpu_quantiles.py).  numpy only.

A cell's sample x is a site's used members of one row, as doubles.  Quantiles: Hyndman & Fan's type 7 from np.sort, h =
(n - 1) q, lo = floor(h), g = h - lo, Q = x[lo] when g == 0, else x[lo] + g (x[lo + 1] - x[lo]) with every operation rounded once
(numpy scalars do not fuse).  Against an observation y: rank = {#(x < y), #(x == y)} and the CRPS in the centred sorted form
(1/n) sum |d_i| - (1/n^2) sum (2 i - n - 1) d_(i), d = x - y, i = 1 .. n.  crps_pairwise is the energy form in np.longdouble."""
import numpy as np


def positions(n, q):
    """-> (lo int32 [n_q], g float64 [n_q]) of the quantiles q of n >= 1 sorted values"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    h = np.float64(n - 1) * q
    lo = np.floor(h)
    return lo.astype(np.int32), h - lo


def quantiles(x, q):
    """the type-7 quantiles of the sample x (no NaN in it; may be empty) -> float64 [n_q]"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    xs = np.sort(np.asarray(x, dtype=np.float64))
    out = np.full(q.size, np.nan)
    if xs.size == 0:
        return out
    lo, g = positions(xs.size, q)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q.size):
            if g[i] == 0.0:
                out[i] = xs[lo[i]]
            else:
                d = xs[lo[i] + 1] - xs[lo[i]]
                t = g[i] * d
                out[i] = xs[lo[i]] + t
    return out


def crps_centred(x, y):
    """(1/n) sum |d_i| - (1/n^2) sum (2 i - n - 1) d_(i) in doubles, one addition after the other"""
    d = np.sort(np.asarray(x, dtype=np.float64)) - np.float64(y)
    n = d.size
    coef = (2.0 * np.arange(1, n + 1) - n - 1.0)
    s1, s2 = np.cumsum(np.abs(d))[-1], np.cumsum(coef * d)[-1]      # (cumsum: in order from the first term)
    return s1 / np.float64(n) - s2 / (np.float64(n) * np.float64(n))


def crps_pairwise(x, y):
    """(1/n) sum |x - y| - (1/2n^2) sum sum |x_i - x_j| in np.longdouble"""
    xl = np.asarray(x, dtype=np.float64).astype(np.longdouble)
    n = xl.size
    pair = np.longdouble(0.0)
    for i0 in range(0, n, 256):                          # (blocks of rows: n^2 longdoubles need not exist at once)
        pair += np.abs(xl[i0:i0 + 256, None] - xl[None, :]).sum()
    return np.abs(xl - np.longdouble(y)).sum() / n - pair / (2 * np.longdouble(n) * n)


def crps_bound(x, y):
    """what any fixed-order double summation of the centred form's terms stays within: 4 (n + 2) 2^-53 mean |x - y|"""
    x = np.asarray(x, dtype=np.float64)
    return 4.0 * (x.size + 2) * 2.0 ** -53 * float(np.abs(x.astype(np.longdouble) - np.longdouble(y)).mean())


def cell(x, q, y=None):
    """one cell: the used values x, the quantiles q, the observation y (None: no scores)
    -> (quant [n_q], n, crps, rank (2,)); crps and rank None without y"""
    x = np.asarray(x, dtype=np.float64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    n = x.size
    nan = np.full(q.size, np.nan)
    if y is not None and np.isinf(y):                    # a bad argument for the cell
        return nan, n, np.nan, np.array([-2, -2], np.int32)
    if np.isnan(x).any():
        return nan, n, (None if y is None else np.nan), (None if y is None else np.array([-1, -1], np.int32))
    quant = quantiles(x, q)
    if y is None:
        return quant, n, None, None
    if np.isnan(y):
        return quant, n, np.nan, np.array([-1, -1], np.int32)
    rank = np.array([(x < y).sum(), (x == y).sum()], np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        crps = crps_centred(x, y) if n else np.nan
    return quant, n, crps, rank


def plane(series, n_sites, M, q, used=None, obs=None):
    """every cell of series [rows][>= n_sites M] (any float dtype; widened): used [n_sites M] bool or None = all members,
    obs [rows][n_sites] or None -> (quant [n_q][rows][n_sites], count [rows][n_sites] int32, crps [rows][n_sites] or None,
    rank [rows][n_sites][2] int32 or None)"""
    series = np.asarray(series)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    rows = series.shape[0]
    quant = np.zeros((q.size, rows, n_sites))
    count = np.zeros((rows, n_sites), np.int32)
    crps = np.zeros((rows, n_sites)) if obs is not None else None
    rank = np.zeros((rows, n_sites, 2), np.int32) if obs is not None else None
    for r in range(rows):
        for s in range(n_sites):
            x = series[r, s * M:(s + 1) * M].astype(np.float64)
            if used is not None:
                x = x[np.asarray(used[s * M:(s + 1) * M], dtype=bool)]
            got = cell(x, q, None if obs is None else float(obs[r, s]))
            quant[:, r, s], count[r, s] = got[0], got[1]
            if obs is not None:
                crps[r, s], rank[r, s] = got[2], got[3]
    return quant, count, crps, rank
