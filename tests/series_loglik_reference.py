"""The numpy reference of sipnet_batch_series_loglik and of sipnet_batch_pf_resample_sites' additions, for
tests/test_series_loglik.py (which pins it by hand-computed cases) and tests/test_gpu_series_loglik.py (which holds the
kernels to it).  The term rules are evaluated in np.longdouble, straight from the header's expressions (a division by sd,
the constants unfused), on the modelled value h that the contract defines as a double (the rows added in ascending order
from 0.0, times scale: formed in fp64 here too, as oracle/pf_oracle.log_weights forms its sum); the effective sample size is an exact rational of Python integers; the keep / reset rule sits on
top of tests/test_pf_sites.py's sites_reference."""
import collections
from fractions import Fraction

import numpy as np

from tests.test_pf_sites import sites_reference

GAUSS, LAPLACE = 0, 1
TILE_ROWS = 256

# one term: series [rows * sum_steps][ld] (any float dtype), obs and sd [n_sites][rows]
Term = collections.namedtuple("Term", "series obs sd kind scale sum_steps", defaults=(GAUSS, 1.0, 1))

Loglik = collections.namedtuple("Loglik", "loglik parts abs_sum used info")


def series_loglik(terms, n_sites, status, normalise=True, add=None):
    """-> Loglik(loglik [ncol] longdouble, parts [n_terms][ncol] longdouble, abs_sum [ncol] longdouble = the sum of |row
    terms| per member, used [n_sites][n_terms] int32, info [n_sites][2] int32 = {code, rows used}).  The
    columns are the first ncol = len(status) of every series."""
    L = np.longdouble
    status = np.asarray(status)
    ncol = len(status)
    M = ncol // n_sites
    parts = np.zeros((len(terms), ncol), dtype=L)
    abs_sum = np.zeros(ncol, dtype=L)
    used = np.zeros((n_sites, len(terms)), dtype=np.int32)
    bad = np.zeros(n_sites, dtype=bool)
    for q, t in enumerate(terms):
        obs = np.asarray(t.obs, dtype=np.float64).reshape(n_sites, -1)
        sd = np.asarray(t.sd, dtype=np.float64).reshape(n_sites, -1)
        rows = obs.shape[1]
        # h is the contract's own double: the sum_steps rows added in ascending order from 0.0, times scale, in fp64 (what
        # the filter's oracle/pf_oracle.log_weights does); the term rules on top of it are evaluated in longdouble
        x = np.asarray(t.series)[:rows * t.sum_steps, :ncol].astype(np.float64).reshape(rows, t.sum_steps, ncol)
        acc = np.zeros((rows, ncol))
        for k in range(t.sum_steps):
            acc += x[:, k, :]
        h = (np.float64(t.scale) * acc).astype(L)
        for s in range(n_sites):
            cols = slice(s * M, (s + 1) * M)
            for r in range(rows):
                y = obs[s, r]
                if np.isnan(y):
                    continue
                b = sd[s, r]
                if not np.isfinite(y) or not (np.isfinite(b) and b > 0):
                    bad[s] = True
                    continue
                used[s, q] += 1
                d = h[r, cols] - L(y)
                if t.kind == GAUSS:
                    term = L(-0.5) * (d / L(b)) ** 2
                    const = -(np.log(L(b)) + L(0.5) * np.log(L(8) * np.arctan(L(1)))) if normalise else L(0)
                else:
                    term = -np.abs(d) / L(b)
                    const = -np.log(L(2) * L(b)) if normalise else L(0)
                parts[q, cols] += term + const
                abs_sum[cols] += np.abs(term + const)
    total = parts.sum(axis=0)
    if add is not None:
        total = total + np.asarray(add).astype(L)
    dead = status != 0
    total[dead] = -np.inf
    parts[:, dead] = -np.inf
    info = np.zeros((n_sites, 2), dtype=np.int32)
    for s in range(n_sites):
        n = int(used[s].sum())
        info[s] = (-2 if bad[s] else 1 if n > 0 else -1, n)
        if bad[s]:
            total[s * M:(s + 1) * M] = np.nan
            parts[:, s * M:(s + 1) * M] = np.nan
    return Loglik(total, parts, abs_sum, used, info)


def ess_exact(w):
    """the effective sample size S^2 / sum w^2 of integer weights as an exact Fraction (0 when S = 0)"""
    w = [int(x) for x in w]
    S = sum(w)
    return Fraction(S * S, sum(x * x for x in w)) if S > 0 else Fraction(0)


def resample_reference(logw, n_sites, u0, fixed, beta=None, ess_min=None):
    """sipnet_batch_pf_resample_sites given the device's integer weights `fixed`: -> (ancestors [ncol], totals [n_sites],
    ess [n_sites] as Fractions, logw afterwards).  Totals: S, 0, -3 kept.  (Bad arguments, -2, are the caller's to mark.)"""
    logw = np.array(logw, dtype=np.float64)
    M = len(logw) // n_sites
    _, anc, tot = sites_reference(logw, n_sites, u0, fixed=fixed)
    ess = [ess_exact(fixed[s * M:(s + 1) * M]) for s in range(n_sites)]
    if ess_min is not None:
        for s in range(n_sites):
            sl = slice(s * M, (s + 1) * M)
            if tot[s] > 0 and float(ess[s]) >= float(ess_min[s]):   # (the tests keep ess_min away from a tie)
                tot[s] = -3
                anc[sl] = np.arange(s * M, (s + 1) * M)
            elif tot[s] > 0:
                logw[sl] = 0.0
    return anc, tot, ess, logw
