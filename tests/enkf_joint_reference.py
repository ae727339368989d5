"""The numpy reference of sipnet_batch_enkf_analysis_joint (include/sipnet_amd.h): the per-site serial square-root filter of
tests/enkf_reference.py over a longer variable list -- the analysed pools, then the analysed parameters (converted rows of
the member's own column), then the predicted observations -- in member space, as the contract states it.
tests/test_enkf_joint.py pins it against the textbook augmented Kalman update; tests/test_gpu_enkf_joint.py holds the
kernels to it."""
import numpy as np

from tests import enkf_reference as er

N_POOLS = er.N_POOLS
PSN_TMIN, PSN_TOPT, PSN_TMAX = 7, 8, 9                        # include/sipnet_params.def
LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC, COARSE_ALLOC = 37, 45, 46, 47
RATE_ROWS = (17, 19, 26, 38, 41, 48, 49, 50, 51)             # converted = file value / 365.0
DERIVED_ROWS = (PSN_TMAX, COARSE_ALLOC)
INIT_ROWS = (0, 1, 2, 3, 28, 29, 60, 61, 62, 63)
PHENOLOGY_ROWS = (14, 15, 16, 54)
CLAMPED_ROWS = (74, 75)


def converted_bounds(params):
    """params: (row, lo, hi) in FILE units -> (rows, lo, hi) in converted units, by the conversion's own expression"""
    rows = [int(p[0]) for p in params]
    lo = np.array([p[1] / 365.0 if p[0] in RATE_ROWS else float(p[1]) for p in params], dtype=np.float64)
    hi = np.array([p[2] / 365.0 if p[0] in RATE_ROWS else float(p[2]) for p in params], dtype=np.float64)
    return rows, lo, hi


def eakf(X, P, H, y, sd, inflation=1.0, param_inflation=1.0):
    """X [n][nA] analysed pools, P [n][nP] analysed parameters, H [n][n_obs] predicted observations -> (X, P) after the serial
    update (no limits).  Pools and H are inflated by `inflation`, the parameters by `param_inflation`; a class at 1 is left
    as it is.  Every column is updated by itself, so X does not depend on P being there."""
    X = np.array(X, dtype=np.float64)
    P = np.array(P, dtype=np.float64).reshape(X.shape[0], -1)
    H = np.array(H, dtype=np.float64)
    n = X.shape[0]
    if inflation != 1.0:
        X = X.mean(0) + inflation * (X - X.mean(0))
        H = H.mean(0) + inflation * (H - H.mean(0))
    if param_inflation != 1.0 and P.shape[1]:
        P = P.mean(0) + param_inflation * (P - P.mean(0))
    for i in range(H.shape[1]):
        if np.isnan(y[i]):
            continue
        h = H[:, i].copy()
        hbar = h.mean()
        dh = h - hbar
        var_h = (dh * dh).sum() / (n - 1)
        R = sd[i] ** 2
        alpha = 1.0 / (1.0 + np.sqrt(R / (var_h + R)))
        for M in (X, P, H[:, i + 1:]):
            if M.shape[1] == 0:
                continue
            cov = ((M - M.mean(0)) * dh[:, None]).sum(0) / (n - 1)
            K = cov / (var_h + R)
            M += K * (y[i] - hbar) - alpha * K * dh[:, None]
    return X, P


def limits(fc_pools, X, analysed, fc_prm, P, rows, lo, hi):
    """forecast pools [n][13] and parameters [n][80], the updated analysed pools X and parameters P (rows `rows`, bounds
    lo / hi in converted units) -> (pools written, parameters written, kept mask): the pools' limits of enkf_reference; the
    parameters clipped into their bounds; a member keeps its forecast, pools and parameters, when a value is not finite,
    the biomass rule fails, or an allocation is analysed and the result fails ensureAllocation's test; the derived rows
    that depend on analysed ones rewritten by the conversion's own expressions"""
    pools, kept = er.limits(fc_pools, X, analysed)
    fc_prm = np.array(fc_prm, dtype=np.float64)
    prm = fc_prm.copy()
    P = np.array(P, dtype=np.float64).reshape(prm.shape[0], -1)
    if P.shape[1]:
        P = np.where(P < lo, lo, np.where(P > hi, hi, P))
        prm[:, rows] = P
        kept = kept | ~np.isfinite(P).all(1)
    alloc = any(r in rows for r in (LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC))
    with np.errstate(invalid="ignore"):
        if alloc:
            leaf, wood, fine = prm[:, LEAF_ALLOC], prm[:, WOOD_ALLOC], prm[:, FINE_ALLOC]
            kept = kept | (leaf >= 1.0) | (wood >= 1.0) | (fine >= 1.0) | (1 - leaf - wood - fine < 0)
            prm[:, COARSE_ALLOC] = 1 - leaf - wood - fine
        if PSN_TOPT in rows or PSN_TMIN in rows:
            prm[:, PSN_TMAX] = prm[:, PSN_TOPT] + (prm[:, PSN_TOPT] - prm[:, PSN_TMIN])
    pools[kept] = fc_pools[kept]
    prm[kept] = fc_prm[kept]
    return pools, prm, kept


def site_code(obs, sd, lam, param_lam, n_live):
    """enkf_reference.site_code, with the parameters' lambda checked like the other"""
    code, used = er.site_code(obs, sd, lam, n_live)
    if not (np.isfinite(param_lam) and param_lam >= 1.0):
        return -2, 0
    return code, used


def analysis(state, status, site_ok, n_sites, ops, analysed, params, obs, sd, inflation=None, param_inflation=None,
             planes=None, prm=None, raw=None):
    """the whole call: the arguments of enkf_reference.analysis, and params: (row, lo, hi) in FILE units, param_inflation
    [n_sites] or None -> (state after, parameters after [ncol][80], info [n_sites][4]).  raw: a dict that gets, per code-1
    site, (live columns, X, P before the limits, kept mask) -- what a test measures its distance from a threshold with"""
    state = np.array(state, dtype=np.float64)
    prm = np.array(prm, dtype=np.float64)
    rows, lo, hi = converted_bounds(params)
    M = state.shape[0] // n_sites
    out, prm_out = state.copy(), prm.copy()
    info = np.zeros((n_sites, 4), dtype=np.int32)
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[(status[cols] == 0) & bool(site_ok[s])]
        lam = 1.0 if inflation is None else float(inflation[s])
        plam = 1.0 if param_inflation is None else float(param_inflation[s])
        y, e = np.asarray(obs[s], dtype=np.float64), np.asarray(sd[s], dtype=np.float64)
        code, used = site_code(y, e, lam, plam, len(live))
        info[s] = (code, used, len(live), 0)
        if code != 1:
            continue
        fc = state[live, :N_POOLS]
        H = np.stack([er.predicted(op, fc, None if planes is None else [None if p is None else p[:, live] for p in planes],
                                   lambda k: prm[live, k]) for op in ops], 1)
        X, P = eakf(fc[:, analysed], prm[live][:, rows], H, y, e, lam, plam)
        pools, rows_out, kept = limits(fc, X, analysed, prm[live], P, rows, lo, hi)
        out[live, :N_POOLS] = pools
        prm_out[live] = rows_out
        info[s, 3] = int(kept.sum())
        if raw is not None:
            raw[s] = (live, X, P, kept)
    return out, prm_out, info
