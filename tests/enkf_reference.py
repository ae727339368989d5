"""The numpy reference of sipnet_batch_enkf_analysis_sites (include/sipnet_amd.h): the ensemble adjustment Kalman filter
(serial EnSRF, Whitaker & Hamill 2002) over every site's live members, as the contract states it.  tests/test_enkf_sites.py
pins it against textbook Kalman formulas; tests/test_gpu_enkf_sites.py holds the kernels to it."""
import numpy as np

N_POOLS = 13
WOOD, DELTA, COARSE, FINE = 0, 12, 6, 7
TINY = 0.000001


def predicted(op, pools, planes, prm_of):
    """h of one operator for n members: pools [n][13] (forecast), planes [3][n_steps][n] or None, prm_of(param) -> [n]"""
    kind, mask, plane, param, scale = op
    if kind == 0:
        s = np.zeros(pools.shape[0])
        for p in range(N_POOLS):
            if mask & (1 << p):
                s = s + pools[:, p]
    else:
        s = planes[plane].astype(np.float64).sum(0)
    h = scale * s
    if param >= 0:
        h = h / prm_of(param)
    return h


def eakf(X, H, y, sd, inflation=1.0):
    """X [n][nA] analysed pools, H [n][n_obs] predicted observations (float64, n >= 2 members), y / sd [n_obs] (NaN y: skipped)
    -> X after the serial update (no limits)"""
    X = np.array(X, dtype=np.float64)
    H = np.array(H, dtype=np.float64)
    n = X.shape[0]
    if inflation != 1.0:
        X = X.mean(0) + inflation * (X - X.mean(0))
        H = H.mean(0) + inflation * (H - H.mean(0))
    for i in range(H.shape[1]):
        if np.isnan(y[i]):
            continue
        h = H[:, i].copy()
        hbar = h.mean()
        dh = h - hbar
        var_h = (dh * dh).sum() / (n - 1)
        R = sd[i] ** 2
        alpha = 1.0 / (1.0 + np.sqrt(R / (var_h + R)))
        for M in (X, H[:, i + 1:]):
            if M.shape[1] == 0:
                continue
            cov = ((M - M.mean(0)) * dh[:, None]).sum(0) / (n - 1)
            K = cov / (var_h + R)
            M += K * (y[i] - hbar) - alpha * K * dh[:, None]
    return X


def limits(forecast, X, analysed):
    """forecast [n][13] pools, X [n][nA] updated analysed pools -> (pools [n][13] written, kept mask [n]): clipped at 0
    (plantCAccountingDelta excepted); a member whose result is not finite or fails hasSufficientBiomass keeps its forecast"""
    out = np.array(forecast, dtype=np.float64)
    X = np.array(X, dtype=np.float64)
    for q, p in enumerate(analysed):
        if p != DELTA:
            X[:, q] = np.where(X[:, q] < 0.0, 0.0, X[:, q])
        out[:, p] = X[:, q]
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(X).all(1) & (out[:, WOOD] > TINY) & (out[:, WOOD] + out[:, DELTA] > TINY)
              & (out[:, FINE] + out[:, COARSE] > TINY))
    out[~ok] = forecast[~ok]
    return out, ~ok


def site_code(obs, sd, lam, n_live):
    """(code, observations used) of one site: -2 bad input, -1 no observation, 0 fewer than 2 live members, 1 analysed"""
    seen = ~np.isnan(obs)
    bad = (~np.isfinite(obs[seen])).any() or (~(np.isfinite(sd[seen]) & (sd[seen] > 0))).any()
    bad = bad or not (np.isfinite(lam) and lam >= 1.0)
    if bad:
        return -2, 0
    if not seen.any():
        return -1, 0
    if n_live < 2:
        return 0, 0
    return 1, int(seen.sum())


def analysis(state, status, site_ok, n_sites, ops, analysed, obs, sd, inflation=None, planes=None, prm=None):
    """the whole call: state [ncol][32] (get_state), status [ncol], site_ok [n_sites] (plan status OK), ops: tuples
    (kind, pool_mask, plane, param, scale), analysed: state slots, obs / sd [n_sites][n_obs], planes [3][n_steps][ncol]
    (float64 / float32), prm [ncol][NPARAMS] the parameters each column carries -> (state after, info [n_sites][4])"""
    state = np.array(state, dtype=np.float64)
    ncol = state.shape[0]
    M = ncol // n_sites
    out = state.copy()
    info = np.zeros((n_sites, 4), dtype=np.int32)
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[(status[cols] == 0) & bool(site_ok[s])]
        lam = 1.0 if inflation is None else float(inflation[s])
        code, used = site_code(np.asarray(obs[s], dtype=np.float64), np.asarray(sd[s], dtype=np.float64), lam, len(live))
        info[s] = (code, used, len(live), 0)
        if code != 1:
            continue
        fc = state[live, :N_POOLS]
        H = np.stack([predicted(op, fc, None if planes is None else [None if p is None else p[:, live] for p in planes],
                                lambda k: prm[live, k]) for op in ops], 1)
        X = eakf(fc[:, analysed], H, np.asarray(obs[s], dtype=np.float64), np.asarray(sd[s], dtype=np.float64), lam)
        pools, kept = limits(fc, X, analysed)
        out[live, :N_POOLS] = pools
        info[s, 3] = int(kept.sum())
    return out, info
