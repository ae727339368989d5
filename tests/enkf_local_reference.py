"""The numpy reference of sipnet_batch_enkf_analysis_local (include/sipnet_amd.h): the serial square-root EnKF (EAKF) over a
joint ensemble of sites, every observation moving the sites of its footprint with a taper, in plain serial order -- no
schedule.  tests/test_enkf_local.py pins it against tests/enkf_reference.py, a hand-computed case and the textbook Kalman
update; tests/test_gpu_enkf_local.py holds the kernels to it."""
import numpy as np

from tests import enkf_reference as er


def footprint(s, ptr, nbr, rho):
    """[(t, rho_st)] of F(s): s itself (rho 1), then its neighbours"""
    return [(s, 1.0)] + [(int(nbr[k]), float(rho[k])) for k in range(int(ptr[s]), int(ptr[s + 1]))]


def codes(obs, sd, inflation, n_live, ptr, nbr):
    """(code [n_sites], own observations used [n_sites]): the per-site codes (er.site_code); the sources are its code-1
    sites; a -1 site that a source reaches (it is in the source's F) gets 1 with >= 2 live members, else 0"""
    n_sites = len(n_live)
    code = np.zeros(n_sites, dtype=np.int32)
    used = np.zeros(n_sites, dtype=np.int32)
    for s in range(n_sites):
        lam = 1.0 if inflation is None else float(inflation[s])
        code[s], used[s] = er.site_code(np.asarray(obs[s], dtype=np.float64), np.asarray(sd[s], dtype=np.float64), lam,
                                        int(n_live[s]))
    source = code == 1
    reached = np.zeros(n_sites, dtype=bool)
    for s in np.flatnonzero(source):
        reached[nbr[int(ptr[s]):int(ptr[s + 1])]] = True
    code = np.where((code == -1) & reached, np.where(np.asarray(n_live) >= 2, 1, 0), code).astype(np.int32)
    return code, used


def update(X, H, live, code, obs, sd, ptr, nbr, rho, inflation=None):
    """X [n_sites][M][nA] analysed pools, H [n_sites][M][n_obs] predicted observations, live [n_sites][M], code [n_sites]
    -> (X, H) after the inflation of every code-1 site and the serial slots (no limits); dead members untouched"""
    X = np.array(X, dtype=np.float64)
    H = np.array(H, dtype=np.float64)
    live = np.asarray(live, dtype=bool)
    n_sites, _, n_obs = H.shape
    for s in range(n_sites):
        lam = 1.0 if inflation is None else float(inflation[s])
        if code[s] != 1 or lam == 1.0:
            continue
        L = live[s]
        for Z in (X[s], H[s]):
            mean = Z[L].mean(0)
            Z[L] = mean + lam * (Z[L] - mean)
    for s in range(n_sites):
        for i in range(n_obs):
            y = float(obs[s][i])
            if np.isnan(y) or code[s] != 1:
                continue
            Ls = live[s]
            n = int(Ls.sum())
            h = H[s][:, i].copy()
            hbar = h[Ls].mean()
            V = ((h[Ls] - hbar) ** 2).sum() / (n - 1)
            R = float(sd[s][i]) ** 2
            D = V + R
            alpha = 1.0 / (1.0 + np.sqrt(R / D))
            innov = y - hbar
            for t, r in footprint(s, ptr, nbr, rho):
                if code[t] != 1:
                    continue
                J = Ls & live[t]
                nJ = int(J.sum())
                if nJ < 2:
                    continue
                first = 0 if t > s else (i + 1 if t == s else n_obs)
                hJ = h[J]
                dhJ = hJ - hJ.mean()
                dh = hJ - hbar
                for Z in (X[t], H[t][:, first:]):
                    if Z.shape[1] == 0:
                        continue
                    ZJ = Z[J]
                    K = r * ((((ZJ - ZJ.mean(0)) * dhJ[:, None]).sum(0) / (nJ - 1)) / D)
                    Z[J] = ZJ + K * innov - alpha * K * dh[:, None]
    return X, H


def analysis(state, status, site_ok, n_sites, ops, analysed, obs, sd, nbr_ptr, nbr, rho, inflation=None, planes=None,
             prm=None):
    """the whole call, arguments as tests/enkf_reference.analysis plus the localization's CSR lists -> (state after,
    info [n_sites][4])"""
    state = np.array(state, dtype=np.float64)
    ncol = state.shape[0]
    M = ncol // n_sites
    n_obs = len(ops)
    live = np.stack([(np.asarray(status[s * M:(s + 1) * M]) == 0) & bool(site_ok[s]) for s in range(n_sites)])
    n_live = live.sum(1)
    code, used = codes(obs, sd, inflation, n_live, nbr_ptr, nbr)
    X = np.zeros((n_sites, M, len(analysed)))
    H = np.zeros((n_sites, M, n_obs))
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        fc = state[cols, :er.N_POOLS]
        X[s] = fc[:, analysed]
        with np.errstate(divide="ignore", invalid="ignore"):
            for i, op in enumerate(ops):
                H[s][:, i] = er.predicted(op, fc, None if planes is None else [None if p is None else p[:, cols] for p in planes],
                                          lambda k: prm[cols, k])
    X, H = update(X, H, live, code, obs, sd, nbr_ptr, nbr, rho, inflation)
    out = state.copy()
    info = np.zeros((n_sites, 4), dtype=np.int32)
    for s in range(n_sites):
        info[s] = (code[s], used[s] if code[s] == 1 else 0, n_live[s], 0)
        if code[s] != 1:
            continue
        cols = np.arange(s * M, (s + 1) * M)[live[s]]
        pools, kept = er.limits(state[cols, :er.N_POOLS], X[s][live[s]], analysed)
        out[cols, :er.N_POOLS] = pools
        info[s, 3] = int(kept.sum())
    return out, info
