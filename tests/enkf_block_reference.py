"""The numpy reference of sipnet_batch_enkf_analysis_block (include/sipnet_amd.h): a block-local EnKF analysis.  Every code-1
target site is analysed on its own, in member space, from private copies of the predicted observations within its reach, with
the observation error of a row divided by its taper (R localization).  Codes, limits and the operators are those of
tests/enkf_reference.py and tests/enkf_local_reference.py.  tests/test_enkf_block.py pins it against both, a hand-computed
case and the batch Kalman update; tests/test_gpu_enkf_block.py holds the kernels to it."""
import numpy as np

from tests import enkf_local_reference as lr
from tests import enkf_reference as er


def in_lists(n_sites, ptr, nbr, rho):
    """[(u, rho_ut)] ascending in u for every site t: the sites u != t that list t as a neighbour"""
    out = [[] for _ in range(n_sites)]
    for u in range(n_sites):
        for k in range(int(ptr[u]), int(ptr[u + 1])):
            out[int(nbr[k])].append((u, float(rho[k])))
    return out


def row_counts(n_sites, n_obs, ptr, nbr):
    """n_obs x (1 + in-neighbours) of every site: what sipnet_enkf_local_rows returns"""
    deg = np.zeros(n_sites, dtype=np.int64)
    for k in range(int(ptr[n_sites])):
        deg[int(nbr[k])] += 1
    return (n_obs * (1 + deg)).astype(np.int32)


def rows_of(t, live, code, obs, ins):
    """the rows of target t in site-major order -> ([(u, i, rho)] used, rows dropped): a row from u != t is dropped when a
    member live at t is not live at u"""
    sources = sorted(ins[t] + [(t, 1.0)])
    used, dropped = [], 0
    for u, r in sources:
        if code[u] != 1:
            continue
        covered = u == t or not (live[t] & ~live[u]).any()
        for i in range(obs.shape[1]):
            if np.isnan(obs[u][i]):
                continue
            if covered:
                used.append((u, i, r))
            else:
                dropped += 1
    return used, dropped


def eakf_rows(X, H, y, R):
    """er.eakf's serial update, expression for expression, with the observation-error variances R [p] given and no inflation:
    X [n][nA], H [n][p], y [p] (NaN: skipped) -> X after"""
    X = np.array(X, dtype=np.float64)
    H = np.array(H, dtype=np.float64)
    n = X.shape[0]
    for i in range(H.shape[1]):
        if np.isnan(y[i]):
            continue
        h = H[:, i].copy()
        hbar = h.mean()
        dh = h - hbar
        var_h = (dh * dh).sum() / (n - 1)
        alpha = 1.0 / (1.0 + np.sqrt(R[i] / (var_h + R[i])))
        for M in (X, H[:, i + 1:]):
            if M.shape[1] == 0:
                continue
            cov = ((M - M.mean(0)) * dh[:, None]).sum(0) / (n - 1)
            K = cov / (var_h + R[i])
            M += K * (y[i] - hbar) - alpha * K * dh[:, None]
    return X


def update_live(Xs, Hs, live, code, obs, sd, ptr, nbr, rho, inflation=None):
    """Xs[s] [n_s][nA], Hs[s] [n_s][n_obs]: the analysed pools and predicted observations of site s's LIVE members, in member
    order (None for a site that is not code 1); live [n_sites][M] -> (Xs after the inflation and every target's own serial
    update (no limits), rows [n_sites][2] = {used, dropped}).  A target's own NaN slots stay in its H as columns that are
    skipped, as er.eakf keeps them."""
    obs = np.asarray(obs, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    live = np.asarray(live, dtype=bool)
    n_sites, n_obs = obs.shape
    Xs, Hs = list(Xs), list(Hs)
    for s in range(n_sites):
        lam = 1.0 if inflation is None else float(inflation[s])
        if code[s] != 1:
            continue
        X, H = np.array(Xs[s], dtype=np.float64), np.array(Hs[s], dtype=np.float64)
        if lam != 1.0:
            X = X.mean(0) + lam * (X - X.mean(0))
            H = H.mean(0) + lam * (H - H.mean(0))
        Xs[s], Hs[s] = X, H
    ins = in_lists(n_sites, ptr, nbr, rho)
    out = list(Xs)
    rows = np.zeros((n_sites, 2), dtype=np.int32)
    for t in range(n_sites):
        if code[t] != 1:
            continue
        used, dropped = rows_of(t, live, code, obs, ins)
        rows[t] = (len(used), dropped)
        cols, y, R = [], [], []
        for u in sorted(set(u for u, _, _ in used) | {t}):
            r = dict((v, w) for v, _, w in used).get(u, 1.0)
            at = (np.cumsum(live[u]) - 1)[live[t]]                    # L_t's members in u's live order
            for i in range(n_obs):
                if u != t and np.isnan(obs[u][i]):
                    continue
                cols.append(Hs[u][:, i] if u == t else Hs[u][at, i])  # the private copies, over L_t
                y.append(obs[u][i])
                R.append(sd[u][i] ** 2 / r)
        out[t] = eakf_rows(Xs[t], np.stack(cols, 1), np.array(y), np.array(R))
    return out, rows


def update(X, H, live, code, obs, sd, ptr, nbr, rho, inflation=None):
    """update_live on whole arrays: X [n_sites][M][nA], H [n_sites][M][n_obs] -> (X after, rows); dead members untouched"""
    live = np.asarray(live, dtype=bool)
    n_sites = len(live)
    Xs, rows = update_live([X[s][live[s]] for s in range(n_sites)], [H[s][live[s]] for s in range(n_sites)], live, code, obs,
                           sd, ptr, nbr, rho, inflation)
    out = np.array(X, dtype=np.float64)
    for s in range(n_sites):
        if code[s] == 1:
            out[s][live[s]] = Xs[s]
    return out, rows


def analysis(state, status, site_ok, n_sites, ops, analysed, obs, sd, nbr_ptr, nbr, rho, inflation=None, planes=None,
             prm=None):
    """the whole call, arguments as tests/enkf_local_reference.analysis -> (state after, info [n_sites][4],
    rows [n_sites][2]).  A site's arrays are made as tests/enkf_reference.analysis makes them."""
    state = np.array(state, dtype=np.float64)
    ncol = state.shape[0]
    M = ncol // n_sites
    live = np.stack([(np.asarray(status[s * M:(s + 1) * M]) == 0) & bool(site_ok[s]) for s in range(n_sites)])
    n_live = live.sum(1)
    code, used = lr.codes(obs, sd, inflation, n_live, nbr_ptr, nbr)
    Xs, Hs, members = [None] * n_sites, [None] * n_sites, [None] * n_sites
    for s in range(n_sites):
        if code[s] != 1:
            continue
        cols = np.arange(s * M, (s + 1) * M)
        lv = members[s] = cols[live[s]]
        fc = state[lv, :er.N_POOLS]
        Hs[s] = np.stack([er.predicted(op, fc, None if planes is None else [None if p is None else p[:, lv] for p in planes],
                                       lambda k: prm[lv, k]) for op in ops], 1)
        Xs[s] = fc[:, analysed]
    Xs, rows = update_live(Xs, Hs, live, code, obs, sd, nbr_ptr, nbr, rho, inflation)
    out = state.copy()
    info = np.zeros((n_sites, 4), dtype=np.int32)
    for s in range(n_sites):
        info[s] = (code[s], used[s] if code[s] == 1 else 0, n_live[s], 0)
        if code[s] != 1:
            continue
        pools, kept = er.limits(state[members[s], :er.N_POOLS], Xs[s], analysed)
        out[members[s], :er.N_POOLS] = pools
        info[s, 3] = int(kept.sum())
    return out, info, rows
