"""The numpy reference of sipnet_batch_enkf_analysis_smooth (include/sipnet_amd.h): enkf_joint_reference's analysis of the
pools and parameters, and every series element of a code-1 site's live members as one more analysed variable of the serial
filter of tests/enkf_reference.py (eakf: the pools' lambda, no limits); dst = src everywhere else.  weights_form is the
covariance-space arithmetic the kernels use (g and G from the chain on the rows' covariance), restated in numpy.
tests/test_enkf_smooth.py pins both against the textbook; tests/test_gpu_enkf_smooth.py holds the kernels to `analysis`."""
import numpy as np

from tests import enkf_joint_reference as jr
from tests import enkf_reference as er


def eakf(Z, H, y, sd, inflation=1.0):
    """Z [n][nz] series elements of the n live members, H [n][n_obs] -> Z after the serial update: the member-space filter"""
    return er.eakf(Z, H, y, sd, inflation)


def weights_form(Z, H, y, sd, lam=1.0):
    """the same through z_a[j] = zbar + lambda (z_j - zbar) + c_z . g + (c_z G) . a_j"""
    Z, H = np.array(Z, dtype=np.float64), np.array(H, dtype=np.float64)
    n = Z.shape[0]
    Zi = Z.mean(0) + lam * (Z - Z.mean(0)) if lam != 1.0 else Z.copy()
    Hi = H.mean(0) + lam * (H - H.mean(0)) if lam != 1.0 else H.copy()
    used = [i for i in range(H.shape[1]) if not np.isnan(y[i])]
    p = len(used)
    A = Hi[:, used] - Hi[:, used].mean(0)               # the rows' forecast anomalies [n][p]
    mean = Hi[:, used].mean(0).copy()
    C = A.T @ A / (n - 1)
    Ec, g, G = np.eye(p), np.zeros(p), np.zeros((p, p))  # unit covariance vectors carried as "pool rows": covariance, shift, transform
    T = np.eye(p)                                       # row l = sum_w T[l][w] a_w
    for l in range(p):
        R = sd[used[l]] ** 2
        D = C[l, l] + R
        alpha = 1.0 / (1.0 + np.sqrt(R / D))
        innov = y[used[l]] - mean[l]
        Kz = Ec[:, l] / D
        g += Kz * innov
        G -= alpha * Kz[:, None] * T[l][None, :]
        Ec -= Kz[:, None] * C[l][None, :]
        K = C[:, l] / D
        for w in range(l + 1, p):
            mean[w] += K[w] * innov
            T[w] -= alpha * K[w] * T[l]
        C -= np.outer(K, C[l].copy())
    Cz = (Zi - Zi.mean(0)).T @ A / (n - 1)               # c_z of every element [nz][p]
    return Zi + (g[None, :] + A @ G.T) @ Cz.T


def analysis(state, status, site_ok, n_sites, ops, analysed, params, obs, sd, series, inflation=None, param_inflation=None,
             planes=None, prm=None):
    """the arguments of enkf_joint_reference.analysis, and series: a list of arrays [rows][>= ncol] (the forecast values)
    -> (state after, parameters after, info, the list of dst as float64 arrays [rows][ncol])"""
    state = np.array(state, dtype=np.float64)
    prm = np.array(prm, dtype=np.float64)
    out, prm_out, info = jr.analysis(state, status, site_ok, n_sites, ops, analysed, params, obs, sd, inflation, param_inflation,
                                     planes, prm)
    ncol = state.shape[0]
    M = ncol // n_sites
    dst = [np.array(z[:, :ncol], dtype=np.float64) for z in series]
    for s in range(n_sites):
        if info[s, 0] != 1:
            continue
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[(status[cols] == 0) & bool(site_ok[s])]
        fc = state[live, :er.N_POOLS]
        H = np.stack([er.predicted(op, fc, None if planes is None else [None if p is None else p[:, live] for p in planes],
                                   lambda k: prm[live, k]) for op in ops], 1)
        lam = 1.0 if inflation is None else float(inflation[s])
        y, e = np.asarray(obs[s], dtype=np.float64), np.asarray(sd[s], dtype=np.float64)
        # (next to the analysed pools, in one call: a series that copies a pool's forecast then gets the pool's value, bit for bit)
        Z = np.concatenate([fc[:, analysed]] + [np.asarray(z[:, live], dtype=np.float64).T for z in series], 1)
        Z = eakf(Z, H, y, e, lam)
        at = len(analysed)
        for k, z in enumerate(series):
            dst[k][:, live] = Z[:, at:at + z.shape[0]].T
            at += z.shape[0]
    return out, prm_out, info, dst
