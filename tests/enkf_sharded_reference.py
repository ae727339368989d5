"""What the tests of the EnKF analysis over an ensemble sharded by member measure against (tests/test_enkf_sharded.py,
tests/test_gpu_enkf_sharded.py; sipnet_batch_enkf_shard_moments / _analysis_sharded in include/sipnet_amd.h).  numpy only.

The layout: rank r's batch holds n_sites x M_r columns, site-major; the union ensemble of site s is rank 0's columns of s,
then rank 1's, ...  interleave() / split() go between the shards' arrays and the union's.

merged_chain64 is tests/enkf_exact_reference.cov_chain64 with its means and covariance formed per shard -- the count, the
means and the centred products about the shard's OWN means -- and merged in shard order by the pairwise update of Chan, Golub
& LeVeque (1983): n = n_a + n_b, d = mean_b - mean_a, C += C_b + d_v d_i (n_a n_b / n), mean = mean_a + d (n_b / n); empty
shards are skipped.  The chain and the application of the transform are cov_chain64's; the members' anomalies are taken about
the union's merged means."""
import numpy as np

CONDITIONING_CUTS = ((0.5,), (0.2, 0.55), (1 / 64, 2 / 64, 0.5))


def interleave(shards, n_sites):
    """shards[r] [n_sites * M_r][...] (site-major) -> the union [n_sites * sum M_r][...], site s = the shards' columns of s in
    shard order"""
    per = [np.asarray(x).reshape((n_sites, -1) + np.asarray(x).shape[1:]) for x in shards]
    u = np.concatenate(per, 1)
    return u.reshape((-1,) + u.shape[2:])


def split(union, n_sites, sizes):
    """the union [n_sites * sum sizes][...] -> the shards' arrays [n_sites * M_r][...]"""
    u = np.asarray(union)
    u = u.reshape((n_sites, -1) + u.shape[1:])
    at = np.cumsum([0] + list(sizes))
    return [u[:, at[r]:at[r + 1]].reshape((-1,) + u.shape[2:]) for r in range(len(sizes))]


def cuts_at(n, fractions):
    """member indices where n members are cut, from fractions of n"""
    return [int(round(f * n)) for f in fractions]


def moment_words(n_analysed, n_obs):
    return 2 + (n_analysed + n_obs) + (n_analysed + n_obs) * n_obs


def shard_moments(V, nA):
    """V [n_r][nA + p] a shard's variables -> (n_r, mean [nA + p], C [nA + p][p] the centred products, not divided)"""
    n = V.shape[0]
    if n == 0:
        return 0, np.zeros(V.shape[1]), np.zeros((V.shape[1], V.shape[1] - nA))
    mean = V.mean(0)
    A = V - mean
    return n, mean, A.T @ A[:, nA:]


def merge(blocks, nA):
    """[(n_r, mean_r, C_r)] in shard order -> (n, mean, C) of the union"""
    n, mean, C = 0, None, None
    for nb, mb, Cb in blocks:
        if nb == 0:
            continue
        if mean is None:
            mean, C = np.zeros_like(mb), np.zeros_like(Cb)
        tot = n + nb
        d = mb - mean
        C = C + (Cb + np.outer(d, d[nA:]) * (n * nb / tot))
        mean = mean + d * (nb / tot)
        n = tot
    return n, mean, C


def merged_chain64(X, H, y, R, cuts=()):
    """cov_chain64 over the members cut at the indices `cuts` into len(cuts) + 1 shards (a shard may be empty): X [n][nA],
    H [n][p], y [p] (NaN: skipped), R [p] -> X after"""
    X = np.array(X, dtype=np.float64)
    H = np.array(H, dtype=np.float64)
    used = [i for i in range(H.shape[1]) if not np.isnan(y[i])]
    nA, p = X.shape[1], len(used)
    if p == 0:
        return X
    V = np.concatenate([X, H[:, used]], 1)
    edges = [0] + list(cuts) + [V.shape[0]]
    n, mean0, C = merge([shard_moments(V[edges[k]:edges[k + 1]], nA) for k in range(len(edges) - 1)], nA)
    rows = V[:, nA:] - mean0[nA:]
    Cm = C / (n - 1)
    mean = mean0.copy()
    T = np.zeros((nA + p, p))
    for l in range(p):
        D = Cm[nA + l, l] + R[used[l]]
        K = Cm[:, l] / D
        alpha = 1.0 / (1.0 + np.sqrt(R[used[l]] / D))
        innov = y[used[l]] - mean[nA + l]
        Tl = T[nA + l].copy()
        Tl[l] += 1.0
        Cl = Cm[nA + l].copy()
        mean += K * innov
        T -= alpha * np.outer(K, Tl)
        Cm -= np.outer(K, Cl)
    return X + (mean[:nA] - mean0[:nA]) + rows @ T[:nA].T


def with_cuts(fractions):
    """merged_chain64 cut at fractions of the members, as a restatement for enkf_exact_reference.own_error"""
    def restatement(X, H, y, R):
        return merged_chain64(X, H, y, R, cuts_at(np.asarray(X).shape[0], fractions))
    return restatement


def conditioning_set():
    """the cases the sharded analysis is held to: the p = 4 cases of the ladder, and 16 rows over the rungs without
    (eps 1e-3, c 1e-4), whose own error at 16 rows (about 9e-9 sharded, 1.3e-8 unsharded) is within 3 x of the cap / 4"""
    from tests import enkf_exact_reference as xr
    p4 = [c for c in xr.ladder() if c["p"] == 4]
    p16 = [xr.make_case(eps, c, off, 16) for off in (1.0, 1e6) for eps, c in xr.RUNGS if (eps, c) != (1e-3, 1e-4)]
    return p4 + p16


def own_error(case, fractions=None):
    """the largest own error of merged_chain64 on the case, over CONDITIONING_CUTS or the one cut given"""
    from tests import enkf_exact_reference as xr
    return max(xr.own_error(with_cuts(f), case) for f in ([fractions] if fractions is not None else CONDITIONING_CUTS))
