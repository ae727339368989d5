"""The localized ensemble Kalman filter across the sites of a batch (sipnet_batch_enkf_analysis_local), host side: the list
checks and the schedule (sa.enkf_local_schedule), the Gaspari-Cohn taper (sa.gaspari_cohn), and the numpy reference
(tests/enkf_local_reference.py) that tests/test_gpu_enkf_local.py holds the kernels to, pinned against the per-site reference,
a hand-computed case and the textbook Kalman update."""
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_local_reference as lr
from tests import enkf_reference as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sipnet_enkf_local_schedule", "sipnet_batch_enkf_local_create", "sipnet_enkf_local_levels", "sipnet_enkf_local_destroy",
       "sipnet_batch_enkf_analysis_local", "sipnet_debug_enkf_local_serial"]


def test_header_declares_and_library_exports_the_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sipnet_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(sa.lib(), name), name
        assert name in _lib.SIGNATURES, name


def test_null_arguments_are_refused():
    L = sa.lib()
    assert L.sipnet_batch_enkf_analysis_local(None, None, 1, None, 1, None, 0, 0, 0, None, None, None, None, None) \
        == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_enkf_analysis_local" in L.sipnet_last_error()
    assert L.sipnet_batch_enkf_local_create(None, 1, None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.sipnet_enkf_local_levels(None) == 0
    assert L.sipnet_debug_enkf_local_serial(None, 1) == _lib.ERR_BAD_ARGUMENT
    L.sipnet_enkf_local_destroy(None)


def refused(ptr, nbr, rho, n_obs=2):
    with pytest.raises(sa.SipnetError) as e:
        sa.enkf_local_schedule(ptr, nbr, rho, n_obs)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT
    return sa.lib().sipnet_last_error().decode()


def test_list_refusals_one_per_rule():
    assert "nbr_ptr[0]" in refused([1, 1, 1], [1], [0.5])
    assert "non-decreasing" in refused([0, 1, 0], [1], [0.5])
    assert "out of range" in refused([0, 1, 1], [2], [0.5])
    assert "out of range" in refused([0, 1, 1], [-1], [0.5])
    assert "own neighbour" in refused([0, 1, 1], [0], [0.5])
    assert "strictly ascending" in refused([0, 2, 2, 2], [2, 1], [0.5, 0.5])
    assert "strictly ascending" in refused([0, 2, 2, 2], [1, 1], [0.5, 0.5])
    for bad in (0.0, -0.5, 1.5, np.nan, np.inf):
        assert "rho" in refused([0, 1, 1], [1], [bad])
    assert "n_obs" in refused([0, 0], [], [], n_obs=0)
    assert "n_obs" in refused([0, 0], [], [], n_obs=17)
    level, n = sa.enkf_local_schedule([0, 1, 1], [1], [1.0], 16)          # rho 1 and 16 observations are fine
    assert n == 32 and level.shape == (2, 16)                         # (site 1 waits behind site 0)


def random_lists(rng, n_sites, p):
    ptr, nbr, rho = [0], [], []
    for s in range(n_sites):
        row = [t for t in range(n_sites) if t != s and rng.random() < p]
        nbr += row
        rho += list(rng.uniform(0.05, 1.0, len(row)))
        ptr.append(len(nbr))
    return np.array(ptr), np.array(nbr, dtype=np.int32), np.array(rho)


@pytest.mark.parametrize("seed", range(6))
def test_schedule_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n_sites, n_obs = int(rng.integers(2, 40)), int(rng.integers(1, 5))
    ptr, nbr, rho = random_lists(rng, n_sites, float(rng.choice([0.02, 0.1, 0.3])))
    level, n_levels = sa.enkf_local_schedule(ptr, nbr, rho, n_obs)
    F = [set([s]) | set(nbr[ptr[s]:ptr[s + 1]].tolist()) for s in range(n_sites)]
    slots = [(s, i) for s in range(n_sites) for i in range(n_obs)]
    assert n_levels == level.max() + 1 and level.min() >= 0
    for a, (s, i) in enumerate(slots):                      # conflicting slots: strictly in serial order
        for (s2, i2) in slots[a + 1:]:
            if F[s] & F[s2]:
                assert level[s, i] < level[s2, i2]
    for lv in range(n_levels):                              # one level: disjoint footprints
        seen = set()
        for s, i in zip(*np.nonzero(level == lv)):
            assert not (seen & F[s])
            seen |= F[s]
    last = np.full(n_sites, -1)                             # the greedy rule
    for s, i in slots:
        want = 1 + max(last[t] for t in F[s])
        assert level[s, i] == want
        for t in F[s]:
            last[t] = want


def test_empty_lists_give_level_i():
    level, n = sa.enkf_local_schedule(np.zeros(8, dtype=np.int64), [], [], 5)
    np.testing.assert_array_equal(level, np.tile(np.arange(5), (7, 1)))
    assert n == 5


def joint(rng, n_sites, M, nA, n_obs):
    X = rng.normal(size=(n_sites, M, nA)) * [3.0, 1.0, 0.5][:nA] + 10.0
    H = np.stack([X[:, :, 0] + 0.3 * X[:, :, -1] + rng.normal(size=(n_sites, M)) * 0.1 * (k + 1) for k in range(n_obs)], 2)
    return X, H


def test_empty_lists_equal_the_per_site_reference():
    rng = np.random.default_rng(11)
    n_sites, M, n_obs = 5, 40, 3
    X, H = joint(rng, n_sites, M, 3, n_obs)
    live = rng.random((n_sites, M)) > 0.1
    live[3, 0], live[3, 1:] = True, False                         # one site with a single live member: code 0
    obs = H.mean(1) + rng.normal(size=(n_sites, n_obs))
    sd = np.abs(rng.normal(1.0, 0.2, (n_sites, n_obs)))
    obs[1] = np.nan                                                # -1
    obs[2, 1] = np.nan
    sd[4, 0] = -1.0                                                # -2
    infl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
    ptr = np.zeros(n_sites + 1, dtype=np.int64)
    code, used = lr.codes(obs, sd, infl, live.sum(1), ptr, np.zeros(0, np.int32))
    assert list(code) == [1, -1, 1, 0, -2]
    X1, _ = lr.update(X, H, live, code, obs, sd, ptr, [], [], infl)
    for s in range(n_sites):
        want = er.site_code(obs[s], sd[s], infl[s], int(live[s].sum()))
        assert (code[s], used[s]) == want
        if code[s] != 1:
            np.testing.assert_array_equal(X1[s], X[s])
            continue
        ref = er.eakf(X[s][live[s]], H[s][live[s]], obs[s], sd[s], infl[s])
        np.testing.assert_allclose(X1[s][live[s]], ref, rtol=1e-13, atol=0)
        np.testing.assert_array_equal(X1[s][~live[s]], X[s][~live[s]])


def test_hand_computed_two_sites_rho_half():
    """site 0: pool a = 1, 2, 3, 4 observed directly (R = 5/3 = var(a): D = 10/3, alpha = 1 / (1 + sqrt(1/2)), y = 4.5,
    innovation 2); site 1: pool b = 2, 4, 6, 8, not observed, rho 1/2: K_b = 1/2 cov(b, a) / D = 1/2, so b moves by 1 and its
    deviations 2 (a - 2.5) lose alpha / 2 (a - 2.5); a as in the per-site case (K_a = 1/2)"""
    a = np.array([1.0, 2.0, 3.0, 4.0])
    X = np.stack([a[:, None], 2.0 * a[:, None]])
    H = np.stack([a[:, None], np.zeros((4, 1))])
    obs = np.array([[4.5], [np.nan]])
    sd = np.full((2, 1), np.sqrt(5.0 / 3.0))
    ptr, nbr, rho = np.array([0, 1, 1]), np.array([1], np.int32), np.array([0.5])
    live = np.ones((2, 4), dtype=bool)
    code, used = lr.codes(obs, sd, None, live.sum(1), ptr, nbr)
    assert list(code) == [1, 1] and list(used) == [1, 0]
    X1, H1 = lr.update(X, H, live, code, obs, sd, ptr, nbr, rho)
    alpha = 1.0 / (1.0 + np.sqrt(0.5))
    da = a - 2.5
    np.testing.assert_allclose(X1[0, :, 0], 2.5 + 1.0 + da * (1.0 - 0.5 * alpha), rtol=0, atol=1e-14)
    np.testing.assert_allclose(X1[1, :, 0], 5.0 + 1.0 + da * (2.0 - 0.5 * alpha), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(H1[0], H[0])                     # h_{s,i} itself is never written
    # the other way round (site 1 lists site 0, site 0 does not list site 1): site 1 is not reached
    code2, _ = lr.codes(obs, sd, None, live.sum(1), np.array([0, 0, 1]), np.array([0], np.int32))
    assert list(code2) == [1, -1]


def test_rho_one_equals_the_kalman_update_of_the_joint_sample_statistics():
    rng = np.random.default_rng(5)
    M = 400
    Z = rng.normal(size=(M, 4)) @ np.array([[2.0, 0.4, 0.9, 0.1], [0.0, 1.0, 0.3, 0.5], [0.0, 0.0, 1.2, 0.2],
                                            [0.0, 0.0, 0.0, 0.7]]) + [5.0, 1.0, 3.0, 2.0]
    X = np.stack([Z[:, :2], Z[:, 2:]])                            # the joint state: 2 pools per site
    Hm = np.array([0.6, 0.4, 0.0, 0.0])                           # one scalar observation of site 0's pools
    H = np.stack([(Z @ Hm)[:, None], np.zeros((M, 1))])
    y, sd = 4.0, 0.9
    obs = np.array([[y], [np.nan]])
    sds = np.array([[sd], [1.0]])
    ptr, nbr, rho = np.array([0, 1, 2]), np.array([1, 0], np.int32), np.array([1.0, 1.0])
    live = np.ones((2, M), dtype=bool)
    code, _ = lr.codes(obs, sds, None, live.sum(1), ptr, nbr)
    X1, _ = lr.update(X, H, live, code, obs, sds, ptr, nbr, rho)
    got = np.concatenate([X1[0], X1[1]], 1)
    P = np.cov(Z, rowvar=False, ddof=1)
    K = P @ Hm / (Hm @ P @ Hm + sd * sd)
    np.testing.assert_allclose(got.mean(0), Z.mean(0) + K * (y - Hm @ Z.mean(0)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), P - np.outer(K, Hm @ P), rtol=0, atol=1e-10)


def test_identical_ensembles_with_rho_one_end_equal():
    rng = np.random.default_rng(8)
    M, n_obs = 60, 3
    X0, H0 = joint(rng, 1, M, 3, n_obs)
    X = np.concatenate([X0, X0])
    H = np.concatenate([H0, H0])
    obs = np.stack([H0[0].mean(0) + rng.normal(size=n_obs), np.full(n_obs, np.nan)])
    sd = np.ones((2, n_obs))
    ptr, nbr, rho = np.array([0, 1, 2]), np.array([1, 0], np.int32), np.array([1.0, 1.0])
    live = np.ones((2, M), dtype=bool)
    code, _ = lr.codes(obs, sd, [1.05, 1.05], live.sum(1), ptr, nbr)
    X1, _ = lr.update(X, H, live, code, obs, sd, ptr, nbr, rho, [1.05, 1.05])
    assert np.abs(X1[0] - X[0]).max() > 1e-3
    np.testing.assert_allclose(X1[1], X1[0], rtol=1e-13, atol=0)


def test_dead_members_and_thin_intersections():
    """J = L_s and L_t: members dead at either site neither count nor move; |J| < 2 skips the target"""
    rng = np.random.default_rng(21)
    M = 30
    X, H = joint(rng, 3, M, 2, 1)
    live = np.ones((3, M), dtype=bool)
    live[0, :5] = False
    live[1, 10:] = False                      # site 1: members 0..9 live, J with site 0 = 5..9
    live[2, 1:] = False                       # site 2: one live member -> code 0 when reached
    obs = np.array([[H[0][live[0], 0].mean() + 1.0], [np.nan], [np.nan]])
    sd = np.ones((3, 1))
    ptr, nbr, rho = np.array([0, 2, 2, 2]), np.array([1, 2], np.int32), np.array([0.8, 0.8])
    code, _ = lr.codes(obs, sd, None, live.sum(1), ptr, nbr)
    assert list(code) == [1, 1, 0]
    X1, _ = lr.update(X, H, live, code, obs, sd, ptr, nbr, rho)
    J = live[0] & live[1]
    assert (X1[1][J] != X[1][J]).all()
    np.testing.assert_array_equal(X1[1][~J], X[1][~J])
    np.testing.assert_array_equal(X1[2], X[2])
    np.testing.assert_array_equal(X1[0][~live[0]], X[0][~live[0]])


def test_gaspari_cohn_taper():
    c = 100.0
    assert sa.enkf_local.taper(0.0) == 1.0
    assert abs(float(sa.enkf_local.taper(1.0)) - 5.0 / 24.0) < 1e-15
    assert float(sa.enkf_local.taper(2.0)) == 0.0 and float(sa.enkf_local.taper(3.0)) == 0.0
    r = np.linspace(0.0, 2.0, 2001)
    g = sa.enkf_local.taper(r)
    assert (np.diff(g) <= 1e-15).all() and (g >= -1e-15).all()
    left, right = sa.enkf_local.taper(1.0 - 1e-9), sa.enkf_local.taper(1.0 + 1e-9)
    assert abs(float(left) - float(right)) < 1e-8                    # continuous at d = c
    # along the equator, 1 degree = 6371 pi / 180 km: sites at 0 and d = c, 2c - eps, 2c + eps
    deg = 180.0 / (np.pi * 6371.0)
    lon = np.array([0.0, c * deg, 2.0 * c * deg * (1 - 1e-6), 2.0 * c * deg * (1 + 1e-6), 0.0])
    lat = np.zeros(5)
    lat[4] = 10.0 * c * deg
    ptr, nbr, rho = sa.gaspari_cohn(lat, lon, c)
    assert ptr.dtype == np.int64 and nbr.dtype == np.int32 and rho.dtype == np.float64
    row0 = dict(zip(nbr[ptr[0]:ptr[1]].tolist(), rho[ptr[0]:ptr[1]].tolist()))
    assert set(row0) == {1, 2} and abs(row0[1] - 5.0 / 24.0) < 1e-9 and 0.0 < row0[2] < 1e-9
    assert ptr[5] - ptr[4] == 0                                     # 10 c away from everything
    assert (rho > 0).all() and (rho <= 1).all()
    for s in range(5):                                              # no self, ascending
        row = nbr[ptr[s]:ptr[s + 1]]
        assert s not in row and (np.diff(row) > 0).all()
    # symmetric in site order: the taper between s and t is the same either way, and after a permutation of the sites
    rng = np.random.default_rng(4)
    la, lo = rng.uniform(30, 50, 40), rng.uniform(-100, -70, 40)
    ptr, nbr, rho = sa.gaspari_cohn(la, lo, 400.0)
    W = np.zeros((40, 40))
    for s in range(40):
        W[s, nbr[ptr[s]:ptr[s + 1]]] = rho[ptr[s]:ptr[s + 1]]
    np.testing.assert_array_equal(W, W.T)
    perm = rng.permutation(40)
    p2, n2, r2 = sa.gaspari_cohn(la[perm], lo[perm], 400.0)
    W2 = np.zeros((40, 40))
    for s in range(40):
        W2[s, n2[p2[s]:p2[s + 1]]] = r2[p2[s]:p2[s + 1]]
    np.testing.assert_array_equal(W2, W[np.ix_(perm, perm)])
    sa.enkf_local_schedule(ptr, nbr, rho, 4)                        # the library accepts what it returns
