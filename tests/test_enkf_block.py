"""The block-local ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_block), host side: the row counts
(sa.enkf_local_rows) and the numpy reference (tests/enkf_block_reference.py) that tests/test_gpu_enkf_block.py holds the kernels
to, pinned against the per-site reference (empty lists), the serial localized reference (complete graph, rho = 1), the batch
Kalman update with the observation errors divided by the tapers, a hand-computed case, and its own locality."""
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_block_reference as br
from tests import enkf_local_reference as lr
from tests import enkf_reference as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sipnet_enkf_local_rows", "sipnet_batch_enkf_analysis_block"]
ANALYSED = [0, 1, 2, 3, 6, 7, 12]
OPS = [(0, 1 << 1, 0, -1, 0.5), (0, (1 << 0) | (1 << 12), 0, -1, 1.0), (0, 1 << 3, 0, -1, 0.1), (0, (1 << 2) | (1 << 4), 0, -1, 1.0)]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(REPO, "include", "sipnet_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(sa.lib(), name), name
        assert name in _lib.SIGNATURES, name
    cap = int(re.search(r"#define\s+SIPNET_ENKF_BLOCK_MAX_ROWS\s+(\d+)", hdr).group(1))
    assert cap >= 128 and cap == sa.ENKF_BLOCK_MAX_ROWS


def test_null_arguments_are_refused():
    L = sa.lib()
    assert L.sipnet_batch_enkf_analysis_block(None, None, 1, None, 1, None, 0, 0, 0, None, None, None, None, None, None) \
        == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_enkf_analysis_block" in L.sipnet_last_error()
    assert L.sipnet_enkf_local_rows(2, 1, None, None, None, None) == _lib.ERR_BAD_ARGUMENT


def random_lists(rng, n_sites, p):
    ptr, nbr, rho = [0], [], []
    for s in range(n_sites):
        row = [t for t in range(n_sites) if t != s and rng.random() < p]
        nbr += row
        rho += list(rng.uniform(0.05, 1.0, len(row)))
        ptr.append(len(nbr))
    return np.array(ptr), np.array(nbr, dtype=np.int32), np.array(rho)


def complete(n_sites, rho=1.0):
    nbr = np.array([t for s in range(n_sites) for t in range(n_sites) if t != s], dtype=np.int32)
    return np.arange(n_sites + 1, dtype=np.int64) * (n_sites - 1), nbr, np.full(nbr.size, rho)


@pytest.mark.parametrize("seed", range(6))
def test_row_counts_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n_sites, n_obs = int(rng.integers(2, 60)), int(rng.integers(1, 17))
    ptr, nbr, rho = random_lists(rng, n_sites, float(rng.choice([0.02, 0.1, 0.3])))
    rows, most = sa.enkf_local_rows(ptr, nbr, n_obs)
    want = br.row_counts(n_sites, n_obs, ptr, nbr)
    np.testing.assert_array_equal(rows, want)
    assert rows.dtype == np.int32 and most == want.max()
    ins = br.in_lists(n_sites, ptr, nbr, rho)
    assert [n_obs * (1 + len(x)) for x in ins] == list(want)
    for t in range(n_sites):                                         # ascending sources, the taper of the entry that lists t
        assert [u for u, _ in ins[t]] == sorted(u for u, _ in ins[t])
        for u, r in ins[t]:
            k = ptr[u] + list(nbr[ptr[u]:ptr[u + 1]]).index(t)
            assert r == rho[k]


def test_row_counts_refuse_what_the_schedule_refuses():
    def refused(ptr, nbr, n_obs=2):
        with pytest.raises(sa.SipnetError) as e:
            sa.enkf_local_rows(ptr, nbr, n_obs)
        assert e.value.code == _lib.ERR_BAD_ARGUMENT
        msg = sa.lib().sipnet_last_error().decode()
        with pytest.raises(sa.SipnetError):                          # and so does the schedule
            sa.enkf_local_schedule(ptr, nbr, np.full(len(nbr), 0.5), n_obs)
        return msg

    assert "nbr_ptr[0]" in refused([1, 1, 1], [1])
    assert "non-decreasing" in refused([0, 1, 0], [1])
    assert "out of range" in refused([0, 1, 1], [2])
    assert "out of range" in refused([0, 1, 1], [-1])
    assert "own neighbour" in refused([0, 1, 1], [0])
    assert "strictly ascending" in refused([0, 2, 2, 2], [2, 1])
    assert "strictly ascending" in refused([0, 2, 2, 2], [1, 1])
    assert "n_obs" in refused([0, 0], [], n_obs=0)
    assert "n_obs" in refused([0, 0], [], n_obs=17)
    rows, most = sa.enkf_local_rows(np.zeros(8, dtype=np.int64), [], 5)
    assert list(rows) == [5] * 7 and most == 5
    rows, most = sa.enkf_local_rows(*complete(40)[:2], 16)            # beyond the cap: counted, not refused
    assert most == 16 * 40 > sa.ENKF_BLOCK_MAX_ROWS


def batch_state(rng, n_sites, M, dead=0.0):
    """a synthetic forecast: get_state()'s layout [ncol][32], pools positive with correlated spread, status in slot 29"""
    ncol = n_sites * M
    st = np.zeros((ncol, 32))
    common = rng.normal(size=(ncol, 1))
    st[:, :13] = np.abs(rng.uniform(1.0, 50.0, 13) * (10.0 + common + 0.5 * rng.normal(size=(ncol, 13))))
    st[:, 12] = rng.normal(size=ncol)                                 # plantCAccountingDelta: either sign
    st[:, 29] = rng.random(ncol) < dead
    return st


def observations(rng, st, n_sites, spread=1.0):
    M = st.shape[0] // n_sites
    obs = np.zeros((n_sites, len(OPS)))
    sd = np.zeros_like(obs)
    for s in range(n_sites):
        fc = st[s * M:(s + 1) * M]
        fc = fc[fc[:, 29] == 0, :13]
        for i, op in enumerate(OPS):
            h = er.predicted(op, fc, None, None) if len(fc) else np.zeros(1)
            obs[s, i] = h.mean() + spread * (h.std() + 1e-3) * rng.normal()
            sd[s, i] = (h.std() + 1e-3) * (0.5, 1.0, 2.0)[(s + i) % 3]
    return obs, sd


def test_empty_lists_equal_the_per_site_reference_exactly():
    rng = np.random.default_rng(11)
    n_sites, M = 6, 48
    st = batch_state(rng, n_sites, M, dead=0.1)
    st[3 * M + 1:4 * M, 29] = 1                                       # one live member: code 0
    obs, sd = observations(rng, st, n_sites)
    obs[1] = np.nan                                                  # -1
    obs[2, 1] = np.nan
    sd[4, 0] = -1.0                                                  # -2
    infl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
    ptr = np.zeros(n_sites + 1, dtype=np.int64)
    got, info, rows = br.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, ptr, np.zeros(0, np.int32),
                                  np.zeros(0), infl)
    want, want_info = er.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, infl)
    assert list(info[:, 0]) == [1, -1, 1, 0, -2, 1]
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(got, want)
    assert np.abs(got - st).max() > 0
    np.testing.assert_array_equal(rows, [[4, 0], [0, 0], [3, 0], [0, 0], [0, 0], [4, 0]])


def test_complete_graph_with_rho_one_equals_the_serial_localized_reference():
    """every target sees every row, in the serial order, so its private copies evolve like the joint ensemble's"""
    rng = np.random.default_rng(12)
    n_sites, M = 6, 64
    st = batch_state(rng, n_sites, M)
    obs, sd = observations(rng, st, n_sites)
    obs[2, 1] = np.nan
    ptr, nbr, rho = complete(n_sites)
    infl = np.full(n_sites, 1.04)
    got, info, rows = br.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, ptr, nbr, rho, infl)
    want, want_info = lr.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, ptr, nbr, rho, infl)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, np.tile([n_sites * len(OPS) - 1, 0], (n_sites, 1)))
    for s in range(n_sites):
        sl = slice(s * M, (s + 1) * M)
        scale = np.maximum(np.abs(want[sl][:, ANALYSED]), st[sl][:, ANALYSED].std(0))
        err = (np.abs(got[sl][:, ANALYSED] - want[sl][:, ANALYSED]) / scale).max()
        print(f"site {s}: block reference against the serial localized reference: {err:.3e}")
        assert err <= 1e-10
    assert np.abs(got - st).max() > 0


def one_target(rng, M, nA, taps):
    """target 0 with n_obs = 2 operators and two neighbours that list it with tapers `taps`: X, H as br.update takes them"""
    n_sites = 3
    Z = rng.normal(size=(M, nA + 6)) @ (rng.normal(size=(nA + 6, nA + 6)) + 2.0 * np.eye(nA + 6)) + 5.0
    X = np.zeros((n_sites, M, nA))
    X[0] = Z[:, :nA]
    X[1:] = rng.normal(size=(2, M, nA))
    H = Z[:, nA:].reshape(M, 3, 2).transpose(1, 0, 2).copy()          # H[u][j][i]: correlated with target 0's pools
    ptr, nbr, rho = np.array([0, 0, 1, 2]), np.array([0, 0], np.int32), np.array(taps)
    obs = H.mean(1) + rng.normal(size=(n_sites, 2))
    sd = np.abs(rng.normal(1.0, 0.2, (n_sites, 2))) + 0.3
    return X, H, obs, sd, ptr, nbr, rho


def test_one_target_equals_the_batch_kalman_update_with_r_over_rho():
    rng = np.random.default_rng(5)
    M, nA = 300, 3
    X, H, obs, sd, ptr, nbr, rho = one_target(rng, M, nA, [0.7, 0.25])
    live = np.ones((3, M), dtype=bool)
    code = np.array([1, 1, 1], dtype=np.int32)
    X1, rows = br.update(X, H, live, code, obs, sd, ptr, nbr, rho)
    assert list(rows[0]) == [6, 0] and list(rows[1]) == [2, 0] and list(rows[2]) == [2, 0]
    Y = np.concatenate([H[0], H[1], H[2]], 1)                        # the rows of target 0, site-major
    R = np.concatenate([sd[0] ** 2, sd[1] ** 2 / 0.7, sd[2] ** 2 / 0.25])
    y = np.concatenate([obs[0], obs[1], obs[2]])
    Zj = np.concatenate([X[0], Y], 1)
    P = np.cov(Zj, rowvar=False, ddof=1)
    Pxy, Pyy, Pxx = P[:nA, nA:], P[nA:, nA:], P[:nA, :nA]
    K = Pxy @ np.linalg.inv(Pyy + np.diag(R))
    mean = X[0].mean(0) + K @ (y - Y.mean(0))
    cov = Pxx - K @ Pxy.T
    got = X1[0]
    np.testing.assert_allclose(got.mean(0), mean, rtol=1e-10, atol=0)
    np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), cov, rtol=1e-10, atol=1e-10 * np.abs(cov).max())
    # the neighbours themselves are analysed from their own rows only: nobody lists them
    for u in (1, 2):
        np.testing.assert_array_equal(X1[u], br.eakf_rows(X[u], H[u], obs[u], sd[u] ** 2))


def test_hand_computed_two_rows():
    """target 0: pool a = 1, 2, 3, 4 (var 5/3), observed directly with R = 5/3 and y = 4.5: D = 10/3, K = 1/2, alpha =
    1 / (1 + sqrt(1/2)): a -> 3.5 + (1 - alpha / 2)(a - 2.5), variance 5/6.  Then site 1's row h = -a (before the first update)
    with sd^2 = 5/12 and rho 1/2, so R = 5/6, y = -2: the private copy became -3.5 - (1 - alpha / 2)(a - 2.5), variance 5/6,
    cov(a, h) = -5/6, D = 5/3, K = -1/2, alpha2 = alpha, innovation 1.5: a -> 2.75 + (1 - alpha / 2)^2 (a - 2.5)"""
    a = np.array([1.0, 2.0, 3.0, 4.0])
    X = np.stack([a[:, None], 7.0 + a[:, None]])
    H = np.stack([a[:, None], -a[:, None]])
    obs = np.array([[4.5], [-2.0]])
    sd = np.array([[np.sqrt(5.0 / 3.0)], [np.sqrt(5.0 / 12.0)]])
    ptr, nbr, rho = np.array([0, 0, 1]), np.array([0], np.int32), np.array([0.5])
    live = np.ones((2, 4), dtype=bool)
    X1, rows = br.update(X, H, live, np.array([1, 1]), obs, sd, ptr, nbr, rho)
    alpha = 1.0 / (1.0 + np.sqrt(0.5))
    np.testing.assert_allclose(X1[0, :, 0], 2.75 + (1.0 - 0.5 * alpha) ** 2 * (a - 2.5), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(rows, [[2, 0], [1, 0]])
    # site 1 sees its own row only (site 0 does not list it): the per-site update
    np.testing.assert_array_equal(X1[1], er.eakf(X[1], H[1], obs[1], sd[1]))


def test_a_target_ignores_what_is_out_of_its_reach():
    rng = np.random.default_rng(31)
    n_sites, M = 7, 40
    st = batch_state(rng, n_sites, M, dead=0.0)
    obs, sd = observations(rng, st, n_sites)
    # 1 and 2 list 0; 4 lists 3; 5 and 6 list each other: target 0 is reached from 1 and 2 only
    ptr, nbr, rho = np.array([0, 0, 1, 2, 2, 3, 4, 5]), np.array([0, 0, 3, 6, 5], np.int32), np.array([0.9, 0.4, 0.8, 0.6, 0.6])

    def run(state, o):
        return br.analysis(state, state[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, o, sd, ptr, nbr, rho)

    base, info, rows = run(st, obs)
    assert list(rows[:, 0]) == [12, 4, 4, 8, 4, 8, 8] and (info[:, 0] == 1).all()
    o2 = obs.copy()
    o2[4, 1] += 3.0 * sd[4, 1]                                        # an observation out of 0's reach
    o2[5, 0] = np.nan
    other, _, _ = run(st, o2)
    np.testing.assert_array_equal(other[:M], base[:M])
    np.testing.assert_array_equal(other[M:3 * M], base[M:3 * M])
    assert np.abs(other[3 * M:4 * M] - base[3 * M:4 * M]).max() > 0   # (site 3 is in that observation's reach)
    st2 = st.copy()
    st2[6 * M:6 * M + 9, 29] = 1                                      # dead members at a site out of 0's reach
    third, _, rows3 = run(st2, obs)
    np.testing.assert_array_equal(third[:3 * M], base[:3 * M])
    assert list(rows3[5]) == [4, 4] and list(rows3[6]) == [8, 0]      # 5 lives where 6 is dead: 6's rows are dropped there
    np.testing.assert_array_equal(third[4 * M:5 * M], base[4 * M:5 * M])
    o3 = obs.copy()
    o3[2, 3] += sd[2, 3]                                              # (and one within its reach does move it)
    moved, _, _ = run(st, o3)
    assert np.abs(moved[:M] - base[:M]).max() > 0


def test_a_source_missing_a_member_is_dropped_where_that_member_lives():
    rng = np.random.default_rng(41)
    n_sites, M = 3, 32
    st = batch_state(rng, n_sites, M)
    st[M + 5, 29] = 1                                                 # member 5 is dead at site 1 only
    obs, sd = observations(rng, st, n_sites)
    ptr, nbr, rho = complete(n_sites, 0.6)
    got, info, rows = br.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, ptr, nbr, rho)
    np.testing.assert_array_equal(rows, [[8, 4], [12, 0], [8, 4]])
    assert list(info[:, 2]) == [M, M - 1, M]
    # with site 1 out of the lists (and every other row as before) sites 0 and 2 end the same
    ptr2, nbr2, rho2 = np.array([0, 1, 1, 2]), np.array([2, 0], np.int32), np.array([0.6, 0.6])
    alone, _, rows2 = br.analysis(st, st[:, 29], np.ones(n_sites), n_sites, OPS, ANALYSED, obs, sd, ptr2, nbr2, rho2)
    np.testing.assert_array_equal(rows2, [[8, 0], [4, 0], [8, 0]])
    np.testing.assert_array_equal(got[:M], alone[:M])
    np.testing.assert_array_equal(got[2 * M:], alone[2 * M:])
    np.testing.assert_array_equal(got[M + 5], st[M + 5])              # the dead member is untouched
