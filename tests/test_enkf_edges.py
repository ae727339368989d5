"""The yardsticks of tests/test_gpu_enkf_edges.py, host side (tests/enkf_exact_reference.py): the extended-precision serial
update against the float64 references, the float64 covariance-space restatement against them, both against the textbook batch
Kalman update; every case of the conditioning ladder under the cap of 1e-7; and the degenerate inputs (no spread in h,
identical members, two live members, one) through the existing references, with their codes and kept counts.

The order of the two bounds: at off = 1 the covariance-space restatement is the less accurate of the two on every rung
(bound "member" <= bound "cov" is asserted).  At off = 1e6 it is the other way round on the collinear rungs with a small R
(eps 1e-3, c 1e-4, 32 rows: member space about 4.4e-10, covariance space about 6.9e-12): the member-space update subtracts a
mean of 1e6 from members of 1e6 again at every row, the covariance-space one centres once.  There the order is not asserted;
the cap is, for both."""
import numpy as np
import pytest

from tests import enkf_block_reference as br
from tests import enkf_exact_reference as xr
from tests import enkf_joint_reference as jr
from tests import enkf_reference as er
from tests import enkf_smooth_reference as sr

IDS = [c["name"] for c in xr.ladder()]


def random_case(seed, n=80, nA=5, p=6, nan=()):
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(n, nA + p)) @ (rng.normal(size=(nA + p, nA + p)) + 2.0 * np.eye(nA + p)) + 5.0
    X, H = Z[:, :nA], Z[:, nA:]
    y = H.mean(0) + H.std(0) * rng.normal(size=p)
    y[list(nan)] = np.nan
    sd = H.std(0) * rng.uniform(0.5, 2.0, p)
    return X, H, y, sd


@pytest.mark.parametrize("seed", range(4))
def test_the_long_double_update_equals_the_float64_references(seed):
    X, H, y, sd = random_case(seed, nan=(2,) if seed % 2 else ())
    truth = xr.eakf_ld(X, H, y, sd ** 2)
    assert truth.dtype == np.float64
    for got in (er.eakf(X, H, y, sd), br.eakf_rows(X, H, y, sd ** 2)):
        assert xr.error(got, truth, X) <= 1e-13
    assert np.abs(truth - X).max() > 1e-3


@pytest.mark.parametrize("seed", range(4))
def test_the_covariance_space_restatement_equals_the_member_space_reference(seed):
    X, H, y, sd = random_case(seed, nan=(0, 3) if seed % 2 else ())
    D = []
    got = xr.cov_chain64(X, H, y, sd ** 2, D)
    assert xr.error(got, br.eakf_rows(X, H, y, sd ** 2), X) <= 1e-12
    assert len(D) == int((~np.isnan(y)).sum()) and min(D) > 0
    # ... and the smoother's weights form of the same chain
    assert xr.error(got, sr.weights_form(X, H, y, sd), X) <= 1e-12


def test_both_agree_with_the_batch_kalman_update_on_two_rows():
    rng = np.random.default_rng(5)
    n, nA = 300, 3
    Z = rng.normal(size=(n, nA + 2)) @ (rng.normal(size=(nA + 2, nA + 2)) + 2.0 * np.eye(nA + 2)) + 5.0
    X, H = Z[:, :nA], Z[:, nA:]
    y = H.mean(0) + rng.normal(size=2)
    R = np.array([0.7, 1.9])
    P = np.cov(Z, rowvar=False, ddof=1)
    Pxy, Pyy, Pxx = P[:nA, nA:], P[nA:, nA:], P[:nA, :nA]
    K = Pxy @ np.linalg.inv(Pyy + np.diag(R))
    mean = X.mean(0) + K @ (y - H.mean(0))
    cov = Pxx - K @ Pxy.T
    for got in (xr.eakf_ld(X, H, y, R), xr.cov_chain64(X, H, y, R)):
        np.testing.assert_allclose(got.mean(0), mean, rtol=1e-10, atol=0)
        np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), cov, rtol=1e-10, atol=1e-10 * np.abs(cov).max())


def test_the_ladder_is_what_the_issue_lists():
    cases = xr.ladder()
    assert len(cases) == len(set(IDS)) == 32
    assert {(c["eps"], c["c"]) for c in cases} == {(1.0, 1.0), (1.0, 1e-2), (1.0, 1e-4), (1e-3, 1.0), (1e-3, 1e-2), (1e-3, 1e-4),
                                                   (0.0, 1.0), (0.0, 1e-2)}
    assert {c["off"] for c in cases} == {1.0, 1e6} and {c["p"] for c in cases} == {4, 32}
    for c in cases:
        assert c["X"].shape == (64, 3) and c["H"].shape == (64, c["p"]) and c["y"].shape == c["R"].shape == (c["p"],)
        if c["eps"] == 0.0:
            assert (c["H"] == c["H"][:, :1]).all()
        spread = c["H"].std(0)
        np.testing.assert_allclose(c["R"], (c["c"] * spread) ** 2, rtol=1e-15)
    again = xr.make_case(1e-3, 1e-2, 1.0, 4)                           # fixed seeds
    np.testing.assert_array_equal(again["H"], xr.case_named("eps0.001-c0.01-off1-p4")["H"])


@pytest.mark.parametrize("name", IDS)
def test_every_ladder_case_is_under_the_cap(name):
    case = xr.case_named(name)
    member, cov = xr.bound(case, "member"), xr.bound(case, "cov")
    print(f"{name}: bound member {member:.3e}, cov {cov:.3e} (cap {xr.CAP:g})")
    assert 1e-10 <= member <= xr.CAP and 1e-10 <= cov <= xr.CAP
    if case["off"] == 1.0:                                             # (the module docstring: why not at off = 1e6)
        assert member <= cov
    D = []
    a = br.eakf_rows(case["X"], case["H"], case["y"], case["R"])
    b = xr.cov_chain64(case["X"], case["H"], case["y"], case["R"], D)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert len(D) == case["p"] and min(D) > 0
    assert np.abs(a - case["X"]).max() > 0


def test_the_steps_left_out_of_the_ladder_are_beyond_the_cap():
    """eps = 1e-6 with c <= 1e-4, and c = 1e-6: 4 x the covariance-space own error at off = 1 is beyond the cap of 1e-7 or
    (eps 1e-3, c 1e-6: 4e-8) within 4 x of it, closer than one ordering of the members varies"""
    for eps, c in xr.BEYOND_THE_CAP:
        worst = max(xr.own_error(xr.cov_chain64, xr.make_case(eps, c, 1.0, p), k=4) for p in (4, 32))
        print(f"eps {eps:g}, c {c:g}: covariance-space own error {worst:.3e}")
        assert xr.FACTOR * worst > xr.CAP / 4


# ---- degenerate inputs through the existing references -----------------------------------------------------------------------
ANALYSED = [1, 2, 12]
OPS = [(0, 1 << 4, 0, -1, 1.0), (0, 1 << 5, 0, -1, 1.0)]


def flat_state(rng, M, live):
    st = np.zeros((M, 32))
    st[:, :13] = 100.0 + rng.normal(size=(M, 13))
    st[:, 29] = 1.0
    st[list(live), 29] = 0.0
    return st


def every_reference(st, obs, sd):
    """(state after, info) of one site through the per-site, joint, block-local (no neighbours) and smoother references"""
    one, ptr = np.ones(1), np.zeros(2, dtype=np.int64)
    out = [er.analysis(st, st[:, 29], one, 1, OPS, ANALYSED, obs, sd)]
    j = jr.analysis(st, st[:, 29], one, 1, OPS, ANALYSED, [], obs, sd, prm=np.zeros((st.shape[0], 80)))
    out.append((j[0], j[2]))
    b = br.analysis(st, st[:, 29], one, 1, OPS, ANALYSED, obs, sd, ptr, np.zeros(0, np.int32), np.zeros(0))
    out.append((b[0], b[1]))
    z = np.arange(3.0 * st.shape[0]).reshape(3, -1)
    s = sr.analysis(st, st[:, 29], one, 1, OPS, ANALYSED, [], obs, sd, [z], prm=np.zeros((st.shape[0], 80)))
    out.append((s[0], s[2]))
    return out, z, s[3][0]


def test_no_spread_in_h_leaves_everything():
    rng = np.random.default_rng(1)
    st = flat_state(rng, 40, range(40))
    st[:, 4] = 7.0                                                     # var_h = 0 in the first row
    st[:, 5] = 3.0
    results, z, z1 = every_reference(st, np.array([[9.0, 1.0]]), np.array([[0.5, 0.5]]))
    for out, info in results:
        assert list(info[0]) == [1, 2, 40, 0]
        np.testing.assert_array_equal(out, st)
    np.testing.assert_array_equal(z1, z)
    X, H = st[:, ANALYSED], st[:, [4, 5]]
    np.testing.assert_array_equal(xr.cov_chain64(X, H, np.array([9.0, 1.0]), np.array([0.25, 0.25])), X)
    np.testing.assert_array_equal(xr.eakf_ld(X, H, np.array([9.0, 1.0]), np.array([0.25, 0.25])), X)


def test_identical_members_stay():
    st = flat_state(np.random.default_rng(2), 33, range(33))
    st[:, :13] = st[0, :13]
    results, z, z1 = every_reference(st, np.array([[120.0, 90.0]]), np.array([[0.5, 2.0]]))
    for out, info in results:
        assert list(info[0]) == [1, 2, 33, 0]
        np.testing.assert_array_equal(out, st)


@pytest.mark.parametrize("live", [(3, 200), (255, 256), (0, 256)])
def test_two_live_members_among_257(live):
    rng = np.random.default_rng(3)
    st = flat_state(rng, 257, live)
    obs, sd = np.array([[101.0, np.nan]]), np.array([[0.3, 1.0]])
    results, z, z1 = every_reference(st, obs, sd)
    dead = st[:, 29] != 0
    X = xr.eakf_ld(st[list(live)][:, ANALYSED], st[list(live)][:, [4, 5]], obs[0], sd[0] ** 2)
    for out, info in results:
        assert list(info[0]) == [1, 1, 2, 0]
        np.testing.assert_array_equal(out[dead], st[dead])
        assert xr.error(out[list(live)][:, ANALYSED], X, st[list(live)][:, ANALYSED]) <= 1e-13
        assert np.abs(out[list(live)][:, ANALYSED] - st[list(live)][:, ANALYSED]).max() > 1e-3
    np.testing.assert_array_equal(z1[:, dead], z[:, dead])
    assert (z1[:, list(live)] != z[:, list(live)]).any()


def test_one_live_member_is_code_0():
    st = flat_state(np.random.default_rng(4), 257, (256,))
    results, z, z1 = every_reference(st, np.array([[101.0, 99.0]]), np.array([[0.3, 1.0]]))
    for out, info in results:
        assert list(info[0]) == [0, 0, 1, 0]
        np.testing.assert_array_equal(out, st)
    np.testing.assert_array_equal(z1, z)
