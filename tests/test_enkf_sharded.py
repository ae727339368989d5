"""The yardsticks of tests/test_gpu_enkf_sharded.py, host side (tests/enkf_sharded_reference.py): the covariance-space update
with its moments formed per shard and merged equals the member-space reference on the union for cuts into 1, 2 and 3 shards
(shards of 0 and 1 member among them); the layout of the union; sipnet_enkf_moment_words; and the conditioning set under the
cap of tests/enkf_exact_reference.py."""
import numpy as np
import pytest

import sipnet_amd as sa
from tests import enkf_block_reference as br
from tests import enkf_exact_reference as xr
from tests import enkf_sharded_reference as shr
from tests.test_enkf_edges import random_case

CUTS = [(), (40,), (0,), (80,), (1,), (79,), (30, 55), (0, 1), (1, 1), (79, 80), (40, 40), (1, 2)]


@pytest.mark.parametrize("cuts", CUTS, ids=[str(c) for c in CUTS])
@pytest.mark.parametrize("seed", range(3))
def test_merged_moments_give_the_member_space_update_of_the_union(seed, cuts):
    X, H, y, sd = random_case(seed, nan=(2,) if seed == 1 else ())
    want = br.eakf_rows(X, H, y, sd ** 2)
    got = shr.merged_chain64(X, H, y, sd ** 2, cuts)
    assert xr.error(got, want, X) <= 1e-10
    assert np.abs(want - X).max() > 1e-3


def test_one_shard_is_the_covariance_space_restatement():
    X, H, y, sd = random_case(7)
    assert xr.error(shr.merged_chain64(X, H, y, sd ** 2), xr.cov_chain64(X, H, y, sd ** 2), X) <= 1e-13


def test_the_merge_is_the_union_moments_at_a_large_offset():
    """centred on the shards' own means the spread survives pool means of 1e6: raw sums would lose it"""
    rng = np.random.default_rng(3)
    V = 1e6 + rng.normal(size=(200, 6))
    blocks = [shr.shard_moments(V[a:b], 4) for a, b in ((0, 1), (1, 1), (1, 90), (90, 200))]
    n, mean, C = shr.merge(blocks, 4)
    A = V.astype(np.longdouble) - V.astype(np.longdouble).mean(0)
    truth = (A.T @ A[:, 4:]).astype(np.float64)
    assert n == 200 and np.abs(mean - V.mean(0)).max() <= 1e-9
    assert np.abs(C - truth).max() <= 1e-9 * np.abs(truth).max()


def test_interleave_and_split_are_inverse_and_site_major():
    n_sites, sizes = 3, (2, 0, 5, 1)
    shards = [np.arange(n_sites * m * 2, dtype=np.float64).reshape(n_sites * m, 2) + 1000 * r for r, m in enumerate(sizes)]
    u = shr.interleave(shards, n_sites)
    assert u.shape == (n_sites * sum(sizes), 2)
    site1 = u[sum(sizes):2 * sum(sizes)]
    np.testing.assert_array_equal(site1[:2], shards[0][2:4])
    np.testing.assert_array_equal(site1[2:7], shards[2][5:10])
    np.testing.assert_array_equal(site1[7:], shards[3][1:2])
    for a, b in zip(shr.split(u, n_sites, sizes), shards):
        np.testing.assert_array_equal(a, b)


def test_moment_words_values_and_refusals():
    L = sa.lib()
    for nA, n_obs in ((1, 1), (7, 4), (13, 16), (1, 16), (13, 1)):
        V = nA + n_obs
        assert L.sipnet_enkf_moment_words(nA, n_obs) == 2 + V + V * n_obs == shr.moment_words(nA, n_obs)
    assert L.sipnet_enkf_moment_words(13, 16) == 495
    for nA, n_obs in ((0, 1), (14, 1), (1, 0), (1, 17), (-1, 4), (4, -1)):
        assert L.sipnet_enkf_moment_words(nA, n_obs) == -1


CONDITIONING = shr.conditioning_set()


def test_the_conditioning_set_is_what_the_issue_lists():
    assert len(CONDITIONING) == 16 + 14
    p16 = [c for c in CONDITIONING if c["p"] == 16]
    assert {(c["eps"], c["c"]) for c in p16} == set(xr.RUNGS) - {(1e-3, 1e-4)} and {c["off"] for c in p16} == {1.0, 1e6}
    assert all(c["p"] == 4 for c in CONDITIONING[:16])


@pytest.mark.parametrize("case", CONDITIONING, ids=[c["name"] for c in CONDITIONING])
def test_every_conditioning_case_is_under_the_cap(case):
    """max(1e-10, 4 x own_error(merged_chain64 with these cuts, case)) <= CAP for the cuts at 1/2, (0.2, 0.55) and
    (1/64, 2/64, 1/2): a shard of one member and one of two among them"""
    for fractions in shr.CONDITIONING_CUTS:
        own = shr.own_error(case, fractions)
        print(f"{case['name']} cuts {fractions}: own error {own:.2e}")
        assert max(xr.FLOOR, xr.FACTOR * own) <= xr.CAP
