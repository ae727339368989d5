"""The ensemble Kalman filter analysis of a batch of many sites (sipnet_batch_enkf_analysis_sites), host side: the C-ABI
boundary, and the numpy reference (tests/enkf_reference.py) that tests/test_gpu_enkf_sites.py holds the kernels to, pinned
by a hand-computed case and by the textbook Kalman formulas."""
import ctypes as C
import os
import re

import numpy as np

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_reference as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sipnet_amd.h")).read(), flags=re.S)
    assert re.search(r"\bsipnet_batch_enkf_analysis_sites\s*\(", hdr)
    assert hasattr(sa.lib(), "sipnet_batch_enkf_analysis_sites")
    assert "sipnet_batch_enkf_analysis_sites" in _lib.SIGNATURES


def test_null_batch_is_a_bad_argument():
    L = sa.lib()
    ops = (_lib.EnkfObs * 1)(sa.enkf_pools(["plantWoodC"]))
    rc = L.sipnet_batch_enkf_analysis_sites(None, 1, ops, 1, None, 0, 0, 0, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_enkf_analysis_sites" in L.sipnet_last_error()


def test_struct_layout_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "sipnet_amd.h")).read()
    body = re.search(r"typedef struct sipnet_enkf_obs \{(.*?)\} sipnet_enkf_obs;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|double)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.EnkfObs._fields_]
    off = 0
    for ty, name in fields:
        size = 4 if ty == "int32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(_lib.EnkfObs, name).offset == off, name
        off += size
    assert C.sizeof(_lib.EnkfObs) == 24 == off
    assert re.search(r"SIPNET_ENKF_POOLS = 0, SIPNET_ENKF_PLANE = 1", hdr)
    assert (_lib.ENKF_POOLS, _lib.ENKF_PLANE) == (0, 1)


def test_pool_names_and_operator_helpers():
    assert len(sa.POOLS) == 13 and sa.POOLS[0] == "plantWoodC" and sa.POOLS[12] == "plantCAccountingDelta"
    lai = sa.enkf_pools(["plantLeafC"], divide_by="leafCSpWt")
    assert (lai.kind, lai.pool_mask, lai.param, lai.scale) == (0, 2, sa.config.param_index("leafCSpWt"), 1.0)
    wood = sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"])
    assert wood.pool_mask == 1 | (1 << 12) and wood.param == -1
    nee = sa.enkf_plane("nee", scale=2.0)
    assert (nee.kind, nee.plane, nee.scale) == (1, 0, 2.0)


def test_hand_computed_four_members_two_pools_one_observation():
    """x = pools (a, b); h = a.  a = 1, 2, 3, 4 (mean 2.5, var 5/3); b = 2, 4, 6, 8 (cov(b, h) = 10/3).  R = 5/3 (sd^2):
    K_a = (5/3) / (10/3) = 1/2, K_b = 1, alpha = 1 / (1 + sqrt(1/2)).  y = 4.5: a moves by 1 (the innovation 2 times 1/2)
    and its deviations shrink by 1 - alpha / 2; b moves by 2 and its deviations 2 (a - 2.5) lose alpha (a - 2.5)."""
    X = np.array([[1.0, 2.0], [2.0, 4.0], [3.0, 6.0], [4.0, 8.0]])
    H = X[:, :1].copy()
    sd = np.sqrt(5.0 / 3.0)
    got = er.eakf(X, H, np.array([4.5]), np.array([sd]))
    alpha = 1.0 / (1.0 + np.sqrt(0.5))
    da = np.array([-1.5, -0.5, 0.5, 1.5])
    np.testing.assert_allclose(got[:, 0], 2.5 + 1.0 + da * (1.0 - 0.5 * alpha), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got[:, 1], 5.0 + 2.0 + da * (2.0 - alpha), rtol=0, atol=1e-14)


def test_directly_observed_pool_follows_the_scalar_kalman_formulas():
    rng = np.random.default_rng(3)
    x = rng.normal(10.0, 2.0, 200)
    y, sd = 13.0, 1.5
    got = er.eakf(x[:, None], x[:, None], np.array([y]), np.array([sd]))[:, 0]
    vx, R = x.var(ddof=1), sd * sd
    assert abs(got.mean() - (x.mean() / vx + y / R) / (1.0 / vx + 1.0 / R)) < 1e-12
    assert abs(got.var(ddof=1) - vx * R / (vx + R)) < 1e-12


def test_two_serial_observations_equal_the_joint_update():
    rng = np.random.default_rng(7)
    n = 300
    X = rng.normal(size=(n, 3)) @ np.array([[2.0, 0.5, 0.1], [0.0, 1.0, 0.7], [0.0, 0.0, 1.5]]) + [5.0, 1.0, 3.0]
    Hm = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 1.0]])       # two linear operators of the state
    H = X @ Hm.T
    y, sd = np.array([6.0, 3.0]), np.array([0.8, 1.3])
    got = er.eakf(X, H, y, sd)
    P = np.cov(X, rowvar=False, ddof=1)
    R = np.diag(sd ** 2)
    K = P @ Hm.T @ np.linalg.inv(Hm @ P @ Hm.T + R)
    mean = X.mean(0) + K @ (y - Hm @ X.mean(0))
    cov = (np.eye(3) - K @ Hm) @ P
    np.testing.assert_allclose(got.mean(0), mean, rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), cov, rtol=0, atol=1e-10)


def test_biomass_rule_and_clipping():
    fc = np.zeros((4, 13))
    fc[:, er.WOOD], fc[:, er.COARSE], fc[:, er.FINE], fc[:, 2] = 5.0, 1.0, 1.0, 7.0
    X = np.array([[4.0, -2.0, 0.5],     # soilC clipped to 0; fine
                  [-1.0, 3.0, 0.5],     # wood clipped to 0: fails the rule -> forecast
                  [2.0, 3.0, -3.0],     # delta stays negative: wood + delta < 0 -> forecast
                  [2.0, 3.0, -1.5]])    # delta -1.5: wood + delta = 0.5 -> fine
    analysed = [er.WOOD, 2, er.DELTA]
    out, kept = er.limits(fc, X, analysed)
    np.testing.assert_array_equal(kept, [False, True, True, False])
    np.testing.assert_array_equal(out[0, analysed], [4.0, 0.0, 0.5])
    np.testing.assert_array_equal(out[1], fc[1])
    np.testing.assert_array_equal(out[2], fc[2])
    np.testing.assert_array_equal(out[3, analysed], [2.0, 3.0, -1.5])
    roots = fc.copy()
    roots[:, er.FINE] = 0.0
    out2, kept2 = er.limits(roots, np.array([[1.0, 1.0, 0.0]] * 4), [er.WOOD, 2, er.COARSE])  # coarse roots to 0: no roots
    assert kept2.all() and (out2 == roots).all()


def test_site_codes():
    nan = np.nan
    assert er.site_code(np.array([1.0, nan]), np.array([1.0, -1.0]), 1.0, 5) == (1, 1)
    assert er.site_code(np.array([nan, nan]), np.array([1.0, 1.0]), 1.0, 5) == (-1, 0)
    assert er.site_code(np.array([np.inf]), np.array([1.0]), 1.0, 5) == (-2, 0)
    assert er.site_code(np.array([1.0]), np.array([0.0]), 1.0, 5) == (-2, 0)
    assert er.site_code(np.array([1.0]), np.array([1.0]), 0.5, 5) == (-2, 0)
    assert er.site_code(np.array([1.0]), np.array([1.0]), 1.0, 1) == (0, 0)
