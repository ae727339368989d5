"""The joint state-parameter ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_joint), host side: the C-ABI
boundary, sipnet_enkf_params_check through ctypes, and the numpy reference (tests/enkf_joint_reference.py) that
tests/test_gpu_enkf_joint.py holds the kernels to, pinned by the textbook augmented Kalman update."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_joint_reference as jr
from tests import enkf_reference as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(params, want_bounds=True):
    """sipnet_enkf_params_check on (index, lo, hi) tuples -> (rc, message, lo_converted, hi_converted)"""
    L = sa.lib()
    n = len(params)
    arr = (_lib.EnkfParam * max(n, 1))(*[_lib.EnkfParam(int(i), 0, float(lo), float(hi)) for i, lo, hi in params])
    lo, hi = (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))()
    rc = L.sipnet_enkf_params_check(n, arr, lo if want_bounds else None, hi if want_bounds else None)
    return rc, L.sipnet_last_error().decode(), np.array(lo[:n]), np.array(hi[:n])


def index(name):
    return sa.config.param_index(name)


def test_header_declares_and_library_exports_the_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sipnet_amd.h")).read(), flags=re.S)
    for name in ("sipnet_enkf_params_check", "sipnet_batch_enkf_analysis_joint", "sipnet_batch_get_params"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(sa.lib(), name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define SIPNET_ENKF_MAX_PARAMS 16\b", hdr)
    assert sa.ENKF_MAX_PARAMS == 16


def test_struct_layout_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "sipnet_amd.h")).read()
    body = re.search(r"typedef struct sipnet_enkf_param \{(.*?)\} sipnet_enkf_param;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ty, names in re.findall(r"(int32_t|double)\s+([\w, ]+);", body):
        fields += [(ty, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in _lib.EnkfParam._fields_]
    off = 0
    for ty, name in fields:
        size = 4 if ty == "int32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(_lib.EnkfParam, name).offset == off, name
        off += size
    assert C.sizeof(_lib.EnkfParam) == 24 == off


def test_enkf_param_helper():
    p = sa.enkf_param("aMax", 1.0, 30.0)
    assert (p.index, p.reserved, p.lo, p.hi) == (index("aMax"), 0, 1.0, 30.0)
    with pytest.raises(ValueError):
        sa.enkf_param("noSuchParameter", 0.0, 1.0)


def test_null_batch_is_a_bad_argument():
    L = sa.lib()
    ops = (_lib.EnkfObs * 1)(sa.enkf_pools(["plantWoodC"]))
    rc = L.sipnet_batch_enkf_analysis_joint(None, 1, ops, 1, 0, None, None, 0, 0, 0, None, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_enkf_analysis_joint" in L.sipnet_last_error()
    assert L.sipnet_batch_get_params(None, None, 0, None) == _lib.ERR_BAD_ARGUMENT


def test_the_reference_tables_name_the_rows_of_the_parameter_file_order():
    names = {"psnTMin": jr.PSN_TMIN, "psnTOpt": jr.PSN_TOPT, "leafAllocation": jr.LEAF_ALLOC, "woodAllocation": jr.WOOD_ALLOC,
             "fineRootAllocation": jr.FINE_ALLOC}
    for name, row in names.items():
        assert index(name) == row, name
    rates = ["baseVegResp", "litterBreakdownRate", "baseSoilResp", "woodTurnoverRate", "leafTurnoverRate",
             "fineRootTurnoverRate", "coarseRootTurnoverRate", "baseCoarseRootResp", "baseFineRootResp"]
    assert sorted(index(n) for n in rates) == sorted(jr.RATE_ROWS)
    inits = ["plantWoodInit", "laiInit", "soilInit", "soilWFracInit", "litterInit", "snowInit", "mineralNInit", "soilOrgNInit",
             "litterOrgNInit", "plantStorageNInit"]
    assert sorted(index(n) for n in inits) == sorted(jr.INIT_ROWS)
    assert sorted(index(n) for n in ["leafOnDay", "leafOffDay", "gddLeafOn", "soilTempLeafOn"]) == sorted(jr.PHENOLOGY_ROWS)
    assert sorted(index(n) for n in ["fAnoxia", "anaerobicDecompRate"]) == sorted(jr.CLAMPED_ROWS)
    unnamed = [i for i in range(80) if sa.lib().sipnet_param_name(i) == b""]
    assert sorted(unnamed) == sorted(jr.DERIVED_ROWS)


# ---- sipnet_enkf_params_check -----------------------------------------------------------------------------------------
def test_params_check_accepts_identity_and_rate_rows_and_converts_the_bounds_exactly():
    lo_rate, hi_rate = 0.0021, 0.0617
    rc, _, lo, hi = check([(index("aMax"), 0.3, 34.0), (index("baseVegResp"), lo_rate, hi_rate), (index("soilWHC"), 0.1, 36.0)])
    assert rc == 0
    assert lo[0].tobytes() == np.float64(0.3).tobytes() and hi[0].tobytes() == np.float64(34.0).tobytes()
    assert lo[1].tobytes() == (np.float64(lo_rate) / np.float64(365.0)).tobytes()
    assert hi[1].tobytes() == (np.float64(hi_rate) / np.float64(365.0)).tobytes()
    assert lo[2].tobytes() == np.float64(0.1).tobytes() and hi[2].tobytes() == np.float64(36.0).tobytes()
    want_rows, want_lo, want_hi = jr.converted_bounds([(index("aMax"), 0.3, 34.0), (index("baseVegResp"), lo_rate, hi_rate)])
    assert want_lo.tobytes() == lo[:2].tobytes() and want_hi.tobytes() == hi[:2].tobytes()
    assert check([(index("aMax"), 0.3, 34.0)], want_bounds=False)[0] == 0
    assert check([])[0] == 0


def test_params_check_accepts_every_row_it_does_not_name_as_refused():
    refused = set(jr.DERIVED_ROWS + jr.INIT_ROWS + jr.PHENOLOGY_ROWS + jr.CLAMPED_ROWS)
    for i in range(80):
        rc, msg, lo, _ = check([(i, 1.0, 2.0)])
        assert (rc != 0) == (i in refused), (i, msg)
        if rc == 0:
            want = np.float64(1.0) / np.float64(365.0) if i in jr.RATE_ROWS else np.float64(1.0)
            assert lo[0].tobytes() == want.tobytes(), i
    rc, _, _, _ = check([(i, 0.0, 1.0) for i in range(80) if i not in refused][:16])
    assert rc == 0


@pytest.mark.parametrize("rows, word", [(jr.DERIVED_ROWS, "derived"), (jr.INIT_ROWS, "initial condition"),
                                        (jr.PHENOLOGY_ROWS, "phenology"), (jr.CLAMPED_ROWS, "clamps")])
def test_params_check_refuses_each_class_by_name(rows, word):
    L = sa.lib()
    for i in rows:
        rc, msg, _, _ = check([(index("aMax"), 1.0, 2.0), (i, 0.0, 1.0)])
        assert rc == _lib.ERR_BAD_ARGUMENT
        assert "sipnet_enkf_params_check" in msg and word in msg, msg
        field = {jr.PSN_TMAX: "psnTMax", jr.COARSE_ALLOC: "coarseRootAllocation", 60: "minNInit"}.get(
            i, L.sipnet_param_name(i).decode())
        assert field in msg, msg


def test_params_check_refuses_duplicates_counts_indices_and_bad_bounds():
    a, q = index("aMax"), index("vegRespQ10")
    for params, word in [([(a, 1.0, 2.0), (q, 1.0, 2.0), (a, 1.5, 3.0)], "twice"),
                         ([(80, 0.0, 1.0)], "index"), ([(-1, 0.0, 1.0)], "index"),
                         ([(a, np.nan, 1.0)], "finite"), ([(a, 0.0, np.inf)], "finite"), ([(a, -np.inf, 1.0)], "finite"),
                         ([(a, 2.0, 2.0)], "lo < hi"), ([(a, 3.0, 2.0)], "lo < hi")]:
        rc, msg, _, _ = check(params)
        assert rc == _lib.ERR_BAD_ARGUMENT and word in msg, (params, msg)
    names = [n for n in sa.config._load_names() if n and index(n) not in
             set(jr.DERIVED_ROWS + jr.INIT_ROWS + jr.PHENOLOGY_ROWS + jr.CLAMPED_ROWS)]
    rc, msg, _, _ = check([(index(n), 0.0, 1.0) for n in names[:17]])
    assert rc == _lib.ERR_BAD_ARGUMENT and "0..16" in msg
    L = sa.lib()
    assert L.sipnet_enkf_params_check(-1, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.sipnet_enkf_params_check(1, None, None, None) == _lib.ERR_BAD_ARGUMENT


# ---- the reference against the textbook augmented Kalman update -----------------------------------------------------------
def augmented_case(seed, n=300):
    """three pools and two parameters, jointly Gaussian and correlated; two operators linear in the pools"""
    rng = np.random.default_rng(seed)
    mix = np.array([[2.0, 0.5, 0.1, 0.3, 0.0], [0.0, 1.0, 0.7, 0.0, 0.2], [0.0, 0.0, 1.5, 0.4, 0.1],
                    [0.0, 0.0, 0.0, 0.6, 0.2], [0.0, 0.0, 0.0, 0.0, 0.05]])
    Z = rng.normal(size=(n, 5)) @ mix + [5.0, 1.0, 3.0, 8.0, 0.4]
    Hm = np.array([[1.0, 0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0, 0.0]])
    return Z, Hm


def test_one_observation_equals_the_augmented_kalman_update():
    Z, Hm = augmented_case(11)
    Hm = Hm[:1]
    y, sd = np.array([6.0]), np.array([0.8])
    X, P = jr.eakf(Z[:, :3], Z[:, 3:], Z @ Hm.T, y, sd)
    got = np.concatenate([X, P], 1)
    Pf = np.cov(Z, rowvar=False, ddof=1)
    K = Pf @ Hm.T @ np.linalg.inv(Hm @ Pf @ Hm.T + np.diag(sd ** 2))
    np.testing.assert_allclose(got.mean(0), Z.mean(0) + K @ (y - Hm @ Z.mean(0)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), (np.eye(5) - K @ Hm) @ Pf, rtol=0, atol=1e-10)
    assert np.abs(K[3:]).min() > 1e-3      # (the parameters do move: their covariance with h is not zero)


def test_several_serial_observations_equal_the_joint_augmented_update():
    Z, Hm = augmented_case(7)
    y, sd = np.array([6.0, 3.0]), np.array([0.8, 1.3])
    X, P = jr.eakf(Z[:, :3], Z[:, 3:], Z @ Hm.T, y, sd)
    got = np.concatenate([X, P], 1)
    Pf = np.cov(Z, rowvar=False, ddof=1)
    K = Pf @ Hm.T @ np.linalg.inv(Hm @ Pf @ Hm.T + np.diag(sd ** 2))
    np.testing.assert_allclose(got.mean(0), Z.mean(0) + K @ (y - Hm @ Z.mean(0)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.cov(got, rowvar=False, ddof=1), (np.eye(5) - K @ Hm) @ Pf, rtol=0, atol=1e-10)


def test_a_nan_observation_is_skipped_and_inflation_is_per_class():
    Z, Hm = augmented_case(5, n=50)
    H = Z @ Hm.T
    X0, P0 = jr.eakf(Z[:, :3], Z[:, 3:], H, np.array([np.nan, 3.0]), np.array([0.8, 1.3]))
    X1, P1 = jr.eakf(Z[:, :3], Z[:, 3:], H[:, 1:], np.array([3.0]), np.array([1.3]))
    assert (X0 == X1).all() and (P0 == P1).all()
    nan = np.array([np.nan, np.nan])
    X, P = jr.eakf(Z[:, :3], Z[:, 3:], H, nan, np.array([1.0, 1.0]), inflation=1.0, param_inflation=1.5)
    assert (X == Z[:, :3]).all()           # (a class at 1 is left as it is, bit for bit)
    np.testing.assert_allclose(P.std(0), 1.5 * Z[:, 3:].std(0), rtol=1e-12)
    np.testing.assert_allclose(P.mean(0), Z[:, 3:].mean(0), rtol=1e-12)
    X, P = jr.eakf(Z[:, :3], Z[:, 3:], H, nan, np.array([1.0, 1.0]), inflation=2.0, param_inflation=1.0)
    assert (P == Z[:, 3:]).all()
    np.testing.assert_allclose(X.std(0), 2.0 * Z[:, :3].std(0), rtol=1e-12)


def test_without_parameters_the_reference_is_the_state_only_reference_exactly():
    rng = np.random.default_rng(2)
    n_sites, M = 3, 40
    state = np.zeros((n_sites * M, 32))
    state[:, :13] = rng.uniform(1.0, 20.0, (n_sites * M, 13))
    state[5, 29] = 1.0
    status = state[:, 29].astype(np.int32)
    prm = rng.uniform(0.5, 2.0, (n_sites * M, 80))
    ops = [(0, 1 << 1, 0, 24, 1.0), (0, 1 | (1 << 12), 0, -1, 1.0), (0, 1 << 3, 0, 23, 1.0)]
    analysed = [0, 1, 2, 3, 6, 7, 12]
    obs = rng.uniform(5.0, 15.0, (n_sites, 3))
    obs[1] = np.nan
    obs[2, 1] = np.nan
    sd = rng.uniform(0.5, 2.0, (n_sites, 3))
    infl = np.array([1.0, 1.2, 1.1])
    want, want_info = er.analysis(state, status, np.ones(n_sites), n_sites, ops, analysed, obs, sd, infl, None, prm)
    got, got_prm, info = jr.analysis(state, status, np.ones(n_sites), n_sites, ops, analysed, [], obs, sd, infl, None, None, prm)
    assert got.tobytes() == want.tobytes() and (info == want_info).all() and got_prm.tobytes() == prm.tobytes()
    # ... and the pools do not depend on the parameters being analysed next to them (every column is updated by itself)
    got2, prm2, info2 = jr.analysis(state, status, np.ones(n_sites), n_sites, ops, analysed, [(4, 0.0, 10.0), (23, 0.0, 10.0)],
                                    obs, sd, infl, None, None, prm)
    assert got2.tobytes() == want.tobytes() and (info2 == want_info).all()
    assert (prm2[:, [4, 23]] != prm[:, [4, 23]]).any()


def hand_made(n=6):
    fc = np.zeros((n, 13))
    fc[:, er.WOOD], fc[:, er.COARSE], fc[:, er.FINE], fc[:, 2] = 5.0, 1.0, 1.0, 7.0
    prm = np.tile(np.arange(80, dtype=np.float64) + 100.0, (n, 1))
    prm[:, jr.LEAF_ALLOC], prm[:, jr.WOOD_ALLOC], prm[:, jr.FINE_ALLOC] = 0.2, 0.2, 0.4
    prm[:, jr.COARSE_ALLOC] = 1 - 0.2 - 0.2 - 0.4
    prm[:, jr.PSN_TMIN], prm[:, jr.PSN_TOPT] = 2.0, 24.0
    prm[:, jr.PSN_TMAX] = 24.0 + (24.0 - 2.0)
    return fc, prm


def test_clipping_the_kept_whole_rule_and_the_derived_temperature_row():
    fc, prm = hand_made(5)
    rows, lo, hi = [4, jr.PSN_TOPT], np.array([1.0, 10.0]), np.array([9.0, 30.0])
    X = np.array([[4.0], [4.0], [-1.0], [4.0], [4.0]])                  # member 2: wood clipped to 0 -> forecast
    P = np.array([[0.5, 20.0], [12.0, 35.0], [5.0, 20.0], [np.nan, 20.0], [5.0, 26.5]])
    pools, out, kept = jr.limits(fc, X, [er.WOOD], prm, P, rows, lo, hi)
    np.testing.assert_array_equal(kept, [False, False, True, True, False])
    np.testing.assert_array_equal(out[0, rows], [1.0, 20.0])          # clipped from below
    np.testing.assert_array_equal(out[1, rows], [9.0, 30.0])          # clipped from above, both
    assert out[2].tobytes() == prm[2].tobytes() and pools[2].tobytes() == fc[2].tobytes()   # biomass: pools and parameters
    assert out[3].tobytes() == prm[3].tobytes() and pools[3].tobytes() == fc[3].tobytes()   # NaN parameter: both as well
    assert pools[0, er.WOOD] == 4.0 and pools[4, er.WOOD] == 4.0
    for j in (0, 1, 4):
        assert out[j, jr.PSN_TMAX] == out[j, jr.PSN_TOPT] + (out[j, jr.PSN_TOPT] - 2.0)
    assert out[4, jr.PSN_TMAX] == 51.0
    other = [k for k in range(80) if k not in rows + [jr.PSN_TMAX]]
    assert out[:, other].tobytes() == prm[:, other].tobytes()       # coarseRootAllocation among them: no allocation analysed


def test_the_allocation_rule_and_the_derived_allocation_row():
    fc, prm = hand_made(6)
    rows, lo, hi = [jr.LEAF_ALLOC, jr.FINE_ALLOC], np.array([0.0, 0.0]), np.array([2.0, 2.0])
    X = np.full((6, 1), 4.0)
    P = np.array([[0.25, 0.45],      # coarse = 1 - .25 - .2 - .45 = 0.1: moved
                  [0.30, 0.55],      # 1 - .3 - .2 - .55 < 0: kept
                  [1.00, 0.10],      # leaf >= 1: kept
                  [0.10, 1.50],      # fine root >= 1: kept
                  [0.40, 0.40],      # sums to 1: the sign of the rounded 1 - .4 - .2 - .4 decides, as in the conversion
                  [0.10, 0.10]])
    pools, out, kept = jr.limits(fc, X, [er.WOOD], prm, P, rows, lo, hi)
    np.testing.assert_array_equal(kept, [False, True, True, True, 1 - 0.4 - 0.2 - 0.4 < 0, False])
    for j in np.nonzero(~kept)[0]:
        assert out[j, jr.COARSE_ALLOC] == 1 - P[j, 0] - 0.2 - P[j, 1]
        np.testing.assert_array_equal(out[j, rows], P[j])
    for j in np.nonzero(kept)[0]:
        assert out[j].tobytes() == prm[j].tobytes() and pools[j].tobytes() == fc[j].tobytes()
    assert (out[:, jr.PSN_TMAX] == prm[:, jr.PSN_TMAX]).all()
    # wood allocation alone analysed: the rule reads the other two from the forecast rows
    pools, out, kept = jr.limits(fc, X, [er.WOOD], prm, np.array([[0.3], [0.5], [1.2], [0.1], [0.39], [0.0]]),
                                 [jr.WOOD_ALLOC], np.array([0.0]), np.array([2.0]))
    np.testing.assert_array_equal(kept, [False, True, True, False, False, False])


def test_site_codes_with_the_parameter_inflation():
    one = np.array([1.0])
    assert jr.site_code(one, one, 1.0, 1.0, 5) == (1, 1)
    assert jr.site_code(one, one, 1.0, 1.5, 5) == (1, 1)
    assert jr.site_code(one, one, 1.0, 0.5, 5) == (-2, 0)
    assert jr.site_code(one, one, 1.0, np.nan, 5) == (-2, 0)
    assert jr.site_code(one, one, 1.0, np.inf, 5) == (-2, 0)
    assert jr.site_code(np.array([np.nan]), one, 1.0, 0.5, 5) == (-2, 0)     # (bad input before "no observation")
    assert jr.site_code(one, one, 1.0, 1.0, 1) == (0, 0)
