"""The ensemble Kalman smoother of a window's series (sipnet_batch_enkf_analysis_smooth), host side: the C-ABI boundary, the
series descriptor's layout, and the numpy reference (tests/enkf_smooth_reference.py) that tests/test_gpu_enkf_smooth.py holds
the kernels to -- pinned by the textbook Kalman update, with the covariance-space form the kernels use held to it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_joint_reference as jr
from tests import enkf_reference as er
from tests import enkf_smooth_reference as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sipnet_amd.h")


def test_header_declares_and_library_exports_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    name = "sipnet_batch_enkf_analysis_smooth"
    assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert hasattr(sa.lib(), name)
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 18
    assert re.search(r"#define SIPNET_ENKF_MAX_SERIES 8\b", hdr)
    assert sa.ENKF_MAX_SERIES == 8 == _lib.ENKF_MAX_SERIES


def test_series_struct_layout_matches_the_header():
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct sipnet_enkf_series \{(.*?)\} sipnet_enkf_series;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const void \*|void \*|int32_t |int64_t )(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.EnkfSeries._fields_] == ["src", "dst", "rows", "elem_is_f32", "ld"]
    off = 0
    for ty, name in fields:
        size = 4 if ty.startswith("int32_t") else 8
        off = (off + size - 1) // size * size
        assert getattr(_lib.EnkfSeries, name).offset == off, name
        assert getattr(_lib.EnkfSeries, name).size == size, name
        off += size
    assert C.sizeof(_lib.EnkfSeries) == 32 == off


def test_null_batch_is_a_bad_argument():
    L = sa.lib()
    ops = (_lib.EnkfObs * 1)(sa.enkf_pools(["plantWoodC"]))
    rc = L.sipnet_batch_enkf_analysis_smooth(None, 1, ops, 1, 0, None, None, 0, 0, 0, None, None, None, None, 0, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_enkf_analysis_smooth" in L.sipnet_last_error()


def test_one_observation_is_the_textbook_update_of_mean_and_variance():
    rng = np.random.default_rng(11)
    n = 300
    V = rng.normal(size=(n, 5)) @ rng.normal(size=(5, 5)) + rng.uniform(-3, 30, 5)
    H, Z = V[:, :1], V[:, 1:]
    y, sd = np.array([H.mean() + 0.7 * H.std()]), np.array([0.8 * H.std()])
    got = sr.eakf(Z, H, y, sd)
    h = H[:, 0]
    var_h, R = h.var(ddof=1), sd[0] ** 2
    cov = ((Z - Z.mean(0)) * (h - h.mean())[:, None]).sum(0) / (n - 1)
    np.testing.assert_allclose(got.mean(0), Z.mean(0) + cov / (var_h + R) * (y[0] - h.mean()), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.var(0, ddof=1), Z.var(0, ddof=1) - cov ** 2 / (var_h + R), rtol=1e-11)


SHAPES = [(16, 4, 5, 1.0), (256, 4, 144, 1.05), (1000, 16, 30, 1.0), (37, 7, 9, 1.3), (2, 3, 4, 1.0), (4096, 16, 8, 1.1)]


@pytest.mark.parametrize("n,p,nz,lam", SHAPES)
def test_the_covariance_space_form_equals_the_member_space_filter(n, p, nz, lam):
    """members, rows, series elements, lambda; a NaN observation wherever there are more than 3 rows.  Bound: 1e-12 of
    max(|x|, ensemble sd) (measured while the form was derived: 9.0e-15 at worst)"""
    rng = np.random.default_rng(3 + n)
    B = rng.normal(size=(p + nz, p + nz + 2))
    V = rng.normal(size=(n, p + nz + 2)) @ B.T * rng.uniform(0.1, 50, p + nz) + rng.uniform(-100, 1000, p + nz)
    H, Z = V[:, :p], V[:, p:]
    y = H.mean(0) + H.std(0) * rng.normal(size=p)
    sd = H.std(0) * rng.uniform(0.3, 2, p) + 1e-3
    if p > 3:
        y[2] = np.nan
    a, b = sr.eakf(Z, H, y, sd, lam), sr.weights_form(Z, H, y, sd, lam)
    scale = np.maximum(np.abs(a), Z.std(0) + 1e-300)
    worst = float((np.abs(a - b) / scale).max())
    print(f"n={n} p={p} nz={nz} lambda={lam}: largest |member space - covariance space| / scale = {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12
    assert np.abs(a - Z).max() > 0


def test_a_series_that_copies_a_pools_forecast_gets_the_pools_value_exactly():
    rng = np.random.default_rng(2)
    n_sites, M = 3, 40
    ncol = n_sites * M
    state = np.zeros((ncol, 32))
    state[:, :13] = rng.uniform(50, 500, (ncol, 13))
    state[[3, 2 * M + 7], 29] = 3.0
    prm = rng.uniform(1, 2, (ncol, 80))
    ops = [(0, 1 << 1, 0, -1, 1.0), (0, (1 << 0) | (1 << 12), 0, -1, 0.5), (0, 1 << 2, 0, 20, 1.0)]
    analysed = [0, 1, 2, 6, 7, 12]
    obs = np.array([[250.0, 260.0, 180.0], [np.nan] * 3, [300.0, np.nan, 150.0]])
    sd = np.full((n_sites, 3), 40.0)
    infl = np.array([1.1, 1.0, 1.0])
    series = [state[:, [2]].T.copy(), state[:, [6, 0]].T.copy()]
    out, _, info, dst = sr.analysis(state, state[:, 29], np.ones(n_sites), n_sites, ops, analysed, [], obs, sd, series, infl,
                                    None, None, prm)
    assert list(info[:, 0]) == [1, -1, 1]
    rest = np.ones(ncol, bool)
    for s in (0, 2):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[state[cols, 29] == 0]
        rest[live] = False
        fc = state[live, :13]
        H = np.stack([er.predicted(op, fc, None, lambda k: prm[live, k]) for op in ops], 1)
        X = er.eakf(np.ascontiguousarray(fc[:, analysed]), H, obs[s], sd[s], infl[s])      # the pools alone, as the filter has them
        np.testing.assert_array_equal(dst[0][0, live], X[:, analysed.index(2)])
        np.testing.assert_array_equal(dst[1][0, live], X[:, analysed.index(6)])
        np.testing.assert_array_equal(dst[1][1, live], X[:, analysed.index(0)])
        assert (dst[0][0, live] != series[0][0, live]).any()
    assert rest.sum() == M + 2
    np.testing.assert_array_equal(dst[0][:, rest], series[0][:, rest])
    np.testing.assert_array_equal(dst[1][:, rest], series[1][:, rest])
