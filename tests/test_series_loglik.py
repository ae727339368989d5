"""Series likelihood weights (sipnet_batch_series_loglik) and the many-site resampling from given weights
(sipnet_batch_pf_resample_sites), host side: the C-ABI boundary, the Python mirror's constants, and the numpy reference of
tests/series_loglik_reference.py pinned by hand-computed cases and by oracle/pf_oracle.log_weights' closed form."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import sipnet_amd as sa
from oracle import pf_oracle as po
from sipnet_amd import _lib
from tests.series_loglik_reference import GAUSS, LAPLACE, TILE_ROWS, Term, ess_exact, resample_reference, series_loglik

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def header():
    return open(os.path.join(REPO, "include", "sipnet_amd.h")).read()


def test_header_declares_and_library_exports_both_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ("sipnet_batch_series_loglik", "sipnet_batch_pf_resample_sites"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(sa.lib(), name), name
        assert name in _lib.SIGNATURES, name


def test_a_null_batch_is_a_bad_argument():
    L = sa.lib()
    rc = L.sipnet_batch_series_loglik(None, 1, None, 0, 64, 1, 0, None, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_series_loglik" in L.sipnet_last_error()
    rc = L.sipnet_batch_pf_resample_sites(None, None, None, None, None, 0, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_pf_resample_sites" in L.sipnet_last_error()


def test_python_constants_and_the_struct_mirror_the_header():
    text = header()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(SIPNET_LOGLIK_[A-Z_]+)\s*=\s*(\d+)", text)}
    assert enums == {"SIPNET_LOGLIK_GAUSS": 0, "SIPNET_LOGLIK_LAPLACE": 1}
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (SIPNET_LOGLIK_[A-Z_]+) (\d+)", text)}
    assert defines == {"SIPNET_LOGLIK_TILE_ROWS": 256, "SIPNET_LOGLIK_MAX_TERMS": 8}
    for name, value in {**enums, **defines}.items():
        assert getattr(sa, name[len("SIPNET_"):]) == value, name
    assert TILE_ROWS == sa.LOGLIK_TILE_ROWS and (GAUSS, LAPLACE) == (sa.LOGLIK_GAUSS, sa.LOGLIK_LAPLACE)
    # the struct: three pointers, four int32, one double, in the header's order
    body = re.search(r"typedef struct sipnet_loglik_term \{(.*?)\} sipnet_loglik_term;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.LoglikTerm._fields_]
    assert C.sizeof(_lib.LoglikTerm) == 48 and _lib.LoglikTerm.scale.offset == 40
    t = sa.loglik_term("series", "obs", "sd", kind=sa.LOGLIK_LAPLACE, scale=0.5, sum_steps=48)
    assert (t.kind, t.scale, t.sum_steps, t.held) == (1, 0.5, 48, ("series", "obs", "sd"))
    with pytest.raises(ValueError):
        sa.loglik_term(None, None, None, kind=2)


# ---- the reference against hand-computed cases -------------------------------------------------------------------------
def one_site(series, obs, sd, **kw):
    series = np.asarray(series, dtype=np.float64)
    return Term(series, np.asarray([obs], dtype=np.float64), np.asarray([sd], dtype=np.float64), **kw)


@pytest.mark.parametrize("normalise", [False, True])
def test_two_rows_and_a_gap(normalise):
    """three rows, the middle one a gap; two members.  Gauss, sd 2 and 0.5: member 0 is off by 2 and 1 -> -0.5 (1 + 4),
    member 1 by 0 and -0.5 -> -0.5 (0 + 1); the constants -(log 2 + c) - (log 0.5 + c) = -2 c.  Laplace, b 2 and 0.5:
    -(1 + 2) and -(0 + 1); the constants -log 4 - log 1."""
    series = [[3.0, 1.0], [7.0, 7.0], [2.0, 0.5]]
    obs, sd = [1.0, NAN, 1.0], [2.0, -1.0, 0.5]          # (the gap's sd is bad and is ignored)
    status = np.zeros(2)
    g = series_loglik([one_site(series, obs, sd, kind=GAUSS)], 1, status, normalise)
    c = -2 * HALF_LOG_2PI if normalise else 0.0
    np.testing.assert_allclose(g.loglik.astype(float), [-2.5 + c, -0.5 + c], rtol=1e-15)
    np.testing.assert_array_equal(g.used, [[2]])
    np.testing.assert_array_equal(g.info, [[1, 2]])
    lp = series_loglik([one_site(series, obs, sd, kind=LAPLACE)], 1, status, normalise)
    c = -math.log(4.0) if normalise else 0.0
    np.testing.assert_allclose(lp.loglik.astype(float), [-3.0 + c, -1.0 + c], rtol=1e-15)
    np.testing.assert_allclose(lp.abs_sum.astype(float), [1.0 + math.log(4.0) + 2.0, math.log(4.0) + 1.0] if normalise else [3.0, 1.0],
                               rtol=1e-15)
    # both together, with add, and a member that did not run
    both = series_loglik([one_site(series, obs, sd, kind=GAUSS), one_site(series, obs, sd, kind=LAPLACE)], 1, np.array([0, 3]),
                         normalise, add=np.array([10.0, 10.0]))
    assert float(both.loglik[0]) == pytest.approx(float(g.loglik[0] + lp.loglik[0]) + 10.0, rel=1e-15)
    assert both.loglik[1] == -np.inf and (both.parts[:, 1] == -np.inf).all()
    np.testing.assert_array_equal(both.used, [[2, 2]])
    np.testing.assert_array_equal(both.info, [[1, 4]])


def test_sum_steps_and_scale():
    """six series rows in groups of three, scale 0.5: h = 0.5 (1 + 2 + 3) = 3 and 0.5 (4 + 5 + 6) = 7.5 against 2 and 8, sd 1"""
    series = np.arange(1.0, 7.0).reshape(6, 1)
    r = series_loglik([one_site(series, [2.0, 8.0], [1.0, 1.0], scale=0.5, sum_steps=3)], 1, np.zeros(1), normalise=False)
    assert float(r.loglik[0]) == -0.5 * (1.0 + 0.25)
    assert float(r.abs_sum[0]) == 0.625


def test_a_site_with_all_gaps_and_bad_input():
    """two sites x two members.  Site 1 has no observation in any term: code -1, live members get 0 + add.  A bad sd at a
    used row is code -2 and NaN for every column of the site, dead ones too; at a gap row it is ignored."""
    series = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]])
    obs = np.array([[1.0, NAN], [NAN, NAN]])
    sd = np.array([[1.0, 0.0], [np.inf, -3.0]])
    status = np.array([0, 0, 0, 5])
    r = series_loglik([Term(series, obs, sd)], 2, status, normalise=False, add=np.array([1.0, 1.0, 1.0, 1.0]))
    np.testing.assert_array_equal(r.info, [[1, 1], [-1, 0]])
    np.testing.assert_array_equal(r.loglik.astype(float), [1.0, 0.5, 1.0, -np.inf])
    sd[0, 0] = 0.0
    r = series_loglik([Term(series, obs, sd)], 2, status, normalise=False)
    np.testing.assert_array_equal(r.info, [[-2, 0], [-1, 0]])
    assert np.isnan(r.loglik[:2]).all() and r.loglik[2] == 0 and r.loglik[3] == -np.inf
    obs[1, 1], sd[1, 1] = np.inf, 1.0                    # a non-NaN non-finite obs
    r = series_loglik([Term(series, obs, sd)], 2, status, normalise=False)
    assert r.info[1, 0] == -2 and np.isnan(r.loglik).all()


def test_one_row_is_the_filter_s_closed_form():
    """one Gauss row over the whole window, scale 1, no constants: oracle/pf_oracle.log_weights"""
    rng = np.random.default_rng(5)
    plane = rng.normal(0.0, 1.0, (48, 7))
    status = np.array([0, 0, 2, 0, 0, 0, 0])
    obs, sigma = 0.3, 1.7
    want = po.log_weights(plane, obs, sigma, status)
    got = series_loglik([one_site(plane, [obs], [sigma], sum_steps=48)], 1, status, normalise=False)
    assert (np.isneginf(want) == np.isneginf(got.loglik)).all() and np.isneginf(want).sum() == 1
    live = status == 0
    np.testing.assert_allclose(got.loglik[live].astype(float), want[live], rtol=1e-13)
    # ... and with the constants it is scipy's normal log-density, written out
    full = series_loglik([one_site(plane, [obs], [sigma], sum_steps=48)], 1, status, normalise=True)
    np.testing.assert_allclose(full.loglik[live].astype(float), want[live] - math.log(sigma) - HALF_LOG_2PI, rtol=1e-13)


def test_effective_sample_size_and_the_keep_rule():
    g = 1 << 30
    assert ess_exact([g, g, g, g]) == 4 and ess_exact([g, 0, 0, 0]) == 1 and ess_exact([0, 0]) == 0
    assert ess_exact([2, 1, 1]) == Fraction(16, 6)
    # two sites x 4: site 0 uniform (ESS 4 >= 2: kept), site 1 one heavy particle (ESS 1.47 < 2: resampled, weights reset)
    ln2 = math.log(2.0)
    logw = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -3 * ln2, -3 * ln2, -3 * ln2])
    fixed = np.array([g, g, g, g, g, g // 8, g // 8, g // 8])
    anc, tot, ess, after = resample_reference(logw, 2, [0.5, 0.5], fixed, ess_min=[2.0, 2.0])
    assert ess == [4, Fraction(121, 67)] and list(tot) == [-3, 11 * g // 8]
    np.testing.assert_array_equal(anc[:4], [0, 1, 2, 3])
    np.testing.assert_array_equal(anc[4:], [4, 4, 4, 6])   # pointers 0.17, 0.52, 0.86, 1.2 (x 2^30) against cdf 1, 1.125, 1.25, 1.375
    np.testing.assert_array_equal(after, [0.0] * 4 + [0.0] * 4)
    assert (after[:4] == logw[:4]).all()
    # without ess_min every site resamples and the log-weights stay
    anc, tot, _, after = resample_reference(logw, 2, [0.5, 0.5], fixed)
    assert (tot > 0).all() and (after == logw).all()
    np.testing.assert_array_equal(anc[:4], [0, 1, 2, 3])
