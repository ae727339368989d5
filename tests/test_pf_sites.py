"""The particle-filter analysis of a batch of many sites (sipnet_batch_pf_analysis_sites), host side: the C-ABI boundary, and
the per-site numpy reference that tests/test_gpu_pf_sites.py holds the kernels to -- oracle/pf_oracle.py applied to every
site's columns on its own (its own maximum, prefix sum and draw), pinned here by a hand-computed case."""
import ctypes as C
import math
import os
import re

import numpy as np

import sipnet_amd as sa
from oracle import pf_oracle as po
from sipnet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sites_reference(logw, n_sites, u0, fixed=None):
    """logw [n_sites * M] (site-major columns) -> (fixed-point weights [ncol], ancestors [ncol] as global columns, site totals
    [n_sites]), every site resampled over its own columns.  fixed given (the device's integers): the ancestors for those.
    A site whose weights are all zero keeps its particles (total 0)."""
    logw = np.asarray(logw, dtype=np.float64)
    M = len(logw) // n_sites
    u0 = np.broadcast_to(np.asarray(u0, dtype=np.float64), (n_sites,))
    fx = np.zeros(len(logw), dtype=np.int64)
    anc = np.zeros(len(logw), dtype=np.int32)
    tot = np.zeros(n_sites, dtype=np.int64)
    for s in range(n_sites):
        sl = slice(s * M, (s + 1) * M)
        with np.errstate(invalid="ignore"):
            w = po.fixed_weights(logw[sl]) if fixed is None else np.asarray(fixed[sl], dtype=np.int64)
        fx[sl] = w
        tot[s] = int(w.sum())
        anc[sl] = s * M + (po.systematic_ancestors(w, float(u0[s])) if tot[s] > 0 else np.arange(M))
    return fx, anc, tot


def test_header_declares_and_library_exports_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sipnet_amd.h")).read(), flags=re.S)
    assert re.search(r"\bsipnet_batch_pf_analysis_sites\s*\(", hdr)
    assert hasattr(sa.lib(), "sipnet_batch_pf_analysis_sites")
    assert "sipnet_batch_pf_analysis_sites" in _lib.SIGNATURES


def test_null_batch_is_a_bad_argument():
    L = sa.lib()
    rc = L.sipnet_batch_pf_analysis_sites(None, None, 0, 48, 64, None, None, None, 0, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_pf_analysis_sites" in L.sipnet_last_error()


def test_per_site_reference_against_a_hand_computed_case():
    """2 sites x 4 particles.  Site 0: weights 2^30, 0, 2^29, 2^30 (S = 2.5 * 2^30), u0 = 0.5: the pointers (j + 0.5) S / 4 =
    0.3125, 0.9375, 1.5625, 2.1875 (x 2^30) against cdf 1, 1, 1.5, 2.5 -> slots 0 0 3 3.  Site 1 lies a million log-units
    lower, weights 2^30, 2^29, 0 (e^-50 2^30 < 0.5), 2^30, u0 = 0.1: pointers 0.0625, 0.6875, 1.3125, 1.9375 against cdf 1, 1.5,
    1.5, 2.5 -> slots 0 0 1 3, i.e. global columns 4 4 5 7.  One maximum over both sites would leave site 1 no weight at all."""
    ln2 = math.log(2.0)
    logw = np.array([0.0, -np.inf, -ln2, 0.0, -1e6, -1e6 - ln2, -1e6 - 50.0, -1e6])
    fx, anc, tot = sites_reference(logw, 2, [0.5, 0.1])
    g = 1 << 30
    np.testing.assert_array_equal(fx, [g, 0, g // 2, g, g, g // 2, 0, g])
    np.testing.assert_array_equal(tot, [5 * g // 2, 5 * g // 2])
    np.testing.assert_array_equal(anc, [0, 0, 3, 3, 4, 4, 5, 7])
    with np.errstate(over="ignore"):
        assert po.fixed_weights(logw)[4:].sum() == 0            # the global maximum's weights for site 1
    # given integers are used as they are; a site with no weight keeps its particles
    fx2, anc2, tot2 = sites_reference(logw, 2, [0.5, 0.1], fixed=np.array([0, 0, 0, 0, 1, 0, 0, 1]))
    np.testing.assert_array_equal(tot2, [0, 2])
    np.testing.assert_array_equal(anc2, [0, 1, 2, 3, 4, 4, 7, 7])
