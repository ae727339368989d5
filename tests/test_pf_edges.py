"""The helpers of tests/pf_edges_reference.py, pinned without a GPU: the high-precision fixed-point weight against mpmath
and the share of points that lie within their tolerance of a rounding point; the crafted patterns' integers against the
numpy oracle at every shape the GPU tests run; two ancestor cases worked by hand; the cancelling planes."""
import numpy as np
import pytest

from oracle import pf_oracle as po
from tests import pf_edges_reference as er
from tests.series_loglik_reference import ess_exact

pytestmark = pytest.mark.skipif(not er.longdouble_is_wide(), reason="np.longdouble has no 64-bit significand on this machine")
G = er.G


def test_fixed_weight_exact_against_mpmath():
    """at the directed points (and under the three maxima of the GPU test): the nearest integer, d and the value itself"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    x, want = er.directed_x()
    for m in (0.0, -1e6, 700.0):
        lw = m + x
        near, d, tol = er.fixed_weight_exact(lw, m)
        assert (tol <= 1.2e-6).all()
        for k in range(len(x)):
            xk = lw[k] - m                                          # fl(lw - m): part of the operation
            if not xk >= er.CUT:
                assert near[k] == 0 and d[k] == np.inf and tol[k] == 0.0
                continue
            w = mpmath.mpf(G) * mpmath.exp(mpmath.mpf(float(xk)))
            assert near[k] == int(mpmath.nint(w)), (m, x[k])
            dk = abs((w - mpmath.floor(w)) - mpmath.mpf(0.5))
            assert abs(dk - mpmath.mpf(float(d[k]))) <= 1e-9 * (1 + w), (m, x[k])   # (longdouble: 2^-64 w, and d's own cast)
            assert d[k] > tol[k], (m, x[k])                         # no directed point is in doubt
        if m == 0.0:
            np.testing.assert_array_equal(near, want)
    # the special values
    near, d, tol = er.fixed_weight_exact(np.array([np.nan, -np.inf, -np.inf, 0.0, -21.5, -21.500001]), 0.0)
    np.testing.assert_array_equal(near, [0, 0, 0, G, 0, 0])
    near, _, _ = er.fixed_weight_exact(np.array([-np.inf, np.nan]), -np.inf)   # nobody ran: -inf - -inf is NaN
    np.testing.assert_array_equal(near, [0, 0])
    # below the cut-off true rounding gives 0 too, and it first gives 1 above it
    assert float(mpmath.mpf(G) * mpmath.exp(mpmath.mpf(er.CUT))) < 0.494
    assert er.CUT < float(mpmath.log(mpmath.mpf(0.5) / G)) < -21.4875


def test_few_points_lie_within_their_tolerance_of_a_rounding_point(capsys):
    """2^20 uniform x in [-21.6, 0]: the share with d <= tol is at most 1e-4 -- the cap the GPU test puts on the points where
    the device may differ by one -- by the reference alone (about 1e-6 is expected: tol is about 1e-6 w / 2^30 wide on
    either side of a rounding point, one per unit of w)"""
    x = er.uniform_x(1 << 20)
    near, d, tol = er.fixed_weight_exact(x, 0.0)
    share = float((d <= tol).mean())
    with capsys.disabled():
        print(f"\n  share of 2^20 uniform points within their tolerance of a half-integer: {share:.3e} ({int((d <= tol).sum())} points)")
    assert share <= 1e-4, share
    assert (near[x < er.CUT] == 0).all() and near.max() <= G
    # glibc's exp agrees with the reference wherever the point is not in doubt
    assert (po.fixed_weights(np.append(x, 0.0))[:-1] == near)[d > tol].all()


@pytest.mark.parametrize("path,M", er.shapes())
def test_patterns_are_what_the_oracle_computes(path, M):
    """the integers known in advance ARE oracle.pf_oracle.fixed_weights of the log-weights (glibc is not one off at these
    points), and the reference agrees; every pattern has a particle at the maximum 0"""
    per, chunk, n_chunks = er.geometry(M, path)
    assert per * er.THREADS == chunk and (n_chunks - 1) * chunk < M <= n_chunks * chunk and n_chunks <= er.MAX_CHUNKS
    cases = [(name, None) for name in er.PATTERNS] + [("k_giants", k) for k in (1, min(7, M), M)]
    for name, k in cases:
        logw, fixed = er.pattern(name, M, per, chunk, seed=M, k=k)
        assert np.nanmax(logw) == 0.0
        with np.errstate(invalid="ignore"):
            got = po.fixed_weights(np.where(np.isnan(logw), -np.inf, logw))
        np.testing.assert_array_equal(got, fixed, err_msg=name)
        near, d, tol = er.fixed_weight_exact(logw, 0.0)
        np.testing.assert_array_equal(near, fixed, err_msg=name)
        assert (d > 1e3 * tol).all()                    # beyond doubt: 0.04 from a rounding point at the least
        assert int(fixed.sum()) < 2 ** 53
        if name == "k_giants":
            assert ess_exact(fixed) == k                   # the effective sample size is exactly k


def test_geometry_of_the_shapes():
    assert er.geometry(4096, "group") == (16, 4096, 1) and er.geometry(257, "group") == (2, 512, 1)
    assert er.geometry(262144, "split") == (1, 256, 1024)
    assert er.geometry(262145, "split") == (2, 512, 513) and 262145 - 512 * 512 == 1     # a last chunk of one column
    assert er.geometry(524289, "split") == (4, 1024, 513) and 524289 - 512 * 1024 == 1
    assert er.geometry(4097, "split") == (1, 256, 17)
    # what the patterns put where, at a shape small enough to read: M = 10 laid out for per = 2 (threads of two slots)
    _, ends = er.pattern("slot_ends", 10, 2, 512)
    _, starts = er.pattern("slot_starts", 10, 2, 512)
    np.testing.assert_array_equal(ends // G, [0, 1] * 5)
    np.testing.assert_array_equal(starts // G, [1, 0] * 5)
    _, gaps = er.pattern("thread_gaps", 1024, 2, 512)
    assert gaps[:4].tolist() == [G] * 4 and gaps[4:508].sum() == 0 and gaps[508:516].tolist() == [G] * 8
    _, cg = er.pattern("chunk_gaps", 1025, 1, 256)
    assert cg[:256].tolist() == [G] * 256 and cg[256:1024].sum() == 0 and cg[1024] == G
    _, lc = er.pattern("last_chunk_only", 1025, 1, 256)
    assert lc[:1024].sum() == 0 and lc[1024] == G


def test_two_ancestor_cases_by_hand():
    """`last`, M = 5: S = 2^30 and the cdf is 0, 0, 0, 0, 2^30, so whatever the pointer p in [0, S - 1] the first slot with
    cdf > p is 4: every ancestor is 4 for any u0.

    `uniform`, M = 4, u0 = 1 - 2^-53 (the largest double below 1): weights 2^30 each, S = 2^32, cdf = 1, 2, 3, 4 (x 2^30).
    j + u0 in double: 0 + u0 is exact; 1 + u0 = 2 - 2^-53 lies halfway between the neighbours 2 - 2^-52 and 2 and goes to
    the even one, 2; 2 + u0 and 3 + u0 are less than half a spacing (2^-51) below 3 and 4 and round to them.  The pointers
    ((j + u0) S) / 4 are then 2^30 - 2^-23 (exact), 2 x 2^30, 3 x 2^30 and S, which the clamp takes to S - 1.  First slot
    with cdf > p: 0 (2^30 > 2^30 - 2^-23), 2 (cdf[1] = 2 x 2^30 is not greater), 3, and 3 by the clamp: 0, 2, 3, 3.  Without
    the clamp the last particle would find no slot at all."""
    for u0 in er.U0S:
        logw, fixed = er.pattern("last", 5, 1, 256)
        np.testing.assert_array_equal(po.systematic_ancestors(fixed, u0), [4] * 5)
    u0 = 1.0 - 2.0 ** -53
    assert u0 < 1.0 and np.nextafter(u0, 2.0) == 1.0 and 1.0 + u0 == 2.0 and 2.0 + u0 == 3.0 and 3.0 + u0 == 4.0
    logw, fixed = er.pattern("uniform", 4, 1, 256)
    np.testing.assert_array_equal(fixed, [G] * 4)
    np.testing.assert_array_equal(po.systematic_ancestors(fixed, u0), [0, 2, 3, 3])
    # u0 = 5e-324 is 0 for every particle but the first, whose pointer is still below every weight
    np.testing.assert_array_equal(po.systematic_ancestors(fixed, 5e-324), [0, 1, 2, 3])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ld_extra", [0, 3])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 7, 8, 9, 16, 17])
def test_cancelling_plane_gives_its_target(n_steps, ld_extra, dtype):
    """through oracle.pf_oracle.log_weights: the target to 1e-3 absolute and the target's integer exactly, also under a
    common shift; the step-order fp64 sum equals a longdouble sum to rtol = 1e-13, the project's figure for log-weights;
    rows do cancel (a dropped row leaves the column without weight); the pad columns hold what no sum survives"""
    M = 300
    per, chunk, _ = er.geometry(M, "group")
    for shift in (0.0, -3.0):
        target, fixed = er.pattern("two_giants", M, per, chunk)
        target[5], fixed[5] = er.LW_OF[1], 1
        target[7:20], fixed[7:20] = -np.inf, 0
        plane = er.cancelling_plane(target + shift, n_steps, M + ld_extra, dtype, seed=n_steps)
        assert plane.dtype == dtype and plane.shape == (n_steps, M + ld_extra)
        lw = po.log_weights(plane[:, :M], 0.0, 1.0)
        live = fixed > 0
        np.testing.assert_allclose(lw[live], (target + shift)[live], rtol=0, atol=1.5e-3)
        assert (lw[~live] == -0.5e6).all()
        np.testing.assert_array_equal(po.fixed_weights(lw), fixed)
        near, d, tol = er.fixed_weight_exact(lw, lw.max())
        np.testing.assert_array_equal(near, fixed)
        assert (d > 1e3 * tol).all()
        acc = plane[:, :M].astype(np.longdouble).sum(axis=0)
        want = (np.longdouble(-0.5) * acc * acc).astype(np.float64)
        np.testing.assert_allclose(lw, want, rtol=1e-13, atol=0)
        if ld_extra:
            assert (plane[:, M:] >= 3e38).all()
        if n_steps >= 3:
            for t in range(n_steps):                    # every row but the one that carries the sum is large
                rest = po.log_weights(np.delete(plane[:, :M], t, axis=0), 0.0, 1.0)
                assert (po.fixed_weights(np.append(rest, 0.0))[:-1][np.abs(plane[t, :M]) > 1e3] == 0).all()
            assert ((np.abs(plane[:, :M].astype(np.float64)) > 1e7).sum(axis=0) == n_steps - 1).all()
            if dtype == np.float64:                     # ... and no float32 holds them
                assert (plane[:, :M].astype(np.float32).astype(np.float64) != plane[:, :M]).mean() > 0.5
