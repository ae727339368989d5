"""The weighted order statistics without a device: tests/wquantile_reference.py against replication (np.repeat and numpy's
"inverted_cdf") and against numpy's own weights= where the installed numpy has it; its moments and CRPS against replication;
and the library's host-only entry points (sipnet_wquantile_target, sipnet_wquantile_lds_members, sipnet_wquantile_path) with
the refusals that need no device.  No GPU."""
import inspect

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import quantile_reference as qr
from tests import wquantile_reference as wr

QS = [0.0, 1.0, 0.5, 0.025, 0.975, 1.0 / 3.0, 0.25, float(np.nextafter(1.0, 0.0))]


def samples():
    rng = np.random.default_rng(21)
    out = {}
    for n in (1, 2, 3, 64, 257):
        out[f"normal {n}"] = (rng.normal(size=n), rng.integers(1, 6, n))
    out["ties, weights differ"] = (rng.integers(0, 4, 100).astype(np.float64), rng.integers(1, 9, 100))
    out["some zero weights"] = (rng.normal(size=200), rng.integers(0, 3, 200))
    out["one member has it all"] = (rng.normal(size=50), np.where(np.arange(50) == 17, 7, 0))
    out["first only"] = (rng.normal(size=50), np.where(np.arange(50) == 0, 3, 0))
    out["last only"] = (rng.normal(size=50), np.where(np.arange(50) == 49, 3, 0))
    out["equal weights"] = (rng.normal(size=101), np.full(101, 4))
    return out


@pytest.mark.parametrize("name", list(samples()))
def test_the_reference_against_replication(name):
    """a sample with small integer weights IS the sample with every value repeated w times: type 1 ("inverted_cdf") of it"""
    x, w = samples()[name]
    rep = np.repeat(x, w)
    got = wr.quantiles(x, w, QS)
    want = np.quantile(rep, QS, method="inverted_cdf")
    np.testing.assert_array_equal(got, want)
    assert got[0] == x[w > 0].min() and got[1] == x[w > 0].max()
    for y in (float(np.median(x)), float(x[0]), float(x.min()) - 1.0, float(x.max()) + 1.0):
        quant, rank, nan = wr.cell(x, w, QS, y)
        assert not nan and list(rank) == [(rep < y).sum(), (rep == y).sum()]
        np.testing.assert_array_equal(quant, want)
        # the CRPS of the replicated sample by the unweighted pairwise form, the moments by numpy's
        crps, tol = wr.crps_pairwise(x, w, y), qr.crps_bound(rep, y)
        assert abs(float(crps - qr.crps_pairwise(rep, y))) <= tol, name
        assert 0.0 <= wr.crps_bound(x, w, y) <= tol                          # (the same mean |x - y|, n <= the replicated size)
    mean, m2 = wr.moments(x, w)
    big = np.abs(rep).max()                                                  # (numpy's own mean and variance are doubles)
    assert abs(float(mean) - rep.mean()) <= 1e-13 * big and abs(float(m2) - rep.var()) <= 1e-12 * big * big


@pytest.mark.skipif("weights" not in inspect.signature(np.quantile).parameters, reason="this numpy's quantile takes no weights")
@pytest.mark.parametrize("name", list(samples()))
def test_the_reference_against_numpys_weights(name):
    """numpy forms q * S in floating point as the contract does; the probabilities here keep the product away from an integer
    (or put it on one exactly), so that a last-bit difference of the two products cannot move an index"""
    x, w = samples()[name]
    qs = [0.0, 1.0, 0.5, 0.25, 0.3, 0.7, 0.9]
    want = np.quantile(x, qs, method="inverted_cdf", weights=w.astype(np.float64))
    np.testing.assert_array_equal(wr.quantiles(x, w, qs), want)


def test_the_target_on_and_next_to_a_cumulative_weight():
    """C = 3, 5, 9 of x = 10, 20, 30 (S = 9): T = 3 reads 10, T = 4 reads 20, T = 5 reads 20, T = 6 reads 30"""
    x, w = np.array([30.0, 10.0, 20.0]), np.array([4, 3, 2])
    for q, T, want in ((3 / 9, 3, 10.0), (3.5 / 9, 4, 20.0), (5 / 9, 5, 20.0), (5.0001 / 9, 6, 30.0), (0.0, 1, 10.0), (1.0, 9, 30.0)):
        assert wr.target(9, q) == T and wr.quantiles(x, w, [q])[0] == want, q


def test_the_reference_cells_codes():
    q = [0.5]
    x, w = np.array([1.0, np.nan, 2.0]), np.array([1, 0, 1])
    quant, rank, nan = wr.cell(x, w, q, 1.5)
    assert quant[0] == 1.0 and list(rank) == [1, 0] and not nan          # a NaN under weight 0 is not in the sample
    quant, rank, nan = wr.cell(x, np.array([1, 1, 1]), q, 1.5)
    assert np.isnan(quant).all() and list(rank) == [-1, -1] and nan
    quant, rank, nan = wr.cell(x, np.zeros(3, np.int64), q, 1.5)
    assert np.isnan(quant).all() and list(rank) == [0, 0] and nan
    quant, rank, nan = wr.cell(x, w, q, 1.5, code=-2)
    assert np.isnan(quant).all() and list(rank) == [-2, -2] and nan
    quant, rank, nan = wr.cell(x, w, q, np.inf)
    assert np.isnan(quant).all() and list(rank) == [-2, -2] and nan
    quant, rank, nan = wr.cell(x, w, q, np.nan)
    assert quant[0] == 1.0 and list(rank) == [-1, -1] and not nan
    w3, d, tol = wr.weights_of([0.0, -np.inf, np.nan, -20.0, -1000.0, 5.0], used=[True, True, True, True, True, False])
    assert list(w3) == [1 << 30, 0, 0, 2, 0, 0]
    assert wr.weights_of([0.0, np.inf])[0].sum() == 0 and wr.site_code([0.0, np.inf]) == -2
    assert wr.site_code([0.0, np.inf], used=[True, False]) == 0
    assert wr.weights_of([-np.inf, np.nan])[0].sum() == 0


S_VALUES = [1, 1 << 30, (1 << 44) + 1, 1 << 52]
Q_VALUES = [0.0, 1.0, 0.5, 1e-300, 1.0 - 2.0 ** -53]


@pytest.mark.parametrize("S", S_VALUES)
def test_the_librarys_target_is_the_references(S):
    for q in Q_VALUES + [1.0 / 3.0, 0.025, 0.975]:
        T = sa.wquantile_target(S, q)
        assert T == wr.target(S, q) and 1 <= T <= S, (S, q)
    assert sa.wquantile_target(S, 0.0) == 1 and sa.wquantile_target(S, 1e-300) == 1 and sa.wquantile_target(S, 1.0) == S
    assert sa.wquantile_target(S, 0.5) == max(1, (S + 1) // 2)
    # 1 - 2^-53: the rounded product lies in (S - 1, S] for every S up to 2^52, so its ceiling is S
    assert sa.wquantile_target(S, 1.0 - 2.0 ** -53) == S


def test_the_target_refuses():
    L = sa.lib()
    for S, q in ((0, 0.5), (-1, 0.5), ((1 << 52) + 1, 0.5), (10, -1e-9), (10, float(np.nextafter(1.0, 2.0))), (10, np.nan), (10, np.inf)):
        assert L.sipnet_wquantile_target(S, q) == -1, (S, q)
        with pytest.raises(ValueError):
            sa.wquantile_target(S, q)


def test_the_sort_paths_capacity_and_the_path_rule():
    L = sa.lib()
    for f32 in (0, 1):
        cap = sa.wquantile_lds_members(bool(f32))
        assert cap == 8192 and cap * 12 <= 96 * 1024
        assert [L.sipnet_wquantile_path(M, f32, 0) for M in (1, cap, cap + 1, 4194304)] == [1, 1, 2, 2]
        assert [L.sipnet_wquantile_path(M, f32, 1) for M in (1, cap, cap + 1)] == [1, 1, -1]
        assert [L.sipnet_wquantile_path(M, f32, 2) for M in (1, cap, cap + 1)] == [2, 2, 2]
        assert [L.sipnet_wquantile_path(64, f32, p) for p in (-1, 3)] == [-1, -1] and L.sipnet_wquantile_path(0, f32, 0) == -1


def test_the_batch_call_refuses_a_null_batch_without_a_device():
    q = np.array([0.5])
    rc = sa.lib().sipnet_batch_plane_quantiles_weighted(None, None, 0, 1, 0, None, 1, q.ctypes.data, 0, 0, None, None, None, None,
                                                        None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_plane_quantiles_weighted" in sa.lib().sipnet_last_error()


# ---- the reference on the edges of tests/test_gpu_wquantiles_edges.py ----------------------------------------------------------
@pytest.mark.parametrize("M", [3, 257, 1000])
def test_the_reference_cell_on_every_kind_of_observation(M):
    """cell() against a loop over the members, and against what the contract says of each kind"""
    rng = np.random.default_rng(600 + M)
    w = rng.integers(1, 1 << 30, M)
    w[1::4] = 0
    x, y = wr.score_rows(rng, M, w > 0)
    S = int(w.sum())
    bare_quant = {}
    for r, kind in enumerate(wr.OBS_KINDS):
        quant, rank, nan = wr.cell(x[r], w, QS, y[r])
        less = eq = 0
        for j in range(M):
            if w[j] > 0 and x[r, j] < y[r]:
                less += int(w[j])
            elif w[j] > 0 and x[r, j] == y[r]:
                eq += int(w[j])
        bare_quant[kind] = wr.cell(x[r], w, QS)[0]
        if kind == "nan":
            assert list(rank) == [-1, -1] and not nan
            np.testing.assert_array_equal(quant, bare_quant[kind])           # the quantiles as without an observation
        elif kind in ("+inf", "-inf"):
            assert list(rank) == [-2, -2] and nan and np.isnan(quant).all()
        else:
            assert list(rank) == [less, eq] and not nan, kind
            np.testing.assert_array_equal(quant, bare_quant[kind])
        want = {"below": [0, 0], "above": [S, 0], "ties weight 0 only": [less, 0]}.get(kind)
        if want is not None:
            assert list(rank) == want, kind
        if kind in ("tied", "+0 against -0"):
            assert rank[1] > 0, kind
        if kind in ("inside", "inside, mean 1e6"):
            assert 0 < rank[0] < S, kind
    # the codes go before the observation's
    for yy in (0.0, np.nan, np.inf, -np.inf):
        assert list(wr.cell(x[0], np.zeros(M, np.int64), QS, yy)[1]) == [0, 0]
        assert list(wr.cell(x[0], w, QS, yy, code=-2)[1]) == [-2, -2]


def test_the_reference_at_equal_weights_is_type_1_with_infinities_and_both_zeros():
    rng = np.random.default_rng(31)
    qs = [0.0, 1.0, 0.5] + [(j + 0.5) / 101 for j in range(0, 101, 9)]
    x = rng.normal(size=101)
    x[[3, 50]], x[[7, 90, 91]] = np.inf, -np.inf
    zeros = np.where(rng.random(101) < 0.5, -0.0, 0.0)
    mixed = np.round(rng.normal(size=101))
    mixed[::5] = -0.0
    for sample in (x, zeros, mixed):
        got = wr.quantiles(sample, np.full(101, 1 << 30), qs)
        np.testing.assert_array_equal(got, np.quantile(sample, qs, method="inverted_cdf"))
    got = wr.quantiles(x, np.full(101, 1 << 30), [0.0, 1.0])
    assert got[0] == -np.inf and got[1] == np.inf


def test_the_denormal_allowance_and_the_large_means_bound_bite():
    """rows 3 and 5 of special_rows at the sizes of the GPU test: the denormal row's relative bounds are 0 as doubles, and
    the allowance that replaces them is a small fraction of the mean; the large-mean row's bound on m2 is a small fraction
    of m2, and a one-pass second moment in doubles misses it by orders of magnitude"""
    for M in (257, 1000):
        rng = np.random.default_rng(700 + M)
        w = rng.integers(1, 1 << 30, 3 * M)
        w[rng.random(3 * M) < 0.1] = 0
        x, y = wr.special_rows(rng, 3, M, False, w > 0)
        assert not np.isnan(x[:8]).any() and np.isnan(x[8]).sum() == 1 and np.isinf(x[2, :M][w[:M] > 0]).sum() >= 2
        xs, ws = x[3, :M], w[:M]
        n = int((ws > 0).sum())
        assert 0.0 < xs.min() and xs.max() < 2.0 ** -1022
        b_mean, b_m2 = wr.moments_bounds(xs, ws)
        assert b_mean == 0.0 and b_m2 == 0.0 and wr.crps_bound(xs, ws, y[3, 0]) == 0.0
        mean, m2 = wr.moments(xs, ws)
        assert float(m2) == 0.0 and 0.0 < wr.denormal_allowance(n) < 1e-7 * float(mean)
        assert wr.denormal_allowance(n) == (2 * n + 8) * 2.0 ** -1074
        xs = x[5, :M]
        mean, m2 = wr.moments(xs, ws)
        b_mean, b_m2 = wr.moments_bounds(xs, ws)
        assert 1e-7 < float(m2) < 1e-5 and 0.0 < b_m2 < 1e-3 * float(m2)
        wd, S = ws.astype(np.float64), float(ws.sum())
        one_pass = (wd * xs * xs).sum() / S - ((wd * xs).sum() / S) ** 2
        two_pass = (wd * (xs - (wd * xs).sum() / S) ** 2).sum() / S
        print(f"M = {M}: m2 {float(m2):.3e}, its bound {b_m2:.3e}, one pass off by {abs(one_pass - float(m2)):.3e}, two passes by "
              f"{abs(two_pass - float(m2)):.3e}")
        assert abs(one_pass - float(m2)) > 100.0 * b_m2 and abs(two_pass - float(m2)) <= b_m2
