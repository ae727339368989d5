"""The host-only entry points of the order statistics (sipnet_quantile_positions, sipnet_quantile_lds_members) against
tests/quantile_reference.py, that reference against numpy's own quantiles and against the CRPS's pairwise form in
np.longdouble, and the refusals that need no device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import quantile_reference as qr

NS = [1, 2, 3, 64, 1000, 16384, 4194304]
QS = [0.0, 1.0, 0.5, 0.025, 0.975, 1.0 / 3.0, float(np.nextafter(1.0, 0.0))]


@pytest.mark.parametrize("n", NS)
def test_positions_are_the_references(n):
    lo, g = sa.quantile_positions(n, QS)
    want_lo, want_g = qr.positions(n, QS)
    assert lo.dtype == np.int32 and g.dtype == np.float64
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(g.view(np.uint64), want_g.view(np.uint64))
    assert (lo >= 0).all() and (lo <= n - 1).all() and (g >= 0).all() and (g < 1).all()
    assert ((g == 0) | (lo + 1 <= n - 1)).all()          # x[lo + 1] is read only where it exists
    assert lo[0] == 0 and g[0] == 0 and lo[1] == n - 1 and g[1] == 0


def samples():
    rng = np.random.default_rng(11)
    out = {"one": np.array([3.5]), "two": np.array([2.0, -1.0]), "three": rng.normal(size=3)}
    for n in (64, 1000, 1025):
        out[f"normal {n}"] = rng.normal(size=n)
    out["skewed 1000"] = -np.exp(rng.normal(size=1000)) + 0.3
    out["ties"] = rng.integers(0, 4, 257).astype(np.float64)
    out["mean 1e6, spread 1"] = 1e6 + rng.normal(size=1000)
    return out


@pytest.mark.parametrize("name", list(samples()))
def test_the_reference_quantiles_against_numpy(name):
    """numpy's lerp rounds differently for g >= 0.5 (it works back from x[lo + 1]): two roundings on each side bound the gap,
    4 x 2^-53 max(|x_lo|, |x_hi|)"""
    x = samples()[name]
    got = qr.quantiles(x, QS)
    want = np.quantile(x, QS, method="linear")
    xs = np.sort(x)
    lo, g = qr.positions(x.size, QS)
    hi = np.minimum(lo + 1, x.size - 1)
    tol = 4 * 2.0 ** -53 * np.maximum(np.abs(xs[lo]), np.abs(xs[hi]))
    print(f"{name}: largest |reference - numpy| / tolerance = {float((np.abs(got - want) / np.maximum(tol, 5e-324)).max()):.3f}")
    assert (np.abs(got - want) <= tol).all()
    assert got[0] == xs[0] and got[1] == xs[-1]


@pytest.mark.parametrize("name", list(samples()))
def test_the_centred_crps_against_the_pairwise_form_in_longdouble(name):
    """the bound any fixed-order double summation of the centred terms meets: 4 (n + 2) 2^-53 mean |x - y|"""
    x = samples()[name]
    xs = np.sort(x)
    for y in (float(xs[0]) - 1.0, float(xs[-1]) + 2.0, float(np.median(x)), float(xs[x.size // 3]), float(x.mean()) + 0.1):
        got, want, tol = qr.crps_centred(x, y), qr.crps_pairwise(x, y), qr.crps_bound(x, y)
        print(f"{name}, y = {y!r}: |centred - pairwise| = {abs(float(got - want)):.3e}, bound {tol:.3e}")
        assert abs(got - want) <= tol
        assert want >= -tol


def test_the_centring_matters_at_a_large_mean():
    """mean 1e6, spread 1: the sorted form over the raw values subtracts two sums of ~1e6 each and misses the bound that the
    form centred on y keeps"""
    x = samples()["mean 1e6, spread 1"]
    y = 1e6 + 0.25
    n = x.size
    xs = np.sort(x)
    raw = np.cumsum(np.abs(xs - y))[-1] / n - np.cumsum((2.0 * np.arange(1, n + 1) - n - 1.0) * xs)[-1] / (float(n) * n)
    want, tol = qr.crps_pairwise(x, y), qr.crps_bound(x, y)
    err_raw, err_centred = abs(float(raw - want)), abs(float(qr.crps_centred(x, y) - want))
    print(f"bound {tol:.3e}: centred {err_centred:.3e}, over the raw values {err_raw:.3e}")
    assert err_centred <= tol
    assert err_raw > err_centred


def test_the_reference_cells_codes():
    q = [0.5]
    quant, n, crps, rank = qr.cell(np.array([1.0, np.nan, 2.0]), q, 1.5)
    assert np.isnan(quant).all() and n == 3 and np.isnan(crps) and list(rank) == [-1, -1]
    quant, n, crps, rank = qr.cell(np.array([1.0, 2.0]), q, np.nan)
    assert quant[0] == 1.5 and np.isnan(crps) and list(rank) == [-1, -1]
    quant, n, crps, rank = qr.cell(np.array([1.0, 2.0]), q, np.inf)
    assert np.isnan(quant).all() and np.isnan(crps) and list(rank) == [-2, -2]
    quant, n, crps, rank = qr.cell(np.array([]), q, 0.0)
    assert np.isnan(quant).all() and n == 0 and np.isnan(crps) and list(rank) == [0, 0]
    quant, n, crps, rank = qr.cell(np.array([1.0, 2.0, 2.0, 3.0]), [0.0, 1.0], 2.0)
    assert list(quant) == [1.0, 3.0] and list(rank) == [1, 2] and crps == 0.125


def call_positions(n, n_q, q):
    q = np.ascontiguousarray(q, dtype=np.float64)
    lo = np.full(max(q.size, 1), -7, np.int32)
    g = np.full(max(q.size, 1), -7.0)
    rc = sa.lib().sipnet_quantile_positions(n, n_q, q.ctypes.data, lo.ctypes.data, g.ctypes.data)
    return rc, lo, g


@pytest.mark.parametrize("n,n_q,q,why", [(0, 1, [0.5], b"n must be"), (-3, 1, [0.5], b"n must be"),
                                          (10, 0, [0.5], b"n_q"), (10, 17, [0.5] * 17, b"n_q"),
                                          (10, 2, [0.5, np.nan], b"q[1]"), (10, 1, [-1e-9], b"q[0]"),
                                          (10, 3, [0.1, 0.2, float(np.nextafter(1.0, 2.0))], b"q[2]"),
                                          (10, 1, [np.inf], b"q[0]")])
def test_positions_refuses(n, n_q, q, why):
    rc, lo, g = call_positions(n, n_q, q)
    assert rc == _lib.ERR_BAD_ARGUMENT
    msg = sa.lib().sipnet_last_error()
    assert b"sipnet_quantile_positions" in msg and why in msg, msg
    assert (lo == -7).all() and (g == -7.0).all()        # nothing written


def test_positions_refuses_null_pointers_and_takes_sixteen():
    L = sa.lib()
    for n, q in ((0, [0.5]), (4, [1.5]), (4, [0.5] * 17)):
        with pytest.raises(sa.SipnetError):
            sa.quantile_positions(n, q)
    q = np.array([0.5])
    lo, g = np.zeros(1, np.int32), np.zeros(1)
    assert L.sipnet_quantile_positions(5, 1, None, lo.ctypes.data, g.ctypes.data) == _lib.ERR_BAD_ARGUMENT
    assert L.sipnet_quantile_positions(5, 1, q.ctypes.data, None, g.ctypes.data) == _lib.ERR_BAD_ARGUMENT
    assert L.sipnet_quantile_positions(5, 1, q.ctypes.data, lo.ctypes.data, None) == _lib.ERR_BAD_ARGUMENT
    lo16, g16 = sa.quantile_positions(5, np.linspace(0, 1, 16))
    assert lo16.size == 16 and lo16[-1] == 4


def test_the_sort_paths_capacity():
    for f32 in (False, True):
        assert sa.quantile_lds_members(f32) >= 1024
        assert sa.quantile_lds_members(f32) * (4 if f32 else 8) <= 160 * 1024      # a compute unit's LDS
    assert sa.quantile_lds_members(False) == 16384


def test_the_batch_call_refuses_a_null_batch_without_a_device():
    q = np.array([0.5])
    rc = sa.lib().sipnet_batch_plane_quantiles(None, None, 0, 1, 0, 1, q.ctypes.data, 0, 0, None, None, None, None, None, None)
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert b"sipnet_batch_plane_quantiles" in sa.lib().sipnet_last_error()


def test_the_path_rule():
    """sipnet_quantile_path: the sort path up to its capacity, selection beyond, -1 where the call would refuse"""
    L = sa.lib()
    for f32 in (0, 1):
        cap = sa.quantile_lds_members(bool(f32))
        assert [L.sipnet_quantile_path(M, f32, 0) for M in (1, cap, cap + 1, 4194304)] == [1, 1, 2, 2]
        assert [L.sipnet_quantile_path(M, f32, 1) for M in (1, cap, cap + 1)] == [1, 1, -1]
        assert [L.sipnet_quantile_path(M, f32, 2) for M in (1, cap, cap + 1)] == [2, 2, 2]
        assert [L.sipnet_quantile_path(64, f32, p) for p in (-1, 3)] == [-1, -1] and L.sipnet_quantile_path(0, f32, 0) == -1
