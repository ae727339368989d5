"""The order statistics of a series on the GPU (sipnet_batch_plane_quantiles, Batch.plane_quantiles) against the numpy
reference (tests/quantile_reference.py): quantiles, counts and ranks bit for bit at the sizes where the kernels change their
way (a wavefront, a workgroup, a power of two, the 16-byte loads' tails), on both paths, both element types and padded rows;
live members only; ties, zeros of both signs, infinities, a NaN, denormals, a large mean; the scores and their codes, the CRPS
within the derived bound of the pairwise form in long double; the q list; the sort path's capacity and what auto picks beyond
it; planes, daily sums and a smoothed series of a forecast; the batch left as it was; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from tests import quantile_reference as qr
from tests.enkf_gpu_common import ANALYSED, BASE, DEV, bits, carried_params, crafted, forecast, observe, operators, sites_batch
from tests.wquantile_gpu_common import Q6, SELECT, SORT, bare, on_device, same, widened

pytestmark = pytest.mark.gpu

Q3 = [0.025, 0.5, 0.975]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def host_of_plain(res):
    """the unweighted call's four outputs as a plain tuple (wquantile_gpu_common.host_of: the weighted call's six, named)"""
    return tuple(None if x is None else x.cpu().numpy() for x in res[:4])


def check_crps(got, series, n_sites, M, obs, used=None):
    """every scored cell within 4 (n + 2) 2^-53 mean |x - y| of the pairwise form in long double; the largest ratio printed"""
    worst = 0.0
    for r in range(series.shape[0]):
        for s in range(n_sites):
            x = series[r, s * M:(s + 1) * M]
            if used is not None:
                x = x[used[s * M:(s + 1) * M]]
            y = obs[r, s]
            if not np.isfinite(y) or np.isnan(x).any() or x.size == 0:
                assert np.isnan(got[r, s]), (r, s)
                continue
            want, tol = qr.crps_pairwise(x, y), qr.crps_bound(x, y)
            err = abs(float(np.longdouble(got[r, s]) - want))
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
    print(f"largest |crps - pairwise long double| / (4 (n + 2) 2^-53 mean|x - y|) = {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024, 1025])
def test_quantiles_counts_and_ranks_are_the_references(M):
    rng = np.random.default_rng(100 + M)
    for n_sites in (1, 3):
        b = bare(n_sites, M)
        for rows in (1, 5):
            host = rng.normal(size=(rows, n_sites * M)) * 3.0 - 1.0
            host[:, ::7] = np.round(host[:, ::7])                       # some ties
            for dtype in (torch.float64, torch.float32):
                x = widened(host, dtype)
                obs = x[:, rng.integers(0, M, n_sites) + M * np.arange(n_sites)].copy()      # a member's value: a tie with y
                obs[0, 0] += 0.37
                want = qr.plane(x, n_sites, M, Q6, obs=obs)
                runs = {}
                for pad in (0, 7):
                    series = on_device(host, dtype, pad)
                    for path in (SORT, SELECT):
                        res = b.plane_quantiles(series, Q6, live_only=False, obs=obs, want_crps=False, path=path)
                        assert res.path == path and res.crps is None and b.pf_info()["fused"] == (1 if path == SORT else 0)
                        got = host_of_plain(res)
                        what = (n_sites, rows, dtype, pad, path)
                        same(got[0], want[0], what)
                        same(got[1], want[1], what)
                        same(got[3], want[3], what)
                        runs[pad, path] = bits(got[0])
                for k in runs:                                          # the same bits whatever the path and the row pitch
                    np.testing.assert_array_equal(runs[k], runs[0, SORT], err_msg=str(k))
        b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_live_members_only(base, prec):
    """site 0: three members dead; site 1: all dead; site 2: one live; site 3: all live.  The dead columns hold NaN."""
    n_sites, M, rows = 4, 70, 3
    dead = [5, 17, 69] + list(range(M, 2 * M)) + [c for c in range(2 * M, 3 * M) if c != 2 * M + 33]
    rng = np.random.default_rng(3)
    b, st = crafted(base, n_sites, M, prec, rng.uniform(1.0, 100.0, (n_sites * M, 13)), dead=dead)
    used = st[:, 29] == 0
    assert used.sum() == n_sites * M - len(dead)
    host = rng.normal(size=(rows, n_sites * M))
    host[:, ~used] = np.nan
    obs = rng.normal(size=(rows, n_sites))
    dtype = torch.float32 if prec == sa.F32_MIXED else torch.float64
    x = widened(host, dtype)
    series = on_device(host, dtype, 3)
    want = qr.plane(x, n_sites, M, Q3, used=used, obs=obs)
    assert list(want[1][0]) == [M - 3, 0, 1, M]
    assert np.isnan(want[0][:, :, 1]).all() and np.array_equal(want[0][1, :, 2], x[:, 2 * M + 33])
    for path in (SORT, SELECT):
        got = host_of_plain(b.plane_quantiles(series, Q3, live_only=True, obs=obs, want_crps=path == SORT, path=path))
        same(got[0], want[0], path)
        same(got[1], want[1], path)
        same(got[3], want[3], path)
        if path == SORT:
            check_crps(got[2], x, n_sites, M, obs, used)
    # all members: the cells with a NaN among them are NaN, the count is M
    want_all = qr.plane(x, n_sites, M, Q3, obs=obs)
    assert np.isnan(want_all[0][:, :, :3]).all() and (want_all[3][:, :3] == -1).all() and not np.isnan(want_all[0][:, :, 3]).any()
    for path in (SORT, SELECT):
        got = host_of_plain(b.plane_quantiles(series, Q3, live_only=False, obs=obs, want_crps=False, path=path))
        same(got[0], want_all[0], path)
        assert (got[1] == M).all()
        same(got[3], want_all[3], path)
    b.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_special_values(dtype):
    n_sites, M = 3, 257
    rng = np.random.default_rng(9)
    rows = {
        "equal": np.full(n_sites * M, 2.5),
        "ties 0..3": rng.integers(0, 4, n_sites * M).astype(np.float64),
        "zeros": np.where(rng.random(n_sites * M) < 0.5, -0.0, 0.0),
        "zeros among others": np.where(rng.random(n_sites * M) < 0.3, -0.0, np.round(rng.normal(size=n_sites * M))),
        "infinities": np.where(rng.random(n_sites * M) < 0.1, np.inf, np.where(rng.random(n_sites * M) < 0.1, -np.inf,
                                                                              rng.normal(size=n_sites * M))),
        "one nan": rng.normal(size=n_sites * M),
        "denormals": rng.integers(-50, 50, n_sites * M) * 5e-324,
        "float denormals": rng.integers(-50, 50, n_sites * M) * 2.0 ** -149,
        "1e6 + spread": 1e6 + 1e-3 * rng.normal(size=n_sites * M),
    }
    names = list(rows)
    host = np.stack([rows[k] for k in names])
    host[names.index("one nan"), M + 100] = np.nan                      # site 1 of that row only
    host[names.index("infinities"), [0, 1]] = [np.inf, -np.inf]         # (site 0 has both for sure)
    x = widened(host, dtype)
    obs = np.stack([x[:, 3], x[:, M + 3], x[:, 2 * M + 3]], axis=1)     # a member's value each: ties
    obs[names.index("one nan")] = 0.1
    obs[names.index("infinities")] = 0.0
    want = qr.plane(x, n_sites, M, Q6, obs=obs)
    r = names.index("one nan")
    assert np.isnan(want[0][:, r, 1]).all() and not np.isnan(want[0][:, r, [0, 2]]).any() and list(want[3][r, 1]) == [-1, -1]
    r = names.index("infinities")
    assert want[0][0, r, 0] == -np.inf and want[0][1, r, 0] == np.inf
    b = bare(n_sites, M)
    series = on_device(host, dtype)
    for path in (SORT, SELECT):
        got = host_of_plain(b.plane_quantiles(series, Q6, live_only=False, obs=obs, want_crps=False, path=path))
        for k, name in enumerate(names):
            same(got[0][:, k], want[0][:, k], (name, path))
            same(got[3][k], want[3][k], (name, path))
        assert (got[1] == M).all()
    b.close()


@pytest.mark.parametrize("M", [3, 257, 1000])
def test_scores(M):
    n_sites = 3
    rng = np.random.default_rng(40 + M)
    kinds = ["below all", "above all", "a tied value", "nan", "+inf", "-inf", "inside", "inside, mean 1e6"]
    host = np.round(rng.normal(size=(len(kinds), n_sites * M)) * 4.0) / 2.0          # halves: many ties
    host[6] = rng.normal(size=n_sites * M)
    host[7] = 1e6 + rng.normal(size=n_sites * M)
    obs = np.zeros((len(kinds), n_sites))
    obs[0] = host[0].min() - 1.5
    obs[1] = host[1].max() + 0.5
    obs[2] = [host[2, s * M + 1] for s in range(n_sites)]
    obs[3] = np.nan
    obs[4] = np.inf
    obs[5] = -np.inf
    obs[6] = rng.normal(size=n_sites)
    obs[7] = 1e6 + rng.normal(size=n_sites)
    obs[6, 1] = np.nan                                                     # one cell of a scored row not scored
    want = qr.plane(host, n_sites, M, Q3, obs=obs)
    assert (want[3][0] == [0, 0]).all() and (want[3][1] == [M, 0]).all() and (want[3][2][:, 1] >= 1).all()
    assert (want[3][3] == -1).all() and (want[3][4] == -2).all() and (want[3][5] == -2).all() and list(want[3][6, 1]) == [-1, -1]
    assert np.isnan(want[0][:, 4:6]).all() and not np.isnan(want[0][:, 3]).any()
    b = bare(n_sites, M)
    series = on_device(host)
    res = b.plane_quantiles(series, Q3, live_only=False, obs=obs)          # (want_crps, want_rank: whenever obs is given)
    assert res.path == SORT and res.crps is not None and res.rank is not None
    got = host_of_plain(res)
    same(got[0], want[0])
    same(got[1], want[1])
    same(got[3], want[3])
    check_crps(got[2], host, n_sites, M, obs)
    scored = np.isfinite(obs)
    assert (got[2][scored] >= 0).all()
    print(f"largest |crps - the reference's centred form| = {np.nanmax(np.abs(got[2] - want[2])):.3e}")
    again = host_of_plain(b.plane_quantiles(series, Q3, live_only=False, obs=obs, out=res))
    for k in range(4):
        np.testing.assert_array_equal(again[k].view(np.uint8), got[k].view(np.uint8))      # a repeated call: the same bits
    sel = host_of_plain(b.plane_quantiles(series, Q3, live_only=False, obs=obs, want_crps=False, path=SELECT))
    same(sel[3], want[3])
    np.testing.assert_array_equal(bits(sel[0]), bits(got[0]))
    b.close()


def test_q_unsorted_repeated_and_sixteen():
    n_sites, M = 3, 129
    rng = np.random.default_rng(5)
    host = rng.normal(size=(2, n_sites * M))
    b = bare(n_sites, M)
    series = on_device(host)
    for q in ([0.9, 0.1, 0.5], [0.5, 0.5, 0.5, 0.0, 0.0], [1.0], list(rng.random(14)) + [0.0, 1.0],
              [k / 128.0 for k in range(16)]):                              # (k / 128: g == 0 everywhere at n = 129)
        want = qr.plane(host, n_sites, M, q)
        for path in (SORT, SELECT):
            res = b.plane_quantiles(series, q, live_only=False, path=path)
            assert res.crps is None and res.rank is None and tuple(res.quant.shape) == (len(q), 2, n_sites)
            same(res.quant.cpu().numpy(), want[0], (q, path))
    b.close()


def test_more_cells_than_one_row_of_the_grid():
    """2^20 + 3 cells of one member each (the grid is rows of 2^20 workgroups): every cell its own value"""
    rows = (1 << 20) + 3
    host = np.random.default_rng(12).normal(size=(rows, 1))
    obs = host + 1.0
    b = bare(1, 1)
    series = on_device(host)
    for path in (SORT, SELECT):
        got = host_of_plain(b.plane_quantiles(series, [0.0, 0.5], live_only=False, obs=obs, want_crps=path == SORT, path=path))
        assert np.array_equal(got[0][0, :, 0], host[:, 0]) and np.array_equal(got[0][1, :, 0], host[:, 0]), path
        assert (got[1] == 1).all() and (got[3] == [1, 0]).all(), path
        if path == SORT:
            assert np.array_equal(got[2][:, 0], np.abs(host[:, 0] - obs[:, 0]))
    b.close()


def test_the_capacity_edge():
    cap = sa.quantile_lds_members(False)
    rng = np.random.default_rng(6)
    for M, auto in ((cap, SORT), (cap + 1, SELECT)):
        host = rng.normal(size=(1, M))
        host[0, ::5] = np.round(host[0, ::5], 1)
        obs = np.array([[host[0, 5]]])
        want = qr.plane(host, 1, M, Q3, obs=obs)
        b = bare(1, M)
        series = on_device(host)
        res = b.plane_quantiles(series, Q3, live_only=False, obs=obs)
        assert res.path == auto and b.pf_info()["fused"] == (1 if auto == SORT else 0)
        assert (res.crps is not None) == (auto == SORT)
        got = host_of_plain(res)
        same(got[0], want[0], M)
        same(got[1], want[1], M)
        same(got[3], want[3], M)
        if auto == SORT:
            sel = host_of_plain(b.plane_quantiles(series, Q3, live_only=False, obs=obs, want_crps=False, path=SELECT))
            np.testing.assert_array_equal(bits(sel[0]), bits(got[0]))
            same(sel[3], got[3])
        else:
            for kw in (dict(path=SORT), dict(obs=obs, want_crps=True)):
                with pytest.raises(sa.SipnetError):
                    b.plane_quantiles(series, Q3, live_only=False, **kw)
        b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_a_forecasts_planes_sums_and_smoothed_series(base, prec):
    n_sites, M, steps = 4, 256, 96
    b, planes = forecast(base, n_sites, M, prec, steps=steps)
    b2 = sites_batch(synth.perturbed_params(base, n_sites * M, seed=1), n_sites, prec)      # (forecast()'s members)
    sums = b2.run_sums(0, steps, 48)
    b2.close()
    st0 = b.get_state()
    used = st0[:, 29] == 0
    nee = planes[0].cpu().numpy()
    obs = np.median(nee.astype(np.float64).reshape(steps, n_sites, M), axis=2) + 0.01
    want = qr.plane(nee, n_sites, M, Q3, used=used, obs=obs)
    got = host_of_plain(b.plane_quantiles(planes[0], Q3, obs=obs))
    for k in (0, 1, 3):
        same(got[k], want[k], k)
    check_crps(got[2][::16], nee.astype(np.float64)[::16], n_sites, M, obs[::16], used)
    for v in range(3):
        want = qr.plane(sums[v].cpu().numpy(), n_sites, M, Q3, used=used)
        got = host_of_plain(b.plane_quantiles(sums[v], Q3))
        same(got[0], want[0], v)
        same(got[1], want[1], v)
    # the smoother analyses the planes in place: the median of what it left
    ops = operators()
    pl = [p.cpu().numpy() for p in planes]
    o, sd = observe(st0, pl, carried_params(b), n_sites, ops, np.random.default_rng(5))
    b.enkf_analysis_smooth(o, sd, ops, ANALYSED, [planes], planes=planes)
    smoothed = planes[0].cpu().numpy()
    assert (smoothed != nee).any()
    used = b.get_state()[:, 29] == 0
    want = qr.plane(smoothed, n_sites, M, [0.5], used=used)
    got = host_of_plain(b.plane_quantiles(planes[0], [0.5]))
    same(got[0], want[0])
    same(got[1], want[1])
    b.close()


def test_the_batch_is_left_as_it_was(base):
    n_sites, M = 2, 64
    rng = np.random.default_rng(8)
    b, _ = crafted(base, n_sites, M, sa.F64, rng.uniform(1.0, 100.0, (n_sites * M, 13)), dead=[3, 70])
    before = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    series = on_device(rng.normal(size=(4, n_sites * M)))
    obs = rng.normal(size=(4, n_sites))
    for path in (SORT, SELECT):
        for live in (True, False):
            b.plane_quantiles(series, Q3, live_only=live, obs=obs, want_crps=path == SORT, path=path)
    after = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    b.close()


def test_refusals_write_nothing():
    L = sa.lib()
    n_sites, M, rows = 2, 64, 3
    cap = sa.quantile_lds_members(False)
    small, big = bare(n_sites, M), bare(1, cap + 1)
    series = on_device(np.zeros((rows, n_sites * M)))
    wide = on_device(np.zeros((rows, cap + 1)))
    quant = torch.full((16, rows, n_sites), -7.0, dtype=torch.float64, device=DEV)
    count = torch.full((rows, n_sites), -7, dtype=torch.int32, device=DEV)
    crps = torch.full((rows, n_sites), -7.0, dtype=torch.float64, device=DEV)
    rank = torch.full((rows, n_sites, 2), -7, dtype=torch.int32, device=DEV)
    obs = torch.zeros((rows, n_sites), dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(b=small, s=series, f32=0, r=rows, ld=n_sites * M, q=(0.5,), n_q=None, live=0, path=0, qt=quant, cnt=count, y=obs,
             cr=None, rk=None):
        qs = None if q is None else (C.c_double * max(len(q), 1))(*q)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return L.sipnet_batch_plane_quantiles(b.h if b is not None else None, ptr(s), f32, r, ld, len(q) if n_q is None else n_q, qs,
                                              live, path, ptr(qt), ptr(cnt), ptr(y), ptr(cr), ptr(rk), stream)

    cases = {
        "a NULL batch": dict(b=None), "a NULL series": dict(s=None), "a NULL q": dict(q=None, n_q=1), "a NULL d_quant": dict(qt=None),
        "rows 0": dict(r=0), "ld below ncol": dict(ld=n_sites * M - 1),
        "n_q 0": dict(q=(), n_q=0), "n_q 17": dict(q=(0.5,) * 17),
        "q nan": dict(q=(0.5, float("nan"))), "q below 0": dict(q=(-0.1,)), "q above 1": dict(q=(0.2, 1.1)), "q inf": dict(q=(float("inf"),)),
        "crps without obs": dict(y=None, cr=crps), "rank without obs": dict(y=None, rk=rank),
        "path -1": dict(path=-1), "path 3": dict(path=3),
        "the sort path beyond its capacity": dict(b=big, s=wide, ld=cap + 1, path=1),
        "crps on the forced selection path": dict(cr=crps, path=2),
        "crps on the selection path by size": dict(b=big, s=wide, ld=cap + 1, cr=crps),
        "live members of a batch that is not set up": dict(live=1),
    }
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_BAD_ARGUMENT, name
        assert b"sipnet_batch_plane_quantiles: " in L.sipnet_last_error(), name
    torch.cuda.synchronize()
    assert (quant == -7.0).all() and (count == -7).all() and (crps == -7.0).all() and (rank == -7).all()
    assert call() == _lib.OK                                             # the call itself is sound
    torch.cuda.synchronize()
    assert (quant[0] == 0.0).all() and (quant[1:] == -7.0).all() and (count == M).all()
    small.close()
    big.close()
