"""The ensemble Kalman smoother on the GPU (sipnet_batch_enkf_analysis_smooth): the series of every site against the numpy
reference (tests/enkf_smooth_reference.py); the state, parameters and site_info of the joint call bit for bit; the same series
bits in place and out of place, on a repeated call, on every path of the pool analysis and with the anomalies in LDS or in
scratch; dst = src where nothing is analysed; a series that copies a pool against the analysed pool; sites whose anomalies do
not fit LDS; a huge sd; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import enkf_smooth_reference as sr
from tests.enkf_gpu_common import (ANALYSED, BASE, DEV, SLOTS, bits, carried_params, forecast, observe, op_tuples, operators,
                                   sites_batch, within)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def force_path(b, path):
    if path == "group":
        b.debug_set_num_cus(1)
    elif path == "split":
        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


def two_params():
    return [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in ("aMax", "baseVegResp")]


def tuples(params):
    return [(p.index, p.lo, p.hi) for p in params]


def raw_bits(x):
    """the bits of a float64 or float32 array"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def series_within(got, want, src, status, info, n_sites, float_store=False, bound=1e-10):
    """|got - want| <= bound max(|want|, the ensemble sd of that element over the site's live members) (+ 2^-23 |want| for a
    float series: one spacing of the rounded store), for every element of a code-1 site's live members; the largest ratio
    is printed first.  Everything else must hold src's bits."""
    ncol = status.shape[0]
    M = ncol // n_sites
    got, src = np.asarray(got)[:, :ncol], np.asarray(src)[:, :ncol]
    worst, checks, moved = 0.0, [], []
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[status[cols] == 0] if info[s, 0] == 1 else cols[:0]
        rest = np.setdiff1d(cols, live)
        np.testing.assert_array_equal(raw_bits(got[:, rest]), raw_bits(src[:, rest]))
        if len(live) == 0:
            continue
        g, w, z = got[:, live].astype(np.float64), want[:, live], src[:, live].astype(np.float64)
        scale = bound * np.maximum(np.abs(w), z.std(1, keepdims=True) + 1e-300)
        if float_store:
            scale = scale + 2.0 ** -23 * np.abs(w)
        worst = max(worst, float((np.abs(g - w) / scale).max()))
        checks.append((s, np.abs(g - w) <= scale))
        moved.append(bool((g != z).any()))
    print(f"largest |got - want| / bound over {n_sites} sites: {worst:.3e} (bound {bound:g} of max(|x|, site ensemble sd)"
          + (" + 2^-23 |x|)" if float_store else ")"))
    for s, ok in checks:
        assert ok.all(), s
    return moved


@pytest.mark.parametrize("M", [256, 1000])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_every_series_against_the_reference(base, prec, M):
    """the three planes in place (one of them read by the NEE operator) and the daily sums of a second identical batch"""
    n_sites, steps = 8, 96
    b, planes = forecast(base, n_sites, M, prec, steps=steps)
    b2 = sites_batch(synth.perturbed_params(base, n_sites * M, seed=1), n_sites, prec)      # (forecast()'s members)
    sums = b2.run_sums(0, steps, 48)
    b2.close()
    assert planes.dtype == (torch.float32 if prec == sa.F32_MIXED else torch.float64) and sums.dtype == torch.float64
    ops = operators()
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    sm = [p.cpu().numpy() for p in sums]
    prm0 = carried_params(b)
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(5), nan_sites=(3,), nan_obs=((0, 1), (5, 3)))
    infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    out = b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [planes, sums], planes=planes, inflation=infl, info_out=info)
    assert len(out) == 6 and all(o.data_ptr() == x.data_ptr() for o, x in zip(out, list(planes) + list(sums)))
    st1 = b.get_state()
    b.close()
    want, _, want_info, want_series = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, [], obs, sd,
                                                  pl + sm, infl, None, pl, prm0)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    assert list(info[:, 0]) == [1, 1, 1, -1, 1, 1, 1, 1]
    within(st1, want, st0, n_sites)
    moved = np.zeros(n_sites - 1, bool)
    for k, (got, src) in enumerate(zip(out, pl + sm)):
        moved |= np.array(series_within(got.cpu().numpy(), want_series[k], src, st0[:, 29], info, n_sites,
                                        float_store=src.dtype == np.float32))
    assert moved.all()


@pytest.mark.parametrize("path", ["group", "split"])
@pytest.mark.parametrize("n_params", [0, 2])
def test_the_series_stage_leaves_state_parameters_and_info_as_the_joint_call_does(base, n_params, path):
    n_sites, M = 8, 256
    params = two_params()[:n_params]
    results = []
    for smooth in (False, True):
        b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=3)
        force_path(b, path)
        st0 = b.get_state()
        pl = [p.cpu().numpy() for p in planes]
        prm0 = carried_params(b)
        ops = operators()
        obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(1), nan_sites=(6,), nan_obs=((2, 0),))
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        infl = np.full(n_sites, 1.1)
        pinfl = np.full(n_sites, 1.05) if n_params else None
        if smooth:
            b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [planes], params, planes=planes, inflation=infl,
                                   param_inflation=pinfl, info_out=info)
            assert (planes.cpu().numpy() != np.stack(pl)).any()
        else:
            b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, inflation=infl, param_inflation=pinfl,
                                  info_out=info)
        assert b.pf_info()["fused"] == (1 if path == "group" else 0)
        results.append((bits(b.get_state()), info.cpu().numpy(), bits(b.get_params())))
        assert (results[-1][0] != bits(st0)).any()
        b.close()
    for k in range(3):
        np.testing.assert_array_equal(results[1][k], results[0][k])


def test_the_series_bits_do_not_depend_on_the_call_the_path_or_the_place(base):
    n_sites, M = 8, 256
    runs = {}
    for name in ("in place", "out of place", "again", "group", "split"):
        b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=3)
        force_path(b, name)
        st0 = b.get_state()
        pl = [p.cpu().numpy() for p in planes]
        ops = operators()
        obs, sd = observe(st0, pl, carried_params(b), n_sites, ops, np.random.default_rng(1), nan_sites=(6,), nan_obs=((2, 0),))
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
        if name == "out of place":
            dst = torch.full_like(planes, -7.0)
            out = b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [(planes, dst)], planes=planes, inflation=infl, info_out=info)
            np.testing.assert_array_equal(bits(planes.cpu().numpy()), bits(np.stack(pl)))      # src as it was
            assert all(o.data_ptr() == d.data_ptr() for o, d in zip(out, dst))
        else:
            out = b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [planes], planes=planes, inflation=infl, info_out=info)
        runs[name] = (bits(torch.stack(list(out)).cpu().numpy()), bits(b.get_state()), info.cpu().numpy())
        assert (runs[name][0] != bits(np.stack(pl))).any()
        b.close()
    for name in runs:
        for k in range(3):
            np.testing.assert_array_equal(runs[name][k], runs["in place"][k], err_msg=name)


def test_dst_is_src_where_nothing_is_analysed(base):
    """the mortality scenario of test_dead_members_are_untouched_and_excluded: all of site 0 dead, one member of site 1, all
    but one of site 2; series with padded rows, whose padding keeps its sentinel"""
    from tests.test_gpu_configs import _scenario
    clim, ev, members = _scenario(base, True)
    M, rows, pad = 50, 96, 6
    members = np.concatenate([members[:M], members[:M], members[:M]]).copy()
    bad = np.r_[0:M, M + 5, 2 * M + 1:3 * M]
    members[bad, pi("leafAllocation")] = 0.8
    members[bad, pi("woodAllocation")] = 0.5
    b = sa.Batch(sa.flags_from(), 3, M, sa.F64, fast_math=True)
    for s in range(3):
        b.set_climate(s, clim)
        b.set_events(s, ev if s == 0 else [])
        b.set_params(s, members[s * M:(s + 1) * M])
    b.setup()
    planes, _ = b.run(0, clim.n_steps)
    ncol = 3 * M
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    ops = operators()[:2] + [sa.enkf_plane("gpp")]
    obs = np.array([[2.0, 5000.0, 10.0]] * 3)
    sd = np.array([[0.5, 500.0, 5.0]] * 3)
    first = clim.n_steps - rows                       # the last two days of the window
    src = torch.full((3, rows, ncol + pad), 4321.0, dtype=torch.float64, device=DEV)
    src[:, :, :ncol] = planes[:, first:, :ncol]
    dst = torch.full_like(src, -1234.5)
    src0 = src.cpu().numpy()
    info = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [(src, dst)], planes=planes, info_out=info)
    st1 = b.get_state()
    b.close()
    status = st0[:, 29]
    want, _, want_info, want_series = sr.analysis(st0, status, np.ones(3), 3, op_tuples(ops), SLOTS, [], obs, sd,
                                                  [z[:, :ncol] for z in src0], None, None, pl, prm)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    dead = status != 0
    assert dead[:M].all() and dead[M:2 * M].sum() == 1 and (~dead[2 * M:]).sum() == 1
    assert list(info[:, 0]) == [0, 1, 0]
    within(st1, want, st0, 3)
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(bits(src.cpu().numpy()), bits(src0))
    assert (got[:, :, ncol:] == -1234.5).all()                                   # the padding is not written
    untouched = dead | (np.arange(ncol) // M != 1)
    np.testing.assert_array_equal(bits(got[:, :, :ncol][:, :, untouched]), bits(src0[:, :, :ncol][:, :, untouched]))
    for k in range(3):
        assert series_within(got[k], want_series[k], src0[k], status, info, 3) == [True]      # site 1, one member dead


def test_a_series_of_a_pools_forecast_follows_the_analysed_pool(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=4)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    ops = operators()
    obs, sd = observe(st0, pl, carried_params(b), n_sites, ops, np.random.default_rng(8))
    soil = sa.POOLS.index("soilC")
    row = torch.tensor(st0[:, soil].reshape(1, -1).copy(), dtype=torch.float64, device=DEV)
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    infl = np.full(n_sites, 1.05)
    b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [row], planes=planes, inflation=infl, info_out=info)
    st1 = b.get_state()
    b.close()
    info = info.cpu().numpy()
    assert (info[:, 0] == 1).all() and (info[:, 3] == 0).all()                    # nobody kept on the forecast
    assert (st1[:, soil] > 0).all()                                               # no analysed soilC sits at the clip
    assert (st1[:, soil] != st0[:, soil]).any()
    # both sides are device results held to 1e-10 of this scale by the reference: 2e-10 between them
    moved = series_within(row.cpu().numpy(), st1[:, soil].reshape(1, -1), st0[:, soil].reshape(1, -1), st0[:, 29], info, n_sites,
                          bound=2e-10)
    assert all(moved)


def test_sites_whose_anomalies_do_not_fit_lds(base):
    """2 sites x 4 096 members x 8 operators: 256 KB of anomalies a site"""
    n_sites, M = 2, 4096
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=2)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm0 = carried_params(b)
    ops = operators() + [sa.enkf_pools(["soilC"]), sa.enkf_pools(["litterC"]), sa.enkf_pools(["coarseRootC", "fineRootC"]),
                         sa.enkf_plane("gpp")]
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(6), nan_obs=((1, 4),))
    series = [planes[0][20:24].clone(), planes[0][40:44].clone()]              # (NEE by day and by night)
    src = [z.cpu().numpy() for z in series]
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    infl = np.array([1.0, 1.1])
    b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, series, planes=planes, inflation=infl, info_out=info)
    st1 = b.get_state()
    b.close()
    want, _, want_info, want_series = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, [], obs, sd,
                                                  src, infl, None, pl, prm0)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    assert list(info[:, 0]) == [1, 1] and list(info[:, 1]) == [8, 7]
    within(st1, want, st0, n_sites)
    for k in range(2):
        assert all(series_within(series[k].cpu().numpy(), want_series[k], src[k], st0[:, 29], info, n_sites))


@pytest.mark.parametrize("M", [100, 300, 1500])
def test_the_other_team_shapes_against_the_reference(base, M):
    """the series kernel's forms that the sizes above do not take: 2 and 8 members a lane of a one-wave team (65..128 and
    257..512 members), 2 members a thread of the sixteen-wave team (1 025..2 048); none a multiple of the team, a dead member"""
    n_sites = 2
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=7)
    st = b.get_state()
    st[[3, M + M // 2], 29] = 3.0
    b.set_state(st)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm0 = carried_params(b)
    ops = operators()
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(9), nan_obs=((1, 2),))
    series = [planes[0][16:21].clone(), planes[2][16:21].clone()]
    src = [z.cpu().numpy() for z in series]
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    infl = np.array([1.1, 1.0])
    b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, series, planes=planes, inflation=infl, info_out=info)
    b.close()
    _, _, want_info, want_series = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, [], obs, sd,
                                               src, infl, None, pl, prm0)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    assert list(info[:, 0]) == [1, 1] and list(info[:, 2]) == [M - 1, M - 1]
    assert all(series_within(series[0].cpu().numpy(), want_series[0], src[0], st0[:, 29], info, n_sites))
    series_within(series[1].cpu().numpy(), want_series[1], src[1], st0[:, 29], info, n_sites)


def test_a_huge_sd_leaves_the_series(base):
    n_sites, M = 2, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    st0 = b.get_state()
    pl = np.stack([p.cpu().numpy() for p in planes])
    ops = operators()
    obs, _ = observe(st0, list(pl), carried_params(b), n_sites, ops, np.random.default_rng(2))
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    out = b.enkf_analysis_smooth(obs, np.full_like(obs, 1e30), ops, ANALYSED, [planes], planes=planes, info_out=info)
    got = torch.stack(list(out)).cpu().numpy()
    b.close()
    assert (info.cpu().numpy()[:, 0] == 1).all()
    assert (np.abs(got - pl) <= 1e-12 * np.abs(pl)).all()


def test_refusals(base):
    n_sites, M = 2, 64
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    ncol = b.ncol
    st0, prm0 = b.get_state(), b.get_params()
    L, h = b.L, b.h
    obs = torch.tensor(st0[:, 0].reshape(n_sites, M).mean(1, keepdims=True) * 1.01, dtype=torch.float64, device=DEV)
    sd = torch.tensor(st0[:, 0].reshape(n_sites, M).std(1, keepdims=True), dtype=torch.float64, device=DEV)
    arr = (_lib.EnkfObs * 1)(sa.enkf_pools(["plantWoodC"]))
    x = torch.arange(4 * ncol, dtype=torch.float64, device=DEV).reshape(4, ncol) + 1.0
    y, z = x.clone(), x.clone()
    x0 = x.cpu().numpy()
    BAD = _lib.ERR_BAD_ARGUMENT

    def call(series, n_series=None, null=False):
        desc = (_lib.EnkfSeries * max(len(series), 1))(*[_lib.EnkfSeries(*q) for q in series])
        return L.sipnet_batch_enkf_analysis_smooth(h, 1, arr, 1, 0, None, None, 0, 0, 0, obs.data_ptr(), sd.data_ptr(), None, None,
                                                   len(series) if n_series is None else n_series, None if null else desc, None,
                                                   b._stream())

    X, Y, Z = x.data_ptr(), y.data_ptr(), z.data_ptr()
    good = (X, X, 4, 0, ncol)
    for series, kw, word in [([good], dict(n_series=9), b"n_series"), ([good], dict(n_series=-1), b"n_series"),
                             ([good], dict(null=True), b"NULL series"),
                             ([good, (None, Y, 4, 0, ncol)], {}, b"series 1"), ([(X, None, 4, 0, ncol)], {}, b"series 0"),
                             ([good, (Y, Y, 0, 0, ncol)], {}, b"series 1"), ([(X, X, 4, 0, ncol - 1)], {}, b"series 0"),
                             ([(X, Z, 4, 0, ncol), (Y, Z, 4, 0, ncol)], {}, b"series 1"),
                             ([(X, Y, 4, 0, ncol), (Y, Z, 4, 0, ncol)], {}, b"series 0")]:
        assert call(series, **kw) == BAD, word
        msg = L.sipnet_last_error()
        assert b"sipnet_batch_enkf_analysis_smooth" in msg and word in msg, msg
    # nothing was written by any of them
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    for t in (x, y, z):
        np.testing.assert_array_equal(bits(t.cpu().numpy()), bits(x0))
    # n_series = 0 is the joint call, and a good series is taken
    twin, _ = forecast(base, n_sites, M, sa.F64, steps=48)
    assert twin.L.sipnet_batch_enkf_analysis_joint(twin.h, 1, arr, 1, 0, None, None, 0, 0, 0, obs.data_ptr(), sd.data_ptr(), None,
                                                   None, None, twin._stream()) == _lib.OK
    assert call([], n_series=0, null=True) == _lib.OK
    np.testing.assert_array_equal(bits(b.get_state()), bits(twin.get_state()))
    np.testing.assert_array_equal(bits(b.get_params()), bits(twin.get_params()))
    assert (b.get_state() != st0).any()
    twin.close()
    assert call([good]) == _lib.OK
    assert (x.cpu().numpy() != x0).any()
    with pytest.raises(ValueError):
        b.enkf_analysis_smooth(obs, sd, [arr[0]], ["plantWoodC"], [x[:, :ncol - 1]])
    with pytest.raises(ValueError):
        b.enkf_analysis_smooth(obs, sd, [arr[0]], ["plantWoodC"], [(x, y.float())])
    b.close()
    # more than 4 096 members per site: only with series
    big, _ = forecast(base, 1, 4352, sa.F64, steps=2)
    w = torch.ones((1, big.ncol), dtype=torch.float64, device=DEV)
    o1, s1 = torch.tensor([[1000.0]], dtype=torch.float64, device=DEV), torch.tensor([[100.0]], dtype=torch.float64, device=DEV)
    with pytest.raises(sa.SipnetError) as e:
        big.enkf_analysis_smooth(o1, s1, [arr[0]], ["plantWoodC"], [w])
    assert e.value.code == BAD and "4096" in str(e.value) and "series" in str(e.value)
    assert (w == 1.0).all()
    big.enkf_analysis_smooth(o1, s1, [arr[0]], ["plantWoodC"], [])
    big.close()
