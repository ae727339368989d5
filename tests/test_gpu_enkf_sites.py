"""The ensemble Kalman filter analysis of a batch of many sites on the GPU (sipnet_batch_enkf_analysis_sites): every site's
analysed pools against the numpy reference (tests/enkf_reference.py) applied to get_state and the planes; nothing else
touched; a forecast that continues from the analysis like one from set_state; the one-workgroup-per-site kernel against the
per-chunk launches bit for bit; the limits, dead members, the biomass rule, parameters behind a resampled index; the
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import enkf_reference as er
from tests.enkf_gpu_common import (ANALYSED, BASE, DEV, SLOTS, bits, carried_params, forecast, observe, op_tuples, operators,
                                   site_clim, sites_batch, within)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def force_path(b, path):
    if path == "group":
        b.debug_set_num_cus(1)
    elif path == "split":
        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


@pytest.mark.parametrize("path", ["auto", "group", "split"])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_every_site_against_the_reference(base, prec, path):
    n_sites, M = 32, 256
    b, planes = forecast(base, n_sites, M, prec)
    force_path(b, path)
    ops = operators()
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(5), nan_sites=(3, 17), nan_obs=((0, 1), (5, 3), (9, 0)))
    infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info)
    st1, rings1 = b.get_state(), b.get_rings()
    if path != "auto":
        assert b.pf_info()["fused"] == (1 if path == "group" else 0)
    b.close()
    want, want_info = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, infl, pl, prm)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert (want_info[:, 0] == 1).sum() == n_sites - 2 and (want_info[[3, 17], 0] == -1).all()
    within(st1, want, st0, n_sites)
    other = [k for k in range(32) if k not in SLOTS]
    np.testing.assert_array_equal(bits(st1[:, other]), bits(st0[:, other]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))
    untouched = np.repeat(want_info[:, 0] != 1, M)
    np.testing.assert_array_equal(bits(st1[untouched]), bits(st0[untouched]))
    assert np.abs(st1[:, SLOTS] - st0[:, SLOTS]).max() > 0


@pytest.mark.parametrize("M", [256, 1000])          # (256: the group path's working copies in LDS; 1000: in scratch)
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_group_and_split_paths_are_bit_identical_and_repeatable(base, prec, M):
    n_sites = 8
    results = []
    for path in ("group", "split", "group"):
        b, planes = forecast(base, n_sites, M, prec, steps=48, seed=3)
        force_path(b, path)
        st0 = b.get_state()
        pl = [p.cpu().numpy() for p in planes]
        ops = operators()
        obs, sd = observe(st0, pl, carried_params(b), n_sites, ops, np.random.default_rng(1), nan_obs=((2, 0),))
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=np.full(n_sites, 1.1), info_out=info)
        results.append((bits(b.get_state()), info.cpu().numpy()))
        b.close()
    for r in results[1:]:
        np.testing.assert_array_equal(r[0], results[0][0])
        np.testing.assert_array_equal(r[1], results[0][1])


def test_big_sites_split_path_against_the_reference(base):
    n_sites, M = 2, 5000                # beyond one workgroup's 4096: the per-chunk launches whatever the device
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=4)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    ops = operators()
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(2))
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes)          # the synchronous form
    st1 = b.get_state()
    b.close()
    want, _ = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, None, pl, prm)
    within(st1, want, st0, n_sites)


def test_forecast_after_the_analysis_equals_one_after_set_state(base):
    n_sites, M = 4, 256
    out = []
    for twin in range(2):
        b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=9)
        if twin == 0:
            st0 = b.get_state()
            pl = [p.cpu().numpy() for p in planes]
            obs, sd = observe(st0, pl, carried_params(b), n_sites, operators(), np.random.default_rng(4))
            b.enkf_analysis_sites(obs, sd, operators(), ANALYSED, planes=planes)
            after = b.get_state()
        else:
            b.set_state(after)
        p2, _ = b.run(96, 48)
        out.append(bits(p2.cpu().numpy()))
        b.close()
    np.testing.assert_array_equal(out[0], out[1])


def test_huge_sd_leaves_the_pools(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    st0 = b.get_state()
    obs = np.ones((n_sites, 4))
    b.enkf_analysis_sites(obs, np.full((n_sites, 4), 1e30), operators(), ANALYSED, planes=planes)
    st1 = b.get_state()
    b.close()
    assert (np.abs(st1[:, SLOTS] - st0[:, SLOTS]) <= 1e-12 * np.abs(st0[:, SLOTS]) + 1e-300).all()


def test_dead_members_are_untouched_and_excluded(base):
    """the forcing and events of the mortality scenario (its clear-cut on site 0); members whose parameters are invalid get a
    non-zero status and are not live: all of site 0, one of site 1, all but one of site 2"""
    from tests.test_gpu_configs import _scenario
    clim, ev, members = _scenario(base, True)
    M = 50
    members = np.concatenate([members[:M], members[:M], members[:M]]).copy()
    bad = np.r_[0:M, M + 5, 2 * M + 1:3 * M]
    members[bad, pi("leafAllocation")] = 0.8
    members[bad, pi("woodAllocation")] = 0.5                             # sum > 1: sipnet.c:1117-1122
    b = sa.Batch(sa.flags_from(), 3, M, sa.F64, fast_math=True)
    for s in range(3):
        b.set_climate(s, clim)
        b.set_events(s, ev if s == 0 else [])
        b.set_params(s, members[s * M:(s + 1) * M])
    b.setup()
    planes, _ = b.run(0, clim.n_steps)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    ops = operators()[:2] + [sa.enkf_plane("gpp")]
    obs = np.array([[2.0, 5000.0, 10.0]] * 3)
    sd = np.array([[0.5, 500.0, 5.0]] * 3)
    info = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, info_out=info)
    st1 = b.get_state()
    b.close()
    status = st0[:, 29]
    want, want_info = er.analysis(st0, status, np.ones(3), 3, op_tuples(ops), SLOTS, obs, sd, None, pl, prm)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    dead = status != 0
    assert dead[:M].all() and dead[M:2 * M].sum() == 1 and (~dead[2 * M:]).sum() == 1
    assert list(info[:, 0]) == [0, 1, 0]
    np.testing.assert_array_equal(bits(st1[dead]), bits(st0[dead]))
    np.testing.assert_array_equal(bits(st1[2 * M:]), bits(st0[2 * M:]))
    within(st1, want, st0, 3)


def test_wood_far_below_keeps_members_on_their_forecast_and_restarts_accept_them(base):
    n_sites, M = 2, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=6)
    st0 = b.get_state()
    wood = st0[:, 0] + st0[:, 12]
    ops = [sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"])]
    w = wood.reshape(n_sites, M)
    sd = w.std(1, keepdims=True)
    obs = np.zeros((n_sites, 1))
    for s in range(n_sites):       # far enough below that the reference keeps some of the site's members on their forecast
        lo, hi = 0.0, 4.0          # (bisection: none kept at obs = mean, all kept at obs = -3 mean)
        for _ in range(80):
            f = 0.5 * (lo + hi)
            obs[s] = w[s].mean() * (1.0 - f)
            kept = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd)[1][s, 3]
            if 0 < kept < M:
                break
            lo, hi = (f, hi) if kept == 0 else (lo, f)
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, info_out=info)
    st1 = b.get_state()
    want, want_info = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd)
    info = info.cpu().numpy()
    np.testing.assert_array_equal(info, want_info)
    assert (info[:, 3] > 0).all() and (info[:, 3] < M).all()
    within(st1, want, st0, n_sites)
    cks = [[b.export_restart(s, m, 96) for m in range(M)] for s in range(n_sites)]
    members = synth.perturbed_params(base, n_sites * M, seed=6)
    b.close()
    b2 = sa.Batch(sa.flags_from(), n_sites, M, sa.F64, fast_math=True)     # the rest of the forcing, resumed
    for s in range(n_sites):
        b2.set_climate(s, site_clim(s).slice(96, 48 * 8))
        b2.set_params(s, members[s * M:(s + 1) * M])
        b2.set_resume(s, cks[s][0])
    b2.setup()
    for s in range(n_sites):
        b2.import_restart(s, cks[s])                                       # (refuses a status its pools contradict)
    np.testing.assert_array_equal(bits(b2.get_state()[:, :13]), bits(st1[:, :13]))
    b2.close()


def test_lai_reads_the_parameters_behind_a_resampled_index(base):
    n_sites, M = 4, 256
    members = synth.perturbed_params(base, n_sites * M, seed=12)
    members[:, pi("leafCSpWt")] *= np.linspace(0.5, 1.5, n_sites * M)
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 48)
    nee = planes[0]
    tot = nee.double().sum(0).cpu().numpy().reshape(n_sites, M)
    b.pf_analysis_sites(nee, np.median(tot, 1), tot.std(1) * 0.3, [0.1, 0.3, 0.5, 0.7], with_params=True)
    st0 = b.get_state()
    prm = carried_params(b)
    ops = [sa.enkf_pools(["plantLeafC"], divide_by="leafCSpWt")]
    lai = st0[:, 1] / prm[:, pi("leafCSpWt")]
    obs = lai.reshape(n_sites, M).mean(1, keepdims=True) * 1.2
    sd = lai.reshape(n_sites, M).std(1, keepdims=True) * 0.5
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED)
    st1 = b.get_state()
    b.close()
    own = members[:, pi("leafCSpWt")]
    assert not np.allclose(prm[:, pi("leafCSpWt")], own)                 # resampled: not the column's own row
    want, _ = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, None, None, prm)
    within(st1, want, st0, n_sites)


def test_refusals(base):
    n_sites, M = 2, 64
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    st0 = b.get_state()
    L, h = b.L, b.h
    obs = torch.ones((n_sites, 1), dtype=torch.float64, device=DEV)
    sd = torch.ones((n_sites, 1), dtype=torch.float64, device=DEV)
    P = [p.data_ptr() for p in planes]

    def call(ops, mask=1, planes_=P, n_steps=48, ld=None, o=obs, s=sd, n_obs=None, h=h):
        arr = (_lib.EnkfObs * max(len(ops), 1))(*ops) if ops is not None else None
        pp = None if planes_ is None else (C.c_void_p * 3)(*planes_)
        return L.sipnet_batch_enkf_analysis_sites(h, (len(ops) if ops else 1) if n_obs is None else n_obs, arr, mask, pp, 0, n_steps,
                                                  b.ncol if ld is None else ld, o.data_ptr() if o is not None else None,
                                                  s.data_ptr() if s is not None else None, None, None, b._stream())

    wood = sa.enkf_pools(["plantWoodC"])
    nee = sa.enkf_plane("nee")
    BAD = _lib.ERR_BAD_ARGUMENT
    assert call(None) == BAD
    assert call([wood], o=None) == BAD
    assert call([wood], s=None) == BAD
    assert call([wood], n_obs=0) == BAD
    assert call([wood] * 17) == BAD
    assert call([wood], mask=0) == BAD
    assert call([wood], mask=1 << 13) == BAD
    assert call([_lib.EnkfObs(0, 0, 0, -1, 1.0)]) == BAD
    assert call([_lib.EnkfObs(0, 1 << 14, 0, -1, 1.0)]) == BAD
    assert call([_lib.EnkfObs(2, 1, 0, -1, 1.0)]) == BAD
    assert call([_lib.EnkfObs(0, 1, 0, _lib.NPARAMS, 1.0)]) == BAD
    assert call([_lib.EnkfObs(0, 1, 0, -2, 1.0)]) == BAD
    assert call([_lib.EnkfObs(1, 0, 3, -1, 1.0)]) == BAD
    assert call([nee], planes_=None) == BAD
    assert call([nee], planes_=[None, P[1], P[2]]) == BAD
    assert call([nee], n_steps=0) == BAD
    assert call([nee], ld=b.ncol - 1) == BAD
    assert call([wood], planes_=None, n_steps=0, ld=0) == _lib.OK            # (no plane read: no plane arguments needed)
    st_ok = b.get_state()
    # the synchronous form refuses a bad sd before anything is written
    bad_sd = torch.tensor([[1.0], [-1.0]], dtype=torch.float64, device=DEV)
    assert call([wood], s=bad_sd) == BAD
    assert b"site 1" in L.sipnet_last_error()
    np.testing.assert_array_equal(bits(b.get_state()), bits(st_ok))
    # ... and the asynchronous form reports it, leaving that site untouched
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites([[1.0], [1.0]], [[1.0], [-1.0]], [wood], ["plantWoodC"], info_out=info)
    assert list(info[:, 0].cpu().numpy()) == [1, -2]
    st2 = b.get_state()
    np.testing.assert_array_equal(bits(st2[M:]), bits(st_ok[M:]))
    with pytest.raises(sa.SipnetError):
        b.enkf_analysis_sites([[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"], inflation=[1.0, 0.5])
    b.close()
    assert st0.shape == st_ok.shape
    # a batch connected across ranks is refused
    c, pc = forecast(base, 1, 64, sa.F64, steps=48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.enkf_analysis_sites([[1.0]], [[1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and "connected" in str(e.value)
    c.close()
    # more than 4 194 304 members (refused before anything is launched: the batch is not even set up)
    big = sa.Batch(sa.flags_from(), 2, (1 << 21) + 1, sa.F32_MIXED)
    with pytest.raises(sa.SipnetError) as e:
        big.enkf_analysis_sites([[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and "4194304" in str(e.value)
    big.close()
