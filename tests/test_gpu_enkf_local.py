"""The localized ensemble Kalman filter across the sites of a batch on the GPU (sipnet_batch_enkf_analysis_local): every site
against the numpy reference (tests/enkf_local_reference.py) on a grid of sites with Gaspari-Cohn tapers; empty lists bit for
bit equal to sipnet_batch_enkf_analysis_sites; the levelled schedule bit for bit equal to one slot per launch, and repeatable;
reached and unreached sites, dead members, bad input; the refusals; a forecast that continues from the analysis like one from
set_state.  The forecasts, observations and lists come from tests/enkf_gpu_common.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import enkf_local_reference as lr
from tests.enkf_gpu_common import (ANALYSED, BASE, DEV, OTHER, SLOTS, bits, carried_params, empty, forecast, grid, observe,
                                   op_tuples, operators, sites_batch, within)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_every_site_against_the_reference(base, prec):
    n_sites, M = 48, 256
    b, planes = forecast(base, n_sites, M, prec)
    ops = operators()
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites, far=(47,)), 45.0)
    assert 6.0 < np.diff(ptr).mean() < 10.0 and ptr[48] == ptr[47]
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    assert loc.n_levels == sa.enkf_local_schedule(ptr, nbr, rho, len(ops))[1]
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(5), nan_sites=(3, 17, 30, 47),
                      nan_obs=((0, 1), (5, 3), (9, 0)))
    infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info)
    st1, rings1 = b.get_state(), b.get_rings()
    b.close()
    assert loc.h is None                                        # (closed with its batch)
    want, want_info = lr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr, nbr, rho,
                                  infl, pl, prm)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert (want_info[[3, 17, 30], 0] == 1).all() and (want_info[[3, 17, 30], 1] == 0).all()   # reached, no own obs
    assert want_info[47, 0] == -1
    within(st1, want, st0, n_sites)
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))
    untouched = np.repeat(want_info[:, 0] != 1, M)
    np.testing.assert_array_equal(bits(st1[untouched]), bits(st0[untouched]))
    for s in (3, 17, 30):
        assert np.abs(st1[s * M:(s + 1) * M, SLOTS] - st0[s * M:(s + 1) * M, SLOTS]).max() > 0


@pytest.mark.parametrize("M", [256, 1000])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_empty_lists_are_bit_identical_to_the_per_site_call(base, prec, M):
    n_sites = 8
    results = []
    for local in (False, True):
        b, planes = forecast(base, n_sites, M, prec, steps=48, seed=3)
        st0 = b.get_state()
        ops = operators()
        obs, sd = observe(st0, [p.cpu().numpy() for p in planes], carried_params(b), n_sites, ops, np.random.default_rng(1),
                          nan_sites=(6,), nan_obs=((2, 0),))
        sd[4, 1] = -1.0                                          # a -2 site
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        infl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
        if local:
            loc = b.enkf_localization(*empty(n_sites), len(ops))
            assert loc.n_levels == len(ops)
            b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info)
        else:
            b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info)
        results.append((bits(b.get_state()), info.cpu().numpy()))
        b.close()
    assert list(results[0][1][:, 0]) == [1, 1, 1, 1, -2, 1, -1, 1]
    np.testing.assert_array_equal(results[1][1], results[0][1])
    np.testing.assert_array_equal(results[1][0], results[0][0])


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_levels_equal_one_slot_per_launch_and_calls_repeat(base, prec):
    n_sites, M = 24, 256
    b, planes = forecast(base, n_sites, M, prec, steps=48, seed=7)
    ops = operators()
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites), 60.0)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    assert loc.n_levels < n_sites * len(ops)                     # (slots do run side by side)
    st0 = b.get_state()
    obs, sd = observe(st0, [p.cpu().numpy() for p in planes], carried_params(b), n_sites, ops, np.random.default_rng(2),
                      nan_sites=(4,), nan_obs=((1, 2),))
    out = []
    for serial in (False, True, False):
        b.set_state(st0)
        loc.debug_serial(serial)
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, inflation=np.full(n_sites, 1.05), info_out=info)
        out.append((bits(b.get_state()), info.cpu().numpy()))
    loc.close()
    b.close()
    assert np.abs(out[0][0].view(np.float64) - st0).max() > 0
    for r in out[1:]:
        np.testing.assert_array_equal(r[0], out[0][0])
        np.testing.assert_array_equal(r[1], out[0][1])


def test_a_reached_site_moves_and_an_unreached_one_does_not(base):
    n_sites, M = 3, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=5)
    ops = operators()
    ptr, nbr, rho = np.array([0, 1, 1, 1]), np.array([1], np.int32), np.array([0.7])   # site 0 reaches site 1 only
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(6), nan_sites=(1, 2))
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, info_out=info)
    st1, rings1 = b.get_state(), b.get_rings()
    b.close()
    info = info.cpu().numpy()
    assert list(info[:, 0]) == [1, 1, -1] and list(info[:, 1]) == [4, 0, 0]
    want, want_info = lr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr, nbr, rho,
                                  None, pl, prm)
    np.testing.assert_array_equal(info, want_info)
    within(st1, want, st0, n_sites)
    assert np.abs(st1[M:2 * M, SLOTS] - st0[M:2 * M, SLOTS]).max() > 0
    np.testing.assert_array_equal(bits(st1[2 * M:]), bits(st0[2 * M:]))
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))


def test_dead_members_are_excluded_from_the_cross_site_sums(base):
    """members with invalid parameters get a non-zero status and are not live: 20 of the observed site 0, 7 others of its
    neighbour site 1; J = both live"""
    n_sites, M = 3, 128
    members = synth.perturbed_params(base, n_sites * M, seed=14)
    bad = np.r_[0:20, M + 40:M + 47]
    members[bad, pi("leafAllocation")] = 0.8
    members[bad, pi("woodAllocation")] = 0.5                             # sum > 1: sipnet.c:1117-1122
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 96)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    dead = st0[:, 29] != 0
    assert dead[:20].all() and dead[M + 40:M + 47].all() and dead.sum() == 27
    ops = operators()
    ptr, nbr, rho = np.array([0, 2, 3, 4]), np.array([1, 2, 0, 1], np.int32), np.array([0.9, 0.4, 0.9, 0.6])
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(9), nan_sites=(1, 2))
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, info_out=info)
    st1 = b.get_state()
    b.close()
    want, want_info = lr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr, nbr, rho,
                                  None, pl, prm)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert list(want_info[:, 2]) == [M - 20, M - 7, M]
    within(st1, want, st0, n_sites)
    np.testing.assert_array_equal(bits(st1[dead]), bits(st0[dead]))
    # site 1's members 0..19 are live there but dead at the observed site: outside J, they get no increment
    np.testing.assert_array_equal(bits(st1[M:M + 20]), bits(st0[M:M + 20]))
    assert np.abs(st1[M + 20:M + 40, SLOTS] - st0[M + 20:M + 40, SLOTS]).max() > 0


def test_bad_input_site_is_never_a_target(base):
    n_sites, M = 3, 128
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=2)
    wood = sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"])
    ptr, nbr, rho = np.array([0, 2, 3, 4]), np.array([1, 2, 0, 1], np.int32), np.array([1.0, 1.0, 1.0, 1.0])
    loc = b.enkf_localization(ptr, nbr, rho, 1)
    st0 = b.get_state()
    w = (st0[:, 0] + st0[:, 12]).reshape(n_sites, M)
    obs = (w.mean(1) * 1.05)[:, None]
    obs[2] = np.nan
    sd = (w.std(1) + 1.0)[:, None]
    sd[1] = -1.0                                                       # site 1: bad input
    with pytest.raises(sa.SipnetError) as e:                           # the synchronous form refuses, writes nothing
        b.enkf_analysis_local(loc, obs, sd, [wood], ANALYSED)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 1" in str(sa.lib().sipnet_last_error())
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_local(loc, obs, sd, [wood], ANALYSED, info_out=info)
    st1 = b.get_state()
    b.close()
    assert list(info[:, 0].cpu().numpy()) == [1, -2, 1]
    np.testing.assert_array_equal(bits(st1[M:2 * M]), bits(st0[M:2 * M]))
    assert np.abs(st1[2 * M:, SLOTS] - st0[2 * M:, SLOTS]).max() > 0
    want, want_info = lr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples([wood]), SLOTS, obs, sd, ptr, nbr, rho)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    within(st1, want, st0, n_sites)


def test_refusals(base):
    n_sites, M = 2, 64
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    wood = sa.enkf_pools(["plantWoodC"])
    ptr, nbr, rho = np.array([0, 1, 2]), np.array([1, 0], np.int32), np.array([0.5, 0.5])
    BAD = _lib.ERR_BAD_ARGUMENT
    with pytest.raises(sa.SipnetError) as e:                           # a list the library refuses
        b.enkf_localization(ptr, np.array([0, 0], np.int32), rho, 1)
    assert e.value.code == BAD
    loc1 = b.enkf_localization(ptr, nbr, rho, 1)
    loc2 = b.enkf_localization(ptr, nbr, rho, 2)
    st0 = b.get_state()
    with pytest.raises(sa.SipnetError) as e:                           # another n_obs
        b.enkf_analysis_local(loc2, [[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and b"n_obs" in sa.lib().sipnet_last_error()
    other, _ = forecast(base, n_sites, M, sa.F64, steps=48)
    with pytest.raises(sa.SipnetError) as e:                           # another batch's localization
        other.enkf_analysis_local(loc1, [[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and b"another batch" in sa.lib().sipnet_last_error()
    other.close()
    L = b.L
    obs = torch.ones((n_sites, 1), dtype=torch.float64, device=DEV)
    arr = (_lib.EnkfObs * 1)(wood)
    assert L.sipnet_batch_enkf_analysis_local(b.h, None, 1, arr, 1, None, 0, 0, 0, C.c_void_p(obs.data_ptr()),
                                              C.c_void_p(obs.data_ptr()), None, None, b._stream()) == BAD
    assert L.sipnet_batch_enkf_analysis_local(b.h, loc1.h, 1, arr, 0, None, 0, 0, 0, C.c_void_p(obs.data_ptr()),
                                              C.c_void_p(obs.data_ptr()), None, None, b._stream()) == BAD   # (per-site checks)
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    b.close()
    assert loc1.h is None and loc2.h is None
    # more than 4096 members per site (refused before anything is launched: the batch is not even set up)
    big = sa.Batch(sa.flags_from(), 1, 4097, sa.F64)
    loc = big.enkf_localization([0, 0], [], [], 1)
    with pytest.raises(sa.SipnetError) as e:
        big.enkf_analysis_local(loc, [[1.0]], [[1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and "4096" in str(sa.lib().sipnet_last_error())
    big.close()
    # a batch connected across ranks
    c, _ = forecast(base, 1, 64, sa.F64, steps=48)
    loc = c.enkf_localization([0, 0], [], [], 1)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.enkf_analysis_local(loc, [[1.0]], [[1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and "connected" in str(sa.lib().sipnet_last_error())
    c.close()


def test_forecast_after_the_analysis_equals_one_after_set_state(base):
    n_sites, M = 6, 256
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites), 60.0)
    out = []
    for twin in range(2):
        b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=9)
        if twin == 0:
            st0 = b.get_state()
            pl = [p.cpu().numpy() for p in planes]
            obs, sd = observe(st0, pl, carried_params(b), n_sites, operators(), np.random.default_rng(4), nan_sites=(2,))
            loc = b.enkf_localization(ptr, nbr, rho, 4)
            b.enkf_analysis_local(loc, obs, sd, operators(), ANALYSED, planes=planes)
            after = b.get_state()
            assert np.abs(after[:, SLOTS] - st0[:, SLOTS]).max() > 0
        else:
            b.set_state(after)
        p2, _ = b.run(96, 48)
        out.append(bits(p2.cpu().numpy()))
        b.close()
    np.testing.assert_array_equal(out[0], out[1])
