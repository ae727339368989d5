"""The block-local ensemble Kalman filter analysis on the GPU (sipnet_batch_enkf_analysis_block): every site against the numpy
reference (tests/enkf_block_reference.py) on a grid of sites with Gaspari-Cohn tapers, in both precisions, at member counts that
are and are not multiples of 256, with the small matrices in LDS and in global memory; empty lists against
sipnet_batch_enkf_analysis_sites and the complete graph with rho = 1 against sipnet_batch_enkf_analysis_local; repeatable, and
independent of sites out of reach; dropped rows, untouched sites, the row cap, the refusals; a forecast that continues from the
analysis.  The forecasts, observations and lists come from tests/enkf_gpu_common.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import enkf_block_reference as br
from tests.enkf_gpu_common import (ANALYSED, BASE, DEV, OTHER, SLOTS, bits, carried_params, empty, forecast, grid, observe,
                                   op_tuples, operators, sites_batch, within)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def complete(n_sites, rho=1.0, of=None):
    """every one of the first n_sites sites lists every other; the sites up to `of` list nobody"""
    nbr = np.array([t for s in range(n_sites) for t in range(n_sites) if t != s], dtype=np.int32)
    ptr = np.arange(n_sites + 1, dtype=np.int64) * (n_sites - 1)
    if of:
        ptr = np.concatenate([ptr, np.full(of - n_sites, ptr[-1])])
    return ptr, nbr, (np.full(nbr.size, rho) if np.isscalar(rho) else rho)


def run_block(b, loc, obs, sd, ops, planes, infl=None, analysed=ANALYSED):
    info = torch.full((b.n_sites, 4), -9, dtype=torch.int32, device=DEV)
    rows = torch.full((b.n_sites, 2), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_block(loc, obs, sd, ops, analysed, planes=planes, inflation=infl, info_out=info, rows_out=rows)
    return b.get_state(), info.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_every_site_against_the_reference(base, prec):
    n_sites, M = 48, 256
    b, planes = forecast(base, n_sites, M, prec)
    ops = operators()
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites, far=(47,)), 45.0)
    assert 6.0 < np.diff(ptr).mean() < 10.0 and ptr[48] == ptr[47]
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    assert loc.max_rows == sa.enkf_local_rows(ptr, nbr, len(ops))[1] == br.row_counts(n_sites, len(ops), ptr, nbr).max()
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(5), nan_sites=(3, 17, 30, 47),
                      nan_obs=((0, 1), (5, 3), (9, 0)))
    infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
    st1, info, rows = run_block(b, loc, obs, sd, ops, planes, infl)
    rings1 = b.get_rings()
    assert b.pf_info()["fused"] == 1                              # (36 rows at most: the matrices are in LDS)
    b.close()
    assert loc.h is None                                        # (closed with its batch)
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, infl, pl, prm)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    assert (want_info[[3, 17, 30], 0] == 1).all() and (want_info[[3, 17, 30], 1] == 0).all()   # reached, no own obs
    assert want_info[47, 0] == -1 and want_rows[:, 0].max() >= 20 and (want_rows[:, 1] == 0).all()
    within(st1, want, st0, n_sites)
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))
    untouched = np.repeat(want_info[:, 0] != 1, M)
    np.testing.assert_array_equal(bits(st1[untouched]), bits(st0[untouched]))
    for s in (3, 17, 30):
        assert np.abs(st1[s * M:(s + 1) * M, SLOTS] - st0[s * M:(s + 1) * M, SLOTS]).max() > 0


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_a_member_count_that_is_no_multiple_of_256(base, prec):
    n_sites, M = 8, 1000
    b, planes = forecast(base, n_sites, M, prec, steps=48, seed=3)
    ops = operators()
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites), 60.0)
    assert np.diff(ptr).min() >= 2
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(1), nan_sites=(6,), nan_obs=((2, 0),))
    infl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
    st1, info, rows = run_block(b, loc, obs, sd, ops, planes, infl)
    b.close()
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, infl, pl, prm)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    within(st1, want, st0, n_sites)
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_the_row_cap_and_both_homes_of_the_matrices(base, prec):
    """33 sites, 4 operators, all 13 pools analysed.  Sites 0..31 list each other: 128 rows, the cap, and (128 + 26) x 128
    doubles of matrices, more than a compute unit's LDS: they live in global memory.  Rings of 3 neighbours: 16 rows, in LDS.
    All 33 listing each other: 132 rows, refused before anything is written."""
    n_sites, M = 33, 64
    pools13 = list(sa.POOLS[:13])
    slots = list(range(13))
    b, planes = forecast(base, n_sites, M, prec, steps=48, seed=11)
    ops = operators()
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(8))
    rng = np.random.default_rng(3)
    ptr, nbr, _ = complete(32, of=33)
    rho = rng.uniform(0.05, 1.0, nbr.size)
    at_cap = b.enkf_localization(ptr, nbr, rho, len(ops))
    assert at_cap.max_rows == sa.ENKF_BLOCK_MAX_ROWS == 128
    ring_nbr = np.array([[(s + d) % n_sites for d in (1, 2, 5)] for s in range(n_sites)])
    ring_nbr.sort(1)
    ring = (np.arange(n_sites + 1, dtype=np.int64) * 3, ring_nbr.reshape(-1).astype(np.int32), rng.uniform(0.05, 1.0, 3 * n_sites))
    small = b.enkf_localization(*ring, len(ops))
    assert small.max_rows == 16
    for loc, lists, fused in ((at_cap, (ptr, nbr, rho), 0), (small, ring, 1)):
        b.set_state(st0)
        st1, info, rows = run_block(b, loc, obs, sd, ops, planes, None, pools13)
        assert b.pf_info()["fused"] == fused
        want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), slots, obs, sd,
                                                 *lists, None, pl, prm)
        np.testing.assert_array_equal(info, want_info)
        np.testing.assert_array_equal(rows, want_rows)
        assert want_rows[:, 0].max() == loc.max_rows
        within(st1, want, st0, n_sites, slots)
        np.testing.assert_array_equal(bits(st1[:, 13:]), bits(st0[:, 13:]))
    b.set_state(st0)
    over = b.enkf_localization(*complete(33), len(ops))                # (creating it succeeds)
    assert over.max_rows == 132
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    with pytest.raises(sa.SipnetError) as e:
        b.enkf_analysis_block(over, obs, sd, ops, pools13, planes=planes, info_out=info)
    msg = sa.lib().sipnet_last_error().decode()
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "132" in msg and "128" in msg
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    assert (info.cpu().numpy() == -9).all()
    b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_empty_lists_against_the_per_site_call_and_rho_one_against_the_serial_call(base, prec):
    n_sites, M = 6, 256
    ops = operators()
    for lists, other in ((empty(n_sites), "sites"), (complete(n_sites), "local")):
        b, planes = forecast(base, n_sites, M, prec, steps=48, seed=3)
        st0 = b.get_state()
        obs, sd = observe(st0, [p.cpu().numpy() for p in planes], carried_params(b), n_sites, ops, np.random.default_rng(1),
                          nan_obs=((2, 0),))
        infl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
        loc = b.enkf_localization(*lists, len(ops))
        got, info, rows = run_block(b, loc, obs, sd, ops, planes, infl)
        b.set_state(st0)
        info2 = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        if other == "sites":
            b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info2)
            np.testing.assert_array_equal(rows, [[4, 0], [4, 0], [3, 0], [4, 0], [4, 0], [4, 0]])
        else:
            b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info2)
            np.testing.assert_array_equal(rows, np.tile([23, 0], (n_sites, 1)))
        want = b.get_state()
        b.close()
        np.testing.assert_array_equal(info, info2.cpu().numpy())
        assert np.abs(want[:, SLOTS] - st0[:, SLOTS]).max() > 0
        within(got, want, st0, n_sites)
        np.testing.assert_array_equal(bits(got[:, OTHER]), bits(want[:, OTHER]))


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_calls_repeat_and_sites_out_of_reach_change_nothing(base, prec):
    n_sites, more, M = 16, 32, 256
    ops = operators()
    ptr, nbr, rho = sa.gaspari_cohn(*grid(n_sites), 60.0)
    b, planes = forecast(base, n_sites, M, prec, steps=48, seed=7, of=more)
    st0 = b.get_state()
    obs, sd = observe(st0, [p.cpu().numpy() for p in planes], carried_params(b), n_sites, ops, np.random.default_rng(2),
                      nan_sites=(4,), nan_obs=((1, 2),))
    infl = np.full(n_sites, 1.05)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    out = []
    for _ in range(2):
        b.set_state(st0)
        out.append(run_block(b, loc, obs, sd, ops, planes, infl))
    b.close()
    assert np.abs(out[0][0] - st0).max() > 0
    np.testing.assert_array_equal(bits(out[1][0]), bits(out[0][0]))
    np.testing.assert_array_equal(out[1][1], out[0][1])
    np.testing.assert_array_equal(out[1][2], out[0][2])
    # the same sites first in a larger batch; the further sites list each other densely, and none of the first sixteen
    b2, planes2 = forecast(base, more, M, prec, steps=48, seed=7)
    st2 = b2.get_state()
    np.testing.assert_array_equal(bits(st2[:n_sites * M]), bits(st0))
    p2, n2, r2 = complete(more - n_sites, 0.8)
    ptr2 = np.concatenate([ptr, ptr[-1] + p2[1:]])
    nbr2 = np.concatenate([nbr, n2 + n_sites]).astype(np.int32)
    rho2 = np.concatenate([rho, r2])
    obs2, sd2 = observe(st2, [p.cpu().numpy() for p in planes2], carried_params(b2), more, ops, np.random.default_rng(9))
    obs2[:n_sites], sd2[:n_sites] = obs, sd
    loc2 = b2.enkf_localization(ptr2, nbr2, rho2, len(ops))
    assert loc2.max_rows > loc.max_rows
    st3, info3, rows3 = run_block(b2, loc2, obs2, sd2, ops, planes2, np.full(more, 1.05))
    b2.close()
    np.testing.assert_array_equal(bits(st3[:n_sites * M]), bits(out[0][0]))
    np.testing.assert_array_equal(info3[:n_sites], out[0][1])
    np.testing.assert_array_equal(rows3[:n_sites], out[0][2])
    assert (rows3[n_sites:, 0] == 4 * (more - n_sites)).all()


def test_a_member_dead_at_one_source_only(base):
    """site 1 lists sites 0 and 2 and loses members 40..46 (invalid parameters); they live at 0 and 2, so site 1's rows are
    dropped there and both are analysed from their own rows, as is site 1, which nobody lists: the per-site analysis"""
    n_sites, M = 3, 128
    members = synth.perturbed_params(base, n_sites * M, seed=14)
    bad = np.r_[M + 40:M + 47]
    members[bad, pi("leafAllocation")] = 0.8
    members[bad, pi("woodAllocation")] = 0.5                             # sum > 1: sipnet.c:1117-1122
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 96)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    dead = st0[:, 29] != 0
    assert dead[M + 40:M + 47].all() and dead.sum() == 7
    ops = operators()
    ptr, nbr, rho = np.array([0, 0, 2, 2]), np.array([0, 2], np.int32), np.array([0.9, 0.4])
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(9))
    st1, info, rows = run_block(b, loc, obs, sd, ops, planes)
    np.testing.assert_array_equal(rows, [[4, 4], [4, 0], [4, 4]])
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, None, pl, prm)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    assert list(info[:, 2]) == [M, M - 7, M]
    within(st1, want, st0, n_sites)
    np.testing.assert_array_equal(bits(st1[dead]), bits(st0[dead]))
    b.set_state(st0)
    info2 = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, info_out=info2)
    per_site = b.get_state()
    np.testing.assert_array_equal(info, info2.cpu().numpy())
    within(st1, per_site, st0, n_sites)
    # the other way round (0 and 2 list 1): site 1's members all live at both, so it takes their rows
    b.set_state(st0)
    ptr, nbr, rho = np.array([0, 1, 1, 2]), np.array([1, 1], np.int32), np.array([0.9, 0.4])
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    st2, info, rows = run_block(b, loc, obs, sd, ops, planes)
    b.close()
    np.testing.assert_array_equal(rows, [[4, 0], [12, 0], [4, 0]])
    want, _, _ = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr, nbr, rho, None, pl,
                             prm)
    within(st2, want, st0, n_sites)
    assert np.abs(st2[M:2 * M, SLOTS] - st1[M:2 * M, SLOTS]).max() > 0
    np.testing.assert_array_equal(bits(st2[dead]), bits(st0[dead]))


def test_sites_that_are_not_analysed_stay_bit_identical(base):
    """site 1: no observation and unreached (-1); site 2: a bad sd (-2); site 3: one live member (0); site 4: reached, no
    observation of its own (1); a NaN slot at site 0"""
    n_sites, M = 6, 128
    members = synth.perturbed_params(base, n_sites * M, seed=21)
    bad = np.r_[3 * M + 1:4 * M]
    members[bad, pi("leafAllocation")] = 0.8
    members[bad, pi("woodAllocation")] = 0.5
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 96)
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm = carried_params(b)
    ops = operators()
    # 0 lists 2, 3, 4; 1 lists 0 (but has no observation); 2 lists 0 (bad input: not used); 5 lists 3 and 4
    ptr, nbr, rho = np.array([0, 3, 4, 5, 5, 5, 7]), np.array([2, 3, 4, 0, 0, 3, 4], np.int32), np.full(7, 0.7)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    obs, sd = observe(st0, pl, prm, n_sites, ops, np.random.default_rng(6), nan_sites=(1, 4), nan_obs=((0, 2),))
    sd[2, 1] = -1.0
    with pytest.raises(sa.SipnetError) as e:                           # the synchronous form refuses, writes nothing
        b.enkf_analysis_block(loc, obs, sd, ops, ANALYSED, planes=planes)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 2" in str(sa.lib().sipnet_last_error())
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    st1, info, rows = run_block(b, loc, obs, sd, ops, planes)
    rings1 = b.get_rings()
    b.close()
    assert list(info[:, 0]) == [1, -1, -2, 0, 1, 1] and list(info[:, 1]) == [3, 0, 0, 0, 0, 4]
    np.testing.assert_array_equal(rows, [[3, 0], [0, 0], [0, 0], [0, 0], [7, 0], [4, 0]])
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, None, pl, prm)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    within(st1, want, st0, n_sites)
    for s in (1, 2, 3):
        np.testing.assert_array_equal(bits(st1[s * M:(s + 1) * M]), bits(st0[s * M:(s + 1) * M]))
    assert np.abs(st1[4 * M:5 * M, SLOTS] - st0[4 * M:5 * M, SLOTS]).max() > 0
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))


def test_refusals(base):
    n_sites, M = 2, 64
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    wood = sa.enkf_pools(["plantWoodC"])
    ptr, nbr, rho = np.array([0, 1, 2]), np.array([1, 0], np.int32), np.array([0.5, 0.5])
    BAD = _lib.ERR_BAD_ARGUMENT
    loc1 = b.enkf_localization(ptr, nbr, rho, 1)
    loc2 = b.enkf_localization(ptr, nbr, rho, 2)
    st0 = b.get_state()
    with pytest.raises(sa.SipnetError) as e:                           # another n_obs
        b.enkf_analysis_block(loc2, [[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and b"n_obs" in sa.lib().sipnet_last_error()
    other, _ = forecast(base, n_sites, M, sa.F64, steps=48)
    with pytest.raises(sa.SipnetError) as e:                           # another batch's localization
        other.enkf_analysis_block(loc1, [[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and b"another batch" in sa.lib().sipnet_last_error()
    other.close()
    with pytest.raises(ValueError):                                    # rows_out of the wrong shape
        b.enkf_analysis_block(loc1, [[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"],
                              rows_out=torch.zeros(3, dtype=torch.int32, device=DEV))
    L = b.L
    obs = torch.ones((n_sites, 1), dtype=torch.float64, device=DEV)
    arr = (_lib.EnkfObs * 1)(wood)
    assert L.sipnet_batch_enkf_analysis_block(b.h, None, 1, arr, 1, None, 0, 0, 0, C.c_void_p(obs.data_ptr()),
                                              C.c_void_p(obs.data_ptr()), None, None, None, b._stream()) == BAD
    assert L.sipnet_batch_enkf_analysis_block(b.h, loc1.h, 1, arr, 0, None, 0, 0, 0, C.c_void_p(obs.data_ptr()),
                                              C.c_void_p(obs.data_ptr()), None, None, None, b._stream()) == BAD   # (per-site checks)
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    b.close()
    # one row beyond the cap: one operator, site 0 listed by 128 others (refused before anything is launched: the batch is
    # not even set up)
    wide = sa.Batch(sa.flags_from(), 130, 2, sa.F64)
    ptr = np.concatenate([[0, 0], np.arange(1, 129), [128]]).astype(np.int64)
    loc = wide.enkf_localization(ptr, np.zeros(128, np.int32), np.full(128, 0.5), 1)
    assert loc.max_rows == sa.ENKF_BLOCK_MAX_ROWS + 1
    with pytest.raises(sa.SipnetError) as e:
        wide.enkf_analysis_block(loc, np.ones((130, 1)), np.ones((130, 1)), [wood], ["plantWoodC"])
    assert e.value.code == BAD and "129" in str(sa.lib().sipnet_last_error())
    wide.close()
    big = sa.Batch(sa.flags_from(), 1, 4097, sa.F64)                   # more than 4096 members per site
    loc = big.enkf_localization([0, 0], [], [], 1)
    with pytest.raises(sa.SipnetError) as e:
        big.enkf_analysis_block(loc, [[1.0]], [[1.0]], [wood], ["plantWoodC"])
    assert e.value.code == BAD and "4096" in str(sa.lib().sipnet_last_error())
    big.close()


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
            b.enkf_analysis_block(loc, obs, sd, operators(), ANALYSED, planes=planes)
            after = b.get_state()
            assert np.abs(after[:, SLOTS] - st0[:, SLOTS]).max() > 0
        else:
            b.set_state(after)
        p2, _ = b.run(96, 48)
        out.append(bits(p2.cpu().numpy()))
        b.close()
    np.testing.assert_array_equal(out[0], out[1])
