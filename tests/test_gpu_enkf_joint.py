"""The joint state-parameter ensemble Kalman filter analysis on the GPU (sipnet_batch_enkf_analysis_joint) and
sipnet_batch_get_params: every site's analysed pools and parameters against the numpy reference
(tests/enkf_joint_reference.py); without parameters the per-site analysis bit for bit; the one-workgroup-per-site kernel
against the per-chunk launches bit for bit; what must stay untouched; the bounds, the kept-whole rule and the allocation rule
with their margins; the parameter inflation; parameters behind a resampled index and a resampling afterwards; a forecast that
continues like a fresh batch given the analysed parameters; the refusals."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import enkf_joint_reference as jr
from tests import enkf_reference as er
from tests.enkf_gpu_common import (ANALYSED, BASE, DEV, OTHER, SLOTS, bits, carried_params, forecast, observe, op_tuples,
                                   operators, site_clim, sites_batch, within)

pytestmark = pytest.mark.gpu

# identity rows, rate rows (baseVegResp, leafTurnoverRate), an operator's divisor (soilWHC), a derived row's sources
# (psnTOpt, psnTMin); the bounds are the ones the synthetic ensembles are drawn within (file units)
NAMES = ["aMax", "halfSatPar", "vegRespQ10", "soilWHC", "psnTOpt", "psnTMin", "baseVegResp", "leafTurnoverRate"]
MARGIN = 1e-7          # a threshold is this far (x the comparison's scale) from every reference value: 1000 x the bound 1e-10


def wide(names=NAMES):
    return [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in names]


def tuples(params):
    return [(p.index, p.lo, p.hi) for p in params]


def rows_of(params):
    return [p.index for p in params]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def force_path(b, path):
    if path == "group":
        b.debug_set_num_cus(1)
    elif path == "split":
        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


def reference(st0, n_sites, ops, params, obs, sd, infl, pinfl, pl, prm, raw=None, slots=SLOTS):
    return jr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), slots, tuples(params), obs, sd, infl, pinfl,
                       pl, prm, raw)


@pytest.mark.parametrize("path", ["auto", "group", "split"])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_every_site_against_the_reference_and_what_must_stay_stays(base, prec, path):
    n_sites, M = 32, 256
    b, planes = forecast(base, n_sites, M, prec)
    st = b.get_state()
    st[11 * M + 1:12 * M, 29] = 3.0                     # site 11: one live member (code 0)
    st[[5, 40, 5 * M + 7, 5 * M + 8, 20 * M + 255], 29] = 3.0     # dead members among live ones
    b.set_state(st)
    force_path(b, path)
    ops, params = operators(), wide()
    rows = rows_of(params)
    st0, rings0 = b.get_state(), b.get_rings()
    pl = [p.cpu().numpy() for p in planes]
    prm0 = carried_params(b)
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(5), nan_sites=(3, 17), nan_obs=((0, 1), (5, 3), (9, 0)))
    sd[7, 2] = -1.0                                     # site 7: bad input (code -2)
    infl = 1.0 + 0.05 * (np.arange(n_sites) % 3)
    pinfl = 1.0 + 0.1 * (np.arange(n_sites) % 2)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, inflation=infl, param_inflation=pinfl, info_out=info)
    st1, rings1, prm1 = b.get_state(), b.get_rings(), b.get_params()
    if path != "auto":
        assert b.pf_info()["fused"] == (1 if path == "group" else 0)
    b.close()
    want, want_prm, want_info = reference(st0, n_sites, ops, params, obs, sd, infl, pinfl, pl, prm0)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert (want_info[:, 0] == 1).sum() == n_sites - 4
    assert (want_info[[3, 17], 0] == -1).all() and want_info[7, 0] == -2 and want_info[11, 0] == 0
    within(st1, want, st0, n_sites)
    within(prm1, want_prm, prm0, n_sites, slots=rows + [jr.PSN_TMAX])
    # untouched: the state outside the mask, the rings; the rows neither analysed nor derived from an analysed one; every
    # parameter and pool of a member that is not live or of a site whose code is not 1
    np.testing.assert_array_equal(bits(st1[:, OTHER]), bits(st0[:, OTHER]))
    np.testing.assert_array_equal(bits(rings1), bits(rings0))
    rest = [k for k in range(80) if k not in rows + [jr.PSN_TMAX]]
    np.testing.assert_array_equal(bits(prm1[:, rest]), bits(prm0[:, rest]))
    untouched = np.repeat(want_info[:, 0] != 1, M) | (st0[:, 29] != 0)
    assert untouched.sum() > 4 * M
    np.testing.assert_array_equal(bits(st1[untouched]), bits(st0[untouched]))
    np.testing.assert_array_equal(bits(prm1[untouched]), bits(prm0[untouched]))
    assert np.abs(st1[:, SLOTS] - st0[:, SLOTS]).max() > 0
    moved = prm1[:, rows] != prm0[:, rows]
    assert moved.any(0).all()                           # every analysed parameter moved somewhere
    live_moved = ~untouched
    np.testing.assert_array_equal(bits(prm1[live_moved][:, jr.PSN_TMAX]),
                                  bits(prm1[live_moved][:, jr.PSN_TOPT] + (prm1[live_moved][:, jr.PSN_TOPT] - prm1[live_moved][:, jr.PSN_TMIN])))


@pytest.mark.parametrize("path", ["group", "split"])
@pytest.mark.parametrize("M", [256, 1000])
def test_without_parameters_it_is_the_per_site_analysis_bit_for_bit(base, M, path):
    n_sites = 8
    results = []
    for joint in (False, True):
        b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=3)
        force_path(b, path)
        st0 = b.get_state()
        pl = [p.cpu().numpy() for p in planes]
        prm0 = carried_params(b)
        ops = operators()
        obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(1), nan_sites=(6,), nan_obs=((2, 0),))
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        infl = np.full(n_sites, 1.1)
        if joint:
            b.enkf_analysis_joint(obs, sd, ops, ANALYSED, [], planes=planes, inflation=infl, info_out=info)
        else:
            b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=infl, info_out=info)
        assert b.pf_info()["fused"] == (1 if path == "group" else 0)
        results.append((bits(b.get_state()), info.cpu().numpy(), bits(b.get_params()), bits(prm0)))
        b.close()
    for k in range(3):
        np.testing.assert_array_equal(results[1][k], results[0][k])
    np.testing.assert_array_equal(results[1][2], results[1][3])           # all 80 rows as they were


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
        b.enkf_analysis_joint(obs, sd, ops, ANALYSED, wide(), planes=planes, inflation=np.full(n_sites, 1.1),
                              param_inflation=np.full(n_sites, 1.05), info_out=info)
        results.append((bits(b.get_state()), info.cpu().numpy(), bits(b.get_params())))
        b.close()
    for r in results[1:]:
        for k in range(3):
            np.testing.assert_array_equal(r[k], results[0][k])


def test_big_sites_split_path_against_the_reference(base):
    n_sites, M = 2, 5000                # beyond one workgroup's 4096: the per-chunk launches whatever the device
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=4)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm0 = carried_params(b)
    ops, params = operators(), wide()
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(2))
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes)          # the synchronous form
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    want, want_prm, _ = reference(st0, n_sites, ops, params, obs, sd, None, None, pl, prm0)
    within(st1, want, st0, n_sites)
    within(prm1, want_prm, prm0, n_sites, slots=rows_of(params) + [jr.PSN_TMAX])


def test_tight_bounds_clip_to_the_bound_exactly(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=8)
    st0 = b.get_state()
    pl = [p.cpu().numpy() for p in planes]
    prm0 = carried_params(b)
    ops = operators()
    names = ["aMax", "baseVegResp", "vegRespQ10"]
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(3))
    # the unclipped analysis first: the bounds are its quartiles (file units), so both ends clip
    raw = {}
    reference(st0, n_sites, ops, wide(names), obs, sd, None, None, pl, prm0, raw)
    free = np.concatenate([raw[s][2] for s in range(n_sites)])
    live = np.concatenate([raw[s][0] for s in range(n_sites)])
    params = []
    for k, name in enumerate(names):
        q = np.quantile(free[:, k], [0.25, 0.75]) * (365.0 if pi(name) in jr.RATE_ROWS else 1.0)
        params.append(sa.enkf_param(name, float(q[0]), float(q[1])))
    rows, lo, hi = jr.converted_bounds(tuples(params))
    raw = {}
    want, want_prm, want_info = reference(st0, n_sites, ops, params, obs, sd, None, None, pl, prm0, raw)
    kept = np.concatenate([raw[s][3] for s in range(n_sites)])
    assert not kept.all()
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, info_out=info)
    prm1 = b.get_params()
    b.close()
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    for k, row in enumerate(rows):
        below, above = (free[:, k] < lo[k]) & ~kept, (free[:, k] > hi[k]) & ~kept
        assert below.sum() > 0 and above.sum() > 0, names[k]
        # the margin: no reference value within MARGIN x scale of a bound, so a flip cannot hide as a tolerance
        scale = max(abs(lo[k]), abs(hi[k]), free[:, k].std())
        gap = min(np.abs(free[:, k] - lo[k]).min(), np.abs(free[:, k] - hi[k]).min())
        print(f"{names[k]}: clipped below {below.sum()}, above {above.sum()}; nearest reference value to a bound {gap / scale:.3e} x scale")
        assert gap > MARGIN * scale, names[k]
        assert (bits(prm1[live[below], row]) == bits(np.float64(lo[k]))).all(), names[k]
        assert (bits(prm1[live[above], row]) == bits(np.float64(hi[k]))).all(), names[k]
        assert ((prm1[live[~kept], row] >= lo[k]) & (prm1[live[~kept], row] <= hi[k])).all()
    within(prm1, want_prm, prm0, n_sites, slots=rows)


def biomass_margin(st0, raw, n_sites, slots=SLOTS):
    """the largest m of 1e-3, 1e-4, .. such that no live member's outcome of the pools' limits changes when every analysed pool
    of the reference moves by m x the comparison's scale, up or down (hasSufficientBiomass is monotone in every pool, so the
    two corners decide); 0.0 if there is none above 1e-12"""
    for m in 10.0 ** -np.arange(3, 13):
        decided = True
        for s in range(n_sites):
            live, X = raw[s][0], raw[s][1]
            fc = st0[live, :13]
            d = m * np.maximum(np.abs(X), fc[:, slots].std(0))
            decided = decided and bool((er.limits(fc, X + d, slots)[1] == er.limits(fc, X - d, slots)[1]).all())
        if decided:
            return m
    return 0.0


def test_members_kept_on_their_forecast_keep_their_forecast_parameters_too(base):
    """above-ground wood observed far below the ensemble.  plantCAccountingDelta is left out of the analysed pools here: with
    it, the update splits the move between plantWoodC and the delta, the rule's wood + delta is the small difference of two
    values of some 500 g, and 512 members 1e-4 g apart cannot all stay 1000 bounds (1e-7 x 500 g) away from the threshold.
    Without it the delta keeps its forecast (some 0.01 g), plantWoodC itself ends near the threshold, and the comparison's
    scale there is the ensemble sd (some 0.03 g)."""
    n_sites, M = 2, 256
    analysed = [p for p in ANALYSED if p != "plantCAccountingDelta"]
    slots = [sa.POOLS.index(p) for p in analysed]
    b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=6)
    st0, prm0 = b.get_state(), carried_params(b)
    wood = st0[:, 0] + st0[:, 12]
    ops = [sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"])]
    params = wide(["aMax", "baseVegResp", "psnTOpt"])
    rows = rows_of(params)
    w = wood.reshape(n_sites, M)
    sd = w.std(1, keepdims=True)
    obs = np.zeros((n_sites, 1))
    for s in range(n_sites):       # far enough below that the reference keeps some of the site's members on their forecast
        lo, hi = 0.0, 4.0
        for _ in range(80):
            f = 0.5 * (lo + hi)
            obs[s] = w[s].mean() * (1.0 - f)
            kept = reference(st0, n_sites, ops, params, obs, sd, None, None, None, prm0, slots=slots)[2][s, 3]
            if 0.25 * M < kept < 0.75 * M:
                break
            lo, hi = (f, hi) if kept <= 0.25 * M else (lo, f)
    raw = {}
    want, want_prm, want_info = reference(st0, n_sites, ops, params, obs, sd, None, None, None, prm0, raw, slots=slots)
    margin = biomass_margin(st0, raw, n_sites, slots)
    print(f"kept {want_info[:, 3]} of {M}; the biomass rule's outcome holds for every member under moves of {margin:.0e} x scale")
    assert margin >= MARGIN                                # a flip cannot hide as a tolerance
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_joint(obs, sd, ops, analysed, params, info_out=info)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert (want_info[:, 3] > 0).all() and (want_info[:, 3] < M).all()
    kept = np.zeros(n_sites * M, dtype=bool)
    for s in range(n_sites):
        kept[raw[s][0][raw[s][3]]] = True
    np.testing.assert_array_equal(bits(prm1[kept]), bits(prm0[kept]))
    np.testing.assert_array_equal(bits(st1[kept]), bits(st0[kept]))
    assert (prm1[~kept][:, rows] != prm0[~kept][:, rows]).all(1).any()
    within(st1, want, st0, n_sites, slots=slots)
    within(prm1, want_prm, prm0, n_sites, slots=rows + [jr.PSN_TMAX])
    np.testing.assert_array_equal(bits(st1[:, 12]), bits(st0[:, 12]))


def test_the_allocation_rule_decides(base):
    """allocations that sum close to 1, spread by the parameter inflation: some members' analysed allocations leave no room
    for the coarse roots and keep their forecast; the rest get the fourth allocation rewritten"""
    n_sites, M = 2, 256
    rng = np.random.default_rng(21)
    members = synth.perturbed_params(base, n_sites * M, seed=13)
    leaf = 0.30 + 0.01 * rng.standard_normal(n_sites * M)
    wood = 0.30 + 0.01 * rng.standard_normal(n_sites * M)
    fine = np.minimum(0.37 + 0.01 * rng.standard_normal(n_sites * M), 0.995 - leaf - wood)   # (every forecast member valid)
    members[:, jr.LEAF_ALLOC], members[:, jr.WOOD_ALLOC], members[:, jr.FINE_ALLOC] = leaf, wood, fine
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 96)
    st0, prm0 = b.get_state(), carried_params(b)
    assert (st0[:, 29] == 0).all()
    pl = [p.cpu().numpy() for p in planes]
    ops = operators()
    params = [sa.enkf_param("leafAllocation", 0.0, 1.5), sa.enkf_param("fineRootAllocation", 0.0, 1.5),
              sa.enkf_param("aMax", *synth.PERTURB["aMax"][:2])]
    rows = rows_of(params)
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(4))
    pinfl = np.full(n_sites, 3.0)
    raw = {}
    want, want_prm, want_info = reference(st0, n_sites, ops, params, obs, sd, None, pinfl, pl, prm0, raw)
    by_rule = moved = 0
    margin = np.inf
    assert biomass_margin(st0, raw, n_sites) >= MARGIN
    for s in range(n_sites):
        live, X, P, kept = raw[s]
        lf, fr, wd = P[:, 0], P[:, 1], prm0[live, jr.WOOD_ALLOC]
        fails = (lf >= 1.0) | (wd >= 1.0) | (fr >= 1.0) | (1 - lf - wd - fr < 0)
        biomass_ok = er.limits(st0[live, :13], X, SLOTS)[1] == False      # noqa: E712
        by_rule += int((fails & biomass_ok).sum())
        moved += int((~kept).sum())
        assert (kept == (fails | ~biomass_ok)).all()
        # the margins (the allocations are O(1), the comparison's scale at least their ensemble sd ~ 0.03)
        margin = min(margin, np.abs(1 - lf - wd - fr).min(), np.abs(lf - 1.0).min(), np.abs(fr - 1.0).min(), np.abs(lf).min(),
                     np.abs(fr).min())
    print(f"kept by the allocation rule {by_rule}, moved {moved}; nearest reference value to a threshold {margin:.3e}")
    assert by_rule >= 1 and moved >= 1
    assert margin > MARGIN
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, param_inflation=pinfl, info_out=info)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    within(st1, want, st0, n_sites)
    within(prm1, want_prm, prm0, n_sites, slots=rows + [jr.COARSE_ALLOC])
    for s in range(n_sites):
        live, _, _, kept = raw[s]
        np.testing.assert_array_equal(bits(prm1[live[kept]]), bits(prm0[live[kept]]))
        np.testing.assert_array_equal(bits(st1[live[kept]]), bits(st0[live[kept]]))
        m = live[~kept]
        np.testing.assert_array_equal(bits(prm1[m, jr.COARSE_ALLOC]),
                                      bits(1 - prm1[m, jr.LEAF_ALLOC] - prm1[m, jr.WOOD_ALLOC] - prm1[m, jr.FINE_ALLOC]))
        assert (prm1[m, jr.COARSE_ALLOC] >= 0).all()
    rest = [k for k in range(80) if k not in rows + [jr.COARSE_ALLOC]]
    np.testing.assert_array_equal(bits(prm1[:, rest]), bits(prm0[:, rest]))


def test_parameter_inflation_against_the_reference_and_a_bad_value(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=5)
    st0, prm0 = b.get_state(), carried_params(b)
    pl = [p.cpu().numpy() for p in planes]
    ops, params = operators(), wide()
    rows = rows_of(params)
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(6))
    # the synchronous form refuses a bad value before anything is written
    for bad in (0.5, np.nan, np.inf):
        with pytest.raises(sa.SipnetError) as e:
            b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, param_inflation=[1.0, 1.0, bad, 1.0])
        assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 2" in str(e.value)
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    # the asynchronous form: code -2, the site untouched; pools not inflated (lambda NULL), parameters by 1, 1.3, -, 2
    pinfl = np.array([1.0, 1.3, 0.5, 2.0])
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes, param_inflation=pinfl, info_out=info)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    want, want_prm, want_info = reference(st0, n_sites, ops, params, obs, sd, None, pinfl, pl, prm0)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    assert list(want_info[:, 0]) == [1, 1, -2, 1]
    np.testing.assert_array_equal(bits(st1[2 * M:3 * M]), bits(st0[2 * M:3 * M]))
    np.testing.assert_array_equal(bits(prm1[2 * M:3 * M]), bits(prm0[2 * M:3 * M]))
    within(st1, want, st0, n_sites)
    within(prm1, want_prm, prm0, n_sites, slots=rows + [jr.PSN_TMAX])
    no_infl = reference(st0, n_sites, ops, params, obs, sd, None, None, pl, prm0)[1]
    assert np.abs(no_infl[3 * M:, rows] - want_prm[3 * M:, rows]).max() > 1e-6      # (the inflation is not a no-op here)


def resampled(base, n_sites=4, M=256, seed=12):
    """a batch after a forecast and a particle-filter resampling that carries the parameters: they are behind an index"""
    members = synth.perturbed_params(base, n_sites * M, seed=seed)
    b = sites_batch(members, n_sites, sa.F64)
    planes, _ = b.run(0, 48)
    tot = planes[0].double().sum(0).cpu().numpy().reshape(n_sites, M)
    b.pf_analysis_sites(planes[0], np.median(tot, 1), tot.std(1) * 0.3, [0.1, 0.3, 0.5, 0.7], with_params=True)
    return b, planes, members


def test_after_a_resampling_with_params_it_analyses_the_carried_parameters(base):
    n_sites, M = 4, 256
    b, planes, members = resampled(base)
    st0, prm0 = b.get_state(), carried_params(b)
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))       # get_params reads through the index
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm0))    # ... and leaves it as it is
    assert not np.allclose(prm0[:, pi("aMax")], members[:, pi("aMax")])   # resampled: not the column's own row
    pl = [p.cpu().numpy() for p in planes]
    ops, params = operators(), wide()
    rows = rows_of(params)
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(9))
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes)
    st1, prm1 = b.get_state(), b.get_params()
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm1))
    b.close()
    want, want_prm, _ = reference(st0, n_sites, ops, params, obs, sd, None, None, pl, prm0)
    within(st1, want, st0, n_sites)
    within(prm1, want_prm, prm0, n_sites, slots=rows + [jr.PSN_TMAX])
    rest = [k for k in range(80) if k not in rows + [jr.PSN_TMAX]]
    np.testing.assert_array_equal(bits(prm1[:, rest]), bits(prm0[:, rest]))


def test_a_resampling_afterwards_carries_the_analysed_rows(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=14)
    st0, prm0 = b.get_state(), carried_params(b)
    pl = [p.cpu().numpy() for p in planes]
    ops, params = operators(), wide()
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(10))
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes)
    st1, prm1 = b.get_state(), b.get_params()
    assert (prm1[:, rows_of(params)] != prm0[:, rows_of(params)]).any()
    tot = planes[0].double().sum(0).cpu().numpy().reshape(n_sites, M)
    anc, _ = b.pf_analysis_sites(planes[0], np.median(tot, 1), tot.std(1) * 0.3, [0.1, 0.3, 0.5, 0.7], with_params=True)
    anc = anc.cpu().numpy()
    assert (anc != np.arange(n_sites * M)).any()
    prm2, st2 = b.get_params(), b.get_state()
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm2))
    b.close()
    np.testing.assert_array_equal(bits(prm2), bits(prm1[anc]))
    np.testing.assert_array_equal(bits(st2[:, :13]), bits(st1[anc][:, :13]))


def test_a_forecast_after_the_analysis_equals_a_fresh_batch_given_its_parameters(base):
    """nothing else caches a parameter: a fresh batch given get_params(file_units=True), the state and the rings continues
    bit for bit in every plane"""
    n_sites, M = 4, 256
    names = ["aMax", "halfSatPar", "vegRespQ10", "soilWHC", "psnTOpt", "psnTMin"]      # identity conversion
    b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=9)
    st0, prm0 = b.get_state(), carried_params(b)
    pl = [p.cpu().numpy() for p in planes]
    ops, params = operators(), wide(names)
    obs, sd = observe(st0, pl, prm0, n_sites, ops, np.random.default_rng(4))
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=planes)
    st1, rings1, prm1, raw1 = b.get_state(), b.get_rings(), b.get_params(), b.get_params(file_units=True)
    assert (prm1[:, rows_of(params)] != prm0[:, rows_of(params)]).any() and (prm1[:, jr.PSN_TMAX] != prm0[:, jr.PSN_TMAX]).any()
    p2, _ = b.run(96, 48)
    out = bits(p2.cpu().numpy())
    b.close()
    twin = sa.Batch(sa.flags_from(), n_sites, M, sa.F64, fast_math=True)
    for s in range(n_sites):
        twin.set_climate(s, site_clim(s))
        twin.set_params(s, raw1[s * M:(s + 1) * M])
    twin.setup()
    np.testing.assert_array_equal(bits(twin.get_params()), bits(prm1))     # the derived row among them
    twin.set_state(st1)
    twin.set_rings(rings1)
    p3, _ = twin.run(96, 48)
    out_twin = bits(p3.cpu().numpy())
    twin.close()
    np.testing.assert_array_equal(out_twin, out)


def test_get_params_is_what_the_columns_carry_in_both_units(base):
    n_sites, M = 3, 64
    members = synth.perturbed_params(base, n_sites * M, seed=2)
    b = sites_batch(members, n_sites, sa.F64)
    conv, file_units = b.get_params(), b.get_params(file_units=True)
    np.testing.assert_array_equal(bits(conv), bits(carried_params(b)))
    rates = list(jr.RATE_ROWS)
    rest = [k for k in range(80) if k not in rates]
    np.testing.assert_array_equal(bits(file_units[:, rates]), bits(conv[:, rates] * 365.0))
    np.testing.assert_array_equal(bits(file_units[:, rest]), bits(conv[:, rest]))
    np.testing.assert_array_equal(bits(conv[:, rates]), bits(members[:, rates] / 365.0))
    same = [k for k in rest if k not in jr.DERIVED_ROWS + jr.PHENOLOGY_ROWS + jr.CLAMPED_ROWS]
    np.testing.assert_array_equal(bits(conv[:, same]), bits(members[:, same]))
    # rows set since the last launch are flushed first
    members2 = members.copy()
    members2[:M, pi("aMax")] += 1.0
    b.set_params(0, members2[:M])
    np.testing.assert_array_equal(bits(b.get_params()[:, pi("aMax")]), bits(members2[:, pi("aMax")]))
    b.close()


def test_refusals(base):
    n_sites, M = 2, 64
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48)
    st0, prm0 = b.get_state(), b.get_params()
    L, h = b.L, b.h
    obs = torch.tensor(st0[:, 0].reshape(n_sites, M).mean(1, keepdims=True) * 1.01, dtype=torch.float64, device=DEV)
    sd = torch.tensor(st0[:, 0].reshape(n_sites, M).std(1, keepdims=True), dtype=torch.float64, device=DEV)
    wood = sa.enkf_pools(["plantWoodC"])
    a, q = pi("aMax"), pi("vegRespQ10")
    BAD = _lib.ERR_BAD_ARGUMENT

    def call(params, ops=(wood,), mask=1, n_params=None, pinfl=None):
        arr = (_lib.EnkfObs * max(len(ops), 1))(*ops)
        prm = (_lib.EnkfParam * max(len(params), 1))(*[_lib.EnkfParam(int(i), 0, float(lo), float(hi)) for i, lo, hi in params])
        return L.sipnet_batch_enkf_analysis_joint(h, len(ops), arr, mask, len(params) if n_params is None else n_params,
                                                  prm if params else None, None, 0, 0, 0, obs.data_ptr(), sd.data_ptr(), None,
                                                  pinfl.data_ptr() if pinfl is not None else None, None, b._stream())

    for rows, word in [(jr.DERIVED_ROWS, b"derived"), (jr.INIT_ROWS, b"initial condition"), (jr.PHENOLOGY_ROWS, b"phenology"),
                       (jr.CLAMPED_ROWS, b"clamps")]:
        for i in rows:
            assert call([(a, 1.0, 20.0), (i, 0.0, 1.0)]) == BAD
            msg = L.sipnet_last_error()
            assert b"sipnet_batch_enkf_analysis_joint" in msg and word in msg, msg
    assert call([(a, 1.0, 20.0), (q, 1.0, 3.0), (a, 1.0, 20.0)]) == BAD and b"twice" in L.sipnet_last_error()
    assert call([(80, 0.0, 1.0)]) == BAD
    assert call([(-1, 0.0, 1.0)]) == BAD
    assert call([(a, 1.0, 20.0)], n_params=17) == BAD
    assert call([(a, 1.0, 20.0)], n_params=-1) == BAD
    assert call([], n_params=1) == BAD
    assert call([(a, np.nan, 20.0)]) == BAD
    assert call([(a, 1.0, np.inf)]) == BAD
    assert call([(a, 20.0, 20.0)]) == BAD
    assert call([(a, 21.0, 20.0)]) == BAD
    # the per-site call's refusals hold
    assert call([(a, 1.0, 20.0)], mask=0) == BAD
    assert call([(a, 1.0, 20.0)], mask=1 << 13) == BAD
    assert call([(a, 1.0, 20.0)], ops=[wood] * 17) == BAD
    assert call([(a, 1.0, 20.0)], ops=[_lib.EnkfObs(0, 1, 0, _lib.NPARAMS, 1.0)]) == BAD
    assert call([(a, 1.0, 20.0)], ops=[sa.enkf_plane("nee")]) == BAD
    bad = torch.tensor([1.0, 0.9], dtype=torch.float64, device=DEV)
    assert call([(a, 1.0, 20.0)], pinfl=bad) == BAD and b"site 1" in L.sipnet_last_error()
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))         # nothing was written by any of them
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    assert call([(a, 1.0, 20.0)]) == _lib.OK
    assert (b.get_params()[:, a] != prm0[:, a]).any()
    with pytest.raises(ValueError):
        b.enkf_analysis_joint([[1.0], [1.0]], [[1.0], [1.0]], [wood], ["plantWoodC"], [], param_inflation=[1.0])
    b.close()
    # a batch connected across ranks is refused
    c, pc = forecast(base, 1, 64, sa.F64, steps=48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.enkf_analysis_joint([[1.0]], [[1.0]], [wood], ["plantWoodC"], [sa.enkf_param("aMax", 1.0, 20.0)])
    assert e.value.code == BAD and "connected" in str(e.value)
    c.close()
