"""Particle rejuvenation on the GPU (sipnet_batch_pf_rejuvenate): every value against the longdouble reference
(tests/pf_rejuvenate_reference.py) over the member counts, parameter counts and paths at which the code changes course; the
device's normals on their own; the group path against the split path, a site alone against the same site inside a batch; site
selection by a real resampling's totals and the codes; the limits at hand-set exact values; rejuvenation after a resampling
that carries the parameters; a forecast afterwards against a fresh batch; the refusals."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import pf_rejuvenate_reference as rr
from tests.enkf_gpu_common import BASE, DEV, bits, carried_params, forecast, site_clim, sites_batch

pytestmark = pytest.mark.gpu

# sixteen rows the joint analysis accepts, bounds the synthetic ensembles are drawn within (file units); rate rows among them
NAMES = ["aMax", "psnTMin", "psnTOpt", "dVpdSlope", "halfSatPar", "baseVegResp", "baseFolRespFrac", "baseFineRootResp",
         "baseCoarseRootResp", "vegRespQ10", "fineRootQ10", "coarseRootQ10", "frozenSoilThreshold", "woodTurnoverRate",
         "leafTurnoverRate", "wueConst"]
IDENTITY = ["aMax", "halfSatPar", "vegRespQ10", "soilWHC", "psnTOpt", "psnTMin"]      # converted value = file value
POOLS8 = 0x10FF                                      # the eight carbon and water pools and plantCAccountingDelta


def listed(names):
    return [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in names]


def tuples(params):
    return [(p.index, p.lo, p.hi) for p in params]


def pool_names(mask):
    return [sa.POOLS[p] for p in range(13) if mask >> p & 1]


def pool_sds(st, n_sites, rel=0.02):
    """per site and slot: rel x the site's mean |pool|, 0.01 where the pool is empty"""
    M = st.shape[0] // n_sites
    sd = np.abs(st[:, :13]).reshape(n_sites, M, 13).mean(1) * rel
    return np.where(sd > 0, sd, 0.01)


def shrinks(n_sites):
    return np.array([0.9, 0.98, 0.5])[np.arange(n_sites) % 3]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def set_path(b, path):
    """auto: the library's choice -- one workgroup per site (group) for sites of one chunk, at most 256 members, else the
    per-chunk launches; split: those launches forced"""
    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH if path == "split" else 0)


def want_fused(path, M):
    return 1 if path == "auto" and M <= 256 else 0


def fused(b):
    return b.pf_info()["fused"]


def call_and_compare(b, n_sites, params, shrink, mask, sd, seed, draw, streams=None, total=None, site_total=None):
    """one call against the reference from the state the batch holds -> (worst parameter ratio, worst pool ratio, info)"""
    st0, prm0, rings0 = b.get_state(), b.get_params(), b.get_rings()
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.pf_rejuvenate(params, shrink if params else None, pool_names(mask), sd if mask else None, seed=seed, draw=draw,
                    streams=streams, site_total=site_total, info_out=info)
    st1, prm1, rings1 = b.get_state(), b.get_params(), b.get_rings()
    want_st, want_prm, want_info, tol_st, tol_prm, margin = rr.rejuvenate(
        st0, prm0, np.zeros(n_sites), n_sites, tuples(params), shrink, mask, sd, seed, draw, streams, total)
    assert margin.min() > 1.0, margin.min()          # no decision within the bound of its threshold: no member is excused
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    err_prm, err_st = np.abs(prm1 - want_prm), np.abs(st1[:, :13] - want_st[:, :13])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst_prm = float(np.where(tol_prm > 0, err_prm / tol_prm, 0.0).max())
        worst_st = float(np.where(tol_st > 0, err_st / tol_st, 0.0).max())
    assert (err_prm <= tol_prm).all(), worst_prm
    assert (err_st <= tol_st).all(), worst_st
    # what must stay: the rings, status and trackers; every row and slot not listed; every column that is not live; every
    # site whose code is not 1
    np.testing.assert_array_equal(bits(rings1), bits(rings0))
    np.testing.assert_array_equal(bits(st1[:, 13:]), bits(st0[:, 13:]))
    rows = [p.index for p in params]
    derived = ([rr.PSN_TMAX] if rr.PSN_TOPT in rows or rr.PSN_TMIN in rows else []) + (
        [rr.COARSE_ALLOC] if {rr.LEAF_ALLOC, rr.WOOD_ALLOC, rr.FINE_ALLOC} & set(rows) else [])
    rest = [k for k in range(80) if k not in rows + derived]
    np.testing.assert_array_equal(bits(prm1[:, rest]), bits(prm0[:, rest]))
    slots = [p for p in range(13) if not mask >> p & 1]
    np.testing.assert_array_equal(bits(st1[:, slots]), bits(st0[:, slots]))
    M = st0.shape[0] // n_sites
    untouched = np.repeat(want_info[:, 0] != 1, M) | (st0[:, 29] != 0)
    np.testing.assert_array_equal(bits(st1[untouched]), bits(st0[untouched]))
    np.testing.assert_array_equal(bits(prm1[untouched]), bits(prm0[untouched]))
    return worst_prm, worst_st, want_info


# (n_params, pool mask, path): the Philox block edges 1, 4, 5, 16; pools alone, parameters alone, both; masks that use one
# block, all four, or skip some
CONFIGS = [(1, 0, "auto"), (4, POOLS8, "split"), (5, 0x1FFF, "auto"), (16, 0, "split"), (0, POOLS8, "auto"), (0, 0x0105, "split"),
           (16, POOLS8, "auto"), (1, 0x1000, "split"), (4, 0, "auto"), (5, 0x0005, "auto"), (16, 0x1FFF, "split"), (0, 0x1FFF, "auto")]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("n_sites", [1, 3])
@pytest.mark.parametrize("M", [2, 63, 64, 65, 256, 257, 1000])
def test_against_the_reference_and_what_must_stay_stays(base, M, n_sites, prec):
    b, _ = forecast(base, n_sites, M, prec, steps=48, seed=M)
    if M >= 63:                                         # dead members at the wave edges of the last site
        st = b.get_state()
        st[[(n_sites - 1) * M + j for j in (0, 62, M - 1)], 29] = 3.0
        b.set_state(st)
    worst = [0.0, 0.0]
    for draw, (n_params, mask, path) in enumerate(CONFIGS):
        set_path(b, path)
        sd = pool_sds(b.get_state(), n_sites)
        w = call_and_compare(b, n_sites, listed(NAMES[:n_params]), shrinks(n_sites), mask, sd, seed=2026 + M, draw=draw)
        assert fused(b) == want_fused(path, M)
        assert (w[2][:, 0] == 1).all() and (w[2][:, 1] == n_params + bin(mask).count("1")).all()
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    b.close()
    print(f"M = {M}, {n_sites} sites: worst |got - want| / bound: parameters {worst[0]:.3f}, pools {worst[1]:.3f}")


def test_where_the_path_changes(base):
    """one workgroup per site takes sites of one chunk, at most 256 members"""
    for M, path, want in ((256, "auto", 1), (256, "split", 0), (257, "auto", 0), (4097, "auto", 0)):
        b, _ = forecast(base, 1, M, sa.F64, steps=48, seed=3)
        set_path(b, path)
        sd = pool_sds(b.get_state(), 1)
        w = call_and_compare(b, 1, listed(NAMES[:5]), [0.95], POOLS8, sd, seed=5, draw=1)
        assert fused(b) == want, (M, path)
        b.close()
        print(f"M = {M} ({path}): worst |got - want| / bound: parameters {w[0]:.3f}, pools {w[1]:.3f}")


@pytest.mark.parametrize("M, path", [(256, "auto"), (256, "split"), (257, "auto")])
def test_the_normals_of_the_device_in_isolation(base, M, path):
    """plantCAccountingDelta = 0 and q = 1: x' = 0 + 1 z = z exactly"""
    n_sites = 2
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48, seed=8)
    set_path(b, path)
    st = b.get_state()
    st[:, rr.DELTA] = 0.0
    b.set_state(st)
    sd = np.zeros((n_sites, 13))
    sd[:, rr.DELTA] = 1.0
    streams = [0, 2 ** 32 - 1]
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.pf_rejuvenate((), None, ["plantCAccountingDelta"], sd, seed=(7 << 32) + 9, draw=2 ** 32 - 1, streams=streams, info_out=info)
    got = b.get_state()[:, rr.DELTA].reshape(n_sites, M)
    b.close()
    np.testing.assert_array_equal(info.cpu().numpy(), [[1, 1, M, 0]] * n_sites)
    worst = 0.0
    for s in range(n_sites):
        z, r = rr.pool_normal((7 << 32) + 9, 2 ** 32 - 1, streams[s], np.arange(M), rr.DELTA)
        ratio = np.abs(got[s].astype(np.longdouble) - z) / (2.0 ** -53 * r)
        for j in (0, 63, 64, M - 1):
            assert ratio[j] <= 8.0, (s, j, ratio[j])
        assert (ratio <= 8.0).all()
        assert (np.abs(got[s]) <= rr.Z_MAX).all()
        worst = max(worst, float(ratio.max()))
    print(f"device normals (M = {M}, {path}): worst |z - z_longdouble| / (2^-53 r) = {worst:.3f} (bound 8)")


def rejuvenated(base, path, M, prec, seed=11, draw=3, n_sites=3, streams=None):
    b, _ = forecast(base, n_sites, M, prec, steps=48, seed=4)
    set_path(b, path)
    st = b.get_state()
    st[[1, M + 63 if M > 63 else M + 1], 29] = 3.0
    b.set_state(st)
    st0 = b.get_state()
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.pf_rejuvenate(listed(NAMES), shrinks(n_sites), pool_names(POOLS8), pool_sds(st0, n_sites), seed=seed, draw=draw,
                    streams=streams, info_out=info)
    out = (b.get_state(), b.get_params(), info.cpu().numpy(), fused(b))
    return b, st0, out


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [65, 256, 1000])
def test_group_and_split_paths_are_bit_identical(base, M, prec):
    results = []
    for path in ("auto", "split", "auto"):
        b, _, out = rejuvenated(base, path, M, prec)
        b.close()
        assert out[3] == want_fused(path, M)
        results.append(out)
    for r in results[1:]:
        np.testing.assert_array_equal(bits(r[0]), bits(results[0][0]))
        np.testing.assert_array_equal(bits(r[1]), bits(results[0][1]))
        np.testing.assert_array_equal(r[2], results[0][2])


def test_a_repeated_call_on_a_restored_checkpoint_gives_the_same_bits(base):
    n_sites, M = 3, 256
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48, seed=4)
    st0, rings0 = b.get_state(), b.get_rings()
    sd = pool_sds(st0, n_sites)
    runs = []
    for path in ("auto", "split", "auto"):
        set_path(b, path)
        b.set_state(st0)
        b.set_rings(rings0)
        b.pf_rejuvenate((), None, pool_names(0x1FFF), sd, seed=1, draw=2)
        runs.append(bits(b.get_state()))
    b.close()
    assert (runs[0] != bits(st0)).any()
    np.testing.assert_array_equal(runs[1], runs[0])
    np.testing.assert_array_equal(runs[2], runs[0])


@pytest.mark.parametrize("M", [200, 257])           # (one workgroup per site; the per-chunk launches)
def test_a_site_does_not_depend_on_the_batch_around_it(base, M):
    """site 1 of three, with streams given, against the same columns alone in a batch of one site"""
    members = synth.perturbed_params(base, 3 * M, seed=6)
    three = sites_batch(members, 3, sa.F64)
    three.run(0, 48)
    alone = sites_batch(members[M:2 * M], 1, sa.F64, clim=lambda s: site_clim(1))
    alone.run(0, 48)
    st3 = three.get_state()
    st3[M + 64, 29] = 3.0
    three.set_state(st3)
    st3 = three.get_state()
    alone.set_state(st3[M:2 * M])
    alone.set_rings(three.get_rings()[M:2 * M])
    np.testing.assert_array_equal(bits(alone.get_params()), bits(three.get_params()[M:2 * M]))
    sd = pool_sds(st3, 3)
    a = shrinks(3)
    three.pf_rejuvenate(listed(NAMES[:7]), a, pool_names(POOLS8), sd, seed=21, draw=5, streams=[5, 77, 9])
    alone.pf_rejuvenate(listed(NAMES[:7]), a[1:2], pool_names(POOLS8), sd[1:2], seed=21, draw=5, streams=[77])
    got3, prm3, got1, prm1 = three.get_state(), three.get_params(), alone.get_state(), alone.get_params()
    three.close()
    alone.close()
    assert (got3[M:2 * M, :13] != st3[M:2 * M, :13]).any()
    np.testing.assert_array_equal(bits(got1), bits(got3[M:2 * M]))
    np.testing.assert_array_equal(bits(prm1), bits(prm3[M:2 * M]))


def test_another_draw_or_seed_changes_every_perturbed_value(base):
    M = 257
    outs = []
    for seed, draw in ((11, 3), (11, 4), (12, 3)):
        b, st0, out = rejuvenated(base, "auto", M, sa.F64, seed=seed, draw=draw)
        b.close()
        outs.append(out)
    live = st0[:, 29] == 0
    rows = [p.index for p in listed(NAMES)]
    slots = [p for p in range(13) if POOLS8 >> p & 1]
    for other in outs[1:]:
        assert (other[1][live][:, rows] != outs[0][1][live][:, rows]).all()
        moved = (outs[0][0][live][:, slots] > 0) | (other[0][live][:, slots] > 0)       # (both clipped at 0: equal)
        assert (other[0][live][:, slots] != outs[0][0][live][:, slots])[moved].all()


def test_site_selection_by_a_resampling_and_the_codes(base):
    n_sites, M = 8, 256
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48, seed=2)
    rng = np.random.default_rng(4)
    logw = torch.tensor(rng.normal(size=n_sites * M), dtype=torch.float64, device=DEV)
    ess_min = np.full(n_sites, 1e9)                     # resample ...
    ess_min[[1, 4]] = 0.0                               # ... but sites 1 and 4 keep their particles
    total = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
    b.pf_resample_sites(logw, rng.random(n_sites), ess_min=ess_min, with_params=True, total_out=total)
    tot = total.cpu().numpy()
    assert (tot[[1, 4]] == -3).all() and (tot[[0, 2, 3, 5, 6, 7]] > 0).all()
    st = b.get_state()
    st[6 * M + 1:7 * M, 29] = 3.0                       # site 6: one live member
    st[[7 * M + j for j in (0, 63, 64, M - 1)], 29] = 3.0  # site 7: dead members at the wave edges
    b.set_state(st)
    shrink = np.array([0.9, 0.9, np.nan, 0.0, 0.9, 1.5, 0.9, 0.9])
    sd = pool_sds(b.get_state(), n_sites)
    for path in ("auto", "split"):
        set_path(b, path)
        _, _, info = call_and_compare(b, n_sites, listed(NAMES[:5]), shrink, POOLS8, sd, seed=3, draw=0, total=tot, site_total=total)
        assert list(info[:, 0]) == [1, -3, -2, -2, -3, -2, 0, 1]
        assert info[7, 2] == M - 4 and info[6, 2] == 1
    sd[0, 2] = -1.0                                     # a negative pool sd: code -2
    sd[7, 12] = np.inf                                  # ... one that is not masked is not looked at
    _, _, info = call_and_compare(b, n_sites, listed(NAMES[:5]), shrink, 0x00FF, sd, seed=3, draw=1, total=tot, site_total=total)
    assert list(info[:, 0]) == [-2, -3, -2, -2, -3, -2, 0, 1]
    b.close()


def crafted_params(base, M, edit):
    """one site, set up and not run, whose raw parameter rows `edit` has changed before the batch was made"""
    members = synth.perturbed_params(base, M, seed=5)
    edit(members)
    return sites_batch(members, 1, sa.F64)


def test_bounds_so_tight_that_every_value_reflects_and_clips(base):
    M = 257
    b = crafted_params(base, M, lambda m: None)
    prm0 = b.get_params()
    info = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    b.pf_rejuvenate([sa.enkf_param("aMax", 1000.0, 1000.5), sa.enkf_param("halfSatPar", -1000.5, -1000.0)], [0.9], info_out=info)
    prm1 = b.get_params()
    b.close()
    assert (prm0[:, pi("aMax")] < 100).all() and (prm0[:, pi("halfSatPar")] > 0).all()
    np.testing.assert_array_equal(prm1[:, pi("aMax")], np.full(M, 1000.5))            # lo + (lo - x') > hi: clipped to hi
    np.testing.assert_array_equal(prm1[:, pi("halfSatPar")], np.full(M, -1000.5))     # hi - (x' - hi) < lo: clipped to lo
    np.testing.assert_array_equal(info.cpu().numpy(), [[1, 2, M, 0]])


def test_an_allocation_at_its_last_valid_value_keeps_the_member_on_any_upward_move(base):
    """leaf = 0.75 - wood and fineRoot = 0.25 exactly: 1 - leaf - wood' - fineRoot is 0 at wood' = wood, below 0 above it"""
    M = 256

    def edit(m):
        m[:, pi("woodAllocation")] = np.array([0.125, 0.25, 0.375])[np.arange(M) % 3]
        m[:, pi("leafAllocation")] = 0.75 - m[:, pi("woodAllocation")]
        m[:, pi("fineRootAllocation")] = 0.25

    b = crafted_params(base, M, edit)
    st0, prm0 = b.get_state(), b.get_params()
    assert (prm0[:, rr.COARSE_ALLOC] == 0).all()
    params = [sa.enkf_param("woodAllocation", 0.01, 0.9), sa.enkf_param("aMax", *synth.PERTURB["aMax"][:2])]
    sd = pool_sds(st0, 1)
    _, _, info = call_and_compare(b, 1, params, [0.9], 0x0004, sd, seed=8, draw=0)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    wood = pi("woodAllocation")
    z, _ = rr.param_normal(8, 0, 0, np.arange(M), 0)
    x = prm0[:, wood].astype(np.longdouble)
    up = np.asarray(rr.move(x, 0.9, z)[0] > x)
    assert 0 < up.sum() < M and info[0, 3] == up.sum()
    np.testing.assert_array_equal(bits(prm1[up]), bits(prm0[up]))                   # kept: parameters and pools
    np.testing.assert_array_equal(bits(st1[up]), bits(st0[up]))
    assert (prm1[~up, wood] < prm0[~up, wood]).all() and (prm1[~up, pi("aMax")] != prm0[~up, pi("aMax")]).all()
    assert (st1[~up, 2] != st0[~up, 2]).all()
    np.testing.assert_array_equal(bits(prm1[~up, rr.COARSE_ALLOC]),
                                  bits(1 - prm1[~up, rr.LEAF_ALLOC] - prm1[~up, rr.WOOD_ALLOC] - prm1[~up, rr.FINE_ALLOC]))
    assert (prm1[~up, rr.COARSE_ALLOC] > 0).all()


def test_noise_that_fails_the_biomass_rule_keeps_pools_and_parameters(base):
    M = 257
    b, _ = forecast(base, 1, M, sa.F64, steps=48, seed=7)
    st = b.get_state()
    st[::2, rr.WOOD] = 2e-6                             # just above TINY: a draw below -1e-6 clips the pool to 0
    st[::2, rr.DELTA] = 1.0
    b.set_state(st)
    st0, prm0 = b.get_state(), b.get_params()
    sd = np.zeros((1, 13))
    sd[0, rr.WOOD] = 1.0
    sd[0, 2] = 5.0
    params = listed(["psnTOpt", "aMax"])
    _, _, info = call_and_compare(b, 1, params, [0.9], 0x0005, sd, seed=13, draw=0)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    z, _ = rr.pool_normal(13, 0, 0, np.arange(M), rr.WOOD)
    fails = np.asarray(st0[:, rr.WOOD].astype(np.longdouble) + z <= rr.TINY)
    assert fails[1::2].sum() == 0 and 40 < fails.sum() < M // 2 and info[0, 3] == fails.sum()
    np.testing.assert_array_equal(bits(st1[fails]), bits(st0[fails]))
    np.testing.assert_array_equal(bits(prm1[fails]), bits(prm0[fails]))
    ok = ~fails
    assert (st1[ok, 2] != st0[ok, 2]).all() and (prm1[ok, pi("aMax")] != prm0[ok, pi("aMax")]).all()
    # psnTMax follows the rows it derives from
    np.testing.assert_array_equal(bits(prm1[ok, rr.PSN_TMAX]), bits(prm1[ok, rr.PSN_TOPT] + (prm1[ok, rr.PSN_TOPT] - prm1[ok, rr.PSN_TMIN])))
    assert (prm1[ok, rr.PSN_TMAX] != prm0[ok, rr.PSN_TMAX]).all()


@pytest.mark.parametrize("path", ["auto", "split"])
def test_a_shrink_of_exactly_one_leaves_the_rows(base, path):
    n_sites, M = 2, 65
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48, seed=9)
    set_path(b, path)
    st0, prm0 = b.get_state(), b.get_params()
    sd = pool_sds(st0, n_sites)
    _, _, info = call_and_compare(b, n_sites, listed(NAMES[:6]), [1.0, 0.9], 0x0004, sd, seed=1, draw=1)
    st1, prm1 = b.get_state(), b.get_params()
    b.close()
    np.testing.assert_array_equal(bits(prm1[:M]), bits(prm0[:M]))
    assert (st1[:M, 2] != st0[:M, 2]).all() and (prm1[M:, pi("aMax")] != prm0[M:, pi("aMax")]).all()
    assert list(info[:, 1]) == [1, 7]


def test_after_a_resampling_that_carries_the_parameters(base):
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=48, seed=12)
    rng = np.random.default_rng(2)
    logw = torch.tensor(3.0 * rng.normal(size=n_sites * M), dtype=torch.float64, device=DEV)
    total = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
    anc = b.pf_resample_sites(logw, [0.1, 0.3, 0.5, 0.7], with_params=True, total_out=total).cpu().numpy()
    twins = np.flatnonzero(anc[1:] == anc[:-1])
    assert len(twins) > n_sites * M // 4
    prm0 = carried_params(b)
    np.testing.assert_array_equal(bits(prm0[twins]), bits(prm0[twins + 1]))
    params = listed(NAMES)
    rows = [p.index for p in params]
    sd = pool_sds(b.get_state(), n_sites)
    call_and_compare(b, n_sites, params, shrinks(n_sites), POOLS8, sd, seed=31, draw=7, total=total.cpu().numpy(), site_total=total)
    prm1, st1 = b.get_params(), b.get_state()
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm1))
    assert (prm1[twins][:, rows] != prm1[twins + 1][:, rows]).all()      # duplicates: pairwise different in every listed row
    anc2 = b.pf_resample_sites(logw, [0.2, 0.4, 0.6, 0.8], with_params=True).cpu().numpy()
    assert (anc2 != np.arange(n_sites * M)).any()
    prm2, st2 = b.get_params(), b.get_state()
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm2))
    b.close()
    np.testing.assert_array_equal(bits(prm2), bits(prm1[anc2]))
    np.testing.assert_array_equal(bits(st2[:, :13]), bits(st1[anc2][:, :13]))


@pytest.mark.parametrize("kernel, family", [(sa.KERNEL_AUTO, "stepCoop"), (sa.KERNEL_ONE_WAVE, "stepFast")], ids=["coop", "one_wave"])
def test_a_forecast_afterwards_equals_a_fresh_batch_given_its_parameters(base, kernel, family):
    """nothing else caches a parameter or a pool: a fresh batch given get_params(file_units=True), the state and the rings
    continues bit for bit in every plane"""
    n_sites, M = 4, 256
    b, planes = forecast(base, n_sites, M, sa.F64, steps=96, seed=9)
    b.set_kernel(kernel)
    rng = np.random.default_rng(5)
    logw = torch.tensor(rng.normal(size=n_sites * M), dtype=torch.float64, device=DEV)
    total = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
    b.pf_resample_sites(logw, [0.1, 0.3, 0.5, 0.7], with_params=True, total_out=total)
    prm0 = b.get_params()
    params = listed(IDENTITY)
    b.pf_rejuvenate(params, shrinks(n_sites), pool_names(POOLS8), pool_sds(b.get_state(), n_sites), seed=4, draw=1, site_total=total)
    st1, rings1, prm1, raw1 = b.get_state(), b.get_rings(), b.get_params(), b.get_params(file_units=True)
    assert (prm1[:, [p.index for p in params]] != prm0[:, [p.index for p in params]]).all()
    assert (prm1[:, rr.PSN_TMAX] != prm0[:, rr.PSN_TMAX]).all()
    p2, _ = b.run(96, 48)
    out = bits(p2.cpu().numpy())
    name = b.last_launch()["kernel"]
    assert name.startswith(family), name
    b.close()
    twin = sa.Batch(sa.flags_from(), n_sites, M, sa.F64, fast_math=True, kernel=kernel)
    for s in range(n_sites):
        twin.set_climate(s, site_clim(s))
        twin.set_params(s, raw1[s * M:(s + 1) * M])
    twin.setup()
    np.testing.assert_array_equal(bits(twin.get_params()), bits(prm1))
    twin.set_state(st1)
    twin.set_rings(rings1)
    p3, _ = twin.run(96, 48)
    out_twin = bits(p3.cpu().numpy())
    assert twin.last_launch()["kernel"] == name
    twin.close()
    np.testing.assert_array_equal(out_twin, out)


def test_refusals(base):
    n_sites, M = 3, 64
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48)
    st0, prm0 = b.get_state(), b.get_params()
    sd = pool_sds(st0, n_sites)
    BAD = _lib.ERR_BAD_ARGUMENT
    # the synchronous form names the site and writes nothing
    for bad in (np.nan, 0.0, 1.5, -0.5, np.inf):
        with pytest.raises(sa.SipnetError) as e:
            b.pf_rejuvenate(listed(NAMES[:2]), [0.9, 0.9, bad], pool_names(POOLS8), sd)
        assert e.value.code == BAD and "site 2" in str(e.value)
    sd_bad = sd.copy()
    sd_bad[1, 3] = -1.0
    with pytest.raises(sa.SipnetError) as e:
        b.pf_rejuvenate((), None, pool_names(POOLS8), sd_bad)
    assert e.value.code == BAD and "site 1" in str(e.value)
    # ... but not a site that is not selected
    total = torch.tensor([5, -3, 5], dtype=torch.int64, device=DEV)
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    b.pf_rejuvenate((), None, pool_names(POOLS8), sd_bad, site_total=total)
    st1 = b.get_state()
    np.testing.assert_array_equal(bits(st1[M:2 * M]), bits(st0[M:2 * M]))
    assert (st1[:M, 2] != st0[:M, 2]).all()
    with pytest.raises(ValueError):
        b.pf_rejuvenate(listed(NAMES[:2]), [0.9, 0.9])
    with pytest.raises(ValueError):
        b.pf_rejuvenate((), None, pool_names(POOLS8), sd, streams=[1, 2])
    with pytest.raises(sa.SipnetError) as e:
        b.pf_rejuvenate((), None)
    assert e.value.code == BAD and "nothing to do" in str(e.value)
    b.close()
    # a batch that was not set up
    c = sa.Batch(sa.flags_from(), 1, 64, sa.F64, fast_math=True)
    c.set_climate(0, site_clim(0))
    c.set_params(0, synth.perturbed_params(base, 64, seed=1))
    with pytest.raises(sa.SipnetError) as e:
        c.pf_rejuvenate(listed(NAMES[:2]), [0.9])
    assert e.value.code == BAD and "set up" in str(e.value)
    c.close()
    # two things wrong at once, at the smallest shape and with no launch: the arguments' refusals answer in their order,
    # and all of them before the batch's
    c = sa.Batch(sa.flags_from(), 1, 2, sa.F64, fast_math=True)
    c.set_climate(0, site_clim(0))
    c.set_params(0, synth.perturbed_params(base, 2, seed=1))
    twice = listed(NAMES[:1]) * 2
    for call, word in ((lambda: c.pf_rejuvenate(twice, None), "twice"),                                  # ... and no d_shrink
                       (lambda: c.pf_rejuvenate(twice, [0.9], ["plantWoodC"], None), "twice"),           # ... and no d_pool_sd
                       (lambda: c.pf_rejuvenate(listed(NAMES[:2]), None, ["plantWoodC"], None), "d_shrink"),
                       (lambda: c.pf_rejuvenate(listed(NAMES[:2]), None), "d_shrink"),                   # ... and not set up
                       (lambda: c.pf_rejuvenate((), None, ["plantWoodC"], None), "d_pool_sd"),
                       (lambda: c.pf_rejuvenate((), None), "nothing to do")):
        with pytest.raises(sa.SipnetError) as e:
            call()
        assert e.value.code == BAD and word in str(e.value) and "set up" not in str(e.value), str(e.value)
    c.close()
    # a batch connected across ranks
    c, _ = forecast(base, 1, 64, sa.F64, steps=48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.pf_rejuvenate(listed(NAMES[:2]), [0.9])
    assert e.value.code == BAD and "connected" in str(e.value)
    c.close()
