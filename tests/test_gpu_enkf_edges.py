"""The five ensemble Kalman analyses on the GPU at the sizes next to a branch of their kernels, on ill-conditioned inputs and
on degenerate ones.  The inputs are crafted, not forecast (tests/enkf_gpu_common.crafted): the pools are written into the
state, and a predicted observation is a pool or the one row of a plane, so a test costs a setup and a few launches.

A. Size edges, well conditioned, against the existing float64 references under their bound of 1e-10: member counts around
   the chunk and wave sizes, M* | M* + 1 members on either side of the one-workgroup kernel's LDS | scratch threshold
   (M* = 40960 // (8 nv); the results of both homes are checked, which home was taken cannot be seen from outside: the
   library may also fall back to scratch when the LDS is not granted), its 4096 | 4097 switch to the per-chunk launches, their one | several segments and the segment length's switch at 262144 | 262145; the
   block kernel's 1, 2, 3, 5, 48 | 49 rows and 31, 32, 33, 512 | 513 members; the smoother's seven instantiations; variable
   counts of 2 and at the caps; a padded row pitch; float32 planes.
B. The conditioning ladder of tests/enkf_exact_reference.py against the extended-precision update under bound(case, space).
   The per-site calls (sites, joint, smooth) take at most 16 observations, so they run the 4-row cases; the 32-row cases run on
   the block and local calls, spread over 8 sites x 4 operators that all list each other with rho = 1.
C. Degenerate inputs: no spread in h, identical members, two live members among 257, whole chunks without a live member,
   one live member."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import synth
from tests import enkf_block_reference as br
from tests import enkf_exact_reference as xr
from tests import enkf_joint_reference as jr
from tests import enkf_local_reference as lr
from tests import enkf_reference as er
from tests import enkf_smooth_reference as sr
from tests.enkf_gpu_common import ANALYSED, BASE, DEV, SLOTS, bits, crafted, observe, op_tuples, within
from tests.test_gpu_enkf_smooth import raw_bits, series_within

pytestmark = pytest.mark.gpu

POOLS13 = list(sa.POOLS[:13])
OFF = 100.0                                   # size edges: pools around 100 with unit spread, so no limit is near
PARAMS4 = ["aMax", "halfSatPar", "vegRespQ10", "baseVegResp"]
PARAMS16 = ["aMax", "psnTMin", "psnTOpt", "dVpdSlope", "halfSatPar", "baseVegResp", "baseFolRespFrac", "baseFineRootResp",
            "baseCoarseRootResp", "vegRespQ10", "fineRootQ10", "coarseRootQ10", "frozenSoilThreshold", "woodTurnoverRate",
            "leafTurnoverRate", "fineRootTurnoverRate"]
# the ladder: three analysed pools (one of them the signed plantCAccountingDelta, which is not clipped), the rows carried by
# pools that are neither analysed nor read by the biomass rule (wood, delta, coarse and fine roots)
LAD_SLOTS = [1, 2, 12]
LAD_ANALYSED = [POOLS13[k] for k in LAD_SLOTS]
CARRIERS = [4, 5, 8, 9]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def force_path(b, path):
    if path == "group":
        b.debug_set_num_cus(1)                # (one workgroup per site needs n_sites >= 4 x the compute units)
    elif path == "split":
        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


def params_of(names):
    return [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in names]


def tuples(params):
    return [(p.index, p.lo, p.hi) for p in params]


def ops4():
    """half the leaf carbon, wood + delta, a tenth of the soil water, the NEE plane"""
    return [sa.enkf_pools(["plantLeafC"], scale=0.5), sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"]),
            sa.enkf_pools(["soilWater"], scale=0.1), sa.enkf_plane("nee")]


def ops16():
    """13 sums of two pools and the three planes"""
    ops = [sa.enkf_pools([POOLS13[k], POOLS13[(5 * k + 1) % 13]], scale=(1.0, 0.5, 0.25)[k % 3]) for k in range(13)]
    return ops + [sa.enkf_plane("nee"), sa.enkf_plane("gpp", scale=0.5), sa.enkf_plane("et", scale=2.0)]


def well_conditioned(seed, n_sites, M, dead=()):
    """pools [ncol][13] = 100 + N(0, 1) + a per-member base, three one-row planes likewise (float32 values), and the state
    as crafted() will hold it in the slots observe() reads"""
    rng = np.random.default_rng(seed)
    ncol = n_sites * M
    common = rng.normal(size=(ncol, 1))
    pools = OFF + rng.normal(size=(ncol, 13)) + common
    planes = [(OFF + rng.normal(size=(1, ncol)) + common.T).astype(np.float32).astype(np.float64) for _ in range(3)]
    fake = np.zeros((ncol, 32))
    fake[:, :13] = pools
    fake[list(dead), 29] = 3.0
    return pools, planes, fake


def upload(planes, f32=False, pad=0):
    """every plane [rows][ncol] as a device tensor [rows][ncol + pad], the pad columns NaN"""
    out = []
    for p in planes:
        t = torch.full((p.shape[0], p.shape[1] + pad), float("nan"), dtype=torch.float32 if f32 else torch.float64, device=DEV)
        t[:, :p.shape[1]] = torch.as_tensor(p, dtype=t.dtype)
        out.append(t)
    return out


def run_sites(base, n_sites, M, prec, path, pools, planes, ops, analysed, obs, sd, params=(), infl=None, pinfl=None, pad=0,
              dead=(), rings=True):
    """the per-site call (with params the joint call) on a crafted batch -> dict(st0, st1, info, prm0, prm1)"""
    b, st0 = crafted(base, n_sites, M, prec, pools, dead)
    force_path(b, path)
    dev = upload(planes, prec == sa.F32_MIXED, pad) if planes else None
    rings0 = b.get_rings() if rings else None
    prm0 = b.get_params()
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    if params:
        b.enkf_analysis_joint(obs, sd, ops, analysed, params, planes=dev, inflation=infl, param_inflation=pinfl, info_out=info)
    else:
        b.enkf_analysis_sites(obs, sd, ops, analysed, planes=dev, inflation=infl, info_out=info)
    out = dict(st0=st0, st1=b.get_state(), info=info.cpu().numpy(), prm0=prm0, prm1=b.get_params())
    if path != "auto":
        assert b.pf_info()["fused"] == (1 if path == "group" else 0)
    if rings:
        np.testing.assert_array_equal(bits(b.get_rings()), bits(rings0))
    for t, p in zip(dev or [], planes):                                # (an analysis writes no plane)
        assert torch.equal(t[:, :p.shape[1]].double().cpu(), torch.as_tensor(p))
    b.close()
    return out


def check_sites(r, n_sites, ops, slots, obs, sd, planes, params=(), infl=None, pinfl=None, bound=1e-10):
    """run_sites' result against the per-site (or joint) reference; everything outside the analysed slots bit for bit"""
    st0 = r["st0"]
    if params:
        want, want_prm, want_info = jr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), slots, tuples(params),
                                                obs, sd, infl, pinfl, planes, r["prm0"])
        rows = [p.index for p in params]
        within(r["prm1"], want_prm, r["prm0"], n_sites, slots=rows + [jr.PSN_TMAX], bound=bound)
        rest = [k for k in range(80) if k not in rows + [jr.PSN_TMAX]]
        np.testing.assert_array_equal(bits(r["prm1"][:, rest]), bits(r["prm0"][:, rest]))
    else:
        want, want_info = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), slots, obs, sd, infl, planes,
                                      r["prm0"])
        np.testing.assert_array_equal(bits(r["prm1"]), bits(r["prm0"]))
    np.testing.assert_array_equal(r["info"], want_info)
    within(r["st1"], want, st0, n_sites, slots, bound=bound)
    other = [k for k in range(32) if k not in slots]
    np.testing.assert_array_equal(bits(r["st1"][:, other]), bits(st0[:, other]))
    untouched = np.repeat(want_info[:, 0] != 1, st0.shape[0] // n_sites) | (st0[:, 29] != 0)
    np.testing.assert_array_equal(bits(r["st1"][untouched]), bits(st0[untouched]))
    return want_info


def both_paths(base, n_sites, M, prec, pools, planes, ops, analysed, slots, obs, sd, paths=("group", "split"), **kw):
    """the call on each path against the reference, and the paths against each other bit for bit"""
    results = [run_sites(base, n_sites, M, prec, path, pools, planes, ops, analysed, obs, sd, **kw) for path in paths]
    kw = {k: v for k, v in kw.items() if k in ("params", "infl", "pinfl")}
    info = check_sites(results[0], n_sites, ops, slots, obs, sd, planes, **kw)
    for r in results[1:]:
        np.testing.assert_array_equal(bits(r["st1"]), bits(results[0]["st1"]))
        np.testing.assert_array_equal(bits(r["prm1"]), bits(results[0]["prm1"]))
        np.testing.assert_array_equal(r["info"], results[0]["info"])
    return results[0], info


# ---- A. size edges ------------------------------------------------------------------------------------------------------------
def m_star(call):
    nv = len(ANALYSED) + len(ops4()) + (len(PARAMS4) if call == "joint" else 0)
    return 40960 // (8 * nv)                  # the most members whose nv working copies of doubles fit 40 KiB of LDS


def edge_members(call):
    return [2, 3, 63, 65, 255, 257, m_star(call), m_star(call) + 1, 4095, 4096]


@pytest.mark.parametrize("call,k", [(c, k) for c in ("sites", "joint") for k in range(10)])
def test_member_counts_next_to_a_branch_on_both_paths(base, call, k):
    M = edge_members(call)[k]
    assert m_star("sites") == 465 and m_star("joint") == 341
    n_sites = 4
    dead = (1, M + M // 2, 4 * M - 1) if M > 3 else ()
    pools, planes, fake = well_conditioned(10 + k, n_sites, M, dead)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(k), nan_obs=((1, 0),))
    infl = np.array([1.0, 1.05, 1.0, 1.1])
    params = params_of(PARAMS4) if call == "joint" else ()
    pinfl = np.array([1.0, 1.0, 1.02, 1.05]) if params else None
    r, info = both_paths(base, n_sites, M, sa.F64, pools, planes, ops, ANALYSED, SLOTS, obs, sd, params=params, infl=infl,
                         pinfl=pinfl, dead=dead)
    assert (info[:, 0] == 1).all() and info[:, 2].sum() == n_sites * M - len(dead)
    assert np.abs(r["st1"][:, SLOTS] - r["st0"][:, SLOTS]).max() > 0


@pytest.mark.parametrize("call", ["sites", "joint"])
def test_4097_members_take_the_per_chunk_launches_with_two_segments(base, call):
    n_sites, M = 2, 4097
    pools, planes, fake = well_conditioned(31, n_sites, M)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(3))
    params = params_of(PARAMS4) if call == "joint" else ()
    r = run_sites(base, n_sites, M, sa.F64, "split", pools, planes, ops, ANALYSED, obs, sd, params=params)
    check_sites(r, n_sites, ops, SLOTS, obs, sd, planes, params=params)


@pytest.mark.parametrize("M", [262144, 262145])
def test_the_segment_length_switch_of_the_per_chunk_launches(base, M):
    """1024 | 1025 chunks: segments of 16 chunks | of ceil(nCh / 64).  One site, two operators, two pools."""
    rng = np.random.default_rng(M)
    common = rng.normal(size=(M, 1))
    pools = OFF + rng.normal(size=(M, 13)) + common
    planes = [(OFF + rng.normal(size=(1, M)) + common.T).astype(np.float32).astype(np.float64)] * 3
    fake = np.zeros((M, 32))
    fake[:, :13] = pools
    ops = [sa.enkf_pools(["soilWater"]), sa.enkf_plane("nee")]
    analysed, slots = ["plantLeafC", "soilC"], [1, 2]
    obs, sd = observe(fake, planes, None, 1, ops, np.random.default_rng(1))
    r = run_sites(base, 1, M, sa.F64, "split", pools, planes, ops, analysed, obs, sd, rings=False)
    info = check_sites(r, 1, ops, slots, obs, sd, planes)
    assert list(info[0]) == [1, 2, M, 0]


@pytest.mark.parametrize("shape", ["1x1", "16x13", "16x13 nan first", "16x13 nan last", "16x13 only last", "joint 16x13x16"])
def test_variable_counts_of_two_and_at_the_caps(base, shape):
    n_sites, M = 4, 257
    pools, planes, fake = well_conditioned(41, n_sites, M)
    params = ()
    if shape == "1x1":
        ops, analysed, slots = [sa.enkf_pools(["soilWater"])], ["soilC"], [2]
    else:
        ops, analysed, slots = ops16(), POOLS13, list(range(13))
        params = params_of(PARAMS16) if shape.startswith("joint") else ()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(7))
    if shape.endswith("nan first"):
        obs[:, 0] = np.nan
    elif shape.endswith("nan last"):
        obs[:, 15] = np.nan
    elif shape.endswith("only last"):
        obs[:, :15] = np.nan
    r, info = both_paths(base, n_sites, M, sa.F64, pools, planes, ops, analysed, slots, obs, sd, params=params)
    assert (info[:, 0] == 1).all() and (info[:, 1] == int((~np.isnan(obs[0])).sum())).all()
    assert np.abs(r["st1"][:, slots] - r["st0"][:, slots]).max() > 0


def complete(n_sites, rho=1.0):
    nbr = np.array([t for s in range(n_sites) for t in range(n_sites) if t != s], dtype=np.int32)
    return np.arange(n_sites + 1, dtype=np.int64) * (n_sites - 1), nbr, np.full(nbr.size, rho)


@pytest.mark.parametrize("M", [2, 65, 257, 4096])
def test_local_member_counts_on_a_complete_graph(base, M):
    n_sites = 3
    pools, planes, fake = well_conditioned(51, n_sites, M)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(M), nan_obs=((2, 1),))
    ptr, nbr, _ = complete(n_sites)
    rho = np.random.default_rng(2).uniform(0.2, 0.9, nbr.size)
    b, st0 = crafted(base, n_sites, M, sa.F64, pools)
    dev = upload(planes)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=dev, info_out=info)
    st1 = b.get_state()
    b.close()
    want, want_info = lr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr, nbr, rho,
                                  None, planes, None)
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    within(st1, want, st0, n_sites)
    other = [k for k in range(32) if k not in SLOTS]
    np.testing.assert_array_equal(bits(st1[:, other]), bits(st0[:, other]))


def star(n_sites, k, rng):
    """sites 1..k list site 0: it has 1 + k sources, every other site itself alone"""
    ptr = np.concatenate([[0], np.minimum(np.arange(n_sites), k)]).astype(np.int64)
    return ptr, np.zeros(k, dtype=np.int32), rng.uniform(0.05, 1.0, k)


def ops7():
    return ops4() + [sa.enkf_pools(["soilC"], scale=0.25), sa.enkf_plane("gpp"), sa.enkf_pools(["litterC", "fineRootC"])]


def run_block(b, loc, obs, sd, ops, analysed, dev):
    info = torch.full((b.n_sites, 4), -9, dtype=torch.int32, device=DEV)
    rows = torch.full((b.n_sites, 2), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_block(loc, obs, sd, ops, analysed, planes=dev, info_out=info, rows_out=rows)
    return b.get_state(), info.cpu().numpy(), rows.cpu().numpy()


# (rows p of the largest target, members, operators, in-neighbours of site 0): p = operators x (1 + in-neighbours)
BLOCK_EDGES = [(1, 33, 1, 0), (2, 31, 1, 1), (3, 32, 1, 2), (5, 33, 1, 4), (3, 512, 1, 2), (5, 513, 1, 4),
               (48, 512, 4, 11), (49, 512, 7, 6), (48, 513, 4, 11)]


@pytest.mark.parametrize("p,M,n_obs,k", BLOCK_EDGES, ids=[f"p{e[0]}-M{e[1]}" for e in BLOCK_EDGES])
def test_block_rows_and_members_next_to_a_branch(base, p, M, n_obs, k):
    n_sites = k + 2                                                    # (the last site neither lists nor is listed)
    pools, planes, fake = well_conditioned(61, n_sites, M)
    ops = (ops7() if n_obs == 7 else ops4())[-n_obs:] if n_obs > 1 else [sa.enkf_pools(["soilWater"], scale=0.1)]
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(p * M))
    ptr, nbr, rho = star(n_sites, k, np.random.default_rng(4))
    b, st0 = crafted(base, n_sites, M, sa.F64, pools)
    dev = upload(planes)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    assert loc.max_rows == p
    st1, info, rows = run_block(b, loc, obs, sd, ops, ANALYSED, dev)
    b.close()
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, None, planes, None)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    assert rows[:, 0].max() == p == rows[0, 0] and (rows[:, 1] == 0).all()
    within(st1, want, st0, n_sites)
    other = [s for s in range(32) if s not in SLOTS]
    np.testing.assert_array_equal(bits(st1[:, other]), bits(st0[:, other]))
    assert np.abs(st1[:M, SLOTS] - st0[:M, SLOTS]).max() > 0


SMOOTH_MEMBERS = [2, 64, 65, 128, 129, 512, 513, 1024, 1025, 2048, 2049]


def two_series(rng, n_sites, M, fake):
    """a float64 and a float32 series of 5 rows each, correlated with the members' pools"""
    ncol = n_sites * M
    z64 = 10.0 + fake[:, 3][None, :] * 0.1 + rng.normal(size=(5, ncol))
    z32 = (50.0 + fake[:, 1][None, :] + rng.normal(size=(5, ncol))).astype(np.float32)
    return [z64, z32]


def run_smooth(base, n_sites, M, pools, planes, ops, obs, sd, series, params, mode, infl=None, pad=0, dead=(), analysed=ANALYSED):
    """mode: "joint" (no series), "in place", "out of place" -> (st0, st1, prm0, prm1, info, the series after as arrays)"""
    b, st0 = crafted(base, n_sites, M, sa.F64, pools, dead)
    dev = upload(planes, pad=pad) if planes else None
    prm0 = b.get_params()
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    out = []
    if mode == "joint":
        b.enkf_analysis_joint(obs, sd, ops, analysed, params, planes=dev, inflation=infl, info_out=info)
    else:
        src = [upload([z], f32=z.dtype == np.float32, pad=pad)[0] for z in series]
        arg = src if mode == "in place" else [(z, torch.full_like(z, -7.0)) for z in src]
        dst = b.enkf_analysis_smooth(obs, sd, ops, analysed, arg, params, planes=dev, inflation=infl, info_out=info)
        ncol = n_sites * M
        out = [d.cpu().numpy() for d in dst]
        for d in out:                                                  # (the pad columns: NaN in place, untouched out of place)
            assert pad == 0 or (np.isnan(d[:, ncol:]).all() if mode == "in place" else (d[:, ncol:] == -7.0).all())
        if mode == "out of place":
            for z, t in zip(series, src):
                np.testing.assert_array_equal(raw_bits(t.cpu().numpy()[:, :ncol]), raw_bits(z))
        out = [d[:, :ncol] for d in out]
    res = (st0, b.get_state(), prm0, b.get_params(), info.cpu().numpy(), out)
    b.close()
    return res


@pytest.mark.parametrize("M", SMOOTH_MEMBERS)
def test_smoother_member_counts_next_to_an_instantiation(base, M):
    n_sites = 3
    dead = (0, M + 1) if M > 2 else ()
    pools, planes, fake = well_conditioned(71, n_sites, M, dead)
    ops, params = ops4(), params_of(PARAMS4[:2])
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(M), nan_obs=((1, 2),))
    obs[2] = np.nan                                                    # (a site that is not analysed: dst = src)
    infl = np.array([1.0, 1.05, 1.0])
    series = two_series(np.random.default_rng(M + 1), n_sites, M, fake)
    runs = {mode: run_smooth(base, n_sites, M, pools, planes, ops, obs, sd, series, params, mode, infl, dead=dead)
            for mode in ("joint", "in place", "out of place")}
    st0, st1, prm0, prm1, info, got = runs["in place"]
    for mode in ("joint", "out of place"):
        np.testing.assert_array_equal(bits(runs[mode][1]), bits(st1))
        np.testing.assert_array_equal(bits(runs[mode][3]), bits(prm1))
        np.testing.assert_array_equal(runs[mode][4], info)
    for a, c in zip(got, runs["out of place"][5]):
        np.testing.assert_array_equal(raw_bits(a), raw_bits(c))
    want, want_prm, want_info, want_series = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS,
                                                         tuples(params), obs, sd, series, infl, None, planes, prm0)
    np.testing.assert_array_equal(info, want_info)
    assert list(info[:, 0]) == [1, 1, -1]
    within(st1, want, st0, n_sites)
    for k, z in enumerate(series):
        moved = series_within(got[k], want_series[k], z, st0[:, 29], info, n_sites, float_store=z.dtype == np.float32)
        assert all(moved)


def test_a_padded_row_pitch_keeps_the_pad_out_of_sites_and_smooth(base):
    """planes and series of ld = ncol + 8, the pad columns NaN"""
    n_sites, M = 4, 257
    pools, planes, fake = well_conditioned(81, n_sites, M)
    ops = ops4()[2:] + [sa.enkf_plane("et", scale=0.5)]
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(8))
    r, info = both_paths(base, n_sites, M, sa.F64, pools, planes, ops, ANALYSED, SLOTS, obs, sd, pad=8)
    assert (info[:, 0] == 1).all() and np.isfinite(r["st1"]).all()
    series = two_series(np.random.default_rng(9), n_sites, M, fake)
    for mode in ("in place", "out of place"):
        st0, st1, prm0, _, sinfo, got = run_smooth(base, n_sites, M, pools, planes, ops, obs, sd, series, (), mode, pad=8)
        np.testing.assert_array_equal(bits(st1), bits(r["st1"]))
        want_series = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, [], obs, sd, series, None,
                                  None, planes, prm0)[3]
        for k, z in enumerate(series):
            assert np.isfinite(got[k]).all()
            series_within(got[k], want_series[k], z, st0[:, 29], sinfo, n_sites, float_store=z.dtype == np.float32)


@pytest.mark.parametrize("M", [257, m_star("sites"), m_star("sites") + 1])
def test_float32_planes_on_both_paths(base, M):
    n_sites = 4
    pools, planes, fake = well_conditioned(91, n_sites, M)
    ops = ops4()[:2] + [sa.enkf_plane("nee"), sa.enkf_plane("gpp", scale=0.5)]
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(M))
    r, info = both_paths(base, n_sites, M, sa.F32_MIXED, pools, planes, ops, ANALYSED, SLOTS, obs, sd)
    assert (info[:, 0] == 1).all()


def test_float32_planes_in_the_block_call(base):
    n_sites, M = 4, 257
    pools, planes, fake = well_conditioned(92, n_sites, M)
    ops = ops4()[:2] + [sa.enkf_plane("nee"), sa.enkf_plane("gpp", scale=0.5)]
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(5))
    ptr, nbr, rho = star(n_sites, 2, np.random.default_rng(6))
    b, st0 = crafted(base, n_sites, M, sa.F32_MIXED, pools)
    dev = upload(planes, f32=True)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    st1, info, rows = run_block(b, loc, obs, sd, ops, ANALYSED, dev)
    b.close()
    want, want_info, want_rows = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, ptr,
                                             nbr, rho, None, planes, None)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rows, want_rows)
    assert rows[0, 0] == 12
    within(st1, want, st0, n_sites)


# ---- B. the conditioning ladder -----------------------------------------------------------------------------------------------
def ladder_state(case, n_sites, n_obs):
    """pools [n_sites x n][13]: every site the case's X in the analysed slots, its n_obs rows of H in the carrier pools, 1000
    where the biomass rule looks -> (pools, obs [n_sites][n_obs], sd, the operators).  At off = 1 about a quarter of the
    entries of slots 1 and 2 (plantLeafC, soilC: 1 + N(0, 2)) are negative before and after the update; the kernels and
    er.limits both clip them to 0, so those entries compare 0 with 0.  What measures the update there is slot 12 (the signed
    plantCAccountingDelta, never clipped), the positive entries, and the smoother's series, which have no limits."""
    n = case["X"].shape[0]
    assert n_sites * n_obs == case["p"] and n_obs <= len(CARRIERS)
    pools = np.full((n_sites * n, 13), 1000.0)
    for s in range(n_sites):
        pools[s * n:(s + 1) * n, LAD_SLOTS] = case["X"]
        pools[s * n:(s + 1) * n, CARRIERS[:n_obs]] = case["H"][:, s * n_obs:(s + 1) * n_obs]
    ops = [sa.enkf_pools([POOLS13[k]]) for k in CARRIERS[:n_obs]]
    sd = np.sqrt(case["R"])
    assert (sd * sd == case["R"]).all()
    return pools, case["y"].reshape(n_sites, n_obs), sd.reshape(n_sites, n_obs), ops


def ladder_truth(case, st0, n_sites, sd):
    """the extended-precision update of the case, through the limits -> (state wanted, members kept on their forecast)"""
    n = case["X"].shape[0]
    X = xr.eakf_ld(case["X"], case["H"], case["y"], sd.reshape(-1) ** 2)
    want = st0.copy()
    kept = 0
    for s in range(n_sites):
        fc = st0[s * n:(s + 1) * n, :13]
        want[s * n:(s + 1) * n, :13], k = er.limits(fc, X, LAD_SLOTS)
        kept += int(k.sum())
    return want, kept, X


def ladder_case(name, n=64):
    case = dict(xr.case_named(name, n))
    sd = np.sqrt(case["R"])
    case["R"] = sd * sd                       # (what a kernel forms from the sd it is given)
    return case


def report(call, case, worst, bound):
    print(f"LADDER {call} {case['name']} error {worst * bound:.3e} bound {bound:.3e} ratio {worst:.3f}")


def ladder_worst(st1, want, st0, n_sites, bound):
    """within() under the case's bound -> the largest error / bound"""
    assert np.isfinite(st1).all()
    return within(st1, want, st0, n_sites, LAD_SLOTS, bound=bound) / bound


P4 = [c["name"] for c in xr.ladder() if c["p"] == 4]
ALL = [c["name"] for c in xr.ladder()]


@pytest.mark.parametrize("name", P4)
@pytest.mark.parametrize("call", ["sites", "joint"])
def test_ladder_per_site_calls(base, call, name):
    """four sites with the same rows, on the one-workgroup path (working copies in LDS) and the per-chunk launches"""
    case = ladder_case(name)
    n_sites, M = 4, 64
    case4 = dict(case, p=16, H=np.tile(case["H"], 4), y=np.tile(case["y"], 4), R=np.tile(case["R"], 4))
    pools, obs, sd, ops = ladder_state(case4, n_sites, 4)
    params = params_of(PARAMS4[:2]) if call == "joint" else ()
    bound = xr.bound(case, "member")
    results = {}
    for path in ("group", "split"):
        r = results[path] = run_sites(base, n_sites, M, sa.F64, path, pools, [], ops, LAD_ANALYSED, obs, sd, params=params)
        want, kept, _ = ladder_truth(case, r["st0"], n_sites, sd[0])
        report(f"{call}-{path}", case, ladder_worst(r["st1"], want, r["st0"], n_sites, bound), bound)
        assert kept == 0 and (r["info"] == [1, 4, M, 0]).all()
    np.testing.assert_array_equal(bits(results["split"]["st1"]), bits(results["group"]["st1"]))
    np.testing.assert_array_equal(bits(results["split"]["prm1"]), bits(results["group"]["prm1"]))


def test_ladder_sites_with_the_working_copies_in_scratch(base):
    """1000 members on the one-workgroup path: 7 x 1000 doubles do not fit the 40 KiB of LDS"""
    n_sites, M = 4, 1000
    case = xr.make_case(1e-3, 1e-2, 1.0, 4, n=M)
    sd = np.sqrt(case["R"])
    case["R"] = sd * sd
    case4 = dict(case, p=16, H=np.tile(case["H"], 4), y=np.tile(case["y"], 4), R=np.tile(case["R"], 4))
    pools, obs, sd, ops = ladder_state(case4, n_sites, 4)
    r = run_sites(base, n_sites, M, sa.F64, "group", pools, [], ops, LAD_ANALYSED, obs, sd)
    want, kept, _ = ladder_truth(case, r["st0"], n_sites, sd[0])
    bound = xr.bound(case, "member")
    report("sites-scratch", case, ladder_worst(r["st1"], want, r["st0"], n_sites, bound), bound)
    assert kept == 0 and (r["info"] == [1, 4, M, 0]).all()


@pytest.mark.parametrize("name", P4)
def test_ladder_smoother(base, name):
    """the series are copies of the analysed pools: the covariance-space stage must give them the filter's values (no limits)"""
    case = ladder_case(name)
    n_sites, M = 2, 64
    case2 = dict(case, p=8, H=np.tile(case["H"], 2), y=np.tile(case["y"], 2), R=np.tile(case["R"], 2))
    pools, obs, sd, ops = ladder_state(case2, n_sites, 4)
    series = [np.ascontiguousarray(pools[:, LAD_SLOTS].T)]
    st0, st1, _, _, info, got = run_smooth(base, n_sites, M, pools, [], ops, obs, sd, series, (), "out of place",
                                           analysed=LAD_ANALYSED)
    want, kept, X = ladder_truth(case, st0, n_sites, sd[0])
    assert kept == 0 and (info == [1, 4, M, 0]).all()
    ladder_worst(st1, want, st0, n_sites, xr.bound(case, "member"))    # (the pools: the joint call's, member space)
    bound = xr.bound(case, "cov")
    assert np.isfinite(got[0]).all()
    scale = np.maximum(np.abs(X), case["X"].std(0) + 1e-300).T
    worst = max(float((np.abs(got[0][:, s * M:(s + 1) * M] - X.T) / scale).max()) for s in range(n_sites)) / bound
    report("smooth", case, worst, bound)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("call", ["block", "local"])
def test_ladder_block_and_local(base, call, name):
    """the rows spread over sites that all list each other with rho = 1: every site's answer is the one-site update"""
    case = ladder_case(name)
    n_sites, n_obs, M = (2, 2, 64) if case["p"] == 4 else (8, 4, 64)
    pools, obs, sd, ops = ladder_state(case, n_sites, n_obs)
    ptr, nbr, rho = complete(n_sites)
    b, st0 = crafted(base, n_sites, M, sa.F64, pools)
    loc = b.enkf_localization(ptr, nbr, rho, n_obs)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    if call == "block":
        rows = torch.full((n_sites, 2), -9, dtype=torch.int32, device=DEV)
        b.enkf_analysis_block(loc, obs, sd, ops, LAD_ANALYSED, info_out=info, rows_out=rows)
        assert (rows.cpu().numpy() == [case["p"], 0]).all()
    else:
        b.enkf_analysis_local(loc, obs, sd, ops, LAD_ANALYSED, info_out=info)
    st1 = b.get_state()
    b.close()
    want, kept, _ = ladder_truth(case, st0, n_sites, sd)
    bound = xr.bound(case, "cov" if call == "block" else "member")
    report(call, case, ladder_worst(st1, want, st0, n_sites, bound), bound)
    assert kept == 0 and (info.cpu().numpy() == [1, n_obs, M, 0]).all()


# ---- C. degenerate inputs -----------------------------------------------------------------------------------------------------
DEG_OPS = [4, 5]                              # the rows: litterC and snow, read as they are


def degenerate(base, call, M, pools, obs, sd, dead=()):
    """one of: sites on the group path, on the split path, block (site 1 lists site 0), smooth -> (st0, st1, info, the
    reference's state and info, series before / after / wanted)"""
    n_sites = 4
    ops = [sa.enkf_pools([POOLS13[k]]) for k in DEG_OPS]
    series = z = zw = None
    if call in ("group", "split"):
        r = run_sites(base, n_sites, M, sa.F64, call, pools, [], ops, LAD_ANALYSED, obs, sd, dead=dead)
        st0, st1, info = r["st0"], r["st1"], r["info"]
        want, want_info = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), LAD_SLOTS, obs, sd)
    elif call == "block":
        ptr, nbr, rho = star(n_sites, 1, np.random.default_rng(1))
        b, st0 = crafted(base, n_sites, M, sa.F64, pools, dead)
        loc = b.enkf_localization(ptr, nbr, rho, len(ops))
        st1, info, _ = run_block(b, loc, obs, sd, ops, LAD_ANALYSED, None)
        b.close()
        want, want_info, _ = br.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), LAD_SLOTS, obs, sd, ptr,
                                         nbr, rho)
    else:
        series = [np.ascontiguousarray(pools[:, LAD_SLOTS].T) + 0.5]
        st0, st1, prm0, _, info, got = run_smooth(base, n_sites, M, pools, [], ops, obs, sd, series, (), "out of place",
                                                  dead=dead, analysed=LAD_ANALYSED)
        want, _, want_info, zw = sr.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), LAD_SLOTS, [], obs, sd,
                                             series, prm=prm0)
        z, zw, series = got[0], zw[0], series[0]
    np.testing.assert_array_equal(info, want_info)
    return st0, st1, info, want, series, z, zw


def spread_pools(seed, ncol):
    rng = np.random.default_rng(seed)
    return OFF + rng.normal(size=(ncol, 13)) + rng.normal(size=(ncol, 1))


CALLS = ["group", "split", "block", "smooth"]


@pytest.mark.parametrize("call", CALLS)
def test_no_spread_in_h_leaves_the_pools_to_the_bit(base, call):
    n_sites, M = 4, 257
    pools = spread_pools(1, n_sites * M)
    pools[:, DEG_OPS] = [7.0, 3.0]                                     # (sums of 257 of these are exact: var_h is 0.0)
    obs, sd = np.tile([9.0, 1.0], (n_sites, 1)), np.full((n_sites, 2), 0.5)
    st0, st1, info, want, series, z, _ = degenerate(base, call, M, pools, obs, sd)
    assert (info == [1, 2, M, 0]).all()
    np.testing.assert_array_equal(bits(st1), bits(st0))
    if z is not None:
        np.testing.assert_array_equal(bits(z), bits(series))


@pytest.mark.parametrize("call", CALLS)
def test_identical_members_stay_to_the_bit(base, call):
    n_sites, M = 4, 257
    pools = np.tile(np.round(spread_pools(2, 1) * 8.0) / 8.0, (n_sites * M, 1))    # (eighths: their sums are exact)
    obs, sd = np.tile([120.0, 90.0], (n_sites, 1)), np.tile([0.5, 2.0], (n_sites, 1))
    st0, st1, info, want, series, z, _ = degenerate(base, call, M, pools, obs, sd)
    assert (info == [1, 2, M, 0]).all()
    np.testing.assert_array_equal(bits(st1), bits(st0))
    if z is not None:
        np.testing.assert_array_equal(bits(z), bits(series))


def live_only(n_sites, M, live):
    return [s * M + j for s in range(n_sites) for j in range(M) if j not in live]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("live", ["two", "two at the end", "last chunk", "no middle chunk", "one"])
def test_few_live_members_and_chunks_without_any(base, call, live):
    n_sites = 4
    M, alive = {"two": (257, {3, 200}), "two at the end": (257, {255, 256}), "last chunk": (600, set(range(512, 600))),
                "no middle chunk": (768, set(range(0, 256)) | set(range(512, 768))), "one": (257, {256})}[live]
    dead = live_only(n_sites, M, alive)
    pools = spread_pools(3, n_sites * M)
    fake = np.zeros((n_sites * M, 32))
    fake[:, :13] = pools
    fake[dead, 29] = 3.0
    ops = [sa.enkf_pools([POOLS13[k]]) for k in DEG_OPS]
    obs, sd = observe(fake, [], None, n_sites, ops, np.random.default_rng(4))
    st0, st1, info, want, series, z, zw = degenerate(base, call, M, pools, obs, sd, dead)
    np.testing.assert_array_equal(bits(st1[dead]), bits(st0[dead]))
    if live == "one":
        assert (info == [0, 0, 1, 0]).all()
        np.testing.assert_array_equal(bits(st1), bits(st0))
        if z is not None:
            np.testing.assert_array_equal(bits(z), bits(series))
        return
    assert (info == [1, 2, len(alive), 0]).all()
    within(st1, want, st0, n_sites, LAD_SLOTS)
    moved = np.setdiff1d(np.arange(n_sites * M), dead)
    assert (st1[moved][:, LAD_SLOTS] != st0[moved][:, LAD_SLOTS]).any(1).all()
    if z is not None:
        series_within(z, zw, series, st0[:, 29], info, n_sites)
