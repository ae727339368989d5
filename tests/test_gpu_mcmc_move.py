"""The Metropolis move over members on the GPU (sipnet_batch_mcmc_propose, sipnet_batch_mcmc_accept): every value and every
decision against the longdouble reference (tests/mcmc_move_reference.py) from the state the batch holds, over the member
counts, row counts, halves, jitters, paths and precisions at which the code changes course; dead members at the wave and chunk
edges; the group path against the split path and a site alone against the same site inside a batch, bit for bit; the accept
step on hand-made log-posteriors; what must stay; the move after a resampling that carries the parameters; the bookkeeping of
a real chain against a fresh pass and the oracle; the sampler against its target; the synchronous form and the refusals.

Worst |got - want| / bound seen on an MI355X over all the comparisons of this file: 0.310 (3 x 255 members, 5 rows, jitter
0.01; the bound is the reference's derived 8 x 2^-53 (|x_j| + |gamma| (|x_r1| + |x_r2|) + w (hi - lo) (|z| + r)); above 1 is a
failure).  The sampler test there: mean off by 0.013 target sds, variance by 0.8 %, covariance by 0.1 %, acceptance 0.362."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import mcmc_move_reference as mr
from tests import pf_rejuvenate_reference as rr
from tests import test_mcmc_move as cpu
from tests.enkf_gpu_common import BASE, DEV, bits, carried_params, forecast, site_clim, sites_batch
from tests.regime_gpu_common import judge

pytestmark = pytest.mark.gpu

# sixteen rows the joint analysis accepts (file units; rate rows among them), as tests/test_gpu_pf_rejuvenate.py lists them
NAMES = ["aMax", "psnTMin", "psnTOpt", "dVpdSlope", "halfSatPar", "baseVegResp", "baseFolRespFrac", "baseFineRootResp",
         "baseCoarseRootResp", "vegRespQ10", "fineRootQ10", "coarseRootQ10", "frozenSoilThreshold", "woodTurnoverRate",
         "leafTurnoverRate", "wueConst"]
JITTERS = {"none": None, "zero": 0.0, "jit": 0.01}


def listed(names):
    return [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in names]


def tuples(params):
    return [(p.index, p.lo, p.hi) for p in params]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def spread_members(base, n, seed, names=NAMES):
    """the listed rows uniform over the middle 96 % of synth.PERTURB's bounds: proposals leave the box"""
    rng = np.random.default_rng(seed)
    members = np.tile(np.asarray(base, dtype=np.float64), (n, 1))
    for name in names:
        lo, hi, _ = synth.PERTURB[name]
        members[:, pi(name)] = lo + (0.02 + 0.96 * rng.random(n)) * (hi - lo)
    return members


def spread_batch(base, n_sites, M, prec, seed=1):
    """set up and not run: the move reads parameters and the status"""
    return sites_batch(spread_members(base, n_sites * M, seed), n_sites, prec)


def kill(b, cols):
    st = b.get_state()
    st[list(cols), 29] = 3.0
    b.set_state(st)


def set_path(b, path):
    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH if path == "split" else 0)


def want_fused(path, M):
    return 1 if path == "auto" and M <= 256 else 0


def gammas(n_sites):
    return np.array([0.42, 0.1, 0.9])[np.arange(n_sites) % 3]


def per_site(x, n_sites):
    return None if x is None else np.full(n_sites, x)


def snapshot(b, rings=True):
    """rings=False: a site of very many columns, whose rings would be gigabytes -- None stands for them"""
    return b.get_state(), b.get_params(), b.get_rings() if rings else None


def propose_and_compare(b, n_sites, params, gamma, jitter, half, seed, draw, streams=None, total=None, site_total=None, rings=True):
    """one proposal against the reference from the state the batch holds -> (worst ratio, saved, moved, info, prm before)"""
    st0, prm0, rings0 = snapshot(b, rings)
    ncol = st0.shape[0]
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    saved = torch.full((len(params), ncol), np.nan, dtype=torch.float64, device=DEV)
    moved = torch.full((ncol,), -7, dtype=torch.int32, device=DEV)
    b.mcmc_propose(params, gamma, jitter, half=half, seed=seed, draw=draw, streams=streams, site_total=site_total, saved=saved,
                   moved=moved, info_out=info)
    st1, prm1, rings1 = snapshot(b, rings)
    want_prm, want_saved, want_moved, want_info, tol, margin = mr.propose(
        st0, prm0, np.zeros(n_sites), n_sites, tuples(params), gamma, jitter, half, seed, draw, streams, total)
    assert margin.min() > 1.0, margin.min()          # no decision within the bound of its threshold: no member is excused
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    got_moved, got_saved = moved.cpu().numpy(), saved.cpu().numpy()
    np.testing.assert_array_equal(got_moved, want_moved)                 # (every column written: no -7 left)
    err = np.abs(prm1 - want_prm)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.where(tol > 0, err / tol, 0.0).max())
    assert (err <= tol).all(), worst
    made = got_moved == 1
    np.testing.assert_array_equal(bits(got_saved[:, made]), bits(want_saved[:, made]))      # the old rows, where a proposal was made
    assert np.isnan(got_saved[:, ~made]).all()                                              # ... and nowhere else
    # what must stay: state, rings and status; the rows neither listed nor derived; every column no proposal was made for
    # (the other half, the dead, the sites whose code is not 1)
    np.testing.assert_array_equal(bits(st1), bits(st0))
    if rings:
        np.testing.assert_array_equal(bits(rings1), bits(rings0))
    rows = [p.index for p in params]
    derived = ([rr.PSN_TMAX] if rr.PSN_TOPT in rows or rr.PSN_TMIN in rows else []) + (
        [rr.COARSE_ALLOC] if set(mr.ALLOC) & set(rows) else [])
    rest = [k for k in range(80) if k not in rows + derived]
    np.testing.assert_array_equal(bits(prm1[:, rest]), bits(prm0[:, rest]))
    np.testing.assert_array_equal(bits(prm1[~made]), bits(prm0[~made]))
    M = ncol // n_sites
    assert not made[np.repeat(want_info[:, 0] != 1, M)].any() and not made[st0[:, 29] != 0].any()
    assert not made[(np.arange(ncol) % M) % 2 != half].any()
    return worst, saved, moved, want_info, prm0


def accept_and_compare(b, n_sites, params, saved, moved, logp_new, logp_cur, beta, seed, draw, prm_before, streams=None, rings=True):
    """the accept step against the reference -> (accepted mask, info); prm_before: the rows before the proposal"""
    st0, prm0, rings0 = snapshot(b, rings)
    moved0, saved0 = moved.cpu().numpy(), saved.cpu().numpy()
    new_t = torch.tensor(logp_new, dtype=torch.float64, device=DEV)
    cur_t = torch.tensor(logp_cur, dtype=torch.float64, device=DEV)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.mcmc_accept(params, saved, moved, new_t, cur_t, beta, seed=seed, draw=draw, streams=streams, info_out=info)
    st1, prm1, rings1 = snapshot(b, rings)
    want_prm, want_moved, want_cur, want_info, margin, acc = mr.accept(
        st0, prm0, np.zeros(n_sites), n_sites, tuples(params), saved0, moved0, logp_new, logp_cur, beta, seed, draw, streams)
    assert margin.min() > 1.0, margin.min()
    np.testing.assert_array_equal(info.cpu().numpy(), want_info)
    np.testing.assert_array_equal(moved.cpu().numpy(), want_moved)
    np.testing.assert_array_equal(bits(cur_t.cpu().numpy()), bits(want_cur))
    np.testing.assert_array_equal(bits(new_t.cpu().numpy()), bits(np.asarray(logp_new, dtype=np.float64)))    # the caller's array stays
    np.testing.assert_array_equal(bits(prm1), bits(want_prm))
    handled = (moved0 == 1) & (want_moved == 0)
    rejected = handled & ~acc
    np.testing.assert_array_equal(bits(prm1[rejected]), bits(prm_before[rejected]))      # all 80 rows as before the proposal
    np.testing.assert_array_equal(bits(prm1[~rejected]), bits(prm0[~rejected]))          # accepted, or not handled: as they were
    np.testing.assert_array_equal(bits(st1), bits(st0))
    if rings:
        np.testing.assert_array_equal(bits(rings1), bits(rings0))
    return acc, want_info


def random_logp(rng, ncol):
    """log-posteriors a few units apart, some of them -inf"""
    new, cur = -50.0 + 3.0 * rng.standard_normal(ncol), -50.0 + 3.0 * rng.standard_normal(ncol)
    new[rng.random(ncol) < 0.05] = -np.inf
    return new, cur


# (n_sites, M, n_params, half, jitter, path, precision): the member counts around a wave, a chunk and two chunks; the Philox
# block edges 1, 4, 5, 16; paired, not the full product
MS = [4, 5, 63, 64, 65, 255, 256, 257, 513]
CASES = []
for rep in range(3):
    for n_sites in (1, 3):
        for M in MS:
            i = len(CASES)
            CASES.append((n_sites, M, (1, 4, 5, 16)[(i + rep) % 4], (i + rep) % 2, ("none", "zero", "jit")[(i + 2 * rep) % 3],
                          "split" if rep == 1 else "auto", sa.F32_MIXED if (i + rep) % 3 == 0 else sa.F64))
CASES += [(3, 513, 16, 1, "jit", "split", sa.F64), (1, 256, 16, 0, "jit", "split", sa.F32_MIXED), (3, 4, 16, 1, "jit", "auto", sa.F64),
          (1, 64, 1, 1, "none", "split", sa.F64), (3, 257, 4, 0, "zero", "auto", sa.F32_MIXED), (1, 1025, 5, 1, "jit", "auto", sa.F64)]


def case_id(c):
    return f"{c[0]}x{c[1]}-p{c[2]}-h{c[3]}-{c[4]}-{c[5]}-{'f32' if c[6] == sa.F32_MIXED else 'f64'}"


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_values_and_decisions(base, case):
    n_sites, M, n_params, half, jit, path, prec = case
    b = spread_batch(base, n_sites, M, prec, seed=M + n_params)
    set_path(b, path)
    if M >= 63:                                         # dead members at the wave edges of the last site
        kill(b, [(n_sites - 1) * M + j for j in (0, 62, M - 1)])
    params = listed(NAMES[:n_params])
    seed, draw = 2026 + M, 3 + n_params
    worst, saved, moved, info, prm_before = propose_and_compare(b, n_sites, params, gammas(n_sites), per_site(JITTERS[jit], n_sites),
                                                                half, seed, draw)
    assert b.pf_info()["fused"] == want_fused(path, M)
    assert (info[:, 0] == 1).all() and (info[:, 2] + info[:, 3] >= M - 3).all()
    rng = np.random.default_rng(M)
    new, cur = random_logp(rng, n_sites * M)
    acc, info2 = accept_and_compare(b, n_sites, params, saved, moved, new, cur, None, seed, draw, prm_before)
    b.close()
    np.testing.assert_array_equal(info2[:, 1], info[:, 1])
    print(f"{case_id(case)}: proposed {info[:, 1].sum()} of {info[:, 2].sum()}, accepted {int(acc.sum())}; "
          f"worst |got - want| / bound {worst:.3f}")


# ---- dead members at the edges ------------------------------------------------------------------------------------------
def odd(js):
    return [j for j in js if j & 1]


DEAD = {"lanes 0 and 63 of a wave": lambda M: [64, 127],
        "the last column of a chunk": lambda M: [255],
        "a whole wave": lambda M: list(range(128, 192)),
        "a whole chunk": lambda M: list(range(256, 512)),
        "the other half but two": lambda M: [j for j in odd(range(M)) if j not in (65, M - 2 if (M - 2) & 1 else M - 1)],
        "the other half but one": lambda M: [j for j in odd(range(M)) if j != 129]}


DEAD_CASES = [(what, M, path) for what in DEAD for M, path in ((256, "auto"), (256, "split"), (513, "auto"))
              if what != "a whole chunk" or M == 513]


@pytest.mark.parametrize("what, M, path", DEAD_CASES, ids=[f"{w.replace(' ', '_')}-{M}-{p}" for w, M, p in DEAD_CASES])
def test_dead_members_at_the_edges(base, what, M, path):
    n_sites = 2
    b = spread_batch(base, n_sites, M, sa.F64, seed=17)
    set_path(b, path)
    dead = DEAD[what](M)
    kill(b, [M + j for j in dead])                       # in site 1
    params = listed(NAMES[:4])
    worst, saved, moved, info, prm_before = propose_and_compare(b, n_sites, params, [0.3, 0.3], [0.0, 0.005], 0, 7, 1)
    n_odd, n_even = M // 2, (M + 1) // 2
    dead_odd, dead_even = len(odd(dead)), len(dead) - len(odd(dead))
    assert info[0].tolist()[2:] == [n_even, n_odd] and info[0, 0] == 1
    assert info[1].tolist()[2:] == [n_even - dead_even, n_odd - dead_odd]
    if what == "the other half but two":
        assert info[1, 0] == 1 and info[1, 3] == 2 and info[1, 1] > 0
    elif what == "the other half but one":
        assert info[1].tolist() == [0, 0, n_even, 1]          # untouched bit for bit: propose_and_compare has compared
    else:
        assert info[1, 0] == 1 and info[1, 1] > 0
    # the odd half moves, its partners are the even members
    worst2, _, _, info2, _ = propose_and_compare(b, n_sites, params, [0.3, 0.3], None, 1, 7, 2)
    assert info2[1].tolist()[2:] == [n_odd - dead_odd, n_even - dead_even] and info2[1, 0] == 1
    b.close()
    print(f"{what}, M = {M} ({path}): worst |got - want| / bound {max(worst, worst2):.3f}")


# ---- the two paths, and a site alone -------------------------------------------------------------------------------------
def moved_once(base, path, M, prec, n_sites=3, streams=None):
    b = spread_batch(base, n_sites, M, prec, seed=23)
    set_path(b, path)
    kill(b, [1, M + (63 if M > 63 else 2)])
    params = listed(NAMES)
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    saved, moved = b.mcmc_propose(params, np.full(n_sites, 0.05), np.full(n_sites, 0.002), half=1, seed=11, draw=3, streams=streams,
                                  info_out=info)
    fused = b.pf_info()["fused"]
    out = [b.get_params(), saved.cpu().numpy(), moved.cpu().numpy(), info.cpu().numpy()]
    rng = np.random.default_rng(M)
    new, cur = random_logp(rng, n_sites * M)
    cur_t = torch.tensor(cur, device=DEV)
    b.mcmc_accept(params, saved, moved, torch.tensor(new, device=DEV), cur_t, seed=11, draw=3, streams=streams, info_out=info)
    out += [b.get_params(), cur_t.cpu().numpy(), info.cpu().numpy()]
    b.close()
    return out, fused


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [4, 64, 256])
def test_group_and_split_paths_are_bit_identical(base, M, prec):
    (first, fused), (second, fused2) = moved_once(base, "auto", M, prec), moved_once(base, "split", M, prec)
    assert (fused, fused2) == (1, 0)
    assert first[2].sum() > 0
    for x, y in zip(first, second):
        if x.dtype == np.float64:
            np.testing.assert_array_equal(bits(x), bits(y))
        else:
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("M", [200, 257])           # (one workgroup per site; the per-chunk launches)
def test_a_site_does_not_depend_on_the_batch_around_it(base, M):
    """site 2 of three, with streams given, against the same columns alone in a batch of one site"""
    members = spread_members(base, 3 * M, seed=6)
    three = sites_batch(members, 3, sa.F64)
    alone = sites_batch(members[2 * M:], 1, sa.F64, clim=lambda s: site_clim(2))
    kill(three, [2 * M + 64, 2 * M + 7])
    kill(alone, [64, 7])
    np.testing.assert_array_equal(bits(alone.get_params()), bits(three.get_params()[2 * M:]))
    params = listed(NAMES[:7])
    rng = np.random.default_rng(M)
    new, cur = random_logp(rng, 3 * M)
    results = []
    for b, sl, streams, g in ((three, slice(2 * M, 3 * M), [5, 9, 77], [0.2, 0.3, 0.1]), (alone, slice(0, M), [77], [0.1])):
        n = len(streams)
        info = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
        saved, moved = b.mcmc_propose(params, g, np.full(n, 0.003), half=0, seed=21, draw=5, streams=streams, info_out=info)
        mine = slice(2 * M, 3 * M)                       # (the site's log-posteriors, wherever the site sits)
        out = [b.get_params()[sl], saved.cpu().numpy()[:, sl], moved.cpu().numpy()[sl], info.cpu().numpy()[-1]]
        cur_t = torch.tensor(cur[mine] if n == 1 else cur, device=DEV)
        b.mcmc_accept(params, saved, moved, torch.tensor(new[mine] if n == 1 else new, device=DEV), cur_t, seed=21, draw=5,
                      streams=streams, info_out=info)
        out += [b.get_params()[sl], cur_t.cpu().numpy()[sl], info.cpu().numpy()[-1]]
        results.append(out)
        b.close()
    assert results[0][2].sum() > 0
    for x, y in zip(*results):
        if x.dtype == np.float64:
            np.testing.assert_array_equal(bits(x), bits(y))
        else:
            np.testing.assert_array_equal(x, y)


# ---- accept ----------------------------------------------------------------------------------------------------------------
def allocation_batch(base, n_sites, M, prec=sa.F64):
    """wood allocations spread so that some proposals fail ensureAllocation's test; psnTOpt and aMax spread too"""
    members = spread_members(base, n_sites * M, seed=31, names=["aMax", "psnTOpt"])
    rng = np.random.default_rng(32)
    members[:, pi("leafAllocation")] = 0.3
    members[:, pi("fineRootAllocation")] = 0.2
    members[:, pi("woodAllocation")] = 0.1 + 0.38 * rng.random(n_sites * M)
    return sites_batch(members, n_sites, prec)


ALLOC_PARAMS = [("psnTOpt", 5.0, 30.0), ("woodAllocation", 0.05, 0.6), ("aMax", 0.0, 34.0)]


@pytest.mark.parametrize("M, path", [(256, "auto"), (300, "auto"), (64, "split")])
def test_accept_on_hand_made_log_posteriors(base, M, path):
    n_sites = 2
    b = allocation_batch(base, n_sites, M)
    set_path(b, path)
    params = [sa.enkf_param(*p) for p in ALLOC_PARAMS]
    worst, saved, moved, info, prm_before = propose_and_compare(b, n_sites, params, [0.4, 0.4], None, 0, 5, 0)
    prm_prop = b.get_params()
    made = np.flatnonzero(moved.cpu().numpy() == 1)
    alive = (np.arange(n_sites * M) % M) % 2 == 0
    assert 8 <= len(made) < alive.sum()                  # some proposals were not made: the bounds, the allocation test
    wood = prm_prop[:, rr.WOOD_ALLOC]
    assert (wood[made] <= 0.5 + 1e-12).all() and (prm_prop[made, rr.COARSE_ALLOC] >= 0).all()
    assert (prm_prop[made, rr.PSN_TMAX] != prm_before[made, rr.PSN_TMAX]).all()
    assert (prm_prop[made, rr.COARSE_ALLOC] != prm_before[made, rr.COARSE_ALLOC]).all()
    rng = np.random.default_rng(1)
    new, cur = random_logp(rng, n_sites * M)
    special = [(-np.inf, -np.inf), (np.inf, 0.0), (np.nan, 0.0), (0.0, np.nan), (1.0, -np.inf), (2.0, 2.0), (-np.inf, 0.0), (5.0, 1.0)]
    want = [False, False, False, False, True, True, False, True]
    for col, (n_, c_) in zip(made, special):
        new[col], cur[col] = n_, c_
    beta = [1.0, 0.25]
    acc, info2 = accept_and_compare(b, n_sites, params, saved, moved, new, cur, beta, 5, 0, prm_before)
    assert [bool(acc[c]) for c in made[:8]] == want
    assert 0 < acc.sum() < len(made) and info2[:, 2].sum() == acc.sum() and (info2[:, 3] == M).all()
    # beta = 0.25 against 1: with the site's draws the tempered comparison accepts whatever the plain one does when new < cur
    site1 = np.arange(M, 2 * M)
    plain = mr.accept(b.get_state(), prm_prop, np.zeros(n_sites), n_sites, tuples(params), saved.cpu().numpy(),
                      (np.isin(np.arange(n_sites * M), made)).astype(np.int32), new, cur, [1.0, 1.0], 5, 0)[5]
    down = site1[(new[site1] < cur[site1]) & np.isin(site1, made)]
    assert (acc[down] >= plain[down]).all() and (acc[down] != plain[down]).any()
    # a second accept changes nothing
    prm2 = b.get_params()
    cur_t = torch.tensor(cur, device=DEV)
    info3 = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
    b.mcmc_accept(params, saved, moved, torch.tensor(new, device=DEV), cur_t, beta, seed=5, draw=0, info_out=info3)
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm2))
    np.testing.assert_array_equal(bits(cur_t.cpu().numpy()), bits(cur))
    np.testing.assert_array_equal(info3.cpu().numpy(), [[1, 0, 0, M], [1, 0, 0, M]])
    b.close()


# ---- after a resampling that carries the parameters ------------------------------------------------------------------------
def test_after_a_resampling_that_carries_the_parameters(base):
    n_sites, M = 4, 256
    b, _ = forecast(base, n_sites, M, sa.F64, steps=48, seed=12)
    rng = np.random.default_rng(2)
    logw = torch.tensor(3.0 * rng.normal(size=n_sites * M), dtype=torch.float64, device=DEV)
    ess_min = np.array([1e9, 0.0, 1e9, 1e9])            # site 1 keeps its particles: total -3
    total = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
    anc = b.pf_resample_sites(logw, [0.1, 0.3, 0.5, 0.7], ess_min=ess_min, with_params=True, total_out=total).cpu().numpy()
    tot = total.cpu().numpy()
    assert tot[1] == -3 and (tot[[0, 2, 3]] > 0).all()
    twins = np.flatnonzero(anc[1:] == anc[:-1])
    assert len(twins) > M
    prm0 = carried_params(b)
    np.testing.assert_array_equal(bits(prm0[twins]), bits(prm0[twins + 1]))
    params = listed(["aMax", "halfSatPar", "vegRespQ10", "psnTOpt"])
    # (the ensemble is narrow: a jitter of 1e-3 of the box separates the twins)
    worst, saved, moved, info, prm_before = propose_and_compare(b, n_sites, params, np.full(n_sites, mr.demc_gamma(4)),
                                                                np.full(n_sites, 1e-3), 0, 31, 7, total=tot, site_total=total)
    assert info[:, 0].tolist() == [1, -3, 1, 1] and info[1, 1] == 0 and (info[[0, 2, 3], 1] > 0).all()
    prm1 = b.get_params()
    np.testing.assert_array_equal(bits(carried_params(b)), bits(prm1))            # every column has its own rows now
    np.testing.assert_array_equal(bits(prm_before), bits(prm0))
    new, cur = random_logp(rng, n_sites * M)
    beta = [0.25, 1.0, np.nan, 0.5]                      # site 2: bad input, untouched, its moved flags stay
    acc, info2 = accept_and_compare(b, n_sites, params, saved, moved, new, cur, beta, 31, 7, prm_before)
    assert info2[:, 0].tolist() == [1, 1, -2, 1] and info2[2].tolist() == [-2, 0, 0, M]
    assert moved.cpu().numpy()[2 * M:3 * M].sum() == info[2, 1] and moved.cpu().numpy()[:2 * M].sum() == 0
    b.close()
    print(f"after a resampling: worst |got - want| / bound {worst:.3f}")


# ---- the bookkeeping of a real chain ----------------------------------------------------------------------------------------
def test_a_real_chain_keeps_its_books(base, oracle):
    """8 half-sweeps of propose -> setup -> run -> series_loglik -> accept on 1 site x 64 members x 96 steps; then one more
    setup -> run -> series_loglik gives every live member the log-posterior the chain holds for it, bit for bit, and the run
    is the oracle's run of the parameters the members now carry"""
    M, T = 64, 96
    members = synth.perturbed_params(base, M, seed=3)
    b = sites_batch(members, 1, sa.F64)
    planes, _ = b.run(0, T)
    nee = planes[0].double().cpu().numpy()
    rng = np.random.default_rng(9)
    spread = nee.std(1) + 1e-3 * np.abs(nee).mean()
    obs = (nee[:, 0] + 0.5 * spread * rng.standard_normal(T))[None, :]
    sd = (2.0 * spread)[None, :]
    params = listed(["aMax", "halfSatPar", "vegRespQ10"])

    def loglik(out=None):
        return b.series_loglik([sa.loglik_term(planes[0], obs, sd)], out=out)

    cur = loglik()
    first = cur.cpu().numpy().copy()
    new = torch.empty_like(cur)
    info = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    proposed = accepted = 0
    for it in range(8):
        saved, moved = b.mcmc_propose(params, [mr.demc_gamma(3)], [1e-4], half=it & 1, seed=77, draw=it, info_out=info)
        proposed += int(info[0, 1])
        b.setup()
        b.run(0, T, planes=planes)
        loglik(out=new)
        b.mcmc_accept(params, saved, moved, new, cur, seed=77, draw=it, info_out=info)
        accepted += int(info[0, 2])
    assert 0 < accepted < proposed <= 8 * (M // 2)
    held = cur.cpu().numpy()
    assert (held != first).sum() >= 1
    b.setup()
    b.run(0, T, planes=planes)
    again = loglik().cpu().numpy()
    live = b.get_status() == 0
    assert live.sum() > M // 2
    np.testing.assert_array_equal(bits(again[live]), bits(held[live]))
    rest, _ = b.run(T, b.n_steps - T)                    # (the oracle runs the whole forcing: so does the batch)
    status, state, raw = b.get_status(), b.get_state(), b.get_params(file_units=True)
    got = np.concatenate([planes.double().cpu().numpy(), rest.double().cpu().numpy()], axis=1)
    b.close()
    pick = np.flatnonzero((held != first) & live)[:2].tolist()
    pick += [int(c) for c in np.flatnonzero(live) if c not in pick][:3 - len(pick)]
    want, final, st = oracle.run_block(sa.flags_from(), raw[pick], site_clim(0))
    judge(f"after 8 half-sweeps, members {pick}", sa.F64, got[:, :, pick], state[pick], status[pick], want, final, st)
    print(f"a real chain: {accepted} of {proposed} proposals accepted")


# ---- the sampler samples the target -------------------------------------------------------------------------------------------
def test_the_sampler_samples_the_target(base):
    """tests/test_mcmc_move.py's Gaussian with 600 full sweeps on 1 x 64 members, the log-density computed on the host from
    get_params each half-sweep: pooled mean, variances and covariance within 2 x the worst deviations of the reference
    sampler over 20 seeds (written down there), the acceptance rate strictly inside (0.05, 0.95)"""
    names = ["aMax", "wueConst"]
    rows = [pi(n) for n in names]
    assert not set(rows) & set(rr.RATE_ROWS)
    seed = 21                                            # (not one of the 20 seeds the constants come from)
    members = np.tile(np.asarray(base, dtype=np.float64), (cpu.MEMBERS, 1))
    members[:, rows] = cpu.start_points(seed)
    b = sites_batch(members, 1, sa.F64)
    params = [sa.enkf_param(n, cpu.BOX_LO[k], cpu.BOX_HI[k]) for k, n in enumerate(names)]
    gamma, jitter = [mr.demc_gamma(2)], [cpu.JITTER]
    cur = torch.tensor(cpu.target_logdens(b.get_params()[:, rows]), device=DEV)
    saved = torch.zeros((2, cpu.MEMBERS), dtype=torch.float64, device=DEV)
    moved = torch.zeros(cpu.MEMBERS, dtype=torch.int32, device=DEV)
    info = torch.zeros((2 * cpu.SWEEPS, 4), dtype=torch.int32, device=DEV)
    samples = np.zeros((cpu.SWEEPS, cpu.MEMBERS, 2))
    for it in range(2 * cpu.SWEEPS):
        b.mcmc_propose(params, gamma, jitter, half=it & 1, seed=seed, draw=it, saved=saved, moved=moved,
                       info_out=info[it:it + 1].view(-1))
        x = b.get_params()[:, rows]
        new = torch.tensor(cpu.target_logdens(x), device=DEV)
        b.mcmc_accept(params, saved, moved, new, cur, seed=seed, draw=it, info_out=info[it:it + 1].view(-1))
        if it & 1:
            samples[it >> 1] = b.get_params()[:, rows]
    b.close()
    counts = info.cpu().numpy()
    assert (counts[:, 0] == 1).all()
    rate = counts[:, 2].sum() / counts[:, 1].sum()
    mean, var, cov = cpu.deviations(samples[cpu.BURN:])
    print(f"GPU sampler: mean off by {mean:.4f} target sds (bound {2 * cpu.WORST_MEAN_SDS:.4f}), variance {var:.4f} "
          f"({2 * cpu.WORST_VAR_REL:.4f}), covariance {cov:.4f} ({2 * cpu.WORST_COV_REL:.4f}); acceptance {rate:.3f}")
    assert mean <= 2 * cpu.WORST_MEAN_SDS and var <= 2 * cpu.WORST_VAR_REL and cov <= 2 * cpu.WORST_COV_REL
    assert 0.05 < rate < 0.95


# ---- the synchronous form and the refusals -----------------------------------------------------------------------------------
def test_synchronous_form_and_refusals(base):
    n_sites, M = 3, 64
    b = spread_batch(base, n_sites, M, sa.F64, seed=4)
    st0, prm0 = b.get_state(), b.get_params()
    params = listed(NAMES[:2])
    BAD = _lib.ERR_BAD_ARGUMENT
    saved = torch.full((2, n_sites * M), np.nan, dtype=torch.float64, device=DEV)
    moved = torch.full((n_sites * M,), -7, dtype=torch.int32, device=DEV)
    # the synchronous form names the site and writes nothing
    for gamma, jitter in (([0.3, 0.3, np.nan], None), ([0.3, 0.3, np.inf], None), ([0.3] * 3, [0.0, 0.0, -1.0]), ([0.3] * 3, [0.0, 0.0, np.nan])):
        with pytest.raises(sa.SipnetError) as e:
            b.mcmc_propose(params, gamma, jitter, saved=saved, moved=moved)
        assert e.value.code == BAD and "site 2" in str(e.value)
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm0))
    assert (moved.cpu().numpy() == -7).all() and np.isnan(saved.cpu().numpy()).all()
    # ... but not a site that is not selected
    total = torch.tensor([5, 5, -3], dtype=torch.int64, device=DEV)
    b.mcmc_propose(params, [0.3, 0.3, np.nan], None, site_total=total, saved=saved, moved=moved)
    prm1, mv = b.get_params(), moved.cpu().numpy()
    np.testing.assert_array_equal(bits(prm1[2 * M:]), bits(prm0[2 * M:]))
    assert mv[:2 * M].sum() > 0 and mv[2 * M:].sum() == 0 and set(mv.tolist()) == {0, 1}
    new = torch.zeros(n_sites * M, dtype=torch.float64, device=DEV)
    cur = torch.zeros(n_sites * M, dtype=torch.float64, device=DEV)
    for beta in ([1.0, 0.0, 1.0], [1.0, np.nan, 1.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(sa.SipnetError) as e:
            b.mcmc_accept(params, saved, moved, new, cur, beta)
        assert e.value.code == BAD and "site 1" in str(e.value)
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm1))
    np.testing.assert_array_equal(moved.cpu().numpy(), mv)
    b.mcmc_accept(params, saved, moved, new, cur)       # equal log-posteriors: every proposal is accepted
    np.testing.assert_array_equal(bits(b.get_params()), bits(prm1))
    assert moved.cpu().numpy().sum() == 0
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    # the binding's own checks
    with pytest.raises(ValueError):
        b.mcmc_propose(params, [0.3, 0.3])
    with pytest.raises(ValueError):
        b.mcmc_propose(params, [0.3] * 3, streams=[1, 2])
    with pytest.raises(ValueError):
        b.mcmc_propose(params, [0.3] * 3, saved=saved[:1])
    with pytest.raises(ValueError):
        b.mcmc_accept(params, saved, moved, new[:5], cur)
    with pytest.raises(sa.SipnetError) as e:
        b.mcmc_propose(params, [0.3] * 3, half=2)
    assert e.value.code == BAD and "half" in str(e.value)
    with pytest.raises(sa.SipnetError) as e:
        b.mcmc_propose([], [0.3] * 3)
    assert e.value.code == BAD and "1..16" in str(e.value)
    b.close()
    # a batch that was not set up
    c = sa.Batch(sa.flags_from(), 1, 64, sa.F64, fast_math=True)
    c.set_climate(0, site_clim(0))
    c.set_params(0, synth.perturbed_params(base, 64, seed=1))
    with pytest.raises(sa.SipnetError) as e:
        c.mcmc_propose(params, [0.3])
    assert e.value.code == BAD and "set up" in str(e.value)
    c.close()
    # two things wrong at once, at the smallest shape and with no launch: n_params, the listed rows, the half and a NULL
    # array answer in that order, and all of them before the batch's
    c = sa.Batch(sa.flags_from(), 1, 2, sa.F64, fast_math=True)
    c.set_climate(0, site_clim(0))
    c.set_params(0, synth.perturbed_params(base, 2, seed=1))
    L, twice = sa.lib(), listed(NAMES[:1]) * 2
    sv, mv2, lp = saved[:, :2].contiguous(), moved[:2].contiguous(), new[:2].contiguous()
    P = _lib.ptr

    def raw_propose(prm, half, gamma, sv_, mv_):
        return L.sipnet_batch_mcmc_propose(c.h, len(prm), (_lib.EnkfParam * len(prm))(*prm), P(gamma), None, half, 1, 0, None, None,
                                           P(sv_), P(mv_), None, None)

    def raw_accept(prm, sv_, mv_, new_, cur_):
        return L.sipnet_batch_mcmc_accept(c.h, len(prm), (_lib.EnkfParam * len(prm))(*prm), P(sv_), P(mv_), P(new_), P(cur_), None,
                                          1, 0, None, None, None)

    for call, word in ((lambda: raw_propose(twice, 2, None, sv, mv2), "twice"),            # ... a bad half, no d_gamma, not set up
                       (lambda: raw_propose(params, 2, None, sv, mv2), "half"),            # ... no d_gamma, not set up
                       (lambda: raw_propose(params, 2, lp, sv, mv2), "half"),              # ... not set up
                       (lambda: raw_propose(params, 1, lp, None, None), "NULL d_saved"),   # ... no d_moved, not set up
                       (lambda: raw_propose(params, 0, lp, sv, None), "NULL d_moved"),     # ... not set up
                       (lambda: raw_accept(twice, None, mv2, lp, lp), "twice"),            # ... no d_saved, not set up
                       (lambda: raw_accept(params, sv, mv2, None, None), "NULL d_logp_new"),
                       (lambda: raw_accept(params, sv, mv2, lp, None), "NULL d_logp_cur")):
        assert call() == BAD
        why = L.sipnet_last_error().decode()
        assert word in why and "set up" not in why, why
    c.close()
    # a batch connected across ranks
    c, _ = forecast(base, 1, 64, sa.F64, steps=48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    for call in (lambda: c.mcmc_propose(params, [0.3]),
                 lambda: c.mcmc_accept(params, saved[:, :64].contiguous(), moved[:64].contiguous(), new[:64].contiguous(), cur[:64].contiguous())):
        with pytest.raises(sa.SipnetError) as e:
            call()
        assert e.value.code == BAD and "connected" in str(e.value)
    c.close()
