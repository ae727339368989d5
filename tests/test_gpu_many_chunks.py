"""The three per-chunk particle moves at sites of many chunks of 256 members: the Liu-West rejuvenation (pf_rejuvenate.inc),
the Metropolis move over members (pf_metropolis.inc) and the tempering search (pf_temper.inc).  Each leaves a few numbers
per chunk in scratch, combines them in a launch per site and reads the result in later launches; the combining code has tile
loops, stride loops and a cap that change course only above 64, 256, 1024 and 2048 chunks.  The suites written with those
features stop at 17, 5 and 65 chunks.  Here every one of them runs at the smallest member counts that reach those turns,
against the references the project has: tests/pf_rejuvenate_reference.py and tests/mcmc_move_reference.py in longdouble with
their derived bounds, tests/pf_temper_reference.search replayed through the filter's own effective sample size, bit for bit.
No tolerance is new.  The inputs, the reason for every shape and what can be decided about them without a device are in
tests/test_many_chunks.py.

Worst |got - want| / bound seen on an MI355X (above 1 is a failure): rejuvenation 0.222 for a pool (1 x 16 384) and 1.24e-4
for a parameter (the parameter bound grows with the live count, (n + 16) 2^-53 ..., so it is loose here: what shows that a lost
chunk is seen is that the tests fail when the kernels are made to lose one -- a tile, a stride turn, a thread's second chunk,
the offsets past the cap --, which was tried for every loop named above); the Metropolis move 0.417 (1 x 525 315, 4 rows,
jitter 0.01).  Every tempering comparison is bit for bit.  The slowest case on the device, the move at 525 315 members with
four rows, takes 8 s, most of it the longdouble reference and the snapshots of 525 315 x 112 doubles."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from tests import pf_temper_reference as tr
from tests import test_gpu_pf_edges as pe
from tests import test_gpu_pf_temper as pt
from tests import test_many_chunks as host
from tests.enkf_gpu_common import DEV, sites_batch
from tests.test_gpu_mcmc_move import NAMES, accept_and_compare, gammas, kill, listed, propose_and_compare, random_logp
from tests.test_gpu_pf_edges import edge_batch
from tests.test_gpu_pf_rejuvenate import call_and_compare, pool_sds
from tests.test_gpu_pf_temper import N_PROBE, SPECS, dev, filter_ess, probe, same, subject, temper

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit significand on this machine")]


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    """the shared batches of this module are tests/test_gpu_pf_edges.py's edge_batch: closed as that module closes them"""
    yield
    edge_batch.cache_clear()
    while pe._open:
        pe._open.pop().close()
    torch.cuda.empty_cache()


# ---- 1. rejuvenation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sites, M", host.REJ_SHAPES)
def test_rejuvenation_over_tiles_of_chunks(n_sites, M):
    """host.REJ_SHAPES says what each member count reaches, host.REJ_CONFIGS what the two calls are: the first with every
    member live, the second after host.rej_dead has been killed.  Pools are set by hand, so that the host file knows them."""
    b = sites_batch(host.rej_members(n_sites, M), n_sites, sa.F64)
    st = b.get_state()
    st[:, :13] = host.rej_pools(n_sites, M)
    b.set_state(st)
    worst = [0.0, 0.0]
    for draw, (n_params, mask, by_parity) in enumerate(host.REJ_CONFIGS):
        if draw == 1:
            kill(b, host.rej_dead(n_sites, M))
        sd = pool_sds(b.get_state(), n_sites)
        w = call_and_compare(b, n_sites, listed(NAMES[:n_params]), host.rej_shrink(n_sites, by_parity), mask, sd,
                             seed=host.REJ_SEED + M, draw=draw)
        assert b.pf_info()["fused"] == 0
        live, kept = host.rej_counts(n_sites, M, killed=draw == 1)
        info = w[2]
        assert (info[:, 0] == 1).all() and (info[:, 1] == n_params + bin(mask).count("1")).all()
        assert info[:, 2].tolist() == live and info[:, 3].tolist() == kept       # the live count against the count killed
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    b.close()
    print(f"rejuvenation, {n_sites} x {M}: worst |got - want| / bound: parameters {worst[0]:.3g}, pools {worst[1]:.3g}")


# ---- 2. the Metropolis move ------------------------------------------------------------------------------------------------------
def move_once(b, n_sites, M, half, n_params, jitter, rings):
    """one proposal and its accept step against the reference -> (worst ratio, info of the proposal)"""
    params = listed(NAMES[:n_params])
    seed, draw = host.MC_SEED + M, host.MC_DRAW + half
    worst, saved, moved, info, prm_before = propose_and_compare(b, n_sites, params, gammas(n_sites),
                                                                None if jitter is None else np.full(n_sites, jitter), half, seed,
                                                                draw, rings=rings)
    assert b.pf_info()["fused"] == 0
    assert (info[:, 0] == 1).all() and (info[:, 1] > 0).all()
    new, cur = random_logp(np.random.default_rng(M + half), n_sites * M)
    acc, info2 = accept_and_compare(b, n_sites, params, saved, moved, new, cur, None, seed, draw, prm_before, rings=rings)
    np.testing.assert_array_equal(info2[:, 1], info[:, 1])
    assert 0 < acc.sum() < info[:, 1].sum()
    return worst, info


def dead_by_half(n_sites, M):
    """the dead of the last site -> (even members, odd members)"""
    j = np.asarray(host.mc_dead(n_sites, M)) - (n_sites - 1) * M
    return int((j % 2 == 0).sum()), int((j % 2 == 1).sum())


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n_sites, M", host.MC_SHAPES)
def test_the_move_where_a_thread_sums_several_chunks(n_sites, M, half):
    """host.MC_SHAPES: 256 chunks, the last with mcSiteKernel's per == 1, and 257, the first with per == 2"""
    b = sites_batch(host.mc_members(n_sites, M), n_sites, sa.F64)
    kill(b, host.mc_dead(n_sites, M))
    n_params, jitter = host.mc_rows(n_sites, M, half)
    worst, info = move_once(b, n_sites, M, half, n_params, jitter, rings=True)
    b.close()
    halves = [(M + 1) // 2, M // 2]
    dead = dead_by_half(n_sites, M)
    assert info[-1].tolist()[2:] == [halves[half] - dead[half], halves[1 - half] - dead[1 - half]]
    assert (info[:-1, 2] == halves[half]).all() and (info[:-1, 3] == halves[1 - half]).all()
    print(f"the move, {n_sites} x {M}, half {half}, {n_params} rows: proposed {info[:, 1].sum()} of {info[:, 2].sum()}; "
          f"worst |got - want| / bound {worst:.3f}")


@pytest.mark.parametrize("n_params, jitter", host.MC_BIG_CASES, ids=["p1-none", "p4-jit"])
def test_the_move_past_the_offsets_staged_in_lds(n_params, jitter):
    """2053 chunks: the bisection of mcProposeKernel leaves the 2048 offsets it staged and reads the rest from global memory
    (tests/test_many_chunks.py: several hundred partner ranks of each half resolve there).  Both halves on one batch.  The
    rings are left out of the snapshots (a gigabyte each); state, parameters, saved, moved and info are compared in full."""
    M = host.MC_BIG
    b = sites_batch(host.mc_members(1, M), 1, sa.F64)
    kill(b, host.mc_dead(1, M))
    dead = dead_by_half(1, M)
    halves = [(M + 1) // 2, M // 2]
    for half in (0, 1):
        worst, info = move_once(b, 1, M, half, n_params, jitter, rings=False)
        assert info[0].tolist()[2:] == [halves[half] - dead[half], halves[1 - half] - dead[1 - half]]
        print(f"the move, 1 x {M}, half {half}, {n_params} rows: proposed {info[0, 1]} of {info[0, 2]}; "
              f"worst |got - want| / bound {worst:.3f}")
    b.close()


# ---- 3. the tempering search ---------------------------------------------------------------------------------------------------
def take_split(b):
    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


def last_only(M, s, ll):
    """the subject's log-likelihoods with site s dead but for its last member, which is also the largest value of all"""
    ll = ll.copy()
    ll[s * M:(s + 1) * M] = -np.inf
    ll[(s + 1) * M - 1] = -0.25
    return ll


@pytest.mark.parametrize("M", host.TEMPER_REPLAY_M)
def test_the_search_over_many_chunks_is_the_replay_through_the_filter(M):
    """tests/test_gpu_pf_temper.py's exact replay at host.TEMPER_REPLAY_M.  Where the last chunk is one column, a second call
    in which that column is the only finite member of site 1 and so its maximum: a maximum or a count lost from the last
    stride turn changes the code (2 -> 0), not a digit."""
    b = edge_batch(N_PROBE, M)
    ll, dmax, target = subject(M)
    take_split(b)
    d, h, e, info, fused = temper(b, ll, target, dmax=dmax)
    assert fused == 0
    codes = set()
    for s in range(N_PROBE):
        site = ll[s * M:(s + 1) * M]
        want = tr.search(probe(b, site), dmax[s], target[s])
        got = (int(info[s, 0]), d[s], h[s], e[s])
        assert got[0] == want[0] and same(got[1:], want[1:]), (M, s, got, want)
        assert info[s, 1] == np.isfinite(site).sum()
        codes.add(want[0])
    assert codes == {tr.FOUND, tr.END, tr.NO_WEIGHT, tr.UNREACHABLE}
    if M % 256 == 1:
        s = 1
        ll1 = last_only(M, s, ll)
        target = target.copy()
        target[s] = 1.0                                  # (one member weighs something: its ESS is 1 at every step)
        d, h, e, info, _ = temper(b, ll1, target, dmax=dmax)
        want = tr.search(probe(b, ll1[s * M:(s + 1) * M]), dmax[s], target[s])
        got = (int(info[s, 0]), d[s], h[s], e[s])
        assert got[0] == want[0] == tr.END and same(got[1:], want[1:]), (M, got, want)
        assert info[s, 1] == 1 and e[s] == 1.0


def outputs(b, ll, target, dmax, base=None):
    """-> (delta, delta_hi, ess, info), the tempered log-weights"""
    out = torch.full((len(ll),), -7.0, dtype=torch.float64, device=DEV)
    d, h, e, info, fused = temper(b, ll, target, base=None if base is None else dev(base), dmax=dmax, out=out)
    assert fused == 0
    return (d, h, e, info.astype(np.float64)), out


def check_identities(b, n_sites, M, ll, dmax, target, minus_inf):
    """the filter's own check, and the two identities that hold the Base = true kernels to the plain ones.  The last member of
    every site is made its largest log-likelihood, so that the last chunk's entry in every maximum matters."""
    last = np.arange(1, n_sites + 1) * M - 1
    ll = ll.copy()
    ll[last] = 0.0                                      # (every other log-likelihood is below 0)
    plain, out = outputs(b, ll, target, dmax)
    code = plain[3][:, 0]
    assert (code > 0).sum() >= min(10, n_sites)
    # the tempered log-weights give the filter exactly the ESS the step was chosen for
    assert same(filter_ess(b, out)[code > 0], plain[2][code > 0])
    # a base of zeros: fma(d, x, 0) = fl(d x)
    zeros, out0 = outputs(b, ll, target, dmax, np.zeros(len(ll)))
    for x, y in zip(zeros, plain):
        assert same(x, y)
    np.testing.assert_array_equal(out0.cpu().numpy(), out.cpu().numpy())          # (as values: NaN where loglik is, -0 = 0)
    if minus_inf:
        # a base of -inf over the last chunk (one column) and 0 elsewhere: the call without base whose loglik is -inf there
        base = np.zeros(len(ll))
        base[last] = -np.inf
        without = ll.copy()
        without[last] = -np.inf
        carried, out1 = outputs(b, ll, target, dmax, base)
        lost, out2 = outputs(b, without, target, dmax)
        for x, y in zip(carried, lost):
            assert same(x, y)
        assert (carried[0] != plain[0]).any()                                     # (the column mattered)
        rest = np.ones(len(ll), dtype=bool)
        rest[last] = False
        np.testing.assert_array_equal(out1.cpu().numpy()[rest], out2.cpu().numpy()[rest])


@pytest.mark.parametrize("M", [65537, 262145])
def test_the_filter_s_ess_and_the_base_identities_over_many_chunks(M):
    b = edge_batch(N_PROBE, M)
    take_split(b)
    check_identities(b, N_PROBE, M, *subject(M), minus_inf=True)


def test_chunks_of_1024_columns():
    """524 289 members: 513 chunks of 1024 with a last one of one column.  Fifteen such sites exceed the library's column
    cap, so no replay: four sites, the first four of SPECS, under the filter's check and the zeros-base identity."""
    M, n = host.TEMPER_WIDE_M, host.TEMPER_WIDE_SITES
    ll = np.concatenate([pt.site_loglik(M, sc, seed=1000 * M + s) for s, (sc, _, _) in enumerate(SPECS[:n])])
    live = np.isfinite(ll).reshape(n, M).sum(1)
    dmax = np.array([dm for _, dm, _ in SPECS[:n]])
    target = np.array([max(fr * k, 1.0) for (_, _, fr), k in zip(SPECS[:n], live)])
    b = edge_batch(n, M)
    take_split(b)
    check_identities(b, n, M, ll, dmax, target, minus_inf=False)
