"""The inputs of tests/test_gpu_many_chunks.py, decided without a GPU.  That file runs the three per-chunk particle moves --
the Liu-West rejuvenation, the Metropolis move over members and the tempering search -- at sites of hundreds and thousands of
chunks of 256 members, where the code that combines the chunks' partial results takes a second tile, a second stride turn or
the branch past a cap.  What it runs on is built here, on the host, from seeds alone, and what can be known about those
inputs before a device is involved is asserted here:

* the partner ranks of the Metropolis move (tests/mcmc_move_reference.draws) do resolve into the chunks the shapes were
  chosen for: past the 2048 chunk offsets that are staged in LDS, into the chunk before and the chunk after that cap, and
  into the last chunk (one member) of the second of two sites;
* no decision of the rejuvenation (the biomass rule) or of the move (the bounds, the accept comparison) lies within the
  reference's bound of its threshold (margin > 1), so the GPU tests' own precondition cannot be what fails there;
* the tempering subjects reach all four codes of the search at every member count, under a plain numpy ESS.

Every shape is the smallest that reaches its branch; the reason stands beside it."""
import functools

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import synth
from tests import mcmc_move_reference as mr
from tests import pf_rejuvenate_reference as rr
from tests import pf_temper_reference as tr
from tests.enkf_gpu_common import BASE
from tests.test_gpu_mcmc_move import NAMES, gammas, listed, random_logp, spread_members, tuples
from tests.test_gpu_pf_rejuvenate import POOLS8, pool_sds
from tests.test_gpu_pf_temper import N_PROBE, SPECS, subject

CHUNK = 256


@functools.lru_cache(maxsize=None)
def base_params():
    return sa.read_params(BASE, sa.flags_from())[0]


def converted(members):
    """raw parameter rows -> the converted rows get_params returns, as far as the listed rows go (the nine rate rows / 365.0)"""
    prm = np.array(members, dtype=np.float64)
    prm[:, list(rr.RATE_ROWS)] = prm[:, list(rr.RATE_ROWS)] / 365.0
    return prm


def chunk_of(M, c):
    """the members of chunk c of a site of M"""
    return list(range(c * CHUNK, min((c + 1) * CHUNK, M)))


# ---- 1. rejuvenation ------------------------------------------------------------------------------------------------------
# (n_sites, M): chunks = ceil(M / 256); rejSiteKernel stages the chunks' sums in tiles of 64 chunks
REJ_SHAPES = [(1, 16384),    # 64 chunks: exactly one full tile
              (1, 16385),    # 65 chunks: a second tile of one chunk, which itself holds one member
              (1, 65537),    # 257 chunks: five tiles, the last of one chunk; the count loops' (c += 256) second turn
              (2, 65537)]    # ... and a second site's scratch at s * nCh, which must not read the first's
# (listed rows, pool mask, shrink by site parity), in the order they run: the staging loop's i % 16 < nPrm at both ends, and
# both shrinks at every site count, so a wrong mean or sd shows in every value.  The first runs before anybody is killed --
# the last chunk (one member) is live and closes a tile --, the second after, with that chunk and a tile's first chunk empty.
REJ_CONFIGS = [(1, 0, (0.5, 0.9)), (16, POOLS8, (0.9, 0.5))]
REJ_SEED = 2026


def rej_members(n_sites, M):
    return synth.perturbed_params(base_params(), n_sites * M, seed=M + n_sites)


def rej_kept(n_sites, M):
    """columns whose plantCAccountingDelta makes wood + delta fail the biomass rule whatever is drawn: members 5, one of
    the last chunk but one, and M - 1 (the last chunk's, chunk 256 at 65 537: the kept-count's second turn) of every site"""
    return [s * M + j for s in range(n_sites) for j in (5, ((M - 1) // CHUNK - 1) * CHUNK + 7, M - 1)]


def rej_dead(n_sites, M):
    """the columns killed before the second configuration, in the last site: members 0, 62 and M - 1; at 65 537 also the
    whole of chunk 64 -- the third tile begins with an empty chunk -- and of chunk 256, which is M - 1: the last chunk is empty"""
    dead = [0, 62, M - 1] + (chunk_of(M, 64) + chunk_of(M, 256) if M == 65537 else [])
    return sorted({(n_sites - 1) * M + j for j in dead})


def rej_pools(n_sites, M):
    """slots 0..12 of every column: pools of 50..150, plantCAccountingDelta about 0; -1e6 in the columns that are to be kept"""
    rng = np.random.default_rng(7 * M + n_sites)
    pools = 50.0 + 100.0 * rng.random((n_sites * M, 13))
    pools[:, rr.DELTA] = 5.0 * rng.standard_normal(n_sites * M)
    pools[rej_kept(n_sites, M), rr.DELTA] = -1e6
    return pools


def rej_shrink(n_sites, by_parity):
    return np.array([by_parity[s % 2] for s in range(n_sites)])


def rej_counts(n_sites, M, killed):
    """-> (live members, members kept) per site, with rej_dead killed or not"""
    dead = set(rej_dead(n_sites, M)) if killed else set()
    kept = [c for c in rej_kept(n_sites, M) if c not in dead]
    return ([M - sum(1 for c in dead if c // M == s) for s in range(n_sites)], [sum(1 for c in kept if c // M == s) for s in range(n_sites)])


@pytest.mark.parametrize("n_sites, M", REJ_SHAPES)
def test_no_rejuvenation_decision_lies_within_the_bound(n_sites, M):
    ncol = n_sites * M
    state = np.zeros((ncol, 32))
    state[:, :13] = rej_pools(n_sites, M)
    prm = converted(rej_members(n_sites, M))
    for draw, (n_params, mask, by_parity) in enumerate(REJ_CONFIGS):
        if draw == 1:
            state[rej_dead(n_sites, M), 29] = 3.0
        sd = pool_sds(state, n_sites)
        _, _, info, _, _, margin = rr.rejuvenate(state, prm, np.zeros(n_sites), n_sites, tuples(listed(NAMES[:n_params])),
                                                 rej_shrink(n_sites, by_parity), mask, sd, REJ_SEED + M, draw)
        assert margin.min() > 1.0, (draw, margin.min())
        live, kept = rej_counts(n_sites, M, killed=draw == 1)
        assert info[:, 0].tolist() == [rr.DONE] * n_sites and info[:, 2].tolist() == live and info[:, 3].tolist() == kept
    nCh = -(-M // CHUNK)
    if M == 65537:                                      # what the shape is for: a live last chunk, then an empty one
        assert nCh == 257 and (n_sites - 1) * M + 64 * CHUNK in rej_dead(n_sites, M) and len(chunk_of(M, 256)) == 1


# ---- 2. the Metropolis move --------------------------------------------------------------------------------------------------
MC_CAP = 2048                                           # kMcOffCap: the chunk offsets staged in LDS
MC_BIG = 2052 * CHUNK + 3                               # 2053 chunks: five past index 2047, the last of members 525 312 .. 525 314
# (n_sites, M): mcSiteKernel gives thread t the chunks [t per, (t + 1) per), per = ceil(chunks / 256)
MC_SHAPES = [(1, 65536), (2, 65536),                    # 256 chunks: per still 1, every thread has one chunk
             (1, 65537), (2, 65537)]                    # 257 chunks: per 2, thread 128 has one chunk, the threads above it
#                                                         none; the last chunk is one even member; the info loops' second turn
# the big shape, one site: (listed rows, jitter); both halves run on one batch
MC_BIG_CASES = [(1, None), (4, 0.01)]
MC_SEED, MC_DRAW = 2026, 3


def mc_rows(n_sites, M, half):
    """rows and jitter of a shape up to 65 537, paired with the half and the site count: the Philox block edges 4 and 16"""
    return (4, 0.01) if (half + n_sites) % 2 else (16, None)


def mc_members(n_sites, M):
    return spread_members(base_params(), n_sites * M, seed=M + n_sites)


def mc_dead(n_sites, M):
    """dead members of the last site, chosen so that chunk offsets tie and ranks shift.  65 537: the whole of chunk 100, in
    the middle, and of chunk 255, the last full one.  The big shape: chunks 2047 -- the last staged offset -- and 2049
    wholly, and lanes 0 and 63 of wave 1 of chunk 2048.  65 536: members at the wave edges, as the smaller shapes have them."""
    if M == 65537:
        dead = chunk_of(M, 100) + chunk_of(M, 255)
    elif M == MC_BIG:
        dead = chunk_of(M, 2047) + chunk_of(M, 2049) + [2048 * CHUNK + 64, 2048 * CHUNK + 127]
    else:
        dead = [0, 62, M - 1]
    return [(n_sites - 1) * M + j for j in dead]


def mc_state(n_sites, M):
    state = np.zeros((n_sites * M, 32))
    state[mc_dead(n_sites, M), 29] = 3.0
    return state


def partners(n_sites, M, site, half, seed, draw):
    """the members (index inside the site) that the two partner ranks of the site's moving members resolve to"""
    status = mc_state(n_sites, M)[site * M:(site + 1) * M, 29]
    j = np.arange(M)
    live = status == 0
    A, B = j[live & ((j & 1) == half)], j[live & ((j & 1) != half)]
    i1, i2, _ = mr.draws(seed, draw, site, A, len(B))
    return np.concatenate([B[i1], B[i2]])


def test_partner_ranks_resolve_past_the_offsets_staged_in_lds():
    M = MC_BIG
    assert -(-M // CHUNK) - MC_CAP >= 4
    for half in (0, 1):
        p = partners(1, M, 0, half, MC_SEED + M, MC_DRAW + half) // CHUNK
        assert (p >= MC_CAP).sum() >= 100, (half, (p >= MC_CAP).sum())          # bisected in global memory
        assert (p == MC_CAP).any() and (p == MC_CAP - 2).any()                   # the chunks either side of the dead 2047
        assert (p == 2052).any()                                                 # both halves have members in the last chunk
        assert not (p == 2047).any() and not (p == 2049).any()


def test_partner_ranks_resolve_into_the_one_member_chunk_of_the_second_site():
    M = 65537
    p = partners(2, M, 1, 1, MC_SEED + M, MC_DRAW + 1)                           # the odd half moves: member 65 536 is a partner
    assert (p == M - 1).any() and (p // CHUNK == 256).sum() == (p == M - 1).sum()
    assert not np.isin(p // CHUNK, (100, 255)).any()


def test_the_one_member_chunk_makes_a_proposal_of_its_own():
    """one site of 65 537, the even half moves: member 65 536 proposes, so chunk 256 has a count for mcInfoKernel's second turn"""
    M = 65537
    n_params, jitter = mc_rows(1, M, 0)
    moved = mr.propose(mc_state(1, M), converted(mc_members(1, M)), np.zeros(1), 1, tuples(listed(NAMES[:n_params])), gammas(1),
                       None if jitter is None else np.full(1, jitter), 0, MC_SEED + M, MC_DRAW)[2]
    assert moved[M - 1] == 1


def mc_replay(n_sites, M, cases):
    """the reference's propose and accept over cases [(half, rows, jitter)] run one after the other on one site set, as the
    GPU test runs them -> the smallest margin of each step"""
    state, prm = mc_state(n_sites, M), converted(mc_members(n_sites, M))
    status = np.zeros(n_sites)
    out = []
    for half, n_params, jitter in cases:
        params = tuples(listed(NAMES[:n_params]))
        seed, draw = MC_SEED + M, MC_DRAW + half
        prop, saved, moved, info, _, margin = mr.propose(state, prm, status, n_sites, params, gammas(n_sites),
                                                         None if jitter is None else np.full(n_sites, jitter), half, seed, draw)
        assert (info[:, 0] == mr.DONE).all() and (info[:, 1] > 0).all()
        new, cur = random_logp(np.random.default_rng(M + half), n_sites * M)
        prm, _, _, info2, margin2, acc = mr.accept(state, prop, status, n_sites, params, saved, moved, new, cur, None, seed, draw)
        assert 0 < acc.sum() < info2[:, 1].sum()
        out.append((float(margin.min()), float(margin2.min())))
    return out


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n_sites, M", MC_SHAPES)
def test_no_decision_of_the_move_lies_within_the_bound(n_sites, M, half):
    (propose, accept), = mc_replay(n_sites, M, [(half,) + mc_rows(n_sites, M, half)])
    assert propose > 1.0 and accept > 1.0, (propose, accept)


def test_no_decision_of_the_move_lies_within_the_bound_at_the_big_shape():
    """(one listed row: the reference in longdouble over 525 315 members is slow, and a margin depends on its own row alone)"""
    for propose, accept in mc_replay(1, MC_BIG, [(0, 1, None), (1, 1, None)]):
        assert propose > 1.0 and accept > 1.0, (propose, accept)


# ---- 3. the tempering search -----------------------------------------------------------------------------------------------------
# sitesGeometry: chunks of 256 columns, doubled while a site would need more than 1024 of them
TEMPER_REPLAY_M = [65536,     # 256 chunks: the last full turn of the q += 256 loops over the chunks' maxima, counts and sums
                   65537,     # 257 chunks: their second turn, over one chunk of one column
                   262144,    # 1024 chunks of 256: the most chunks a site has
                   262145]    # 513 chunks of 512 and a last one of one column: the member loops' (i += 256) second turn
TEMPER_WIDE_M = 524289        # 513 chunks of 1024: four turns of the member loops; 15 sites of it exceed the column cap, four fit
TEMPER_WIDE_SITES = 4


def numpy_ess(ll):
    """-> search()'s callable: the effective sample size of exp(d ll - max) in float64, NaN and -inf weighing nothing"""
    x = ll[np.isfinite(ll)]

    def ess(ds):
        if len(x) == 0:
            return np.zeros(len(ds))
        w = np.exp(np.multiply.outer(np.asarray(ds, dtype=np.float64), x - x.max()))
        return w.sum(1) ** 2 / (w * w).sum(1)
    return ess


@pytest.mark.parametrize("M", TEMPER_REPLAY_M)
def test_the_tempering_subjects_reach_all_four_codes(M):
    ll, dmax, target = subject(M)
    codes = {tr.search(numpy_ess(ll[s * M:(s + 1) * M]), dmax[s], target[s])[0] for s in range(N_PROBE)}
    assert codes == {tr.FOUND, tr.END, tr.NO_WEIGHT, tr.UNREACHABLE}
    assert len(SPECS) == N_PROBE
