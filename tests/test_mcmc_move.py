"""The Metropolis move over members without a GPU: the library's host draws (sa.mcmc_draws) against the numpy reference
(tests/mcmc_move_reference.py), the constants the binding mirrors, the refusals that answer before a device is touched, the
reference's own rules on a hand-made site, and the stationarity of the reference sampler -- whose worst deviations, written
down below, bound the GPU test of the same sampler (tests/test_gpu_mcmc_move.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from sipnet_amd.config import param_index as pi
from tests import helpers
from tests import mcmc_move_reference as mr
from tests import pf_rejuvenate_reference as rr

# ---- the target of the stationarity tests (here and on the GPU) ----------------------------------------------------------
# a 2-d Gaussian inside the box with correlation 0.8 and sd a tenth of the box; 1 site x 64 members, 600 full sweeps, the
# first 100 dropped
BOX_LO, BOX_HI = np.array([2.0, 10.0]), np.array([22.0, 50.0])
T_MEAN = 0.5 * (BOX_LO + BOX_HI)
T_SD = 0.1 * (BOX_HI - BOX_LO)
T_RHO = 0.8
MEMBERS, SWEEPS, BURN = 64, 600, 100
JITTER = 1e-3
# The worst deviations over seeds 1..20 of the pooled sample (500 sweeps x 64 members) from the target: the two means in
# target sds, the two variances and the covariance relative to the target's.  Produced by
#     python -m tests.test_mcmc_move
# and asserted by test_stationarity_of_the_reference_sampler (the reference is deterministic).  The GPU test's bound is
# 2 x these: it is one more draw from the same distribution of deviations, and the worst of 20 itself would fail about one
# run in 20.
WORST_MEAN_SDS = 0.0338
WORST_VAR_REL = 0.0724
WORST_COV_REL = 0.0804       # (acceptance 0.357 .. 0.366)


def target_logdens(x):
    z = (np.asarray(x, dtype=np.float64) - T_MEAN) / T_SD
    return -0.5 * (z[:, 0] ** 2 - 2 * T_RHO * z[:, 0] * z[:, 1] + z[:, 1] ** 2) / (1 - T_RHO ** 2)


def start_points(seed):
    """over-dispersed inside the box: uniform on its middle half"""
    rng = np.random.default_rng(1000 + seed)
    return BOX_LO + (0.25 + 0.5 * rng.random((MEMBERS, 2))) * (BOX_HI - BOX_LO)


def deviations(samples):
    """pooled samples [n][2] -> (worst mean deviation in target sds, worst relative variance deviation, relative covariance
    deviation)"""
    x = np.asarray(samples).reshape(-1, 2)
    mean = np.abs(x.mean(0) - T_MEAN) / T_SD
    cov = np.cov(x.T)
    var = np.abs(np.diag(cov) / T_SD ** 2 - 1)
    c = abs(cov[0, 1] / (T_RHO * T_SD[0] * T_SD[1]) - 1)
    return float(mean.max()), float(var.max()), float(c)


def reference_deviations(seeds=range(1, 21)):
    worst = np.zeros(3)
    rates = []
    for seed in seeds:
        out, rate = mr.chain(target_logdens, start_points(seed), BOX_LO, BOX_HI, mr.demc_gamma(2), JITTER, SWEEPS, seed)
        worst = np.maximum(worst, deviations(out[BURN:]))
        rates.append(rate)
    return worst, rates


def test_host_draws_equal_the_reference():
    rng = np.random.default_rng(5)
    n = 10000
    member = rng.integers(0, 2 ** 22, size=n)
    draw = rng.integers(0, 2 ** 32, size=n)
    stream = rng.integers(0, 2 ** 32, size=n)
    n_other = np.array([2, 3, 64, 255, 2 ** 20])[np.arange(n) % 5]
    seed = 0x1234567890abcdef
    for i in range(n):
        i1, i2, u = sa.mcmc_draws(seed, draw[i], stream[i], member[i], n_other[i])
        w1, w2, wu = mr.draws(seed, draw[i], stream[i], member[i], n_other[i])
        assert (i1, i2) == (int(w1), int(w2)) and u == float(wu), i
        assert i1 != i2 and 0 <= i1 < n_other[i] and 0 <= i2 < n_other[i] and 0.0 < u < 1.0
    # the seed's halves are the key, the counter is {member, stream, 8, draw}
    x = sa.philox4x32_10([5, 6, 8, 7], [0x89abcdef, 0x01234567])
    i1, i2, u = sa.mcmc_draws(0x0123456789abcdef, 7, 6, 5, 1000)
    assert i1 == (int(x[0]) * 1000) >> 32 and u == (float(x[2]) + 0.5) * 2.0 ** -32
    raw = (int(x[1]) * 999) >> 32
    assert i2 == raw + (raw >= i1)


def test_each_rank_is_uniform_over_three_partners():
    n = 10000
    member = np.arange(n)
    i1, i2, _ = mr.draws(77, 3, 9, member, 3)
    for i in (0, 1234, 9999):
        assert sa.mcmc_draws(77, 3, 9, i, 3)[:2] == (int(i1[i]), int(i2[i]))
    sd = np.sqrt(n * (1 / 3) * (2 / 3))
    for idx in (i1, i2):
        hist = np.bincount(idx, minlength=3)
        assert hist.sum() == n and (np.abs(hist - n / 3) <= 5 * sd).all(), hist
    assert (i1 != i2).all()
    with pytest.raises(sa.SipnetError):
        sa.mcmc_draws(1, 0, 0, 0, 1)


def test_constants_and_gamma():
    text = open(os.path.join(helpers.REPO, "include", "sipnet_amd.h")).read()
    assert int(re.search(r"#define SIPNET_MCMC_INFO_WORDS (\d+)", text).group(1)) == sa.MCMC_INFO_WORDS == mr.INFO_WORDS == 4
    codes = dict(re.findall(r"SIPNET_MCMC_(DONE|TOO_FEW|BAD_INPUT|NOT_SELECTED) = (-?\d+)", text))
    assert {k: int(v) for k, v in codes.items()} == {"DONE": sa.MCMC_DONE, "TOO_FEW": sa.MCMC_TOO_FEW,
                                                     "BAD_INPUT": sa.MCMC_BAD_INPUT, "NOT_SELECTED": sa.MCMC_NOT_SELECTED}
    assert (mr.DONE, mr.TOO_FEW, mr.BAD_INPUT, mr.NOT_SELECTED) == (1, 0, -2, -3) == (
        sa.MCMC_DONE, sa.MCMC_TOO_FEW, sa.MCMC_BAD_INPUT, sa.MCMC_NOT_SELECTED)
    for n in (1, 2, 16):
        assert sa.demc_gamma(n) == 2.38 / np.sqrt(2.0 * n) == mr.demc_gamma(n)
    # blocks 0..7 are the rejuvenation's, 8 the move's ranks and uniform, 12..15 the jitter's normals
    assert mr.BLOCK == 8 and {mr.JITTER_BLOCK + (k >> 2) for k in range(16)} == {12, 13, 14, 15}


def test_refusals_that_need_no_device():
    """the parameter, half and array checks answer before the batch is looked at"""
    L = sa.lib()
    BAD = _lib.ERR_BAD_ARGUMENT
    a, q = pi("aMax"), pi("vegRespQ10")
    one = C.c_double(0.9)        # (never dereferenced: every call is refused before a device is touched)
    P = C.addressof(one)

    def propose(params, n_params=None, half=0, gamma=True, saved=True, moved=True):
        prm = (_lib.EnkfParam * max(len(params), 1))(*[_lib.EnkfParam(int(i), 0, float(lo), float(hi)) for i, lo, hi in params])
        return L.sipnet_batch_mcmc_propose(None, len(params) if n_params is None else n_params, prm if params else None,
                                           P if gamma else None, None, half, 1, 0, None, None, P if saved else None,
                                           P if moved else None, None, None)

    def accept(params, n_params=None, saved=True, moved=True, new=True, cur=True):
        prm = (_lib.EnkfParam * max(len(params), 1))(*[_lib.EnkfParam(int(i), 0, float(lo), float(hi)) for i, lo, hi in params])
        return L.sipnet_batch_mcmc_accept(None, len(params) if n_params is None else n_params, prm if params else None,
                                          P if saved else None, P if moved else None, P if new else None, P if cur else None,
                                          None, 1, 0, None, None, None)

    def why():
        return L.sipnet_last_error()

    good = [(a, 1.0, 20.0)]
    for call, name in ((propose, b"sipnet_batch_mcmc_propose"), (accept, b"sipnet_batch_mcmc_accept")):
        assert call(good, n_params=0) == BAD and name in why() and b"1..16" in why()
        assert call(good, n_params=17) == BAD and name in why() and b"1..16" in why()
        assert call(good, n_params=-1) == BAD
        assert call([], n_params=1) == BAD and b"NULL params" in why()
        assert call([(a, 1.0, 20.0), (q, 1.0, 3.0), (a, 1.0, 20.0)]) == BAD and b"twice" in why()
        for row, word in [(rr.PSN_TMAX, b"derived"), (rr.COARSE_ALLOC, b"derived"), (pi("plantWoodInit"), b"initial condition"),
                          (pi("leafOnDay"), b"phenology"), (pi("fAnoxia"), b"clamps")]:
            assert call(good + [(row, 0.0, 1.0)]) == BAD and word in why() and name in why()
        assert call([(80, 0.0, 1.0)]) == BAD and call([(-1, 0.0, 1.0)]) == BAD
        assert call([(a, np.nan, 20.0)]) == BAD and call([(a, 1.0, np.inf)]) == BAD and call([(a, 20.0, 20.0)]) == BAD
        assert call(good, saved=False) == BAD and b"NULL d_saved" in why()
        assert call(good, moved=False) == BAD and b"NULL d_moved" in why()
        # well-formed arguments get as far as the batch
        assert call(good) == BAD and b"NULL batch" in why() and name in why()
        # two things wrong at once: the earlier check answers -- n_params, the listed rows, (the half,) a NULL array, the batch
        assert call([(a, 20.0, 20.0)], n_params=0, saved=False) == BAD and b"1..16" in why()
        assert call(good + [(a, 1.0, 20.0)], saved=False) == BAD and b"twice" in why()
        assert call(good, saved=False, moved=False) == BAD and b"NULL d_saved" in why()
    assert propose(good + [(a, 1.0, 20.0)], half=2) == BAD and b"twice" in why()
    assert propose(good, half=2, gamma=False) == BAD and b"half" in why()
    assert propose(good, gamma=False, saved=False) == BAD and b"NULL d_gamma" in why()
    assert accept(good, moved=False, new=False) == BAD and b"NULL d_moved" in why()
    assert accept(good, new=False, cur=False) == BAD and b"NULL d_logp_new" in why()
    assert propose(good, half=2) == BAD and b"half" in why()
    assert propose(good, half=-1) == BAD and b"half" in why()
    assert propose(good, gamma=False) == BAD and b"NULL d_gamma" in why()
    assert accept(good, new=False) == BAD and b"NULL d_logp_new" in why()
    assert accept(good, cur=False) == BAD and b"NULL d_logp_cur" in why()


def hand_made(n_sites=4, M=10, seed=3):
    rng = np.random.default_rng(seed)
    state = np.zeros((n_sites * M, 32))
    prm = np.zeros((n_sites * M, 80))
    prm[:, 4] = 8.0 + 4.0 * rng.random(n_sites * M)
    prm[:, rr.PSN_TOPT] = 20.0 + 5.0 * rng.random(n_sites * M)
    prm[:, rr.PSN_TMIN] = 1.0 + rng.random(n_sites * M)
    prm[:, rr.PSN_TMAX] = prm[:, rr.PSN_TOPT] + (prm[:, rr.PSN_TOPT] - prm[:, rr.PSN_TMIN])
    return state, prm


def test_the_reference_rules_on_a_hand_made_batch():
    n_sites, M = 4, 10
    state, prm = hand_made(n_sites, M)
    state[M + 1, 29] = 3.0                                   # site 1: an odd member dead
    state[2 * M + 3:3 * M:2, 29] = 3.0                       # site 2: one odd member left
    params = [(4, 0.0, 11.0), (rr.PSN_TOPT, 5.0, 40.0)]      # (aMax's upper bound cuts the ensemble: some proposals leave)
    total = np.array([5, 5, 5, -3])
    out, saved, moved, info, tol, margin = mr.propose(state, prm, np.zeros(n_sites), n_sites, params, [0.8] * 4, None, 0, 9, 1,
                                                      site_total=total)
    assert [list(r) for r in info[1:]] == [[1, info[1, 1], 5, 4], [0, 0, 5, 1], [-3, 0, 5, 5]]
    assert info[0, 0] == 1 and info[0, 2:].tolist() == [5, 5] and 0 < info[:2, 1].sum() < 10
    assert moved[1::2].sum() == 0 and moved[2 * M:].sum() == 0          # the other half, the sites whose code is not 1
    made = moved == 1
    assert moved.sum() == info[:2, 1].sum()
    np.testing.assert_array_equal(out[~made], prm[~made])
    assert (out[made][:, [4, rr.PSN_TOPT]] != prm[made][:, [4, rr.PSN_TOPT]]).all()
    assert (out[made, 4] <= 11.0).all() and (out[made, 4] >= 0.0).all()
    np.testing.assert_array_equal(saved[0, made], prm[made, 4])
    assert np.isnan(saved[:, ~made]).all()
    np.testing.assert_array_equal(out[made, rr.PSN_TMAX], out[made, rr.PSN_TOPT] + (out[made, rr.PSN_TOPT] - out[made, rr.PSN_TMIN]))
    rest = [k for k in range(80) if k not in (4, rr.PSN_TOPT, rr.PSN_TMAX)]
    np.testing.assert_array_equal(out[:, rest], prm[:, rest])
    # the partners come from the other half: every new aMax is x_j + 0.8 (x_r1 - x_r2) for odd r1 != r2 of its site
    for col in np.flatnonzero(made):
        s, jm = divmod(col, M)
        B = [k for k in range(1, M, 2) if state[s * M + k, 29] == 0]
        i1, i2, _ = mr.draws(9, 1, s, jm, len(B))
        want = prm[col, 4] + 0.8 * (prm[s * M + B[int(i1)], 4] - prm[s * M + B[int(i2)], 4])
        assert abs(out[col, 4] - want) <= tol[col, 4] and tol[col, 4] > 0
    # gamma and jitter that are bad input
    for gamma, jitter in (([0.8, np.nan, 0.8, 0.8], None), ([0.8] * 4, [0.0, -1.0, 0.0, 0.0]), ([0.8, np.inf, 0.8, 0.8], [0.0] * 4)):
        bad = mr.propose(state, prm, np.zeros(n_sites), n_sites, params, gamma, jitter, 0, 9, 1)[3]
        assert bad[:, 0].tolist() == [1, -2, 0, 1]
    # accept: hand-made log-posteriors
    new = np.zeros(n_sites * M)
    cur = np.zeros(n_sites * M)
    cols = np.flatnonzero(made)
    cases = [(-np.inf, -np.inf, False), (np.inf, 0.0, False), (np.nan, 0.0, False), (0.0, np.nan, False), (1.0, -np.inf, True),
             (2.0, 2.0, True), (-np.inf, 0.0, False), (5.0, 1.0, True)]
    for col, (n_, c_, _) in zip(cols, cases):
        new[col], cur[col] = n_, c_
    back, moved2, cur2, info2, margin2, acc = mr.accept(state, out, np.zeros(n_sites), n_sites, params, saved, moved, new, cur,
                                                       None, 9, 1)
    for col, (n_, c_, want) in zip(cols, cases):
        assert acc[col] == want, (col, n_, c_)
    assert moved2.sum() == 0 and info2[:, 0].tolist() == [1, 1, 1, 1] and info2[:, 1].sum() == made.sum()
    assert info2[:, 3].tolist() == [10, 9, 6, 10] and info2[:, 2].sum() == acc.sum()
    np.testing.assert_array_equal(back[~acc].view(np.uint64), prm[~acc].view(np.uint64))      # all 80 rows, psnTMax too
    np.testing.assert_array_equal(back[acc], out[acc])
    np.testing.assert_array_equal(cur2[acc], new[acc])
    keep = ~acc
    np.testing.assert_array_equal(cur2[keep].view(np.uint64), cur[keep].view(np.uint64))
    # a second accept is a no-op; a bad beta leaves the site and its moved flags
    again = mr.accept(state, back, np.zeros(n_sites), n_sites, params, saved, moved2, new, cur2, None, 9, 1)
    np.testing.assert_array_equal(again[0], back)
    assert again[3][:, 1].sum() == 0
    bad = mr.accept(state, out, np.zeros(n_sites), n_sites, params, saved, moved, new, cur, [1.0, 0.0, 1.0, np.inf], 9, 1)
    assert bad[3][:, 0].tolist() == [1, -2, 1, -2] and bad[1][M:2 * M].sum() == moved[M:2 * M].sum()
    np.testing.assert_array_equal(bad[0][M:2 * M], out[M:2 * M])


def test_stationarity_of_the_reference_sampler():
    worst, rates = reference_deviations()
    print(f"reference sampler, 20 seeds: worst mean {worst[0]:.4f} target sds, variance {worst[1]:.4f}, covariance {worst[2]:.4f} "
          f"(relative); acceptance {min(rates):.3f} .. {max(rates):.3f}")
    assert abs(worst[0] - WORST_MEAN_SDS) < 5e-5 and abs(worst[1] - WORST_VAR_REL) < 5e-5 and abs(worst[2] - WORST_COV_REL) < 5e-5
    # what the sampler must do whatever the constants are: the sample is the target's to Monte-Carlo error.  500 x 64 draws
    # with an integrated autocorrelation time of some tens of sweeps leave about a thousand independent ones: 0.2 sd and 25 %
    assert worst[0] < 0.2 and worst[1] < 0.25 and worst[2] < 0.25
    assert 0.05 < min(rates) and max(rates) < 0.95


if __name__ == "__main__":
    w, r = reference_deviations()
    print(f"WORST_MEAN_SDS = {w[0]:.4f}\nWORST_VAR_REL = {w[1]:.4f}\nWORST_COV_REL = {w[2]:.4f}")
    print(f"# acceptance {min(r):.3f} .. {max(r):.3f}")
