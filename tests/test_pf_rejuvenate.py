"""Particle rejuvenation without a GPU: the library's host Philox4x32-10 and Box-Muller normals against known answers and the
numpy reference (tests/pf_rejuvenate_reference.py), the block and lane a listed parameter and a state slot take, the shrink
factor, the constants the binding mirrors, the refusals that need no device, and the reference's own moment preservation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib
from sipnet_amd.config import param_index as pi
from tests import helpers
from tests import pf_rejuvenate_reference as rr

KNOWN = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert " ".join("%08x" % x for x in sa.philox4x32_10(ctr, key)) == want
        assert " ".join("%08x" % x for x in rr.philox4x32_10(ctr, key)) == want


def test_philox_equals_the_numpy_philox_on_random_counters_and_keys():
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, size=(10000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(10000, 2), dtype=np.uint64)
    want = rr.philox4x32_10(ctr, key)
    got = np.stack([sa.philox4x32_10(ctr[i], key[i]) for i in range(len(ctr))])
    np.testing.assert_array_equal(got.astype(np.uint64), want)


def test_host_normals_against_the_longdouble_normals():
    rng = np.random.default_rng(12)
    n = 4000
    seed = [int(x) for x in rng.integers(0, 2 ** 63, size=n)]
    draw, stream, member = (rng.integers(0, 2 ** 32, size=n, dtype=np.uint64) for _ in range(3))
    block = rng.integers(0, 8, size=n, dtype=np.uint64)
    worst = 0.0
    for i in range(n):
        got = sa.rejuvenate_normals(seed[i], draw[i], stream[i], member[i], block[i])
        want, r = rr.normals(seed[i], draw[i], stream[i], member[i], block[i])
        assert (np.abs(got) <= rr.Z_MAX).all()
        ratio = float((np.abs(got.astype(np.longdouble) - want) / (2.0 ** -53 * r)).max())
        worst = max(worst, ratio)
    print(f"host normals: worst |z - z_longdouble| / (2^-53 r) = {worst:.3f} (bound 8)")
    assert worst <= 8.0
    # the seed's halves are the key, the counter is {member, stream, block, draw}
    x = sa.philox4x32_10([5, 6, 7, 8], [0x89abcdef, 0x01234567])
    u, v = (float(x[0]) + 0.5) * 2.0 ** -32, (float(x[1]) + 0.5) * 2.0 ** -32
    z = sa.rejuvenate_normals(0x0123456789abcdef, 8, 6, 5, 7)
    assert abs(z[0] - np.sqrt(-2 * np.log(u)) * np.cos(2 * np.pi * v)) < 1e-14
    assert abs(z[1] - np.sqrt(-2 * np.log(u)) * np.sin(2 * np.pi * v)) < 1e-14


def test_block_and_lane_of_parameters_and_slots():
    seed, draw, stream, member = 99, 4, 17, 300
    for k in range(16):
        z, _ = rr.param_normal(seed, draw, stream, member, k)
        assert float(z) == pytest.approx(sa.rejuvenate_normals(seed, draw, stream, member, k >> 2)[k & 3], abs=1e-14)
    for p in range(13):
        z, _ = rr.pool_normal(seed, draw, stream, member, p)
        assert float(z) == pytest.approx(sa.rejuvenate_normals(seed, draw, stream, member, 4 + (p >> 2))[p & 3], abs=1e-14)
    blocks = {k >> 2 for k in range(16)} | {4 + (p >> 2) for p in range(13)}
    assert blocks == set(range(8))          # parameters 0..3, slots 4..7: no block serves both


def test_liu_west_shrink():
    for delta in (0.95, 0.98, 0.99, 1.0, 0.5):
        assert sa.liu_west_shrink(delta) == (3 * delta - 1) / (2 * delta) == rr.liu_west_shrink(delta)
    assert sa.liu_west_shrink(1.0) == 1.0
    a = sa.liu_west_shrink(0.98)
    assert 0 < a < 1 and abs((1 - a * a) - (1 - ((3 * 0.98 - 1) / (2 * 0.98)) ** 2)) < 1e-15


def test_constants_mirror_the_header():
    text = open(os.path.join(helpers.REPO, "include", "sipnet_amd.h")).read()
    assert int(re.search(r"#define SIPNET_REJUVENATE_INFO_WORDS (\d+)", text).group(1)) == sa.REJUVENATE_INFO_WORDS == rr.INFO_WORDS == 4
    codes = dict(re.findall(r"SIPNET_REJUVENATE_(DONE|TOO_FEW|BAD_INPUT|NOT_SELECTED) = (-?\d+)", text))
    assert {k: int(v) for k, v in codes.items()} == {"DONE": sa.REJUVENATE_DONE, "TOO_FEW": sa.REJUVENATE_TOO_FEW,
                                                     "BAD_INPUT": sa.REJUVENATE_BAD_INPUT, "NOT_SELECTED": sa.REJUVENATE_NOT_SELECTED}
    assert (rr.DONE, rr.TOO_FEW, rr.BAD_INPUT, rr.NOT_SELECTED) == (1, 0, -2, -3) == (
        sa.REJUVENATE_DONE, sa.REJUVENATE_TOO_FEW, sa.REJUVENATE_BAD_INPUT, sa.REJUVENATE_NOT_SELECTED)
    assert sa.ENKF_MAX_PARAMS == 16


def test_refusals_that_need_no_device():
    """the parameter, shrink and mask checks answer before the batch is looked at"""
    L = sa.lib()
    BAD = _lib.ERR_BAD_ARGUMENT
    a, q = pi("aMax"), pi("vegRespQ10")
    one = C.c_double(0.9)        # (never dereferenced: every call is refused before a device is touched)
    sd = (C.c_double * 13)()

    def call(params, n_params=None, shrink=True, mask=0, pool_sd=False):
        prm = (_lib.EnkfParam * max(len(params), 1))(*[_lib.EnkfParam(int(i), 0, float(lo), float(hi)) for i, lo, hi in params])
        return L.sipnet_batch_pf_rejuvenate(None, len(params) if n_params is None else n_params, prm if params else None,
                                            C.addressof(one) if shrink else None, mask, C.addressof(sd) if pool_sd else None,
                                            1, 0, None, None, None, None)

    def why():
        return L.sipnet_last_error()

    assert call([(a, 1.0, 20.0)], n_params=17) == BAD and b"sipnet_batch_pf_rejuvenate" in why() and b"0..16" in why()
    assert call([(a, 1.0, 20.0)], n_params=-1) == BAD
    assert call([], n_params=1) == BAD and b"NULL params" in why()
    assert call([(a, 1.0, 20.0), (q, 1.0, 3.0), (a, 1.0, 20.0)]) == BAD and b"twice" in why()
    for row, word in [(rr.PSN_TMAX, b"derived"), (rr.COARSE_ALLOC, b"derived"), (pi("plantWoodInit"), b"initial condition"),
                      (pi("leafOnDay"), b"phenology"), (pi("fAnoxia"), b"clamps")]:
        assert call([(a, 1.0, 20.0), (row, 0.0, 1.0)]) == BAD and word in why() and b"sipnet_batch_pf_rejuvenate" in why()
    assert call([(80, 0.0, 1.0)]) == BAD and call([(-1, 0.0, 1.0)]) == BAD
    assert call([(a, np.nan, 20.0)]) == BAD and call([(a, 1.0, np.inf)]) == BAD and call([(a, 20.0, 20.0)]) == BAD
    assert call([(a, 1.0, 20.0)], shrink=False) == BAD and b"d_shrink" in why()
    assert call([(a, 1.0, 20.0)], mask=1 << 13, pool_sd=True) == BAD and b"pools 0..12" in why()
    assert call([(a, 1.0, 20.0)], mask=-1, pool_sd=True) == BAD and b"pools 0..12" in why()
    assert call([], mask=0x10FF) == BAD and b"d_pool_sd" in why()
    assert call([]) == BAD and b"nothing to do" in why()
    # well-formed arguments get as far as the batch
    assert call([(a, 1.0, 20.0)], mask=0x10FF, pool_sd=True) == BAD and b"NULL batch" in why()
    assert call([], mask=1, pool_sd=True, shrink=False) == BAD and b"NULL batch" in why()
    # two things wrong at once: the earlier check answers -- the listed rows, d_shrink, the mask, d_pool_sd, nothing to do
    assert call([(a, 20.0, 20.0)], shrink=False) == BAD and b"d_shrink" not in why() and b"NULL batch" not in why()
    assert call([(a, 1.0, 20.0), (a, 1.0, 20.0)], mask=1 << 13) == BAD and b"twice" in why()
    assert call([(a, 1.0, 20.0)], shrink=False, mask=1 << 13) == BAD and b"d_shrink" in why()
    assert call([(a, 1.0, 20.0)], mask=(1 << 13) | 1) == BAD and b"pools 0..12" in why()
    assert call([], mask=1) == BAD and b"d_pool_sd" in why()


@pytest.mark.parametrize("n", [4096, 65536])
def test_the_reference_move_preserves_mean_and_variance(n):
    """Liu & West's point: x' = m + a (x - m) + h sd z has mean m and variance a^2 sd^2 + h^2 sd^2 = sd^2.  Given x, the
    mean of x' is m + h sd zbar and zbar has standard error 1 / sqrt(n); the sample variance of n draws has relative standard
    error sqrt(2 / (n - 1)).  Six of each."""
    rng = np.random.default_rng(n)
    x = (10.0 + 2.0 * rng.standard_normal(n)).astype(np.longdouble)
    member = np.arange(n)
    worst_mean = worst_var = 0.0
    for a in (0.5, 0.9, 0.995):
        for seed in (1, 2026):
            for draw in range(4):
                z, _ = rr.param_normal(seed, draw, 0, member, 0)
                v, m, sd, h = rr.move(x, a, z)
                mean_units = float(abs(v.mean() - m) / (h * sd / np.sqrt(np.longdouble(n))))
                var_units = float(abs(v.var(ddof=1) / sd ** 2 - 1) / np.sqrt(2.0 / (n - 1)))
                worst_mean, worst_var = max(worst_mean, mean_units), max(worst_var, var_units)
                assert mean_units <= 6.0, (a, seed, draw, mean_units)
                assert var_units <= 6.0, (a, seed, draw, var_units)
    print(f"n = {n}: worst mean {worst_mean:.2f} standard errors, worst variance {worst_var:.2f} (bound 6)")


def test_the_reference_limits_and_codes():
    """reflection once, then the clip; a == 1 and q == 0 leave the bits; the codes"""
    lo, hi = np.longdouble(1.0), np.longdouble(2.0)
    v = rr.reflect_clip(np.array([0.75, 2.5, 1.5, -5.0, 9.0], dtype=np.longdouble), lo, hi)
    np.testing.assert_array_equal(v.astype(float), [1.25, 1.5, 1.5, 2.0, 1.0])
    n_sites, M = 5, 8
    rng = np.random.default_rng(3)
    state = np.zeros((n_sites * M, 32))
    state[:, :13] = 5.0 + rng.random((n_sites * M, 13))
    state[M + 1:2 * M, 29] = 3.0                          # site 1: one live member
    prm = 1.0 + rng.random((n_sites * M, 80))
    shrink = [0.9, 0.9, np.nan, 0.9, 1.0]
    total = np.array([5, 5, 5, -3, 5])
    sd = np.zeros((n_sites, 13))
    sd[:, 2] = 0.1
    out_state, out_prm, info, _, _, _ = rr.rejuvenate(state, prm, np.zeros(n_sites), n_sites, [(4, 0.0, 34.0)], shrink, 0b101, sd, 7, 0,
                                                      site_total=total)
    assert [list(r) for r in info] == [[1, 2, M, 0], [0, 0, 1, 0], [-2, 0, M, 0], [-3, 0, M, 0], [1, 1, M, 0]]
    for s in (1, 2, 3):
        np.testing.assert_array_equal(out_state[s * M:(s + 1) * M], state[s * M:(s + 1) * M])
        np.testing.assert_array_equal(out_prm[s * M:(s + 1) * M], prm[s * M:(s + 1) * M])
    np.testing.assert_array_equal(out_prm[4 * M:], prm[4 * M:])             # a == 1: the rows' bits
    np.testing.assert_array_equal(out_state[:, 0], state[:, 0])             # q == 0: the slot's bits
    assert (out_state[:M, 2] != state[:M, 2]).all() and (out_prm[:M, 4] != prm[:M, 4]).all()
    rest = [k for k in range(80) if k != 4]
    np.testing.assert_array_equal(out_prm[:, rest], prm[:, rest])
