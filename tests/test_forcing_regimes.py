"""The forcing regimes of tests/forcing_regimes.py, without a GPU: that each regime HAS the properties it is there for
(read from its ClimTable and from the oracle's records -- a regime that silently degenerates into the temperate
climate fails here), that the file regimes survive write_clim / read_clim bit for bit, that the oracle runs the GPU
tests' member set on them (status 0, finite planes), and the conditioning yardstick: the reference alone, on these
inputs, does not amplify a one-ulp move or an fp32 rounding of the forcing.  That yardstick is what lets
tests/test_gpu_forcing_regimes.py hold the kernels to the fuzzer's bounds here; if a regime fails it, the regime is
changed, not the bound.

One property is read with the model's own floor: soilWaterFluxes leaves TINY = 1e-6 cm when evaporation empties the
soil (sipnet.c:963-1031), and nothing below it is ever clamped to 0 while the snow pack is empty, so "the soil water
reaches 0" is asserted as "reaches that floor"."""
import os

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from sipnet_amd.io import ClimTable
from tests import forcing_regimes as fr
from tests import helpers

BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
FLAGS = sa.flags_from()
ALL = list(fr.FILE_REGIMES) + ["tiny"]
TINY = 0.000001
SNOW, WATER = 19, 17          # record columns (include/sipnet_amd.h)


@pytest.fixture(scope="module")
def members():
    return fr.hard_members(sa.read_params(BASE, FLAGS)[0])


@pytest.fixture(scope="module")
def runs(oracle, members):
    """name -> (clim, planes, final, status) of the oracle, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = fr.clim(name)
            cache[name] = (c,) + tuple(oracle.run_block(FLAGS, members, c))
        return cache[name]
    return get


def longest_run(mask):
    """length of the longest run of True"""
    m = np.concatenate([[False], np.asarray(mask, dtype=bool), [False]])
    edges = np.flatnonzero(m[1:] != m[:-1])
    return int((edges[1::2] - edges[::2]).max()) if len(edges) else 0


def test_member_set_is_two_chunks_a_ragged_third_and_the_hard_members(members):
    base = sa.read_params(BASE, FLAGS)[0]
    assert members.shape == (133, 80)
    assert np.array_equal(members[:130][:, [k for k in range(80) if k != pi("frozenSoilThreshold")]],
                          synth.perturbed_params(base, 130, scale=3.0)[:, [k for k in range(80) if k != pi("frozenSoilThreshold")]])
    assert members[130, pi("plantWoodInit")] == base[pi("plantWoodInit")] * 0.001
    assert members[131, pi("soilWFracInit")] == 0.02 and members[132, pi("leafTurnoverRate")] == 0.9
    thr = members[:, pi("frozenSoilThreshold")]
    assert ((thr == np.round(thr)) & (thr >= 0)).sum() >= 6          # whole degrees `threshold`'s soil sits on


def test_polar(oracle, members):
    c = fr.clim("polar")
    d = c.data
    assert c.n_steps == 17520 and np.all(d[:, 0] == 1 / 48)
    assert d[:60 * 48, 1].max() <= 0 and d[:, 1].min() <= -40
    assert d[:, 2].min() <= -25 and np.all(d[1:, 2] != d[:-1, 2])           # FAST_TSOIL_SAME never set
    par = d[:, 3].reshape(-1, 48)
    dark, lit = (par == 0).all(axis=1), (par > 0).all(axis=1)
    assert dark[:60].all() and longest_run(dark) >= 60                      # whole 16-step tiles without light
    first_lit = int(np.argmax(~dark))
    assert longest_run(lit[first_lit:]) >= 20
    st, rec, _ = oracle.run_member(FLAGS, members[0], c)
    assert st == 0
    peak = int(rec[:, SNOW].argmax())
    assert rec[peak, SNOW] > 10.0                                            # cm water equivalent
    assert peak < 200 * 48 and (rec[peak:, SNOW] == 0.0).any()               # the summer melts all of it
    assert d[:, 1].max() > 10                                                # ... and is a summer


def test_arid(oracle, members):
    raw, c = fr.raw("arid"), fr.clim("arid")
    d = c.data
    assert d[:, 1].max() >= 45 and d[:, 5].max() >= 8.0                      # deg C, kPa
    assert longest_run(raw["precip"] == 0) >= 200 * 48
    bursts = raw["precip"][raw["precip"] > 0]
    assert 3 <= len(bursts) <= 10 and bursts.min() >= 100.0                  # mm in single steps
    calm = (raw["wspd"] == 0).mean()
    assert 0.07 < calm < 0.13 and np.all(d[raw["wspd"] == 0, 8] == TINY)
    dry = 0
    for m in range(members.shape[0]):
        st, rec, _ = oracle.run_member(FLAGS, members[m], c)
        assert st == 0
        dry += bool(rec[:, WATER].min() <= TINY * (1 + 1e-9))
    assert dry >= members.shape[0] / 4, dry
    # water-limited photosynthesis: the same members on a soil that never runs short assimilate more
    wet = members.copy()
    wet[:, pi("soilWHC")] = 36.0
    wet[:, pi("soilWFracInit")] = 1.0
    gpp = oracle.run_block(FLAGS, members, c)[0][1]
    gpp_wet = oracle.run_block(FLAGS, wet, c)[0][1]
    limited = (gpp_wet - gpp > 1e-6 * gpp.max()).sum(axis=0)
    assert (limited > 100).sum() >= members.shape[0] / 4, limited
    assert (gpp > 0).mean() > 0.1                                            # not a dead landscape either


def test_threshold(members):
    raw, c = fr.raw("threshold"), fr.clim("threshold")
    d = c.data
    for col in (1, 2):
        v = d[:, col]
        assert np.all(v == np.round(v))
        assert (v == 0).sum() >= 100
        assert ((v == 0) & np.signbit(v)).sum() >= 10 and ((v == 0) & ~np.signbit(v)).sum() >= 10
    assert d[:, 1].min() < -5 and d[:, 1].max() > 5                          # both sides of every zero
    assert np.all(d[:480, 2] == d[0, 2]) and np.all(d[480:, 2] != d[479:-1, 2])
    thr = members[:, pi("frozenSoilThreshold")]
    whole = np.unique(thr[thr == np.round(thr)])
    assert len(whole) >= 3
    for v in whole:
        assert longest_run(d[:, 2] == v) >= 1 and (d[:, 2] == v).sum() >= 480, v
    assert longest_run(d[:, 2] == 1.0) >= 480                                # a ten-day stretch ON a threshold
    p = raw["par"]
    assert set(np.unique(p[p < 0.00015])) == {0.0, 0.0001}
    flips = ((p[1:] == 0.0001) & (p[:-1] == 0.0)).sum() + ((p[1:] == 0.0) & (p[:-1] == 0.0001)).sum()
    assert flips >= 2000
    assert (p > 0.1).any()                                                   # and daylight besides
    zero_vpd = raw["vpd"] == 0
    assert 0.05 < zero_vpd.mean() < 0.15 and np.all(d[zero_vpd, 5] == TINY)


def test_lengths():
    want = {"lengths_12h": {0.5}, "lengths_alternating": {0.6, 0.4}, "lengths_3h": {0.125}, "lengths_switching": {1 / 48, 0.5}}
    for name, lens in want.items():
        c = fr.clim(name)
        assert set(np.unique(c.data[:, 0])) == lens, name
        assert abs(c.data[:, 0].sum() - 365.0) < 1e-9                        # a year long
        t = c.day + c.data[:, 10] / 24.0
        assert np.all(np.diff(t) > 0) and c.day[0] == 1 and c.day[-1] == 365
    alt = fr.clim("lengths_alternating").data[:, 0]
    assert np.all(alt[0::2] == 0.6) and np.all(alt[1::2] == 0.4)
    sw = fr.clim("lengths_switching").data[:, 0]
    a, b = fr.SWITCH_STEPS
    assert a % 16 != 0 and b % 16 != 0 and a // 16 != b // 16
    assert np.all(sw[:a] == 1 / 48) and np.all(sw[a:b] == 0.5) and np.all(sw[b:] == 1 / 48)
    assert a >= 40 * 48 and b - a == 120 and len(sw) - b > 16 * 100


def test_tiny():
    c, t = fr.clim("threshold"), fr.clim("tiny")
    assert t.n_steps == c.n_steps
    for col in (1, 2, 3):
        v = t.data[:, col]
        small = (v != 0) & (np.abs(v) < 1e-200)
        assert np.all(c.data[small, col] == 0) and np.array_equal(v[~small], c.data[~small, col])
        for x in fr.TINY_VALUES:
            assert (v == x).sum() >= 10, (col, x)
        assert np.all(v[small].astype(np.float32) == 0)                      # zero once narrowed
        assert (v == 0).sum() >= 100                                         # and exact zeros are left
    assert np.array_equal(t.data[:, 9], np.maximum(t.data[:, 1] * t.data[:, 0], 0.0))
    assert np.array_equal(np.delete(t.data, [1, 2, 3, 9], axis=1), np.delete(c.data, [1, 2, 3, 9], axis=1))


def test_tiny_vpd_reaches_a_potential_transpiration_below_the_reciprocals_range(oracle):
    """the divisor of moisture()'s removable / potTrans: with a VPD of 1e-307 in the first light it is positive and below 2^-1024
    for most members (the GPP plane of a member with water is potGrossPsn * length; potTrans = potGrossPsn * vpd / wueConst, and
    wueConst is above 1), and a member with no soil water divides 0 by it: the oracle's GPP is exactly 0 there, positive next door"""
    c = fr.tiny_vpd()
    m = fr.dry_members(sa.read_params(BASE, FLAGS)[0])
    assert c.n_steps == 144 and c.data[0, 3] > 0.1                            # starts by day
    v = c.data[:, 5]
    assert set(np.unique(v[np.arange(144) % 4 != 3])) == set(fr.VPD_TINY) and (v[3::4] >= TINY).all()
    assert (m[::2, pi("soilWFracInit")] == 0.0).all() and (m[1::2, pi("soilWFracInit")] > 0.0).sum() >= 55
    planes, final, st = oracle.run_block(FLAGS, m, c)
    ok = st == 0
    assert ok.sum() >= 125 and np.isfinite(planes[:, :, ok]).all()
    gpp0 = planes[1, 0, :]
    dry, wet = ok & (np.arange(133) % 2 == 0), ok & (np.arange(133) % 2 == 1)
    assert (m[:, pi("wueConst")] > 1.0).all()
    pot = gpp0[wet] / c.data[0, 0]                                           # potential photosynthesis of the members with water
    assert (gpp0[dry] == 0.0).all() and (pot >= 1e-6).sum() >= 40
    pot_trans = pot * c.data[0, 5] / m[wet, pi("wueConst")]
    assert ((pot >= 1e-6) & (pot_trans < 2.0 ** -1024)).sum() >= 30          # ... in the window, and their dry neighbours alike


@pytest.mark.parametrize("name", fr.FILE_REGIMES)
def test_file_round_trip_is_bit_for_bit(name, tmp_path):
    raw = fr.raw(name)
    path = tmp_path / (name + ".clim")
    synth.write_clim(str(path), raw)
    got, want = sa.read_clim(str(path)), synth.convert_raw(raw)
    assert np.array_equal(got.year, want.year) and np.array_equal(got.day, want.day)
    # bytes: the sign of -0.0 too.  The derived growing-degree-day column by value: max(-0.0 * length, 0) keeps the
    # zero's sign in numpy and drops it in the reader, and a sum of degree days does not see it
    assert np.delete(got.data, 9, axis=1).tobytes() == np.delete(want.data, 9, axis=1).tobytes()
    assert np.array_equal(got.data[:, 9], want.data[:, 9])


@pytest.mark.parametrize("name", ALL)
def test_oracle_runs_the_member_set(name, runs):
    c, planes, final, status = runs(name)
    assert (status == 0).all()
    assert np.isfinite(planes).all() and np.isfinite(final).all()
    assert planes[1].max() > 0.01 and (planes[1] == 0).any() and planes[2].max() > 0.01


def away_from_zero(x):
    """every value one ulp further from zero: none crosses or reaches 0"""
    return np.where(x > 0, np.nextafter(x, np.inf), np.where(x < 0, np.nextafter(x, -np.inf), x))


def narrowed(x):
    """rounded to fp32 -- except what fp32 would flush to zero (`tiny`): there the sign is the whole value, and keeping
    it is what the fp32-mixed kernels are asked to do"""
    y = x.astype(np.float32).astype(np.float64)
    return np.where((y == 0) & (x != 0), x, y)


@pytest.mark.parametrize("name", ALL)
def test_conditioning_yardstick(name, runs, oracle, members):
    c, want, _, _ = runs(name)
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-3)
    d = c.data.copy()
    d[:, 1:9] = away_from_zero(d[:, 1:9])
    d[:, 9] = np.maximum(d[:, 1] * d[:, 0], 0.0)
    moved = oracle.run_block(FLAGS, members, ClimTable(d, c.year, c.day))[0]
    ulp = (np.abs(moved - want) / scale).max()
    d = c.data.copy()
    d[:, 1:9] = narrowed(d[:, 1:9])
    rounded = oracle.run_block(FLAGS, members, ClimTable(d, c.year, c.day))[0]
    f32 = (np.abs(rounded - want) / scale).max()
    sums = (np.abs(rounded.sum(1) - want.sum(1)) / (np.abs(want).sum(1) + 1.0)).max()
    print(f"{name}: one ulp away from zero {ulp:.2e}; forcing rounded to fp32: max {f32:.2e}, time sums {sums:.2e}")
    assert ulp <= 1e-12
    assert f32 <= 1e-4 and sums <= 1e-6
