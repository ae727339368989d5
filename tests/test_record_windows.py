"""The record windows of tests/record_windows.py, without a GPU: each window still holds what it is there for -- read from
the oracle's records alone, so a window that has drifted back into ordinary weather fails here, before any GPU run -- and the
members an fp32-mixed run is not held to by value on a window (one-ulp figure, scaled to a float's ulp, above 1e-4) are
named here, from the oracle, and are at most 5 % of a set.

Measured:
  melt   default [9683, 9870), the three other flag sets [10403, 10590); every member melts out at the same step (the snow
         parameters are not perturbed), 103 and 93 steps into the window; no member left out of the fp32-mixed comparison
         (largest one-ulp figure, in float ulps: 1.6e-5 of the column maximum)
  thaw   members 2 and 129 have the ten constant days' soil temperature as their frozenSoilThreshold; no member left out
         (largest figure 1.8e-6)"""
import numpy as np
import pytest

from sipnet_amd.config import param_index as pi
from tests import forcing_regimes as fr
from tests import record_windows as rw

FLAGSETS = list(rw.FLAG_SETS)
SNOW = rw.SNOW


@pytest.fixture(scope="module")
def ref(oracle):
    return rw.Reference(oracle)


def test_flag_and_member_sets():
    from tests.test_gpu_full import EVERYTHING
    assert rw.EVERYTHING == EVERYTHING and FLAGSETS == ["default", "russell_3", "ncycle", "everything"]
    for fs in FLAGSETS:
        m, f = rw.members(fs), rw.members(fs, flipped=True)
        assert m.shape == (133, 80) and np.array_equal(m, fr.hard_members(m[0]))
        plain = lambda x: bool((x[:, pi("dVpdExp")] == 2.0).all() and (x[:, pi("soilRespMoistEffect")] == 1.0).all())
        assert plain(m) == (fs == "default") and plain(f) != plain(m)         # the other exponent instantiation
        assert (np.delete(m, pi("dVpdExp"), axis=1) == np.delete(f, pi("dVpdExp"), axis=1)).all()


def test_the_melt_rule_moves_with_the_melt():
    """a window 400 steps off fails the condition the GPU tests rely on"""
    snow = np.zeros((1500, 5))
    for m, t in enumerate((500, 510, 520, 530, 900)):
        snow[:t, m] = 1.0
    assert list(rw.first_melt_out(snow)) == [500, 510, 520, 530, 900]
    a, b = rw.melt_window(snow)
    assert (a, b) == (419, 606) and a % 16 == 3 and b - a == 187
    ok = lambda a, b: ((snow[a] > 0) & (snow[b - 1] == 0)).sum() * 2 >= snow.shape[1]
    assert ok(a, b) and not ok(a + 400, b + 400) and not ok(a - 400, b - 400)
    never = np.ones((100, 3))
    assert list(rw.first_melt_out(never)) == [-1, -1, -1]
    with pytest.raises(AssertionError):
        rw.melt_window(never)


@pytest.mark.parametrize("flipped", [False, True], ids=["members", "flipped"])
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_melt(flagset, flipped, ref):
    w = ref.window("melt", flagset, flipped)
    assert (w.status == 0).all() and np.isfinite(w.rows).all()
    assert w.b - w.a == 187 and w.a % 16 == 3 and 0 < w.a and w.b < w.T
    if flagset == "default":
        assert (w.a, w.b) == (9683, 9870)
    snow = w.rows[:, SNOW]
    melts = (snow[0] > 0) & (snow[-1] == 0)
    first = rw.first_melt_out(snow)
    print(f"melt {flagset}: [{w.a}, {w.b}), {int(melts.sum())} of {len(melts)} members melt out inside, the median one {int(np.median(first[melts]))} "
          f"steps in; {(snow == 0).mean():.0%} of the window's snow values are 0")
    assert melts.sum() * 2 >= len(melts)
    assert 187 // 2 - 16 < np.median(first[melts]) <= 187 // 2 + 16                 # near the middle
    assert w.colmax[SNOW].min() > 10.0                                               # a deep pack (cm water equivalent)


@pytest.mark.parametrize("flagset", FLAGSETS)
def test_switch(flagset, ref):
    w = ref.window("switch", flagset)
    assert (w.a, w.b) == (1900, 2080) and (w.status == 0).all() and np.isfinite(w.rows).all()
    # both switches strictly inside and off a 16-step tile; the record launch starts inside a tile.  (Its end, 2080, IS a
    # multiple of 16: the lean launch behind it starts on a tile, the lean launch in front of it ends inside one.)
    assert all(w.a < s < w.b and s % 16 != 0 for s in fr.SWITCH_STEPS) and w.a % 16 != 0 and (w.b - w.a) % 16 != 0
    assert set(np.unique(w.clim.data[w.a:w.b, 0])) == {1 / 48, 0.5}


@pytest.mark.parametrize("flagset", FLAGSETS)
def test_thaw(flagset, ref):
    w = ref.window("thaw", flagset)
    assert (w.a, w.b) == (0, 544) and (w.status == 0).all() and np.isfinite(w.rows).all()
    tsoil = w.clim.data[:, 2]
    assert w.a < 480 < w.b and np.all(tsoil[:480] == tsoil[0]) and np.all(tsoil[480:w.b] != tsoil[479:w.b - 1])
    on = np.isin(w.members[:, pi("frozenSoilThreshold")], tsoil[w.a:w.b])
    print(f"thaw {flagset}: members whose frozenSoilThreshold is a soil temperature of the window: {np.flatnonzero(on).tolist()}")
    assert on.any() and (w.members[on, pi("frozenSoilThreshold")] == tsoil[0]).any()      # ... the ten constant days' among them


@pytest.mark.parametrize("case", ["halfday_12h", "halfday_alternating"])
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_halfday(flagset, case, ref):
    w = ref.window(case, flagset)
    assert (w.a, w.b, w.T) == (0, 730, 730) and (w.status == 0).all() and np.isfinite(w.rows).all()
    assert set(np.unique(w.clim.data[:, 0])) == ({0.5} if case == "halfday_12h" else {0.6, 0.4})
    assert w.colmax[SNOW].max() > 0 and (w.rows[:, SNOW] == 0).any()                 # snow in winter, none in summer


@pytest.mark.parametrize("flagset", FLAGSETS)
def test_newyear(flagset, ref):
    w = ref.window("newyear", flagset)
    c = w.clim
    assert w.T == 960 and (w.a, w.b) == (473, 487) and (w.status == 0).all() and np.isfinite(w.rows).all()
    assert set(c.year) == {2021, 2022} and c.year[479] == 2021 and c.year[480] == 2022 and c.day[479] == 365 and c.day[480] == 1
    yearly_gpp, yearly_rtot, tot_rtot = w.debug[56], w.debug[57], w.debug[63]
    tot_gpp = w.last[35]
    print(f"newyear {flagset}: member 0 yearlyGpp {yearly_gpp[0]:.3g} of totGpp {tot_gpp[0]:.3g}, yearlyRtot {yearly_rtot[0]:.3g} of totRtot {tot_rtot[0]:.3g}")
    assert ((0 < yearly_rtot) & (yearly_rtot < tot_rtot)).all()
    if flagset == "default":
        assert ((0 < yearly_gpp) & (yearly_gpp < tot_gpp)).all()


ALL = [("melt", False), ("melt", True), ("thaw", False)]


@pytest.mark.parametrize("case,flipped", ALL, ids=[c + ("_flipped" if f else "") for c, f in ALL])
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_one_ulp_figures_name_the_members_fp32_is_not_held_to(flagset, case, flipped, ref):
    w = ref.window(case, flagset, flipped)
    out = w.f32_excluded()
    kept = w.figure[~out]
    print(f"{case} {flagset}{' flipped' if flipped else ''}: left out of the fp32-mixed value comparison: {np.flatnonzero(out).tolist()} "
          f"(figures {[float('%.2g' % x) for x in w.figure[out]]}); the others' largest figure {kept.max():.2e} of the column maximum in float ulps")
    assert np.isfinite(w.figure).all()
    assert out.sum() <= 0.05 * len(out)
