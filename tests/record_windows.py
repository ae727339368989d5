"""Windows of the forcing regimes (tests/forcing_regimes.py) in which the 44-column record is worth asking for, picked from
the oracle alone: tests/test_gpu_record_regimes.py runs the record-writing ("Full") builds of the step kernels on them,
tests/test_record_windows.py asserts on the CPU that each window still holds what it is there for.

  melt      `polar`: 187 steps that start three steps past a multiple of 16, the median member's first melt-out (record column
            19 reaches 0 after being positive) near the middle -- found per flag set and member set, because the pack of
            allflags_forest.param melts 710 steps later than base_forest.param's
  switch    `lengths_switching` [1900, 2080): both changes of the step length inside, neither end on a 16-step tile
  thaw      `threshold` [0, 544): the ten days of constant soil temperature ON a member's frozenSoilThreshold, then the soil
            changing on every step; the record launch comes first
  halfday   `lengths_12h` and `lengths_alternating`, the whole run of 730 records
  newyear   the last ten days of an `arid` year and the first ten of the next: 960 steps, the new year at step 480

The members are forcing_regimes.hard_members (133: two chunks and a ragged third) of base_forest.param for `default` and of
allflags_forest.param for `russell_3`, `ncycle` and `everything`; `flipped` is the same set with the other plain-exponent
instantiation selected (default: one member's dVpdExp = 1.7; the others: every member's dVpdExp = 2).

Of each (case, flag set) the oracle's run keeps the window's rows, every member's column maxima over the whole run (the scale
of the record criterion) and -- of melt and thaw, whose snow and frozen-soil thresholds an fp32-mixed run may take a step apart
-- the one-ulp figure: the forcing moved one ulp away from zero as in
tests/test_forcing_regimes.py, the largest change of a window value in units of the column maximum, scaled from a double's
ulp to a float's.  Members whose figure exceeds 1e-4 are the ones an fp32-mixed run cannot be held to by value on that
window (a threshold the reference itself takes a step apart); tests/test_record_windows.py caps them at 5 % of a set."""
import os

import numpy as np

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from sipnet_amd.io import ClimTable
from tests import forcing_regimes as fr
from tests import helpers
from tests.regime_gpu_common import FLAG_SETS as REGIME_FLAG_SETS

DATA = os.path.join(helpers.REPO, "sipnet_amd", "data")
EVERYTHING = dict(litterPool=1, anaerobic=1, nitrogenCycle=1, carbonSaturation=1, flooding=1, growthResp=1, leafWater=1)   # (test_gpu_full.EVERYTHING)
FLAG_SETS = {"default": REGIME_FLAG_SETS["default"], "russell_3": REGIME_FLAG_SETS["russell_3"], "ncycle": REGIME_FLAG_SETS["ncycle"],
             "everything": EVERYTHING}
CASES = {"melt": "polar", "switch": "lengths_switching", "thaw": "threshold", "halfday_12h": "lengths_12h",
         "halfday_alternating": "lengths_alternating", "newyear": "arid"}
MELT_LEN, MELT_PHASE = 187, 3
SWITCH_WINDOW = (1900, 2080)
THAW_WINDOW = (0, 544)
NEWYEAR_SLICE, NEWYEAR_STEP, NEWYEAR_RECORD = (17040, 18000), 480, (473, 487)
SNOW, NREC = 19, 36
F32_ULPS = float(np.finfo(np.float32).eps / np.finfo(np.float64).eps)
F32_FIGURE_MAX = 1e-4
F32_FIGURE_CASES = ("melt", "thaw")
KEPT_WINDOWS = 3


def flags(flagset):
    return sa.flags_from(**FLAG_SETS[flagset])


def members(flagset, flipped=False):
    path = os.path.join(DATA, "base_forest.param" if flagset == "default" else "allflags_forest.param")
    out = fr.hard_members(sa.read_params(path, flags(flagset))[0])
    if flipped and flagset == "default":
        out[3, pi("dVpdExp")] = 1.7                                # the general-exponent instantiation (tests/test_gpu_sums.py)
    elif flipped:
        out[:, pi("dVpdExp")] = 2.0                                # ... and the plain one: soilRespMoistEffect is 1 in the file
        assert (out[:, pi("soilRespMoistEffect")] == 1.0).all()
    return out


def clim(case):
    if case == "newyear":
        whole = synth.convert_raw(synth.round_like_file(fr.arid(n_steps=17520 + NEWYEAR_STEP)))
        return whole.slice(*NEWYEAR_SLICE)
    return fr.clim(CASES[case])


def first_melt_out(snow):
    """snow [T][M] -> every member's first step with snow == 0 after snow > 0 (-1: none)"""
    hit = (snow[1:] == 0) & (snow[:-1] > 0)
    return np.where(hit.any(axis=0), hit.argmax(axis=0) + 1, -1)


def melt_window(snow):
    """the rule: the last start three steps past a multiple of 16 that leaves the median first melt-out at or after the
    window's middle"""
    first = first_melt_out(snow)
    assert (first >= 0).sum() * 2 > len(first), "the pack of most members never melts"
    t = int(np.median(first[first >= 0]))
    a = 16 * ((t - MELT_LEN // 2 - MELT_PHASE) // 16) + MELT_PHASE
    return a, a + MELT_LEN


def away_from_zero(c):
    """the forcing one ulp further from zero, the growing degree days of the new air temperature (test_forcing_regimes)"""
    d = c.data.copy()
    x = d[:, 1:9]
    d[:, 1:9] = np.where(x > 0, np.nextafter(x, np.inf), np.where(x < 0, np.nextafter(x, -np.inf), x))
    d[:, 9] = np.maximum(d[:, 1] * d[:, 0], 0.0)
    return ClimTable(d, c.year, c.day)


class Window:
    """a, b, T; clim, flags, members; rows [b - a][36][M], colmax [36][M] and last [36][M] (the final record) of the oracle; status [M]; figure [M]: the
    one-ulp figure in float ulps (0 outside melt and thaw); newyear only: debug [72][M], the oracle's last debug row, and abs_nee [2][M]: the sums of
    |NEE| over the run and over the new year's steps"""

    def scale(self):
        return np.maximum(self.colmax, 1e-3)

    def f32_excluded(self):
        return self.figure > F32_FIGURE_MAX


def _pass(oracle, fl, mem, c, keep, debug=False):
    status = np.zeros(mem.shape[0], dtype=np.int32)
    for m in range(mem.shape[0]):
        if debug:
            status[m], rec, dbg = oracle.run_member_debug(fl, mem[m], c)
            keep(m, rec, dbg)
        else:
            status[m], rec, _ = oracle.run_member(fl, mem[m], c)
            keep(m, rec)
    return status


class Reference:
    """the oracle's windows per (case, flag set, flipped), each computed once; a whole year of records is never held"""

    def __init__(self, oracle):
        self.oracle, self.cache, self.clims, self.year = oracle, {}, {}, (None, None)

    def clim(self, case):
        if case not in self.clims:
            self.clims[case] = clim(case)
        return self.clims[case]

    def window(self, case, flagset, flipped=False):
        key = (case, flagset, flipped)
        if key not in self.cache:
            while len(self.cache) >= KEPT_WINDOWS:                  # (a half-day window is 28 MB: the tests ask window by window)
                self.cache.pop(next(iter(self.cache)))
            self.cache[key] = self._window(case, flagset, flipped)
        return self.cache[key]

    def planes(self, case, flagset, flipped=False):
        """the oracle's planes, final records and status of the whole run (run_block: what regime_gpu_common.judge takes);
        only the last one asked for is kept"""
        key = (case, flagset, flipped)
        if self.year[0] != key:
            self.year = (None, None)
            w = self.window(*key)
            self.year = (key, self.oracle.run_block(w.flags, w.members, w.clim))
        return self.year[1]

    def _window(self, case, flagset, flipped):
        w = Window()
        w.case, w.flagset, w.clim, w.flags, w.members = case, flagset, self.clim(case), flags(flagset), members(flagset, flipped)
        c, M = w.clim, w.members.shape[0]
        w.T = T = c.n_steps
        if case == "melt":
            snow = np.zeros((T, M))

            def keep_snow(m, rec):
                snow[:, m] = rec[:, SNOW]
            _pass(self.oracle, w.flags, w.members, c, keep_snow)
            w.a, w.b = melt_window(snow)
        else:
            w.a, w.b = {"switch": SWITCH_WINDOW, "thaw": THAW_WINDOW, "newyear": NEWYEAR_RECORD}.get(case, (0, T))
        a, b = w.a, w.b
        w.rows, w.colmax, w.last = np.zeros((b - a, NREC, M)), np.zeros((NREC, M)), np.zeros((NREC, M))
        if case == "newyear":
            w.debug, w.abs_nee = np.zeros((72, M)), np.zeros((2, M))

        def keep(m, rec, dbg=None):
            w.rows[:, :, m], w.colmax[:, m], w.last[:, m] = rec[a:b], np.abs(rec).max(axis=0), rec[-1]
            if dbg is not None:
                w.debug[:, m] = dbg[-1]
                w.abs_nee[:, m] = np.abs(rec[:, 0]).sum(), np.abs(rec[NEWYEAR_STEP:, 0]).sum()
        w.status = _pass(self.oracle, w.flags, w.members, c, keep, debug=case == "newyear")
        # the one-ulp figure (melt and thaw, where a threshold decides): the same members on the forcing moved one ulp away
        # from zero, up to the window's end
        w.figure = np.zeros(M)
        if case in F32_FIGURE_CASES:
            moved = np.zeros_like(w.rows)

            def keep_moved(m, rec):
                moved[:, :, m] = rec[a:b]
            _pass(self.oracle, w.flags, w.members, away_from_zero(c).slice(0, b), keep_moved)
            w.figure = (np.abs(moved - w.rows) / w.scale()).max(axis=(0, 1)) * F32_ULPS
        return w
