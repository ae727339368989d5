"""Deterministic overwrites of member pools between launches, for tests/test_oracle_edits.py (CPU) and
tests/test_gpu_state_edits.py: what a filter's analysis or a caller's set_state does to a batch, as hand-made edit sets.

One site is M = 200 members: three full chunks of 64 and a ragged chunk of 8.  The forcing is a window of the synthetic
half-hourly year (T steps from day START_DAY on); every member's gddLeafOn is set so that its leaf-on falls between the first
and the last cut.  The edits fall at three cuts: CUTS[0] is a multiple of 16 steps (a midnight), CUTS[1] is one step
after a midnight, CUTS[2] is neither.

An edit set is built from a get_state() array [ncol][32] and the converted parameters [ncol][80]; it changes pools
(slots 0..12) only and hands every other slot back exactly as read.  Kinds are dealt round-robin over the lanes, so dying
and living lanes share every wavefront; the sharp kinds are pinned at lanes 0, 63, 64, 127, 128 and 199:

  untouched      nothing changes
  scale          every carbon pool (wood, leaf, soil, litter, both roots, the accounting delta) x a factor in [0.25, 4],
                 another one at every cut
  leaf_0         plantLeafC = 0 at the last cut (after leaf-on: the growing season)
  leaf_12        plantLeafC = 12 x leafCSpWt at the first cut
  water_0        soilWater = 0 at the second cut
  water_2whc     soilWater = 2 x soilWHC at the last cut (above capacity)
  snow_0         snow = 0 at the first cut
  snow_30        snow = 30 at the last cut (snow in the growing season)
  litter_0       litterC = 0 at the second cut (the litter pool without the nitrogen cycle: with it the reference divides by
                 the empty pool -- litterC / litterN is 0, rLitter / 0 is 0 / 0 -- and every plane of the member is NaN from
                 the next step on, which tests/parameter_regimes.py's `edges` already put next to living lanes)
  min_n_0        minN = 0 at the second cut (nitrogen cycle)
  storage_n_0    plantStorageN = 0 at the first cut (nitrogen cycle)
  just_dying     plantCAccountingDelta such that plantWoodC + delta is the largest double sum <= 1e-6 (hasSufficientBiomass
                 asks for > 1e-6): dead at the head of the next step, without a death step
  just_surviving the smallest sum > 1e-6: alive at the head of the next step, which decides
  emptied        wood and both root pools 0 at the first cut; at the last cut the pools the member had before are put back

Negative or non-finite pools are out of scope (set_state defines nothing for them)."""
import numpy as np

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from tests import parameter_regimes as pr

M = 200
T = 1913
START_DAY = 100
CUTS = (480, 961, 1411)
SUM_GROUP, SUM_CUTS = 7, (483, 966, 1407)          # run_sums: cuts at multiples of the group
TINY = 1e-6
PINNED = {0: "emptied", 63: "just_dying", 64: "just_surviving", 127: "emptied", 128: "just_dying", 199: "just_surviving"}
WOOD, LEAF, SOILC, WATER, LITTER, SNOW, COARSE, FINE, MIN_N, ORG_N, LITTER_N, STORAGE_N, DELTA = range(13)
CARBON = (WOOD, LEAF, SOILC, LITTER, COARSE, FINE, DELTA)
# the kinds whose written values are continuous quantities (computed from pools or parameters): the conditioning yardstick
# moves them one ulp.  The others write exact constants (0, 30) or a delta placed on a threshold the model compares it with,
# which the yardstick holds (the rule of tests/parameter_regimes.py: `held`, COMPARED)
CONTINUOUS = ("scale", "emptied", "leaf_12", "water_2whc")
assert CUTS[0] % 16 == 0 and CUTS[1] % 16 != 0 and CUTS[2] % 16 != 0 and CUTS[1] % 48 == 1 and all(c % SUM_GROUP == 0 for c in SUM_CUTS)


def clim(site=0):
    a = (START_DAY - 1) * 48
    raw = synth.half_hourly_year_raw(a + T + 48 - (a + T) % 48, site=site)
    return synth.convert_raw(synth.round_like_file({k: v[a:a + T] for k, v in raw.items()}))


def kinds(flagset):
    out = ["untouched", "scale", "leaf_0", "leaf_12", "water_0", "water_2whc", "snow_0", "snow_30"]
    if pr.FLAG_SETS[flagset].get("litterPool") and not pr.FLAG_SETS[flagset].get("nitrogenCycle"):
        out.append("litter_0")
    if pr.FLAG_SETS[flagset].get("nitrogenCycle"):
        out += ["min_n_0", "storage_n_0"]
    return out + ["just_dying", "just_surviving", "emptied"]


def lane_kinds(flagset, ncol=M):
    """-> the kind of every column; a batch of several sites repeats the deal site by site"""
    ks = kinds(flagset)
    free = [m for m in range(M) if m not in PINNED]
    deal = dict(PINNED)
    deal.update({m: ks[i % len(ks)] for i, m in enumerate(free)})
    return [deal[c % M] for c in range(ncol)]


def members(flagset, site=0):
    """the perturbed forest of the flag set's parameter file, deciduous, each member's leaf-on threshold at the growing
    degree days the window has accumulated somewhere between the first and the last cut"""
    out = synth.perturbed_params(pr.base(flagset), M, seed=synth.SEED_PARAMS + 17 * site)
    if flagset == "default":                                  # (the other file is deciduous already)
        out[:, pi("leafGrowth")], out[:, pi("fracLeafFall")] = 60.0, 0.3
    cum = np.cumsum(clim(site).data[:, 9])
    at = np.linspace(CUTS[0] + 60, CUTS[2] - 60, M).astype(int)[np.random.default_rng(5).permutation(M)]
    out[:, pi("gddLeafOn")] = 0.5 * (cum[at] + cum[at + 1])
    return out


def factors(ci, ncol):
    u = np.random.default_rng(100 + ci).random(ncol)
    return 0.25 * 16.0 ** u


def threshold_delta(wood, above):
    """the delta for which fl(wood + delta) is the smallest double sum > 1e-6 (above) or the largest <= 1e-6"""
    d = TINY - wood
    if above:
        while not wood + d > TINY:
            d = np.nextafter(d, np.inf)
        while wood + np.nextafter(d, -np.inf) > TINY:
            d = np.nextafter(d, -np.inf)
    else:
        while wood + d > TINY:
            d = np.nextafter(d, -np.inf)
        while not wood + np.nextafter(d, np.inf) > TINY:
            d = np.nextafter(d, np.inf)
    return d


def apply(flagset, ci, state, conv, memo):
    """the edit at cut ci (0, 1, 2): -> a copy of `state` with pools changed; memo (a dict the caller keeps over the three
    cuts) remembers the pools that `emptied` puts back"""
    out = np.array(state, dtype=np.float64, copy=True)
    ncol = out.shape[0]
    p = out[:, :13]                                           # (a view: slots 13.. are never touched)
    f = factors(ci, ncol)
    if ci == 0:
        memo["before"] = p.copy()
    for c, kind in enumerate(lane_kinds(flagset, ncol)):
        if kind == "scale":
            p[c, list(CARBON)] *= f[c]
        elif kind == "leaf_0" and ci == 2:
            p[c, LEAF] = 0.0
        elif kind == "leaf_12" and ci == 0:
            p[c, LEAF] = 12.0 * conv[c, pi("leafCSpWt")]
        elif kind == "water_0" and ci == 1:
            p[c, WATER] = 0.0
        elif kind == "water_2whc" and ci == 2:
            p[c, WATER] = 2.0 * conv[c, pi("soilWHC")]
        elif kind == "snow_0" and ci == 0:
            p[c, SNOW] = 0.0
        elif kind == "snow_30" and ci == 2:
            p[c, SNOW] = 30.0
        elif kind == "litter_0" and ci == 1:
            p[c, LITTER] = 0.0
        elif kind == "min_n_0" and ci == 1:
            p[c, MIN_N] = 0.0
        elif kind == "storage_n_0" and ci == 0:
            p[c, STORAGE_N] = 0.0
        elif kind in ("just_dying", "just_surviving") and ci == (c % M) % 3 and p[c, WOOD] > 1.0:
            p[c, DELTA] = threshold_delta(p[c, WOOD], kind == "just_surviving")
        elif kind == "emptied" and ci == 0:
            p[c, [WOOD, COARSE, FINE]] = 0.0
        elif kind == "emptied" and ci == 2:
            p[c] = memo["before"][c]
    return out


def alive(pools):
    """hasSufficientBiomass (sipnet.c:1530-1536) of pools [ncol][13]"""
    p = np.asarray(pools)
    return (p[:, WOOD] > TINY) & (p[:, WOOD] + p[:, DELTA] > TINY) & (p[:, FINE] + p[:, COARSE] > TINY)


def table(before, after):
    """what the oracle is given for one cut: all 13 pools of every member the edit changed, as they were written -- a pool
    the edit left alone belongs to the edit all the same where another is placed against it (the delta that puts
    plantWoodC + delta on the threshold means nothing next to the oracle's own, slightly different plantWoodC) -- and
    NaN (keep your own) for the members it did not touch: those are not re-synchronised with the batch at the cuts"""
    a, b = np.ascontiguousarray(np.asarray(after)[:, :13]), np.ascontiguousarray(np.asarray(before)[:, :13])
    touched = (a.view(np.uint64) != b.view(np.uint64)).any(axis=1)
    return np.where(touched[:, None], a, np.nan)


def flags(flagset):
    return sa.flags_from(**pr.FLAG_SETS[flagset])
