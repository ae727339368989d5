"""What the GPU tests of the three ensemble Kalman filter analyses share (test_gpu_enkf_sites.py, test_gpu_enkf_local.py,
test_gpu_enkf_block.py): the analysed pools and operators, a forecast of a batch of many sites, observations near its ensemble,
the comparison with a reference, and the grids and lists of a localization."""
import functools
import os

import numpy as np
import torch

import sipnet_amd as sa
from sipnet_amd import synth
from tests import enkf_reference as er
from tests import helpers

BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
DEV = "cuda"
ANALYSED = ["plantWoodC", "plantLeafC", "soilC", "soilWater", "coarseRootC", "fineRootC", "plantCAccountingDelta"]
SLOTS = [sa.POOLS.index(p) for p in ANALYSED]
OTHER = [k for k in range(32) if k not in SLOTS]


@functools.lru_cache(maxsize=None)
def site_clim(s):
    """every site its own forcing"""
    return synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(48 * 8, site=s)))


def operators():
    """LAI, above-ground wood, soil wetness, the NEE sum"""
    return [sa.enkf_pools(["plantLeafC"], divide_by="leafCSpWt"),
            sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"]),
            sa.enkf_pools(["soilWater"], divide_by="soilWHC"),
            sa.enkf_plane("nee")]


def op_tuples(ops):
    return [(o.kind, o.pool_mask, o.plane, o.param, o.scale) for o in ops]


def sites_batch(members, n_sites, prec, clim=site_clim, events=None):
    M = members.shape[0] // n_sites
    b = sa.Batch(sa.flags_from(), n_sites, M, prec, fast_math=True)
    for s in range(n_sites):
        b.set_climate(s, clim(s))
        if events is not None:
            b.set_events(s, events)
        b.set_params(s, members[s * M:(s + 1) * M])
    b.setup()
    return b


def carried_params(b):
    w = 32 + (125 if b.precision == sa.F32_MIXED else 250)
    idx = torch.arange(b.ncol, dtype=torch.int32, device=DEV)
    return b.pack_members(idx, True)[w:].cpu().numpy().T        # [ncol][NPARAMS]


def observe(state, planes, prm, n_sites, ops, rng, nan_sites=(), nan_obs=()):
    """per site and operator: an observation near the live ensemble's mean, sd ~ the ensemble's spread"""
    M = state.shape[0] // n_sites
    obs = np.zeros((n_sites, len(ops)))
    sd = np.zeros_like(obs)
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[state[cols, 29] == 0]
        for i, op in enumerate(op_tuples(ops)):
            h = er.predicted(op, state[live, :13], [p[:, live] for p in planes], lambda k: prm[live, k]) if len(live) else [0.0]
            spread = float(np.std(h)) + 1e-3 * (abs(float(np.mean(h))) + 1e-3)
            obs[s, i] = float(np.mean(h)) + spread * rng.normal()
            sd[s, i] = spread * (0.5, 1.0, 2.0)[(s + i) % 3]
    for s in nan_sites:
        obs[s] = np.nan
    for s, i in nan_obs:
        obs[s, i] = np.nan
    return obs, sd


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def within(got, want, fc, n_sites, slots=SLOTS, bound=1e-10):
    """|got - want| <= bound (1e-10) max(|x|, the site's ensemble sd) per analysed pool; the largest ratio is printed first"""
    M = got.shape[0] // n_sites
    worst = 0.0
    for s in range(n_sites):
        sl = slice(s * M, (s + 1) * M)
        scale = np.maximum(np.abs(want[sl][:, slots]), fc[sl][:, slots].std(0) + 1e-300)
        worst = max(worst, float((np.abs(got[sl][:, slots] - want[sl][:, slots]) / scale).max()))
    print(f"largest |got - want| / max(|x|, site ensemble sd) over {n_sites} sites: {worst:.3e} (bound {bound:g})")
    for s in range(n_sites):
        sl = slice(s * M, (s + 1) * M)
        scale = np.maximum(np.abs(want[sl][:, slots]), fc[sl][:, slots].std(0) + 1e-300)
        assert (np.abs(got[sl][:, slots] - want[sl][:, slots]) <= bound * scale).all(), s
    return worst


def forecast(base, n_sites, M, prec, steps=96, seed=1, of=None):
    """of: the members are the first n_sites * M of a batch of `of` sites (the same forecast, site for site)"""
    members = synth.perturbed_params(base, (of or n_sites) * M, seed=seed)[:n_sites * M]
    b = sites_batch(members, n_sites, prec)
    planes, _ = b.run(0, steps)
    return b, planes


def crafted(base, n_sites, M, prec, pools, dead=()):
    """a batch whose pools are given, not forecast: set up from perturbed parameters, its state read, slots 0..12 of every
    column overwritten with pools [n_sites * M][13], the columns `dead` given a non-zero status, and written back
    -> (batch, the state it now holds).  No run() is needed before an analysis."""
    b = sites_batch(synth.perturbed_params(base, n_sites * M, seed=1), n_sites, prec)
    st = b.get_state()
    st[:, :13] = pools
    st[list(dead), 29] = 3.0
    b.set_state(st)
    return b, b.get_state()


def grid(n_sites, far=()):
    """sites on a 0.5 degree grid 8 wide; `far` sites moved 20 degrees north, out of everyone's reach"""
    r, c = np.divmod(np.arange(n_sites), 8)
    lat = 45.0 + 0.5 * r
    lat[list(far)] += 20.0
    return lat, -85.0 + 0.5 * c


def empty(n_sites):
    return np.zeros(n_sites + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)
