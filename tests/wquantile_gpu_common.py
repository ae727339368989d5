"""What the GPU tests of the weighted order statistics share (test_gpu_wquantiles.py, test_gpu_wquantiles_edges.py): tensors on
the device, the comparison of a call's outputs with tests/wquantile_reference.py (the bounds are derived in the docstring of
tests/test_gpu_wquantiles.py), random log-weights and batches of crafted scenarios."""
import collections

import numpy as np
import torch

import sipnet_amd as sa
from tests import pf_edges_reference as er
from tests import wquantile_reference as wr
from tests.enkf_gpu_common import DEV, bits

Q6 = [0.0, 1.0, 0.5, 0.025, 0.975, 1.0 / 3.0]
SORT, SELECT = 1, 2
G = er.G
Host = collections.namedtuple("Host", "quant site crps rank moments fixed")


def bare(n_sites, M, prec=sa.F64):
    """a batch that was created and nothing else: all that live_only = 0 needs"""
    return sa.Batch(sa.flags_from(), n_sites, M, prec)


def on_device(host, dtype=torch.float64, pad=0):
    """host [rows][ncol] -> a device tensor [rows][ncol + pad] of dtype, the padding full of NaN"""
    host = np.asarray(host, dtype=np.float64)
    full = np.full((host.shape[0], host.shape[1] + pad), np.nan)
    full[:, :host.shape[1]] = host
    return torch.tensor(full, dtype=dtype, device=DEV)


def dev(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, device=DEV)


def widened(host, dtype):
    """what the device reads of host through a tensor of dtype, as doubles"""
    return np.asarray(host, dtype=np.float64).astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)


def host_of(res):
    return Host(*(None if x is None else x.cpu().numpy() for x in res[:6]))


def same(got, want, what=""):
    """equal as values (a NaN equals a NaN, -0.0 equals +0.0)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, got, want)


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8), err_msg=str(what))


def same_outputs(one, two, what=""):
    """two Hosts: the same outputs are there, and they are the same bits"""
    for name, x, y in zip(Host._fields, one, two):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            same_bits(x, y, (what, name))


def check_integers(fixed, logw, M, used=None):
    """the device's integers against the exact ones -> the sites' codes (0 or -2)"""
    codes = []
    for s in range(fixed.size // M):
        sl = slice(s * M, (s + 1) * M)
        us = None if used is None else used[sl]
        want, d, tol = wr.weights_of(logw[sl], us)
        codes.append(wr.site_code(logw[sl], us))
        assert (np.abs(fixed[sl] - want) <= 1).all(), s
        sure = d > tol
        np.testing.assert_array_equal(fixed[sl][sure], want[sure])
    return codes


def check_floats(got, x, fixed, n_sites, M, obs, nan, crps_cells=None, denormal_rows=()):
    """moments and CRPS of every cell (crps_cells: of those cells only) within the docstring's bounds
    -> the largest fractions met (mean, m2, crps).  A cell with an infinite value under weight is left out (the contract says
    nothing of its moments and CRPS).  denormal_rows: the mean's and the CRPS's bounds of those rows get the absolute
    (2 n + 8) 2^-1074 (tests/test_gpu_wquantiles_edges.py, B), and an m2 that is below every double must be 0."""
    worst = [0.0, 0.0, 0.0]

    def frac(err, tol):
        return err / tol if tol > 0 else (0.0 if err == 0 else np.inf)

    for r in range(x.shape[0]):
        for s in range(n_sites):
            xs, ws = x[r, s * M:(s + 1) * M], fixed[s * M:(s + 1) * M]
            if nan[r, s]:
                assert np.isnan(got.moments[r, s]).all() and (got.crps is None or np.isnan(got.crps[r, s])), (r, s)
                continue
            if not np.isfinite(xs[ws > 0]).all():
                continue
            (mean, m2), (b_mean, b_m2) = wr.moments(xs, ws), wr.moments_bounds(xs, ws)
            extra = wr.denormal_allowance(int((ws > 0).sum())) if r in denormal_rows else 0.0
            worst[0] = max(worst[0], frac(abs(float(np.longdouble(got.moments[r, s, 0]) - mean)), b_mean + extra))
            if r in denormal_rows and float(m2) == 0.0:
                assert got.moments[r, s, 1] == 0.0, (r, s, got.moments[r, s, 1])
            else:
                worst[1] = max(worst[1], frac(abs(float(np.longdouble(got.moments[r, s, 1]) - m2)), b_m2))
            if got.crps is None or obs is None:
                continue
            y = obs[r, s]
            if np.isnan(y):
                assert np.isnan(got.crps[r, s]), (r, s)
            elif crps_cells is None or (r, s) in crps_cells:
                want, tol = wr.crps_pairwise(xs, ws, y), wr.crps_bound(xs, ws, y)
                worst[2] = max(worst[2], frac(abs(float(np.longdouble(got.crps[r, s]) - want)), tol + extra))
    print("largest fraction of the bounds: mean %.3e, m2 %.3e, crps %.3e" % tuple(worst))
    assert max(worst) <= 1.0, worst
    return worst


class Worst:
    """the largest fractions of the bounds (mean, m2, crps) over the calls of analyse that were given it"""

    def __init__(self, group):
        self.group, self.worst, self.calls = group, [0.0, 0.0, 0.0], 0

    def add(self, met):
        self.worst = [max(a, c) for a, c in zip(self.worst, met)]
        self.calls += 1

    def report(self):
        print("wq-edges %s: mean %.3e, m2 %.3e, crps %.3e" % ((self.group,) + tuple(self.worst)))
        assert self.calls > 0 and max(self.worst) <= 1.0, (self.group, self.calls, self.worst)


def analyse(b, host, logw, q, obs=None, dtype=torch.float64, pad=0, used=None, live=False, paths=(SORT, SELECT), crps_cells=None,
            what="", series=None, denormal_rows=(), worst=None):
    """both paths of the call over host [rows][ncol] and logw [ncol], everything held to the reference -> the sort path's
    (or the only path's) outputs on the host, and the reference's.  series: the device tensor to pass (host is then what it
    holds, widened); worst: a Worst that takes the fractions of the bounds every path met."""
    n_sites, M = b.n_sites, b.n_members
    x = widened(host, dtype)
    if series is None:
        series = on_device(host, dtype, pad)
    lw = dev(logw)
    runs = {}
    for path in paths:
        crps = obs is not None and path == SORT
        res = b.plane_quantiles_weighted(series, lw, q, live_only=live, obs=obs, want_crps=crps, want_moments=True, path=path,
                                         return_fixed=True)
        assert res.path == path and b.pf_info()["fused"] == (1 if path == SORT else 0), (what, path)
        assert (res.crps is not None) == crps and (res.rank is not None) == (obs is not None)
        runs[path] = host_of(res)
    first = runs[paths[0]]
    codes = check_integers(first.fixed, np.asarray(logw, dtype=np.float64), M, used)
    want = wr.plane(x, n_sites, M, first.fixed, q, obs, codes)
    for path, got in runs.items():
        same(got.quant, want[0], (what, path))
        np.testing.assert_array_equal(got.site, want[1], err_msg=str((what, path)))
        if obs is not None:
            np.testing.assert_array_equal(got.rank, want[2], err_msg=str((what, path)))
        np.testing.assert_array_equal(bits(got.quant), bits(first.quant), err_msg=str((what, path)))      # the paths: the same bits
        same_bits(got.fixed, first.fixed, (what, path))
        same_bits(got.site, first.site, (what, path))
        if obs is not None:
            same_bits(got.rank, first.rank, (what, path))
        met = check_floats(got, x, first.fixed, n_sites, M, obs, want[3], crps_cells, denormal_rows)
        if worst is not None:
            worst.add(met)
    return first, want


def random_logw(rng, n, spread=3.0):
    """log-weights with everything in them: most within a few units, some -inf, a NaN, some far below the cut-off"""
    lw = rng.normal(size=n) * spread - 700.0
    lw[rng.random(n) < 0.1] = -np.inf
    lw[rng.random(n) < 0.03] = np.nan
    lw[rng.random(n) < 0.05] -= 40.0
    return lw


def scenario_batches(M, scenarios, q, rows=3, dtype=torch.float64):
    """the scenarios (name -> (logw [M], host [rows][M], obs [rows])) three sites to a bare batch -> name -> (the site's
    outputs: quant [n_q][rows], site (3,), crps [rows], rank [rows][2], moments [rows][2], fixed [M])"""
    names, out = list(scenarios), {}
    for k0 in range(0, len(names), 3):
        group = [names[(k0 + i) % len(names)] for i in range(3)]
        logw = np.concatenate([scenarios[n][0] for n in group])
        host = np.concatenate([scenarios[n][1] for n in group], axis=1)
        obs = np.stack([scenarios[n][2] for n in group], axis=1)
        b = bare(3, M)
        got, _ = analyse(b, host, logw, q, obs, dtype, what=group)
        b.close()
        for i, n in enumerate(group):
            out[n] = Host(got.quant[:, :, i], got.site[i], got.crps[:, i], got.rank[:, i], got.moments[:, i], got.fixed[i * M:(i + 1) * M])
    return out
