"""Series likelihood weights on the GPU (sipnet_batch_series_loglik) and the many-site resampling from given weights
(sipnet_batch_pf_resample_sites): against the longdouble reference of tests/series_loglik_reference.py at the shapes where
the kernels can go wrong (members 1 .. 1000 per site, 1 and 3 sites, 1 .. 600 observation rows around the 256-row tile,
sum_steps 1 / 48 / 96, 1 and 3 terms of mixed kinds, both element types, ld > ncol, gaps at tile edges, as whole tiles and as
whole terms); the two paths, a repeated call and an aliased add bit for bit; chained with the existing filter (one Gauss
row = sipnet_batch_pf_analysis_sites, exactly, on both site paths); the resampling alone (effective sample size, tempering,
the keep rule, sites that weigh nothing or have bad arguments); the refusals.

The bound of test 1 is the issue's: |device - reference| <= (n_used + 16) 2^-53 sum |row terms| per member -- a recursive
sum of n_used terms, each formed with a few roundings.  h, the modelled value of a row, is the contract's own double (the
sum in ascending order from 0.0, times scale), so the reference forms it in fp64 too and evaluates the term rules on it in
longdouble."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from oracle import pf_oracle as po
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import helpers
from tests import series_loglik_reference as ref
from tests.test_gpu_pf_sites import bits, force_path, observations, sites_batch, snapshot
from tests.test_pf_sites import sites_reference

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
DEV = "cuda"
G, LP = sa.LOGLIK_GAUSS, sa.LOGLIK_LAPLACE
T = 96            # steps of the short forecast the series come from


@functools.lru_cache(maxsize=None)
def base_params():
    return sa.read_params(BASE, sa.flags_from())[0]


_open = []


@functools.lru_cache(maxsize=None)
def forecast(M, n_sites, prec):
    """a batch after its 96-step forecast (series_loglik does not change it: shared) -> (batch, planes, status); member 1
    of site 0 did not run when the site has five members or more"""
    members = synth.perturbed_params(base_params(), n_sites * M, seed=M + n_sites)
    if M >= 5:
        members[1, pi("leafAllocation")] = 0.9
        members[1, pi("woodAllocation")] = 0.9
    b = sites_batch(members, n_sites, prec)
    planes, _ = b.run(0, T)
    _open.append(b)
    return b, planes, b.get_status()


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    forecast.cache_clear()
    while _open:
        _open.pop().close()


def stretched(plane, rows):
    """a synthetic series of `rows` rows in the plane's dtype: the forecast's rows over and over, drifting"""
    k = torch.arange(rows, device=DEV)
    return (plane[k % plane.shape[0]].double() * (1.0 + 0.003 * k.double())[:, None]).to(plane.dtype).contiguous()


def gaps(pattern, n_sites, rows, rng):
    """-> bool [n_sites][rows], True = a gap.  edges: rows 0, 255, 256 and the last; tile: the whole second tile (or the
    first, of a term of one tile) and a third of the rest; all: every row; odd sites take the other of edges / tile, and in
    a batch of several sites `site1` leaves site 1 without any observation"""
    out = np.zeros((n_sites, rows), dtype=bool)
    for s in range(n_sites):
        p = pattern
        if pattern == "site1":
            p = "all" if (s == 1 and n_sites > 1) else "edges"
        elif s % 2 == 1 and pattern in ("edges", "tile"):
            p = "tile" if pattern == "edges" else "edges"
        if p == "edges":
            out[s, [r for r in (0, 255, 256, rows - 1) if r < rows]] = True
            if rows == 1:
                out[s, 0] = False
        elif p == "tile":
            out[s] = rng.random(rows) < 0.33
            out[s, 256:512] = True
            if rows <= 256:
                out[s, :] = rng.random(rows) < 0.5
        elif p == "all":
            out[s] = True
    return out


# a case: (terms, pad, normalise); a term: (source, rows, sum_steps, kind, scale, gap pattern); source: a plane index of the
# forecast (0 NEE, 2 ET) read as it is, or "s0" / "s2": that plane stretched to rows x sum_steps rows
CASES = {
    "r1": ([(0, 1, 96, G, 1.0, "none")], 0, True),
    "r255": ([("s0", 255, 1, LP, 1.0, "site1")], 0, True),
    "r256": ([("s0", 256, 1, G, 1.0, "edges")], 3, False),
    "r257x3": ([("s0", 257, 1, G, 1.0, "edges"), (2, 2, 48, LP, 0.5, "none"), ("s2", 600, 1, LP, 2.0, "tile")], 0, True),
    "r600x3": ([("s0", 600, 1, G, 1.0, "tile"), ("s2", 300, 1, LP, 1.0, "all"), (0, 96, 1, G, 1.0, "edges")], 5, True),
    "r5x48": ([("s2", 5, 48, G, 1e-3, "edges")], 0, True),
}
SHAPES = [(1, 1), (5, 3), (64, 1), (65, 3), (257, 1), (1000, 3)]


def build_terms(case, M, n_sites, prec, bad_site=None):
    """-> (batch, status, sa terms, reference terms, normalise)"""
    b, planes, status = forecast(M, n_sites, prec)
    specs, pad, normalise = CASES[case]
    rng = np.random.default_rng(len(case) + M)
    ncol = n_sites * M
    live = (status == 0).reshape(n_sites, M)
    site_scale = (1.0, 30.0, 1e3)
    sa_terms, ref_terms = [], []
    for q, (src, rows, ss, kind, scale, pattern) in enumerate(specs):
        series = planes[src][:rows * ss] if isinstance(src, int) else stretched(planes[int(src[1])], rows * ss)
        if pad:
            wide = torch.full((rows * ss, ncol + pad), float("nan"), dtype=series.dtype, device=DEV)
            wide[:, :ncol] = series
            series = wide
        host = series[:, :ncol].cpu().numpy()
        raw = host.astype(np.float64).reshape(rows, ss, ncol).sum(axis=1)
        # the unit conversion also brings the modelled values to the scale of the errors below (a power of two times the
        # case's own scale, so r5x48's 1e-3 still rounds): a spread of about 5 between the members
        spread = np.abs(raw[:, live.reshape(-1)]).mean() * 0.1 + 1e-300
        scale = scale * 2.0 ** np.round(np.log2(5.0 / (spread * scale)))
        h = scale * raw
        obs, sd = np.zeros((n_sites, rows)), np.zeros((n_sites, rows))
        for s in range(n_sites):
            hs = h[:, s * M:(s + 1) * M][:, live[s]]
            # obs and sd on scales that differ by orders of magnitude between sites.  sd >= 1 throughout: below 1 / sqrt(2 pi)
            # (Gauss; 1 / 2 for Laplace) a row's constant is positive and cancels against its negative quadratic part, and
            # near those values log sd cancels against the constant's other half -- there the sum of |row terms| no longer
            # bounds the roundings of the parts, for any fp64 evaluation, and the issue's bound says nothing
            sd[s] = site_scale[s % 3] * (1.0 + rng.random(rows))
            obs[s] = np.median(hs, axis=1) + sd[s] * rng.normal(0.0, 1.0, rows)
        gap = gaps(pattern, n_sites, rows, rng)
        obs[gap] = np.nan
        sd[gap] = -1.0                                   # (never read)
        if bad_site is not None and q == len(specs) - 1:
            r = int(np.flatnonzero(~gap[bad_site])[0])
            sd[bad_site, r] = 0.0
        sa_terms.append(sa.loglik_term(series, obs, sd, kind=kind, scale=scale, sum_steps=ss))
        ref_terms.append(ref.Term(host, obs, sd, kind, scale, ss))
    return b, status, sa_terms, ref_terms, normalise


def outputs(b, n_terms):
    return dict(out=torch.full((b.ncol,), 7.0, dtype=torch.float64, device=DEV),
                parts_out=torch.full((n_terms, b.ncol), 7.0, dtype=torch.float64, device=DEV),
                used_out=torch.full((b.n_sites, n_terms), -7, dtype=torch.int32, device=DEV),
                info_out=torch.full((b.n_sites, 2), -7, dtype=torch.int32, device=DEV))


def same_bits(x, y):
    assert len(x) == len(y)
    for u, v in zip(x, y):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        np.testing.assert_array_equal(bits(u) if u.dtype == np.float64 else u, bits(v) if v.dtype == np.float64 else v)


# ---- 1. against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M,n_sites", SHAPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_against_the_reference(case, M, n_sites, prec):
    bad_site = n_sites - 1 if (case == "r600x3" and n_sites > 1) else None
    b, status, terms, ref_terms, normalise = build_terms(case, M, n_sites, prec, bad_site)
    o = outputs(b, len(terms))
    b.series_loglik(terms, normalise=normalise, **o)
    want = ref.series_loglik(ref_terms, n_sites, status, normalise)
    got = o["out"].cpu().numpy()
    np.testing.assert_array_equal(o["used_out"].cpu().numpy(), want.used)
    np.testing.assert_array_equal(o["info_out"].cpu().numpy(), want.info)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want.loglik))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want.loglik))
    fin = np.isfinite(want.loglik.astype(np.float64))
    assert np.isfinite(got[fin]).all() and not np.isposinf(got).any()
    n_used = np.repeat(want.info[:, 1], M).astype(np.longdouble)
    bound = (n_used + 16) * np.longdouble(2.0) ** -53 * want.abs_sum
    with np.errstate(invalid="ignore"):                  # (-inf - -inf of a member that did not run)
        err = np.abs(got.astype(np.longdouble) - want.loglik)
    if fin.any():
        worst = int(np.argmax(np.where(fin, err - bound, -np.inf)))
        print(f"{case} M={M} sites={n_sites}: worst err {float(err[worst]):.3e} bound {float(bound[worst]):.3e} "
              f"value {got[worst]:.6e} used {int(n_used[worst])}")
    assert (err[fin] <= bound[fin]).all()
    if bad_site is not None:
        assert want.info[bad_site, 0] == -2 and np.isnan(got[bad_site * M:]).all()
    if case == "r255" and n_sites > 1:
        assert want.info[1, 0] == -1 and (got[M:2 * M] == 0.0).all()
    # the parts: each term's own sum, by the same bound with that term's rows
    parts = o["parts_out"].cpu().numpy()
    for q in range(len(terms)):
        one = ref.series_loglik([ref_terms[q]], n_sites, status, normalise)
        ok = np.isfinite(want.loglik.astype(np.float64))
        bq = (np.repeat(one.info[:, 1], M) + 16) * np.longdouble(2.0) ** -53 * one.abs_sum
        with np.errstate(invalid="ignore"):
            assert (np.abs(parts[q].astype(np.longdouble) - one.loglik)[ok] <= bq[ok]).all(), q


# ---- 2. the same bits whatever the path, the call, the aliasing -----------------------------------------------------------
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("case,M,n_sites", [("r257x3", 65, 3), ("r600x3", 257, 1), ("r600x3", 1000, 3), ("r1", 5, 3),
                                            ("r256", 1, 1), ("r5x48", 64, 1)])
def test_paths_repeats_and_aliasing_give_the_same_bits(case, M, n_sites, prec):
    bad_site = n_sites - 1 if (case == "r600x3" and n_sites > 1) else None
    b, status, terms, _, normalise = build_terms(case, M, n_sites, prec, bad_site)
    res = []
    for path in (1, 2, 0, 2):
        o = outputs(b, len(terms))
        b.series_loglik(terms, normalise=normalise, path=path, **o)
        res.append([o[k] for k in ("out", "parts_out", "used_out", "info_out")])
    for other in res[1:]:
        same_bits(res[0], other)
    add = torch.linspace(-3.0, 5.0, b.ncol, dtype=torch.float64, device=DEV)
    apart, parts = {}, {}
    for path in (1, 2):
        o = outputs(b, len(terms))
        b.series_loglik(terms, normalise=normalise, add=add, path=path, **o)
        apart[path], parts[path] = o["out"], o["parts_out"]
        alias = add.clone()
        assert b.series_loglik(terms, normalise=normalise, add=alias, out=alias, info_out=o["info_out"], path=path) is alias
        same_bits([apart[path]], [alias])
    same_bits([apart[1], parts[1]], [apart[2], parts[2]])
    total = torch.zeros(b.ncol, dtype=torch.float64, device=DEV)
    for q in range(len(terms)):
        total = total + parts[1][q]
    total = total + add
    got, want = apart[1].cpu().numpy(), total.cpu().numpy()
    dead = status != 0
    site_bad = np.isnan(res[0][0].cpu().numpy())
    np.testing.assert_array_equal(bits(got[~dead & ~site_bad]), bits(want[~dead & ~site_bad]))
    assert np.isneginf(got[dead & ~site_bad]).all() and np.isnan(got[site_bad]).all()


# ---- 3. chained with the existing filter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["group", "split"])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 5, 1000, 4096])
@pytest.mark.parametrize("n_sites", [1, 3, 32])
def test_one_gauss_row_is_the_existing_filter(n_sites, M, prec, path):
    """one Gauss term of one row over the window, scale 1, no constants = pf_analysis_sites' log-weights; pf_resample_sites
    on them with the same u0 = its ancestors, integer weights, totals, and the batch afterwards"""
    members = synth.perturbed_params(base_params(), n_sites * M, seed=n_sites + M)
    if M >= 5:
        members[2, pi("leafAllocation")] = 0.9
        members[2, pi("woodAllocation")] = 0.9
    twins = [sites_batch(members, n_sites, prec) for _ in range(2)]
    planes = [b.run(0, 48)[0] for b in twins]
    for b in twins:
        force_path(b, path)
    obs, sig = observations(planes[0][0], n_sites, far=n_sites - 1)
    u0 = (np.arange(n_sites) * 0.377 + 0.05) % 1.0
    t1 = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    t2 = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    anc1, logw1, fixed1 = twins[0].pf_analysis_sites(planes[0][0], obs, sig, u0, with_params=True, total_out=t1, return_fixed=True)
    term = sa.loglik_term(planes[1][0], obs, sig, sum_steps=48)
    logw2 = twins[1].series_loglik([term], normalise=False)
    np.testing.assert_array_equal(logw2.cpu().numpy(), logw1.cpu().numpy())          # (the signs of zero may differ)
    if n_sites == 1:
        np.testing.assert_array_equal(logw2.cpu().numpy(), twins[1].pf_log_weights(planes[1][0], obs[0], sig[0]).cpu().numpy())
    anc2, fixed2 = twins[1].pf_resample_sites(logw2, u0, with_params=True, total_out=t2, return_fixed=True)
    assert twins[1].pf_info()["fused"] == twins[0].pf_info()["fused"] == (1 if path == "group" else 0)
    assert torch.equal(anc1, anc2) and torch.equal(fixed1, fixed2) and torch.equal(t1, t2)
    assert (t1 > 0).all()
    s1, s2 = snapshot(twins[0], prec), snapshot(twins[1], prec)
    np.testing.assert_array_equal(s1[0], s2[0])
    np.testing.assert_array_equal(s1[1][:, :49], s2[1][:, :49])     # (ring slots no step has written are uninitialised)
    np.testing.assert_array_equal(s1[2], s2[2])
    for b in twins:
        b.close()


# ---- 4. the resampling alone ----------------------------------------------------------------------------------------------
def synthetic_logw(n_sites, M, seed):
    """log-weights whose spread differs from site to site; site 0 lies a million log-units lower; a NaN and a -inf"""
    rng = np.random.default_rng(seed)
    lw = np.concatenate([rng.normal(0.0, (0.3, 2.0, 6.0)[s % 3], M) for s in range(n_sites)])
    lw[:M] -= 1e6
    if M > 4:
        lw[3] = np.nan
        lw[M + 4 if n_sites > 1 else 4] = -np.inf
    return lw


def dev(x):
    return torch.tensor(x, dtype=torch.float64, device=DEV)


def resample_batch(n_sites, M, path):
    b = sites_batch(synth.perturbed_params(base_params(), n_sites * M, seed=11), n_sites, sa.F64)
    b.run(0, 48)
    force_path(b, path)
    return b


@pytest.mark.parametrize("n_sites,M", [(4, 300), (3, 5), (2, 5000)])
def test_resampling_from_given_weights(n_sites, M):
    lw = synthetic_logw(n_sites, M, seed=M)
    u0 = (np.arange(n_sites) * 0.61 + 0.13) % 1.0
    nan_as_inf = np.where(np.isnan(lw), -np.inf, lw)
    per_path = []
    for path in ("group", "split"):
        b = resample_batch(n_sites, M, path)
        total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
        ess = torch.full((n_sites,), -7.0, dtype=torch.float64, device=DEV)
        logw = dev(lw)
        anc, fixed = b.pf_resample_sites(logw, u0, with_params=True, total_out=total, ess_out=ess, return_fixed=True)
        assert b.pf_info()["fused"] == (1 if path == "group" and M <= 4096 else 0)
        np.testing.assert_array_equal(bits(logw.cpu().numpy()), bits(lw))       # without ess_min the log-weights stay
        anc, fixed, total, ess = anc.cpu().numpy(), fixed.cpu().numpy(), total.cpu().numpy(), ess.cpu().numpy()
        want_fx, _, _ = sites_reference(nan_as_inf, n_sites, u0)
        assert np.abs(fixed - want_fx).max() <= 1                               # device exp vs glibc exp: one unit
        assert (fixed[np.isnan(lw) | np.isneginf(lw)] == 0).all()               # a NaN weighs nothing
        want_anc, want_tot, want_ess, _ = ref.resample_reference(lw, n_sites, u0, fixed)
        np.testing.assert_array_equal(anc, want_anc)
        np.testing.assert_array_equal(total, want_tot)
        assert (total > 0).all() and (anc // M == np.arange(n_sites * M) // M).all()
        np.testing.assert_allclose(ess, [float(e) for e in want_ess], rtol=1e-14)
        per_path.append((anc, fixed, total, bits(ess)))
        # tempering: beta = 0.25 is the call on 0.25 * logw
        a1, f1 = b.pf_resample_sites(dev(lw), u0, beta=np.full(n_sites, 0.25), return_fixed=True)
        a2, f2 = b.pf_resample_sites(dev(lw) * 0.25, u0, return_fixed=True)
        assert torch.equal(a1, a2) and torch.equal(f1, f2)
        # the keep rule: even sites lie above their threshold and keep their particles, odd sites below and resample
        ess_min = np.where(np.arange(n_sites) % 2 == 0, ess * 0.5, ess * 2.0)
        before = snapshot(b, sa.F64)
        logw = dev(lw)
        tot = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
        anc = b.pf_resample_sites(logw, u0, ess_min=ess_min, with_params=True, total_out=tot)
        after = snapshot(b, sa.F64)
        anc, tot, logw = anc.cpu().numpy(), tot.cpu().numpy(), logw.cpu().numpy()
        want_anc, want_tot, _, want_lw = ref.resample_reference(lw, n_sites, u0, fixed, ess_min=ess_min)
        np.testing.assert_array_equal(anc, want_anc)
        np.testing.assert_array_equal(tot, want_tot)
        np.testing.assert_array_equal(bits(logw), bits(want_lw))
        for s in range(n_sites):
            sl = slice(s * M, (s + 1) * M)
            if s % 2 == 0:
                assert tot[s] == -3
                np.testing.assert_array_equal(anc[sl], np.arange(s * M, (s + 1) * M))
                np.testing.assert_array_equal(after[0][sl], before[0][sl])
                np.testing.assert_array_equal(after[1][sl], before[1][sl])
                np.testing.assert_array_equal(after[2][:, sl], before[2][:, sl])
            else:
                assert tot[s] > 0 and (logw[sl] == 0.0).all()
        b.close()
    for x, y in zip(*per_path):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("path", ["group", "split"])
def test_sites_that_weigh_nothing_or_have_bad_arguments(path):
    """site 0: nobody weighs anything (total 0); site 1: a +inf log-weight; 2: u0 = 1; 3: beta = 0; 4: fine.  -2: identity
    ancestors and the total, nothing else of the site is written."""
    n_sites, M = 5, 300
    b = resample_batch(n_sites, M, path)
    lw = synthetic_logw(n_sites, M, seed=2)
    lw[:M] = -np.inf
    lw[M + 7] = np.inf
    u0 = np.array([0.1, 0.2, 1.0, 0.4, 0.5])
    beta = np.array([1.0, 1.0, 1.0, 0.0, 0.5])
    logw = torch.tensor(lw, dtype=torch.float64, device=DEV)
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    ess = torch.full((n_sites,), -7.0, dtype=torch.float64, device=DEV)
    before = snapshot(b, sa.F64)
    anc, fixed = b.pf_resample_sites(logw, u0, beta=beta, ess_min=np.zeros(n_sites) + 1e9, with_params=True, total_out=total,
                                     ess_out=ess, return_fixed=True)
    after = snapshot(b, sa.F64)
    anc, total, ess = anc.cpu().numpy(), total.cpu().numpy(), ess.cpu().numpy()
    np.testing.assert_array_equal(total[:4], [0, -2, -2, -2])
    assert total[4] > 0 and ess[0] == 0.0 and 1.0 <= ess[4] <= M
    np.testing.assert_array_equal(ess[1:4], [-7.0] * 3)
    np.testing.assert_array_equal(anc[:4 * M], np.arange(4 * M))
    np.testing.assert_array_equal(bits(logw[:4 * M].cpu().numpy()), bits(lw[:4 * M]))
    assert (logw[4 * M:] == 0).all()
    for k in range(3):
        x, y = (before[k][:4 * M], after[k][:4 * M]) if k < 2 else (before[k][:, :4 * M], after[k][:, :4 * M])
        np.testing.assert_array_equal(x, y)
    # an ess_min that is NaN is a bad argument of its site too
    bad_min = np.array([1.0, 1.0, 1.0, 1.0, np.nan])
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    b.pf_resample_sites(dev(lw), u0, beta=beta, ess_min=bad_min, total_out=total)
    assert total.cpu().numpy()[4] == -2
    # the synchronous form: -2 is a bad argument, else 0 a bad parameter, naming the site; nothing is resampled
    before = snapshot(b, sa.F64)
    with pytest.raises(sa.SipnetError) as e:
        b.pf_resample_sites(torch.tensor(lw, dtype=torch.float64, device=DEV), u0, beta=beta, with_params=True)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 1" in str(e.value) and "sipnet_batch_pf_resample_sites" in str(e.value)
    lw[M + 7] = 0.0
    with pytest.raises(sa.SipnetError) as e:
        b.pf_resample_sites(torch.tensor(lw, dtype=torch.float64, device=DEV), [0.1, 0.2, 0.3, 0.4, 0.5], with_params=True)
    assert e.value.code == _lib.ERR_BAD_PARAMETER and "site 0" in str(e.value)
    for x, y in zip(before, snapshot(b, sa.F64)):
        np.testing.assert_array_equal(x, y)
    b.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_of_series_loglik():
    L = sa.lib()
    b, planes, status = forecast(64, 1, sa.F64)
    nee = planes[0]
    obs, sd = np.zeros((1, T)), np.ones((1, T))
    good = sa.loglik_term(nee, obs, sd)
    with pytest.raises(ValueError):
        b.series_loglik([])
    with pytest.raises(ValueError):
        b.series_loglik([good] * 9)
    with pytest.raises(ValueError):                                   # ld < ncol
        b.series_loglik([sa.loglik_term(nee[:, :63].contiguous(), obs, sd)])
    with pytest.raises(ValueError):                                   # rows that are no multiple of sum_steps
        b.series_loglik([sa.loglik_term(nee, obs, sd, sum_steps=7)])
    with pytest.raises(ValueError):                                   # obs of another length
        b.series_loglik([sa.loglik_term(nee, obs[:, :5], sd)])
    with pytest.raises(ValueError):                                   # terms of two dtypes
        b.series_loglik([good, sa.loglik_term(nee.float(), obs, sd)])
    with pytest.raises(ValueError):
        b.series_loglik([good], out=torch.zeros(63, dtype=torch.float64, device=DEV))
    for bad in (dict(scale=float("inf")), dict(scale=float("nan"))):
        with pytest.raises(sa.SipnetError) as e:
            b.series_loglik([sa.loglik_term(nee, obs, sd, **bad)])
        assert e.value.code == _lib.ERR_BAD_ARGUMENT and "term 0" in str(e.value)
    with pytest.raises(sa.SipnetError) as e:
        b.series_loglik([good], path=3)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT
    # the C boundary itself
    d_obs = torch.zeros(T, dtype=torch.float64, device=DEV)
    d_sd = torch.ones(T, dtype=torch.float64, device=DEV)
    out = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)

    def call(n_terms=1, ld=64, out_ptr=out.data_ptr(), **fields):
        t = _lib.LoglikTerm(nee.data_ptr(), d_obs.data_ptr(), d_sd.data_ptr(), T, 1, G, 0, 1.0)
        for k, v in fields.items():
            setattr(t, k, v)
        arr = (_lib.LoglikTerm * 9)(*([t] * 9))
        return L.sipnet_batch_series_loglik(b.h, n_terms, arr, 0, ld, 1, 0, None, C.c_void_p(out_ptr), None, None, None, b._stream())

    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert (out != 7.0).all()
    out.fill_(7.0)
    for kw in (dict(n_terms=0), dict(n_terms=9), dict(ld=63), dict(out_ptr=None), dict(kind=2), dict(kind=-1), dict(rows=0),
               dict(sum_steps=0), dict(d_series=None), dict(d_obs=None), dict(d_sd=None)):
        assert call(**kw) == _lib.ERR_BAD_ARGUMENT, kw
        assert b"sipnet_batch_series_loglik" in L.sipnet_last_error()
    assert L.sipnet_batch_series_loglik(b.h, 1, None, 0, 64, 1, 0, None, C.c_void_p(out.data_ptr()), None, None, None,
                                        b._stream()) == _lib.ERR_BAD_ARGUMENT
    # a batch that was not set up: its members' status cannot be read
    raw = sa.Batch(sa.flags_from(), 1, 64, sa.F64, fast_math=True)
    with pytest.raises(sa.SipnetError) as e:
        raw.series_loglik([good])
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "set up" in str(e.value)
    raw.close()
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_the_synchronous_form_names_the_bad_site_and_term():
    b, planes, status = forecast(65, 3, sa.F64)
    obs, sd = np.zeros((3, T)), np.ones((3, T))
    obs[1, 3] = np.nan
    sd[1, 3] = -1.0                                                 # a gap's sd is not looked at
    fine = sa.loglik_term(planes[0], obs, sd)
    out = torch.full((b.ncol,), 7.0, dtype=torch.float64, device=DEV)
    b.series_loglik([fine, fine], out=out)
    assert not torch.isnan(out).any() and (out != 7.0).all()
    out.fill_(7.0)
    for what in ("sd", "obs"):
        o2, s2 = obs.copy(), sd.copy()
        if what == "sd":
            s2[2, 40] = np.inf
        else:
            o2[2, 40] = -np.inf
        with pytest.raises(sa.SipnetError) as e:
            b.series_loglik([fine, sa.loglik_term(planes[2], o2, s2, kind=LP)], out=out)
        assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 2, term 1" in str(e.value), str(e.value)
        assert (out == 7.0).all()                                   # nothing was written
        info = torch.zeros((3, 2), dtype=torch.int32, device=DEV)  # asynchronous: the site's columns become NaN
        b.series_loglik([fine, sa.loglik_term(planes[2], o2, s2, kind=LP)], out=out, info_out=info)
        np.testing.assert_array_equal(info.cpu().numpy(), [[1, 2 * T], [1, 2 * T - 2], [-2, 2 * T - 1]])
        assert torch.isnan(out[130:]).all() and not torch.isnan(out[:130]).any()
        out.fill_(7.0)


def test_refusals_of_pf_resample_sites():
    L = sa.lib()
    b = resample_batch(2, 64, "group")
    logw = torch.zeros(128, dtype=torch.float64, device=DEV)
    u0 = torch.full((2,), 0.5, dtype=torch.float64, device=DEV)
    anc = torch.empty(128, dtype=torch.int32, device=DEV)
    full = [logw.data_ptr(), u0.data_ptr(), anc.data_ptr()]
    for k in range(3):
        a = [C.c_void_p(x) for x in full]
        a[k] = None
        assert L.sipnet_batch_pf_resample_sites(b.h, a[0], a[1], None, None, 0, a[2], None, None, None, b._stream()) == _lib.ERR_BAD_ARGUMENT, k
    for bad in (dict(logw=logw[:127]), dict(logw=logw.float()), dict(u0=[0.5]), dict(beta=[1.0]), dict(ess_min=[1.0, 2.0, 3.0]),
                dict(total_out=torch.zeros(3, dtype=torch.int64, device=DEV)), dict(ess_out=torch.zeros(2, dtype=torch.float32, device=DEV))):
        kw = dict(logw=logw, u0=[0.5, 0.5])
        kw.update(bad)
        with pytest.raises(ValueError):
            b.pf_resample_sites(**kw)
    b.close()
    c = sites_batch(synth.perturbed_params(base_params(), 64, seed=1), 1, sa.F64)
    c.run(0, 48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.pf_resample_sites(logw[:64].contiguous(), [0.5])
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "connected" in str(e.value)
    c.close()
