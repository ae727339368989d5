"""The particle filter's weight and many-site resampling kernels at their edges (pf_weights.inc, pf_sites.inc), with no
allowance wherever the answer is known in advance:

1. pfFixedWeight against an exponential of higher precision (tests/pf_edges_reference.fixed_weight_exact): 2^20 uniform
   points and directed ones under three maxima, alone and through both many-site paths, also tempered;
2. ancestors, totals and effective sample sizes of crafted weights (a thread's first or last slot only, threads and chunks
   that weigh nothing, a last chunk of one column, u0 at the S - 1 clamp) at M next to 256, 512 and kSitesLds on both
   paths and where the split path's chunk doubles;
3. a site does not depend on its neighbours;
4. the keep rule at ess == ess_min;
5. the plane-driven analysis over step counts around logWeightOf's unroll of 8, ld > ncol and both element types.

Not covered: sites of more than 2^21 particles (per = 16 on the split path) and the 2^22 cap -- such a batch takes
gigabytes and its test more than the few seconds a test may take here."""
import functools

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from oracle import pf_oracle as po
from sipnet_amd import dist as sd
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from tests import pf_edges_reference as er
from tests.series_loglik_reference import ess_exact
from tests.test_gpu_pf_sites import BASE, bits, force_path, site_clim, sites_batch, snapshot
from tests.test_pf_sites import sites_reference

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not er.longdouble_is_wide(), reason="np.longdouble has no 64-bit significand on this machine")]
DEV = "cuda"
G = er.G
DEAD = 5          # the member of site 1 with an invalid allocation (batches made with dead=True)
_open = []


@functools.lru_cache(maxsize=None)
def few_rows():
    return synth.perturbed_params(sa.read_params(BASE, sa.flags_from())[0], 7, seed=5)


@functools.lru_cache(maxsize=None)
def edge_batch(n_sites, M, prec=sa.F32_MIXED, dead=False, tag=""):
    """a batch after setup() alone (the resampling needs no forecast), its members a few parameter rows tiled; shared by
    the tests (tag: a batch of its own, e.g. one whose path is never forced)"""
    rows = np.tile(few_rows(), (-(-M // 7), 1))[:M]
    if n_sites <= 3:
        members = np.tile(rows, (n_sites, 1))
        if dead:
            members[M + DEAD, pi("leafAllocation")] = 0.9
            members[M + DEAD, pi("woodAllocation")] = 0.9
        b = sites_batch(members, n_sites, prec)
    else:                                               # (many sites: the same members at every site, one upload)
        b = sa.Batch(sa.flags_from(), n_sites, M, prec, fast_math=True)
        b.set_climates([site_clim(s % 4) for s in range(n_sites)])
        b.set_params(None, rows)
        b.setup()
    _open.append(b)
    return b


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    edge_batch.cache_clear()
    while _open:
        _open.pop().close()
    torch.cuda.empty_cache()


def take_path(b, path):
    """a shared batch onto "group" or "split" (tests/test_gpu_pf_sites.force_path, after whatever was forced before)"""
    b.set_kernel(sa.KERNEL_AUTO, 0)
    force_path(b, path)


def dev(x, dtype=torch.float64):
    return torch.tensor(x, dtype=dtype, device=DEV)


def resample(b, lw, u0, **kw):
    """pf_resample_sites with totals and effective sample sizes -> (anc, fixed, total, ess, logw afterwards, fused) as numpy"""
    total = torch.full((b.n_sites,), -7, dtype=torch.int64, device=DEV)
    ess = torch.full((b.n_sites,), -7.0, dtype=torch.float64, device=DEV)
    logw = dev(lw)
    anc, fixed = b.pf_resample_sites(logw, u0, total_out=total, ess_out=ess, return_fixed=True, **kw)
    fused = b.pf_info()["fused"]
    return anc.cpu().numpy(), fixed.cpu().numpy(), total.cpu().numpy(), ess.cpu().numpy(), logw.cpu().numpy(), fused


def check_ess(ess, fixed, n_sites, what):
    """bit-equal where the exact rational is an integer, else rtol = 1e-14 (tests/test_gpu_series_loglik.py's figure)"""
    M = len(fixed) // n_sites
    for s in range(n_sites):
        want = ess_exact(fixed[s * M:(s + 1) * M])
        if want.denominator == 1:
            assert bits(ess[s:s + 1])[0] == bits(np.array([float(want)]))[0], (what, s, ess[s], want)
        else:
            np.testing.assert_allclose(ess[s], float(want), rtol=1e-14, err_msg=str((what, s)))


def crafted(n_sites, M, layout, rnd, seed=0):
    """the log-weights, integers and u0 of one round (er.rounds): site s holds pattern rnd[s][0] laid out for `layout`"""
    per, chunk, _ = er.geometry(M, layout)
    lw, fx = zip(*[er.pattern(name, M, per, chunk, seed=seed + s) for s, (name, _) in enumerate(rnd)])
    return np.concatenate(lw), np.concatenate(fx), np.array([u for _, u in rnd])


def check_against_patterns(b, n_sites, M, layout, fused, what):
    """every round of crafted weights through the batch's current path: integers, ancestors, totals and effective sample
    sizes as known in advance -> the results, for comparisons between paths"""
    out = []
    for r, rnd in enumerate(er.rounds(n_sites)):
        lw, fx, u0 = crafted(n_sites, M, layout, rnd, seed=M + r)
        anc, fixed, total, ess, lw_after, was_fused = resample(b, lw, u0)
        msg = f"{what}, layout {layout}, round {r}: {rnd}"
        assert was_fused == fused, msg
        np.testing.assert_array_equal(fixed, fx, err_msg=msg)
        _, want_anc, want_tot = sites_reference(lw, n_sites, u0, fixed=fx)     # base + po.systematic_ancestors(fx, u0)
        np.testing.assert_array_equal(anc, want_anc, err_msg=msg)
        np.testing.assert_array_equal(total, want_tot, err_msg=msg)
        check_ess(ess, fx, n_sites, msg)
        np.testing.assert_array_equal(bits(lw_after), bits(lw), err_msg=msg)   # without ess_min the log-weights stay
        out.append((anc, fixed, total, bits(ess)))
    return out


# ---- 1. the fixed-point weight against the high-precision exponential --------------------------------------------------------
C1_SITES, C1_M = 257, 4096


@functools.lru_cache(maxsize=None)
def c1_points(m):
    """-> (lw [257 * 4096], index of the first directed point, want of the directed points): m + x for 2^20 uniform x, the
    directed x behind them, uniform x to fill the last site; every stretch of 4096 holds one entry that is exactly m, so
    that every site of the many-site call has the maximum of the whole array"""
    x = er.uniform_x(1 << 20)
    dx, want = er.directed_x()
    fill = er.uniform_x(C1_SITES * C1_M - len(x) - len(dx), seed=21)
    with np.errstate(invalid="ignore"):
        lw = np.float64(m) + np.concatenate([x, dx, fill])
    at = np.arange(C1_SITES) * C1_M + 64 + (np.arange(C1_SITES) * 37) % (C1_M - 64)
    assert not ((at >= len(x)) & (at < len(x) + len(dx))).any()
    lw[at] = m
    return lw, len(x), want


def compare_with_exact(fixed, lw, m, first_directed, n_directed, what):
    """fixed == the reference wherever the point is not in doubt; where it is, one unit; few are -> (in doubt, differing)"""
    near, d, tol = er.fixed_weight_exact(lw, m)
    sure = d > tol
    bad = np.flatnonzero((fixed != near) & sure)
    assert bad.size == 0, (f"{what}: {bad.size} integers differ from rint(2^30 exp(x)) outside their tolerance; the first: "
                           f"lw {lw[bad[0]]!r}, x {(lw - m).flat[bad[0]]!r}, device {fixed[bad[0]]}, exact {near[bad[0]]}, d {d[bad[0]]:.3e}, "
                           f"tol {tol[bad[0]]:.3e}")
    n_doubt, n_diff = int((~sure).sum()), int((fixed != near).sum())
    report = f"{what}: {n_doubt} of {len(lw)} points within their tolerance of a rounding point, {n_diff} of them differ"
    assert np.abs(fixed - near)[~sure].max(initial=0) <= 1, report
    assert n_doubt <= 1e-4 * len(lw), report
    assert sure[first_directed:first_directed + n_directed].all(), report
    return report


@pytest.mark.parametrize("m", [0.0, -1e6, 700.0])
def test_fixed_weight_against_high_precision_exp(m, capsys):
    lw, nd0, want = c1_points(m)
    m_eff = np.nanmax(lw)                               # (m; 5e-324 under m = 0, where that directed point is the largest)
    assert m_eff == (5e-324 if m == 0.0 else m)
    _, alone = sd.pf_systematic_ancestors(dev(lw), 0.3, return_fixed=True)
    report = compare_with_exact(alone.cpu().numpy(), lw, m_eff, nd0, len(want), f"m = {m}")
    with capsys.disabled():
        print("\n  " + report)
    np.testing.assert_array_equal(alone.cpu().numpy()[nd0:nd0 + len(want)], want)
    # one function serves all, and the many-site paths feed it the site's maximum: the same integers, bit for bit
    b = edge_batch(C1_SITES, C1_M)
    u0 = (np.arange(C1_SITES) * 0.377 + 0.05) % 1.0
    for path in ("group", "split"):
        take_path(b, path)
        _, fixed, total, _, _, fused = resample(b, lw, u0)
        assert fused == (1 if path == "group" else 0)
        assert np.array_equal(fixed, alone.cpu().numpy()), (path, m, int((fixed != alone.cpu().numpy()).sum()))
        np.testing.assert_array_equal(total, fixed.reshape(C1_SITES, C1_M).sum(axis=1))
        # tempered: the reference forms fl(beta * lw) first, and the maximum is that of the products
        _, tempered, _, _, _, _ = resample(b, lw, u0, beta=np.full(C1_SITES, 0.25))
        prod = (0.25 * lw).reshape(C1_SITES, C1_M)
        m_site = np.repeat(np.nanmax(prod, axis=1), C1_M)
        compare_with_exact(tempered, prod.reshape(-1), m_site, nd0, len(want), f"m = {m}, beta = 0.25, {path}")


# ---- 2. crafted weights: ancestors, totals and effective sample sizes known in advance ------------------------------------------
@pytest.mark.parametrize("M", er.GROUP_M)
def test_crafted_weights_on_both_paths(M):
    """3 sites of M particles, patterns laid out for the group path's slots and for the split path's, each through both
    paths: everything as known in advance, and the two paths bit for bit"""
    n_sites = 3
    b = edge_batch(n_sites, M)
    res = {}
    for path in ("group", "split"):
        take_path(b, path)
        for layout in ("group", "split"):
            res[path, layout] = check_against_patterns(b, n_sites, M, layout, 1 if path == "group" else 0, f"M = {M}, path {path}")
    for layout in ("group", "split"):
        for g, s in zip(res["group", layout], res["split", layout]):
            for x, y in zip(g, s):
                np.testing.assert_array_equal(x, y)


def test_crafted_weights_just_above_the_lds_limit():
    """4097 = kSitesLds + 1: the split path, forced and by the library's own choice (a batch nothing was forced on)"""
    n_sites, M = 3, 4097
    forced = edge_batch(n_sites, M)
    take_path(forced, "split")
    a = check_against_patterns(forced, n_sites, M, "split", 0, "M = 4097, forced")
    b = check_against_patterns(edge_batch(n_sites, M, tag="auto"), n_sites, M, "split", 0, "M = 4097, unforced")
    for g, s in zip(a, b):
        for x, y in zip(g, s):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("M", er.BIG_M)
def test_crafted_weights_where_the_chunk_doubles(M):
    """one site: 262 144 = 1024 chunks of 256 (every chunk prefix in use); 262 145 = 513 chunks of 512, 524 289 = 513 chunks
    of 1024, both with a last chunk of one column"""
    check_against_patterns(edge_batch(1, M), 1, M, "split", 0, f"M = {M}")


# ---- 3. a site does not depend on its neighbours --------------------------------------------------------------------------------
@pytest.mark.parametrize("M,path", [(257, "group"), (257, "split"), (4097, "split")])
def test_a_site_does_not_depend_on_its_neighbours(M, path):
    per, chunk, _ = er.geometry(M, path)
    mine, mine_fx = er.pattern("slot_ends", M, per, chunk)
    u_mine = 0.377

    def run(b, names, u0, site):
        lw = np.concatenate([mine if n == "mine" else er.pattern(n, M, per, chunk, seed=3)[0] for n in names])
        anc, fixed, total, ess, _, _ = resample(b, lw, u0)
        sl = slice(site * M, (site + 1) * M)
        return anc[sl] - site * M, fixed[sl], total[site:site + 1], bits(ess[site:site + 1])

    b3 = edge_batch(3, M, sa.F64)
    take_path(b3, path)
    hood_a = ("uniform", "mine", "two_giants")
    hood_b = ("last_chunk_only", "mine", "sparse")
    in_a = run(b3, hood_a, [0.5, u_mine, 0.0], 1)
    in_b = run(b3, hood_b, [1.0 - 2.0 ** -53, u_mine, 5e-324], 1)
    b1 = edge_batch(1, M, sa.F64)
    take_path(b1, path)
    alone = run(b1, ("mine",), [u_mine], 0)
    np.testing.assert_array_equal(in_a[1], mine_fx)
    np.testing.assert_array_equal(in_a[0], po.systematic_ancestors(mine_fx, u_mine))
    for other in (in_b, alone):
        for x, y in zip(in_a, other):
            np.testing.assert_array_equal(x, y)
    # a site with u0 = 1 (a bad argument: total -2) between two good ones: they are as they were with a good neighbour ...
    good = [run(b3, hood_a, [0.5, u_mine, 0.0], s) for s in (0, 2)]
    b3.setup()
    before = snapshot(b3, sa.F64)
    lw = np.concatenate([mine if n == "mine" else er.pattern(n, M, per, chunk, seed=3)[0] for n in hood_a])
    anc, fixed, total, ess, lw_after, _ = resample(b3, lw, [0.5, 1.0, 0.0])
    after = snapshot(b3, sa.F64)
    for k, s in enumerate((0, 2)):
        sl = slice(s * M, (s + 1) * M)
        for x, y in zip(good[k], (anc[sl] - s * M, fixed[sl], total[s:s + 1], bits(ess[s:s + 1]))):
            np.testing.assert_array_equal(x, y)
    # ... and nothing of it is touched: identity, its log-weights, state, rings and parameters
    mid = slice(M, 2 * M)
    assert total[1] == -2 and ess[1] == -7.0
    np.testing.assert_array_equal(anc[mid], np.arange(M, 2 * M))
    np.testing.assert_array_equal(bits(lw_after), bits(lw))
    np.testing.assert_array_equal(after[0][mid], before[0][mid])
    np.testing.assert_array_equal(after[1][mid], before[1][mid])
    np.testing.assert_array_equal(after[2][:, mid], before[2][:, mid])


# ---- 4. the keep rule at equality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,path", [(300, "group"), (300, "split"), (4097, "split")])
def test_the_keep_rule_at_equality(M, path):
    """k giants and nothing else: the effective sample size is exactly k.  The three sites hold k = 1, 7 and M."""
    ks = np.array([1, 7, M])
    per, chunk, _ = er.geometry(M, path)
    lw, fx = zip(*[er.pattern("k_giants", M, per, chunk, seed=s, k=int(k)) for s, k in enumerate(ks)])
    lw, fx = np.concatenate(lw), np.concatenate(fx)
    u0 = np.array([0.377, 1.0 - 2.0 ** -53, 0.0])
    b = edge_batch(3, M)
    take_path(b, path)
    identity = np.arange(3 * M)
    _, want_anc, want_tot = sites_reference(lw, 3, u0, fixed=fx)
    np.testing.assert_array_equal(want_tot, ks * G)

    def kept(ess_min, what):
        anc, fixed, total, ess, lw_after, _ = resample(b, lw, u0, ess_min=ess_min)
        np.testing.assert_array_equal(bits(ess), bits(ks.astype(np.float64)), err_msg=what)
        np.testing.assert_array_equal(fixed, fx, err_msg=what)
        np.testing.assert_array_equal(total, [-3] * 3, err_msg=what)
        np.testing.assert_array_equal(anc, identity, err_msg=what)
        np.testing.assert_array_equal(bits(lw_after), bits(lw), err_msg=what)

    def resampled(ess_min, what):
        anc, fixed, total, ess, lw_after, _ = resample(b, lw, u0, ess_min=ess_min)
        np.testing.assert_array_equal(bits(ess), bits(ks.astype(np.float64)), err_msg=what)
        np.testing.assert_array_equal(fixed, fx, err_msg=what)
        np.testing.assert_array_equal(total, ks * G, err_msg=what)
        np.testing.assert_array_equal(anc, want_anc, err_msg=what)
        np.testing.assert_array_equal(bits(lw_after), bits(np.zeros(3 * M)), err_msg=what)

    anc, fixed, total, ess, _, fused = resample(b, lw, u0)            # no ess_min: every site resamples
    assert fused == (1 if path == "group" else 0)
    np.testing.assert_array_equal(bits(ess), bits(ks.astype(np.float64)))
    np.testing.assert_array_equal(anc, want_anc)
    kept(ks.astype(np.float64), "ess_min = k: ess >= ess_min holds with equality")
    resampled(np.nextafter(ks.astype(np.float64), np.inf), "ess_min = the next double above k")
    kept(np.full(3, -np.inf), "ess_min = -inf")
    resampled(np.full(3, np.inf), "ess_min = +inf")


# ---- 5. the plane-driven analysis: step tail, stride and element type -----------------------------------------------------------
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("ld_extra", [0, 3])
@pytest.mark.parametrize("n_steps", [1, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("M", [257, 4097])
def test_analysis_of_a_cancelling_plane(M, n_steps, ld_extra, prec):
    """three sites whose plane columns sum (large rows cancelling) to crafted targets; site 1's targets lie 3 lower and its
    member DEAD -- an invalid allocation, so weight 0 -- has the one column that would be the best of the site"""
    n_sites, ncol = 3, 3 * M
    dtype = np.float64 if prec == sa.F64 else np.float32
    b = edge_batch(n_sites, M, prec, dead=True)
    for path in (("group", "split") if M <= er.SITES_LDS else ("split",)):
        per, chunk, _ = er.geometry(M, path)
        names = ("two_giants", "ones_and_a_giant", "thread_gaps")
        tg, fx = zip(*[er.pattern(n, M, per, chunk, seed=n_steps) for n in names])
        tg, fx = [t.copy() for t in tg], [f.copy() for f in fx]
        tg[1] -= 3.0
        tg[1][DEAD], fx[1][DEAD] = 0.0, 0
        fx = np.concatenate(fx)
        plane = er.cancelling_plane(np.concatenate(tg), n_steps, ncol + ld_extra, dtype, seed=n_steps + M)
        u0 = np.array(er.U0S)[(np.arange(3) + n_steps) % len(er.U0S)]
        b.setup()                                       # (an earlier resampling has replaced the dead member by its ancestor)
        take_path(b, path)
        status = b.get_status()
        assert status[M + DEAD] != 0 and (np.delete(status, M + DEAD) == 0).all()
        total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
        anc, logw, fixed = b.pf_analysis_sites(torch.from_numpy(plane).to(DEV), [0.0] * 3, [1.0] * 3, u0, total_out=total,
                                               return_fixed=True)
        what = f"path {path}"
        assert b.pf_info()["fused"] == (1 if path == "group" else 0), what
        anc, logw, fixed, total = anc.cpu().numpy(), logw.cpu().numpy(), fixed.cpu().numpy(), total.cpu().numpy()
        want_lw = np.concatenate([po.log_weights(plane[:, s * M:(s + 1) * M], 0.0, 1.0, status[s * M:(s + 1) * M])
                                  for s in range(n_sites)])
        with np.errstate(invalid="ignore"):             # (the test's own construction: the oracle's integers are the crafted ones)
            np.testing.assert_array_equal(sites_reference(want_lw, n_sites, u0)[0], fx)
        assert logw[M + DEAD] == -np.inf and want_lw[M + DEAD] == -np.inf
        ok = np.isfinite(want_lw)
        assert ok.sum() == ncol - 1 and np.isfinite(logw[ok]).all(), what     # nobody has read a pad column (1e300 / 3e38)
        same = np.array_equal(bits(logw), bits(want_lw))
        what += ", log-weights bit-equal to the oracle's" if same else ", log-weights NOT bit-equal to the oracle's"
        np.testing.assert_allclose(logw[ok], want_lw[ok], rtol=1e-13, atol=1e-13, err_msg=what)
        assert same, what                               # (every sum is exact and so is the rest: measured bit-equal throughout)
        np.testing.assert_array_equal(fixed, fx, err_msg=what)                 # site 1's maximum came from the others
        _, want_anc, want_tot = sites_reference(want_lw, n_sites, u0, fixed=fx)
        np.testing.assert_array_equal(anc, want_anc, err_msg=what)
        np.testing.assert_array_equal(total, want_tot, err_msg=what)
