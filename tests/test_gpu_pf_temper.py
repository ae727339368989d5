"""sipnet_batch_pf_temper_sites on the device (Batch.pf_temper_sites).  The yardstick is pf_resample_sites' effective sample
size (ess_out), code that was there before: one site's log-likelihoods copied into 15 sites of a batch, one call with beta =
b_1 .. b_15 gives a round's 15 ESS values, and eight such calls drive tests/pf_temper_reference.search -- the device's step,
bracket end, ESS and code must equal that replay bit for bit.  Then: the step gives the filter exactly the ESS it was chosen
for; both paths give the same bits; every code; a site does not depend on its neighbours; and against a longdouble ESS of
real weights the step keeps the target within a derived margin."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from tests import pf_temper_reference as tr
from tests.test_gpu_pf_sites import BASE, bits, force_path, site_clim

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit significand on this machine")]
DEV = "cuda"
BAD = _lib.ERR_BAD_ARGUMENT
N_PROBE = tr.SECTIONS - 1  # the sites of a batch: one per candidate of a round
GROUP_M = (255, 256, 257, 1000, 4096)
SPLIT_M = (257, 4097, 16385)
SHAPES = [("group", M) for M in GROUP_M] + [("split", M) for M in SPLIT_M]
TINY = 2.0 ** -40
# the sites of a subject batch: (scale of the -0.5 chi^2-like log-likelihoods, delta_max, target as a fraction of the live
# members; "dead": nobody weighs anything).  Scales 1, 30, 3000 put the root near 1, 1e-2, 1e-4; 3e13 under delta_max = 2^-40.
SPECS = [(1.0, 1.0, 0.7), (30.0, 1.0, 0.5), (3000.0, 1.0, 0.5), (1.0, 0.25, 0.9), (30.0, 0.25, 0.3), (3000.0, 0.25, 0.5),
         (3e13, TINY, 0.5), (1.0, TINY, 0.5), (30.0, 1.0, 0.999), (3000.0, 1.0, 0.01), (30.0, 1.0, 1.0 + 2.0 ** -40),
         ("dead", 1.0, 0.5), (3e13, 1.0, 0.5), (1.0, 1.0, 0.2), (30.0, 0.25, 0.99)]
_open = []
worst = {"lo": 0.0, "hi": 0.0}   # test 6: the largest fraction of the margin seen


@functools.lru_cache(maxsize=None)
def few_rows():
    return synth.perturbed_params(sa.read_params(BASE, sa.flags_from())[0], 7, seed=5)


@functools.lru_cache(maxsize=None)
def batch_of(n_sites, M):
    """a batch after setup() alone (nothing here needs a forecast), the same few members at every site"""
    b = sa.Batch(sa.flags_from(), n_sites, M, sa.F64, fast_math=True)
    b.set_climates([site_clim(s % 4) for s in range(n_sites)])
    b.set_params(None, np.tile(few_rows(), (-(-M // 7), 1))[:M])
    b.setup()
    _open.append(b)
    return b


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    batch_of.cache_clear()
    while _open:
        _open.pop().close()
    torch.cuda.empty_cache()
    print("\npf_temper: worst fraction of the real-arithmetic margin: lo %.3g, hi %.3g" % (worst["lo"], worst["hi"]))


def take_path(b, path):
    b.set_kernel(sa.KERNEL_AUTO, 0)
    force_path(b, path)


def dev(x, dtype=torch.float64):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV)


def site_loglik(M, scale, seed):
    """one site's log-likelihoods, some members -inf and NaN"""
    if scale == "dead":
        ll = np.full(M, -np.inf)
        ll[1::3] = np.nan
        return ll
    rng = np.random.default_rng(seed)
    ll = -0.5 * scale * rng.chisquare(3, M)
    ll[3::17] = -np.inf
    ll[5::29] = np.nan
    return ll


@functools.lru_cache(maxsize=None)
def subject(M):
    """-> (loglik [15 M], delta_max [15], target [15]) of a subject batch, by SPECS"""
    ll = np.concatenate([site_loglik(M, sc, seed=1000 * M + s) for s, (sc, _, _) in enumerate(SPECS)])
    live = np.isfinite(ll).reshape(N_PROBE, M).sum(1)
    dmax = np.array([dm for _, dm, _ in SPECS])
    target = np.array([max(fr * n, 1.0) for (_, _, fr), n in zip(SPECS, live)])
    for a in (ll, dmax, target):
        a.setflags(write=False)
    return ll, dmax, target


def temper(b, ll, target, base=None, dmax=None, out=None, info=True):
    """pf_temper_sites -> (delta, delta_hi, ess, info [n_sites][2], fused) as numpy"""
    inf = torch.full((b.n_sites, 2), -7, dtype=torch.int32, device=DEV) if info else None
    d, h, e = b.pf_temper_sites(ll if torch.is_tensor(ll) else dev(ll), target, base=base, delta_max=dmax, out=out, info_out=inf)
    fused = b.pf_info()["fused"]
    return d.cpu().numpy(), h.cpu().numpy(), e.cpu().numpy(), (inf.cpu().numpy() if info else None), fused


def filter_ess(b, logw, beta=None):
    """the yardstick: pf_resample_sites' effective sample sizes of logw (a tensor, not written) under beta"""
    ess = torch.full((b.n_sites,), -7.0, dtype=torch.float64, device=DEV)
    total = torch.zeros(b.n_sites, dtype=torch.int64, device=DEV)       # (given: a site that weighs nothing does not raise)
    b.pf_resample_sites(logw, np.zeros(b.n_sites), beta=beta, total_out=total, ess_out=ess)
    return ess.cpu().numpy()


def fma(d, x, y):
    """fl(d x + y), one rounding"""
    if not (np.isfinite(d) and np.isfinite(x) and np.isfinite(y)):
        with np.errstate(invalid="ignore"):
            return float(np.float64(d) * np.float64(x) + np.float64(y))
    return float(Fraction(float(d)) * Fraction(float(x)) + Fraction(float(y)))


def probe(b, ll_site, base_site=None):
    """-> the callable of pf_temper_reference.search that asks the filter: the site's columns in all 15 sites of b, one
    call per list of steps.  Without base, ESS(0) is the number of members with a finite log-likelihood (every one of them
    weighs 2^30; the filter refuses beta = 0); with base the host forms fl(d loglik + base) exactly."""
    M = len(ll_site)
    tiled = dev(np.tile(ll_site, N_PROBE))

    def ess(ds):
        ds = np.asarray(ds, dtype=np.float64)
        padded = np.concatenate([ds, np.full(N_PROBE - len(ds), ds[0])])
        if base_site is not None:
            v = np.array([[fma(d, x, y) for x, y in zip(ll_site, base_site)] for d in ds])
            v = np.concatenate([v, np.tile(v[:1], (N_PROBE - len(ds), 1))])
            return filter_ess(b, dev(v.reshape(-1)))[:len(ds)]
        if len(ds) == 1 and ds[0] == 0.0:
            return np.array([float(np.isfinite(ll_site).sum())])
        return filter_ess(b, tiled, beta=padded)[:len(ds)]
    assert M == b.n_members
    return ess


def same(a, b):
    return bits(np.asarray(a, dtype=np.float64)).tolist() == bits(np.asarray(b, dtype=np.float64)).tolist()


# ---- 1. exact replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,M", SHAPES)
def test_the_search_is_the_replay_through_the_filter(path, M):
    b = batch_of(N_PROBE, M)
    ll, dmax, target = subject(M)
    take_path(b, path)
    d, h, e, info, fused = temper(b, ll, target, dmax=dmax)
    assert fused == (1 if path == "group" else 0)
    codes = set()
    for s, (scale, _, _) in enumerate(SPECS):
        site = ll[s * M:(s + 1) * M]
        want = tr.search(probe(b, site), dmax[s], target[s])
        got = (int(info[s, 0]), d[s], h[s], e[s])
        assert got[0] == want[0] and same(got[1:], want[1:]), (path, M, s, got, want)
        assert info[s, 1] == np.isfinite(site).sum()
        codes.add(want[0])
    assert codes == {tr.FOUND, tr.END, tr.NO_WEIGHT, tr.UNREACHABLE}


@pytest.mark.parametrize("path", ["group", "split"])
def test_the_search_over_carried_weights_is_the_replay(path):
    M = 257
    b = batch_of(N_PROBE, M)
    ll, dmax, _ = subject(M)
    rng = np.random.default_rng(9)
    base = -rng.chisquare(2, N_PROBE * M)
    base[7::31] = -np.inf
    base[11::37] = np.nan
    take_path(b, path)
    e0 = filter_ess(b, dev(np.where(np.isfinite(ll), base, np.nan)))
    target = np.maximum(0.6 * e0, 1.0)
    d, h, e, info, fused = temper(b, ll, target, base=dev(base), dmax=dmax)
    assert fused == 0                                  # (carried weights always take the launches per chunk and stage)
    for s in (0, 1, 2, 5, 6, 11, 12):                  # (12: the root lies below delta_max 2^-32, the step stays 0 and ess is ESS(0))
        sl = slice(s * M, (s + 1) * M)
        want = tr.search(probe(b, ll[sl], base[sl]), dmax[s], target[s])
        got = (int(info[s, 0]), d[s], h[s], e[s])
        assert got[0] == want[0] and same(got[1:], want[1:]), (path, s, got, want)
        with np.errstate(invalid="ignore"):
            assert info[s, 1] == np.isfinite(0.0 * ll[sl] + base[sl]).sum()
    assert d[12] == 0.0 and info[12, 0] == tr.FOUND and same(e[12], e0[12])
    # a target that cannot be reached: every site reports its ESS(0), the filter's over the carried weights
    d, h, e, info, _ = temper(b, ll, np.where(e0 > 0, 1.5 * e0, 1.0), base=dev(base), dmax=dmax)
    assert (info[e0 > 0, 0] == tr.UNREACHABLE).all() and same(e, e0) and (d == 0).all() and (h == 0).all()


# ---- 2. consistency with the filter -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,M", SHAPES)
def test_the_step_gives_the_filter_the_ess_it_was_chosen_for(path, M):
    b = batch_of(N_PROBE, M)
    ll, dmax, target = subject(M)
    take_path(b, path)
    d, h, e, info, _ = temper(b, ll, target, dmax=dmax)
    code = info[:, 0]
    moved = (code > 0) & (d > 0)           # (a root below delta_max 2^-32 leaves the step at 0, which the filter refuses as beta)
    assert moved.sum() >= 10 and (code == tr.FOUND).sum() >= 6
    at_lo = filter_ess(b, dev(ll), beta=np.where(moved, d, 1.0))
    at_hi = filter_ess(b, dev(ll), beta=np.where(code > 0, h, 1.0))
    assert same(at_lo[moved], e[moved]) and (e[moved] >= target[moved]).all()
    found = code == tr.FOUND
    assert (at_hi[found] < target[found]).all() and (h[found] > d[found]).all()
    assert (h[found] - d[found] <= dmax[found] * 16.0 ** -8 * (1 + 2.0 ** -40)).all()


@pytest.mark.parametrize("path,M", [("group", 1000), ("group", 4096), ("split", 4097)])
def test_with_carried_weights_the_tempered_weights_give_the_filter_that_ess(path, M):
    b = batch_of(N_PROBE, M)
    ll, dmax, _ = subject(M)
    rng = np.random.default_rng(M)
    base = -rng.chisquare(2, N_PROBE * M)
    base[7::31] = -np.inf
    take_path(b, path)
    e0 = filter_ess(b, dev(np.where(np.isfinite(ll), base, np.nan)))
    target = np.maximum(0.6 * e0, 1.0)
    out = torch.full((N_PROBE * M,), -7.0, dtype=torch.float64, device=DEV)
    d, h, e, info, _ = temper(b, ll, target, base=dev(base), dmax=dmax, out=out)
    moved = np.repeat(info[:, 0] > 0, M)
    assert (info[:, 0] > 0).sum() >= 10
    got = out.cpu().numpy()
    assert (got[~moved] == -7.0).all()                                     # (codes 0, -1: what was there stays)
    with np.errstate(invalid="ignore"):
        near = np.repeat(d, M) * ll + base
    fin = moved & np.isfinite(near)
    np.testing.assert_allclose(got[fin], near[fin], rtol=4e-16, atol=0)     # (one rounding against two)
    assert same(filter_ess(b, out)[info[:, 0] > 0], e[info[:, 0] > 0])
    inplace = dev(base)                                                    # out is base
    d2, h2, e2, info2, _ = temper(b, ll, target, base=inplace, dmax=dmax, out=inplace)
    assert same(d2, d) and same(h2, h) and same(e2, e) and (info2 == info).all()
    assert same(inplace.cpu().numpy()[moved], got[moved]) and same(inplace.cpu().numpy()[~moved], base[~moved])


# ---- 3. the paths agree, 5. a site does not depend on its neighbours -------------------------------------------------------
def all_outputs(b, ll, target, dmax, base=None):
    out = torch.full((len(ll),), -7.0, dtype=torch.float64, device=DEV)
    d, h, e, info, fused = temper(b, ll, target, base=None if base is None else dev(base), dmax=dmax, out=out)
    return (d, h, e, info.astype(np.float64), out.cpu().numpy()), fused


@pytest.mark.parametrize("with_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("M", [257, 4096, 4097, 16385])
def test_both_paths_give_the_same_bits(M, with_base):
    b = batch_of(N_PROBE, M)
    ll, dmax, target = subject(M)
    base = -np.random.default_rng(M + 1).chisquare(2, len(ll)) if with_base else None
    if with_base:
        target = 0.5 * target
    if M <= 4096:
        take_path(b, "group")
    else:
        b.set_kernel(sa.KERNEL_AUTO, 0)     # (sites this large take the per-chunk launches unforced)
    one, fused = all_outputs(b, ll, target, dmax, base)
    assert fused == (1 if M <= 4096 and not with_base else 0)
    take_path(b, "split")
    two, fused = all_outputs(b, ll, target, dmax, base)
    assert fused == 0
    for x, y in zip(one, two):
        assert same(x, y)
    assert (one[3][:, 0] == tr.FOUND).sum() >= 5


@pytest.mark.parametrize("with_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("path,M", [("group", 1000), ("split", 1000), ("split", 4097)])
def test_a_site_alone_and_among_neighbours(path, M, with_base):
    many, alone = batch_of(8, M), batch_of(1, M)
    ll, dmax, target = subject(M)
    ll, dmax, target = ll[:8 * M], dmax[:8], target[:8]
    base = -np.random.default_rng(M + 2).chisquare(2, len(ll)) if with_base else None
    take_path(many, path)
    take_path(alone, path)
    full, _ = all_outputs(many, ll, target, dmax, base)
    for s in (1, 4, 6):
        sl = slice(s * M, (s + 1) * M)
        own, _ = all_outputs(alone, ll[sl], target[s:s + 1], dmax[s:s + 1], None if base is None else base[sl])
        for x, y in zip(own[:4], full[:4]):
            assert same(x[0], y[s]), (path, M, s)
        assert same(own[4], full[4][sl])


# ---- 4. the codes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,M", [("group", 1000), ("split", 1000), ("split", 4097)])
def test_the_codes_at_their_edges(path, M):
    b = batch_of(N_PROBE, M)
    ll, _, _ = subject(M)
    ll = ll.copy()
    live = np.isfinite(ll).reshape(N_PROBE, M).sum(1).astype(np.float64)
    dmax = np.array([1.0, 0.25, TINY] * 5)
    take_path(b, path)
    at_end = filter_ess(b, dev(ll), beta=dmax)
    dead = live == 0
    # the target IS the ESS at delta_max: the end is reached; one ulp above: not any more
    target = np.where(dead, 1.0, at_end)
    d, h, e, info, _ = temper(b, ll, target, dmax=dmax)
    assert (info[~dead, 0] == tr.END).all() and same(d[~dead], dmax[~dead]) and same(h[~dead], dmax[~dead]) and same(e[~dead], at_end[~dead])
    assert (info[dead, 0] == tr.NO_WEIGHT).all() and (d[dead] == 0).all() and (h[dead] == 0).all() and (e[dead] == 0).all()
    above = np.nextafter(at_end, np.inf)
    reach = ~dead & (above <= live)
    d, h, e, info, _ = temper(b, ll, np.where(dead, 1.0, above), dmax=dmax)
    assert (info[reach, 0] == tr.FOUND).all() and (d[reach] < dmax[reach]).all() and (e[reach] >= above[reach]).all()
    # the target one ulp above ESS(0): not reachable; at ESS(0): reachable
    out = torch.full((len(ll),), -7.0, dtype=torch.float64, device=DEV)
    target = np.where(dead, 1.0, np.nextafter(live, np.inf))
    d, h, e, info = temper(b, ll, target, dmax=dmax, out=out)[:4]
    assert (info[~dead, 0] == tr.UNREACHABLE).all() and (d == 0).all() and (h == 0).all() and same(e[~dead], live[~dead])
    assert (out.cpu().numpy() == -7.0).all()                                # (codes 0 and -1 write no log-weights)
    d, h, e, info = temper(b, ll, np.where(dead, 1.0, live), dmax=dmax)[:4]
    assert (info[~dead, 0] > 0).all()


BAD_CAUSES = ["delta_max 0", "delta_max -1", "delta_max inf", "delta_max nan", "target 0", "target -3", "target nan", "loglik +inf",
              "base +inf"]


@pytest.mark.parametrize("path,M", [("group", 1000), ("split", 1000), ("split", 4097)])
def test_bad_input_is_one_site_s_own(path, M):
    b = batch_of(N_PROBE, M)
    ll0, dmax0, target0 = subject(M)
    base0 = -np.random.default_rng(M + 3).chisquare(2, len(ll0))
    take_path(b, path)
    clean, _ = all_outputs(b, ll0, 0.5 * target0, dmax0, base0)
    for k, cause in enumerate(BAD_CAUSES):
        s = 1 + k
        ll, dmax, target, base = ll0.copy(), dmax0.copy(), 0.5 * target0, base0.copy()
        what, value = cause.split()
        if what == "delta_max":
            dmax[s] = float(value)
        elif what == "target":
            target[s] = float(value)
        elif what == "loglik":
            ll[s * M + M - 1] = np.inf
        else:
            base[s * M + 3] = np.inf
        got, _ = all_outputs(b, ll, target, dmax, base)
        assert got[3][s].tolist() == [tr.BAD_INPUT, 0] and got[0][s] == 0 and got[1][s] == 0 and got[2][s] == 0, cause
        assert (got[4][s * M:(s + 1) * M] == -7.0).all(), cause
        others = np.arange(N_PROBE) != s
        for x, y in zip(got[:4], clean[:4]):
            assert same(x[others], y[others]), cause
        assert same(got[4][np.repeat(others, M)], clean[4][np.repeat(others, M)]), cause
        # the synchronous form: the site is named, nothing is written
        out = torch.full((len(ll),), -7.0, dtype=torch.float64, device=DEV)
        with pytest.raises(sa.SipnetError) as err:
            b.pf_temper_sites(dev(ll), target, base=dev(base), delta_max=dmax, out=out)
        assert err.value.code == BAD and ("site %d:" % s) in str(err.value), cause
        assert (out.cpu().numpy() == -7.0).all()
    d, h, e = b.pf_temper_sites(dev(ll0), 0.5 * target0, base=dev(base0), delta_max=dmax0)     # (clean input: no info needed)
    assert same(d.cpu().numpy(), clean[0]) and same(h.cpu().numpy(), clean[1]) and same(e.cpu().numpy(), clean[2])


# ---- 6. against real arithmetic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("path,M", SHAPES)
def test_against_a_longdouble_ess_of_real_weights(path, M, with_base):
    """Each integer weight is within 0.5 + 1e-6 units of 2^30 e^x (tests/test_gpu_pf_edges.py) and the largest is 2^30, so S is
    off by at most about M 2^-31 of itself and sum w^2 by M 2^-30, the ESS by M 2^-29; the margin is twice that."""
    b = batch_of(N_PROBE, M)
    ll, dmax, target = subject(M)
    base = None
    if with_base:
        base = -np.random.default_rng(M + 4).chisquare(2, len(ll))
        target = 0.5 * target
    take_path(b, path)
    d, h, e, info, _ = temper(b, ll, target, base=None if base is None else dev(base), dmax=dmax)
    margin = M * 2.0 ** -28
    seen = 0
    for s in range(N_PROBE):
        if info[s, 0] <= 0:
            continue
        sl = slice(s * M, (s + 1) * M)
        bs = None if base is None else base[sl]
        at_lo = tr.ess_real(d[s], ll[sl], bs)
        frac = float((target[s] - at_lo) / (target[s] * margin))
        worst["lo"] = max(worst["lo"], frac)
        print("pf_temper margin: %s M=%d base=%d site %d code %d: lo %.3g" % (path, M, with_base, s, info[s, 0], frac), end="")
        assert at_lo >= target[s] * (1 - margin), (s, frac)
        if info[s, 0] == tr.FOUND:
            at_hi = tr.ess_real(h[s], ll[sl], bs)
            frac = float((at_hi - target[s]) / (target[s] * margin))
            worst["hi"] = max(worst["hi"], frac)
            print(", hi %.3g" % frac, end="")
            assert at_hi < target[s] * (1 + margin), (s, frac)
            seen += 1
        print()
    assert seen >= 5


# ---- 7. the binding's refusals ----------------------------------------------------------------------------------------------
def test_the_binding_refuses():
    M = 256
    b = batch_of(2, M)
    b.set_kernel(sa.KERNEL_AUTO, 0)
    ll = dev(site_loglik(2 * M, 30.0, seed=1))
    good = dict(loglik=ll, ess_target=[100.0, 100.0])
    b.pf_temper_sites(**good)
    for change in (dict(loglik=ll.float()), dict(loglik=ll[:-1]), dict(loglik=ll.cpu()), dict(loglik=None), dict(base=ll.float()),
                   dict(base=ll.cpu()), dict(base=ll[:M]), dict(out=ll.cpu()), dict(out=ll[1:]), dict(out=ll.to(torch.float32)),
                   dict(ess_target=[100.0]), dict(ess_target=None), dict(delta_max=[1.0, 1.0, 1.0]),
                   dict(info_out=torch.zeros(4, dtype=torch.int64, device=DEV)), dict(info_out=torch.zeros(3, dtype=torch.int32, device=DEV)),
                   dict(info_out=torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="pf_temper_sites"):
            b.pf_temper_sites(**{**good, **change})
    c = sa.Batch(sa.flags_from(), 1, 64, sa.F64, fast_math=True)      # a batch connected across ranks
    c.set_climates([site_clim(0)])
    c.set_params(None, np.tile(few_rows(), (10, 1))[:64])
    c.setup()
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.pf_temper_sites(ll[:64].contiguous(), [10.0])
    assert e.value.code == BAD and "connected" in str(e.value)
    c.close()
