"""The particle-filter analysis of a batch of many sites on the GPU (sipnet_batch_pf_analysis_sites): every site resampled
over its own columns, against the per-site oracle (tests/test_pf_sites.py: oracle/pf_oracle.py site by site); one site
against sipnet_batch_pf_analysis bit for bit; forecast -> analysis cycles whose particles continue like their ancestors;
sites without an observation, with bad arguments or with no surviving particle; the one-workgroup-per-site kernel against the
split path; the refusals."""
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
from tests.test_pf_sites import sites_reference

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
DEV = "cuda"


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


@functools.lru_cache(maxsize=None)
def site_clim(s):
    """every site its own forcing"""
    return synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(48 * 8, site=s)))


def force_path(b, path):
    """after the forecast: "group" -- one workgroup per site (the batch believes the device has one CU, so that the sites
    fill it), "split" -- the three-launch path"""
    if path == "group":
        b.debug_set_num_cus(1)
    else:
        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)


def sites_batch(members, n_sites, prec, kernel_options=0):
    M = members.shape[0] // n_sites
    b = sa.Batch(sa.flags_from(), n_sites, M, prec, fast_math=True, kernel_options=kernel_options)
    for s in range(n_sites):
        b.set_climate(s, site_clim(s))
        b.set_params(s, members[s * M:(s + 1) * M])
    b.setup()
    return b


def observations(nee, n_sites, far=None):
    """per-site obs and sigma on scales that differ by orders of magnitude; site `far`'s best particle sits at -1e6"""
    tot = nee.double().sum(0).cpu().numpy().reshape(n_sites, -1)
    obs, sig = np.zeros(n_sites), np.zeros(n_sites)
    for s in range(n_sites):
        t = tot[s][np.isfinite(tot[s])]
        if t.size == 0:                      # (nobody of the site ran)
            t = np.zeros(1)
        sd = float(t.std()) if t.size > 1 and t.std() > 0 else abs(float(t[0])) * 0.1 + 1e-3
        if s == far:
            sig[s] = 2000.0 * sd
            obs[s] = float(t.min()) - sig[s] * np.sqrt(2e6)
        else:
            sig[s] = sd * (0.5, 1.0, 2.0, 4.0)[s % 4]
            obs[s] = float(np.median(t)) + 0.5 * sd * (s % 3 - 1)
    return obs, sig


def everyone(n):
    return torch.arange(n, dtype=torch.int32, device=DEV)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def snapshot(b, prec):
    """state, rings (bit patterns) and the parameters as the particles carry them"""
    w = 32 + (125 if prec == sa.F32_MIXED else 250)
    return bits(b.get_state()), bits(b.get_rings()), b.pack_members(everyone(b.ncol), True)[w:].cpu().numpy()


@pytest.mark.parametrize("path", ["group", "split"])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 5, 1000, 4096])
@pytest.mark.parametrize("n_sites", [1, 3, 32])
def test_every_site_resamples_over_its_own_columns(base, n_sites, M, prec, path):
    members = synth.perturbed_params(base, n_sites * M, seed=n_sites + M)
    b = sites_batch(members, n_sites, prec)
    planes, _ = b.run(0, 48)
    nee = planes[0]
    force_path(b, path)
    far = n_sites - 1
    obs, sig = observations(nee, n_sites, far)
    u0 = (np.arange(n_sites) * 0.377 + 0.05) % 1.0
    status = b.get_status()
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    anc, logw, fixed = b.pf_analysis_sites(nee, obs, sig, u0, with_params=True, total_out=total, return_fixed=True)
    assert b.pf_info()["fused"] == (1 if path == "group" else 0)
    anc, logw, fixed, total = anc.cpu().numpy(), logw.cpu().numpy(), fixed.cpu().numpy(), total.cpu().numpy()
    nee_np = nee.cpu().numpy()
    b.close()
    want_lw = np.concatenate([po.log_weights(nee_np[:, s * M:(s + 1) * M], obs[s], sig[s], status[s * M:(s + 1) * M])
                              for s in range(n_sites)])
    ok = np.isfinite(want_lw)
    assert (np.isfinite(logw) == ok).all()
    np.testing.assert_allclose(logw[ok], want_lw[ok], rtol=1e-13, atol=1e-13)
    want_fx, _, _ = sites_reference(want_lw, n_sites, u0)
    assert np.abs(fixed - want_fx).max() <= 1                      # device exp vs glibc exp: one unit
    _, want_anc, want_tot = sites_reference(logw, n_sites, u0, fixed=fixed)
    np.testing.assert_array_equal(anc, want_anc)                   # exact, given the device's integers
    np.testing.assert_array_equal(total, want_tot)
    assert (total > 0).all()
    site_of = np.arange(n_sites * M) // M
    assert (anc // M == site_of).all()                             # no ancestor leaves its site
    # the far-off site: its best particle at -1e6, and it still resamples (a single maximum over all sites leaves it nothing)
    lw_far = logw[far * M:(far + 1) * M]
    assert -1.01e6 < lw_far.max() < -0.99e6
    if n_sites > 1:
        with np.errstate(over="ignore", invalid="ignore"):
            assert po.fixed_weights(logw)[far * M:].sum() == 0
    if M >= 1000:
        assert 1 < len(np.unique(anc[far * M:(far + 1) * M])) < M


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_one_site_equals_the_one_site_call(base, prec):
    """n_sites = 1: log-weights, ancestors, total weight and the state, rings and parameters afterwards are
    sipnet_batch_pf_analysis's, bit for bit"""
    n = 1000
    members = synth.perturbed_params(base, n, seed=3)
    members[17, pi("leafAllocation")] = 0.9            # status 3: weight -inf
    members[17, pi("woodAllocation")] = 0.9
    twins = [sites_batch(members, 1, prec) for _ in range(2)]
    planes = [b.run(0, 96)[0] for b in twins]
    assert torch.equal(planes[0], planes[1])
    nee = planes[0][0]
    tot = nee.double().sum(0)
    obs, sigma = float(tot[torch.isfinite(tot)].median()), float(tot[torch.isfinite(tot)].std()) * 0.7
    t1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    t2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    anc1, logw1 = twins[0].pf_analysis_local(nee, obs, sigma, 0.37, with_params=True, total_out=t1)
    anc2, logw2 = twins[1].pf_analysis_sites(planes[1][0], [obs], [sigma], [0.37], with_params=True, total_out=t2)
    assert torch.equal(logw1.view(torch.int64), logw2.view(torch.int64))
    assert torch.equal(anc1, anc2) and torch.equal(t1, t2) and int(t1.item()) > 0
    assert 1 < int(torch.unique_consecutive(anc1).numel()) < n
    s1, s2 = snapshot(twins[0], prec), snapshot(twins[1], prec)
    np.testing.assert_array_equal(s1[0], s2[0])
    # (ring slots no step has written yet are uninitialised memory: slot 0 and the 96 inserts)
    np.testing.assert_array_equal(s1[1][:, :97], s2[1][:, :97])
    np.testing.assert_array_equal(s1[2], s2[2])
    p1, _ = twins[0].run(96, 96)
    p2, _ = twins[1].run(96, 96)
    assert torch.equal(p1, p2)
    for b in twins:
        b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("with_params", [True, False])
def test_cycles_continue_like_their_ancestors(base, prec, with_params):
    """4 sites x 256 particles: forecast 96 -> analysis -> forecast 96 -> analysis -> forecast 96.  The planes and the
    carried state equal an unfiltered twin's columns at the composed ancestors, bit for bit."""
    n_sites, M, T = 4, 256, 96
    n = n_sites * M
    if with_params:
        members = synth.perturbed_params(base, n, seed=8)
    else:   # state-only filter: particles differ in their initial pools (see test_gpu_pf.py)
        rng = np.random.default_rng(4)
        members = np.tile(base, (n, 1))
        for name in ("plantWoodInit", "soilInit", "litterInit", "soilWFracInit", "laiInit"):
            members[:, pi(name)] *= np.exp(rng.normal(0, 0.1, n))
        members[:, pi("soilWFracInit")] = np.clip(members[:, pi("soilWFracInit")], 0.05, 1.0)
    twin = sites_batch(members, n_sites, prec)
    twin_planes = [twin.run(k * T, T)[0].cpu().numpy() for k in range(3)]
    twin_state = twin.get_state()
    twin.close()
    b = sites_batch(members, n_sites, prec)
    lineage = np.arange(n)
    for k in range(3):
        p, _ = b.run(k * T, T)
        np.testing.assert_array_equal(p.cpu().numpy(), twin_planes[k][:, :, lineage])
        if k == 2:
            break
        obs, sig = observations(p[0], n_sites)
        anc, _ = b.pf_analysis_sites(p[0], obs, sig, [0.43, 0.1, 0.77, 0.5], with_params=with_params)
        anc = anc.cpu().numpy()
        assert (anc // M == np.arange(n) // M).all()
        assert any(1 < len(np.unique(anc[s * M:(s + 1) * M])) < M for s in range(n_sites))   # the filter did select
        lineage = lineage[anc]
    np.testing.assert_array_equal(b.get_state()[:, :28], twin_state[lineage][:, :28])
    b.close()


def _special_case_batch(base, prec, n_sites=3, M=256, collapsed=None):
    members = synth.perturbed_params(base, n_sites * M, seed=21)
    if collapsed is not None:
        members[collapsed * M:(collapsed + 1) * M, pi("leafAllocation")] = 0.9     # status 3 for the whole site
        members[collapsed * M:(collapsed + 1) * M, pi("woodAllocation")] = 0.9
    b = sites_batch(members, n_sites, prec)
    planes, _ = b.run(0, 48)
    return b, planes[0]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_a_site_without_an_observation_keeps_its_particles(base, prec):
    M = 256
    b, nee = _special_case_batch(base, prec)
    obs, sig = observations(nee, 3)
    obs[1] = np.nan
    before = snapshot(b, prec)
    total = torch.zeros(3, dtype=torch.int64, device=DEV)
    anc, logw, fixed = b.pf_analysis_sites(nee, obs, sig, [0.2, 0.3, 0.4], with_params=True, total_out=total,
                                           return_fixed=True)
    after = snapshot(b, prec)
    total, anc = total.cpu().numpy(), anc.cpu().numpy()
    assert total[1] == -1 and total[0] > 0 and total[2] > 0
    np.testing.assert_array_equal(anc[M:2 * M], np.arange(M, 2 * M))
    assert (logw[M:2 * M] == 0).all() and (fixed[M:2 * M] == 0).all()
    site1 = slice(M, 2 * M)
    np.testing.assert_array_equal(after[0][site1], before[0][site1])
    np.testing.assert_array_equal(after[1][site1], before[1][site1])
    np.testing.assert_array_equal(after[2][:, site1], before[2][:, site1])
    for s in (0, 2):
        assert 1 < len(np.unique(anc[s * M:(s + 1) * M])) < M
    # the synchronous call: no observation is no error
    b.pf_analysis_sites(nee, obs, sig, [0.2, 0.3, 0.4], with_params=True)
    b.close()


@pytest.mark.parametrize("bad", ["sigma0", "sigma_inf", "u0"])
def test_a_site_with_bad_arguments(base, bad):
    """synchronous: SipnetError (SIPNET_ERR_BAD_ARGUMENT) naming the site, the whole batch untouched; asynchronous: -2 and
    identity for that site, the others resampled"""
    M, prec = 256, sa.F64
    b, nee = _special_case_batch(base, prec)
    obs, sig = observations(nee, 3)
    u0 = np.array([0.2, 0.3, 0.4])
    if bad == "sigma0":
        sig[2] = 0.0
    elif bad == "sigma_inf":
        sig[2] = np.inf
    else:
        u0[2] = 1.0
    before = snapshot(b, prec)
    with pytest.raises(sa.SipnetError) as e:
        b.pf_analysis_sites(nee, obs, sig, u0, with_params=True)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "site 2" in str(e.value)
    after = snapshot(b, prec)
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    total = torch.zeros(3, dtype=torch.int64, device=DEV)
    anc, _ = b.pf_analysis_sites(nee, obs, sig, u0, with_params=True, total_out=total)
    total, anc = total.cpu().numpy(), anc.cpu().numpy()
    assert total[2] == -2 and total[0] > 0 and total[1] > 0
    np.testing.assert_array_equal(anc[2 * M:], np.arange(2 * M, 3 * M))
    assert 1 < len(np.unique(anc[:M])) < M
    b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_a_site_with_no_surviving_particle(base, prec):
    """every member of site 0 has invalid allocations (status 3): synchronous SIPNET_ERR_BAD_PARAMETER with nothing
    resampled; asynchronous total 0 and identity for that site while the others resample"""
    M = 256
    b, nee = _special_case_batch(base, prec, collapsed=0)
    st = b.get_status()
    assert (st[:M] != 0).all() and (st[M:] == 0).all()
    obs, sig = observations(nee, 3)
    obs[0], sig[0] = 0.0, 1.0
    before = snapshot(b, prec)
    with pytest.raises(sa.SipnetError) as e:
        b.pf_analysis_sites(nee, obs, sig, [0.2, 0.3, 0.4], with_params=True)
    assert e.value.code == _lib.ERR_BAD_PARAMETER and "site 0" in str(e.value)
    after = snapshot(b, prec)
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    total = torch.zeros(3, dtype=torch.int64, device=DEV)
    anc, logw = b.pf_analysis_sites(nee, obs, sig, [0.2, 0.3, 0.4], with_params=True, total_out=total)
    total, anc = total.cpu().numpy(), anc.cpu().numpy()
    assert total[0] == 0 and total[1] > 0 and total[2] > 0
    assert torch.isinf(logw[:M]).all()
    np.testing.assert_array_equal(anc[:M], np.arange(M))
    assert 1 < len(np.unique(anc[M:2 * M])) < M
    b.close()


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("n_sites,M", [(3, 1000), (32, 64), (2, 4096), (5, 1)])
def test_the_split_path_gives_the_same_bits(base, prec, n_sites, M):
    """the three-launch path (SIPNET_KOPT_PF_MULTI_LAUNCH forces it for every site) gives the same log-weights, integer
    weights, ancestors, totals and resampled batch as one workgroup per site -- also with a site without an observation, one
    with a bad sigma and one with no surviving particle"""
    members = synth.perturbed_params(base, n_sites * M, seed=M)
    if n_sites >= 3:
        members[:M, pi("leafAllocation")] = 0.9
        members[:M, pi("woodAllocation")] = 0.9
    res = []
    for path in ("group", "split"):
        b = sites_batch(members, n_sites, prec)
        p, _ = b.run(0, 48)
        force_path(b, path)
        obs, sig = observations(p[0], n_sites)
        if n_sites >= 3:
            obs[0], sig[0] = 0.0, 1.0
            obs[1] = np.nan
            sig[2] = -1.0
        total = torch.zeros(n_sites, dtype=torch.int64, device=DEV)
        anc, logw, fixed = b.pf_analysis_sites(p[0], obs, sig, (np.arange(n_sites) * 0.61) % 1.0, with_params=True,
                                               total_out=total, return_fixed=True)
        info = b.pf_info()
        assert info["fused"] == (1 if path == "group" else 0), info
        res.append((anc.cpu().numpy(), bits(logw.cpu().numpy()), fixed.cpu().numpy(), total.cpu().numpy()) + snapshot(b, prec))
        b.close()
    for x, y in zip(res[0], res[1]):
        np.testing.assert_array_equal(x, y)
    if n_sites >= 3:
        np.testing.assert_array_equal(res[0][3][:3], [0, -1, -2])


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [65536, 300007])
def test_a_big_site_takes_the_split_path_and_equals_the_one_site_call(base, prec, M):
    """(65 536: 256 chunks of 256 columns; 300 007: 586 chunks of 512, the last one ragged)"""
    members = synth.perturbed_params(base, M, seed=65)
    twins = [sites_batch(members, 1, prec) for _ in range(2)]
    planes = [b.run(0, 48)[0] for b in twins]
    nee = planes[0][0]
    tot = nee.double().sum(0)
    obs, sigma = float(tot.median()), float(tot.std()) * 0.5
    t1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    t2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    anc1, logw1 = twins[0].pf_analysis_local(nee, obs, sigma, 0.29, with_params=True, total_out=t1)
    anc2, logw2, fixed = twins[1].pf_analysis_sites(planes[1][0], [obs], [sigma], [0.29], with_params=True, total_out=t2,
                                                    return_fixed=True)
    assert twins[1].pf_info()["fused"] == 0
    assert torch.equal(logw1.view(torch.int64), logw2.view(torch.int64)) and torch.equal(anc1, anc2) and torch.equal(t1, t2)
    _, want, _ = sites_reference(logw2.cpu().numpy(), 1, 0.29, fixed=fixed.cpu().numpy())
    np.testing.assert_array_equal(anc2.cpu().numpy(), want)
    s1, s2 = snapshot(twins[0], prec), snapshot(twins[1], prec)
    np.testing.assert_array_equal(s1[0], s2[0])
    np.testing.assert_array_equal(s1[1][:, :49], s2[1][:, :49])
    np.testing.assert_array_equal(s1[2], s2[2])
    for b in twins:
        b.close()


def test_shape_at_scale_256_sites_of_1024(base):
    """(as many sites as the MI355X has CUs: one workgroup per site by default)"""
    n_sites, M, prec = 256, 1024, sa.F32_MIXED
    members = synth.perturbed_params(base, n_sites * M, seed=256)
    b = sites_batch(members, n_sites, prec)
    p, _ = b.run(0, 48)
    obs, sig = observations(p[0], n_sites, far=77)
    u0 = (np.arange(n_sites) * 0.137 + 0.01) % 1.0
    anc, logw, fixed = b.pf_analysis_sites(p[0], obs, sig, u0, return_fixed=True)
    assert b.pf_info()["fused"] == (1 if n_sites >= torch.cuda.get_device_properties(0).multi_processor_count else 0)
    logw, fixed = logw.cpu().numpy(), fixed.cpu().numpy()
    _, want, _ = sites_reference(logw, n_sites, u0, fixed=fixed)
    np.testing.assert_array_equal(anc.cpu().numpy(), want)
    want_fx, _, _ = sites_reference(logw, n_sites, u0)
    assert np.abs(fixed - want_fx).max() <= 1
    b.close()


def test_refusals(base):
    L = sa.lib()
    members = synth.perturbed_params(base, 2 * 64, seed=1)
    b = sites_batch(members, 2, sa.F64)
    p, _ = b.run(0, 48)
    nee = p[0]
    with pytest.raises(sa.SipnetError) as e:                       # ld < ncol
        b.pf_analysis_sites(nee[:, :127], [0.0, 0.0], [1.0, 1.0], [0.5, 0.5])
    assert e.value.code == _lib.ERR_BAD_ARGUMENT
    d = torch.zeros(2, dtype=torch.float64, device=DEV)
    logw = torch.empty(128, dtype=torch.float64, device=DEV)
    anc = torch.empty(128, dtype=torch.int32, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())                       # noqa: E731
    full = [ptr(nee), ptr(d), ptr(d), ptr(d), ptr(logw), ptr(anc)]
    for k in range(len(full)):                                     # each required pointer NULL in turn
        args = list(full)
        args[k] = None
        rc = L.sipnet_batch_pf_analysis_sites(b.h, args[0], 0, 48, 128, args[1], args[2], args[3], 0, args[4], args[5],
                                              None, None, b._stream())
        assert rc == _lib.ERR_BAD_ARGUMENT, k
    rc = L.sipnet_batch_pf_analysis_sites(b.h, ptr(nee), 0, 0, 128, ptr(d), ptr(d), ptr(d), 0, ptr(logw), ptr(anc),
                                          None, None, b._stream())
    assert rc == _lib.ERR_BAD_ARGUMENT                              # n_steps <= 0
    with pytest.raises(sa.SipnetError) as e:                       # the one-site resampling still refuses many sites
        b.resample(everyone(128), None, (), False)
    assert e.value.code == _lib.ERR_BAD_ARGUMENT
    b.close()
    # a connected batch resamples through sipnet_batch_pf_resample_peers
    c = sites_batch(members[:64], 1, sa.F64)
    p, _ = c.run(0, 48)
    c.pf_connect([c.pf_publish(with_params=True)], 0)
    with pytest.raises(sa.SipnetError) as e:
        c.pf_analysis_sites(p[0], [0.0], [1.0], [0.5])
    assert e.value.code == _lib.ERR_BAD_ARGUMENT and "connected" in str(e.value)
    c.close()
