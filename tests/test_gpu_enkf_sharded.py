"""The EnKF analysis of an ensemble sharded by member across ranks on the GPU (sipnet_batch_enkf_shard_moments,
sipnet_batch_enkf_analysis_sharded, sipnet_amd.dist.enkf_analysis_sharded).  All but the last test run on one GPU in one
process: the k shards are k batches on the device and the "all-gather" is a torch.stack of their moment tensors.  The inputs are
crafted, not forecast (tests/enkf_gpu_common.crafted, as tests/test_gpu_enkf_edges.py): pools around 100 with unit spread, so
no limit is near, but for one member pushed under the biomass rule.

The shards' results, put back into the union's layout (tests/enkf_sharded_reference.interleave), are held to the member-space
reference over the union ensemble (tests/enkf_reference.analysis) under within()'s 1e-10; the conditioning set to the
extended-precision update under max(1e-10, 4 x own_error(merged_chain64 cut as the test cuts, case)).

Conditioning, what could not be carried: a crafted batch has 13 pool slots and 3 planes to carry a case in.  The 4-row cases fit
(3 analysed pools, 4 rows).  A 16-row case needs 3 + 16 carriers and there are 16, so the 16-row cases run here on their first
10 rows (7 pool slots that neither are analysed nor feed the biomass rule, and the 3 float64 planes), each under the bound of
that 10-row case; all 16 rows are held to the cap on the host (tests/test_enkf_sharded.py).

Two processes: RCCL refuses two ranks on one device (tests/test_gpu_multirank.py), so the two-process rehearsal runs over the
process group (gloo, host copies) and the DirectComm path runs as one rank of its own."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import enkf_exact_reference as xr
from tests import enkf_reference as er
from tests import enkf_sharded_reference as shr
from tests import helpers
from tests.enkf_gpu_common import ANALYSED, BASE, DEV, SLOTS, bits, crafted, empty, observe, op_tuples, within
from tests.test_gpu_enkf_edges import (LAD_ANALYSED, LAD_SLOTS, POOLS13, ladder_state, ladder_truth, ladder_worst, ops4, ops16,
                                       run_sites, upload, well_conditioned)

pytestmark = pytest.mark.gpu

DELTA = 12


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def ucol(s, r, j, sizes):
    """the union's column of member j of shard r at site s"""
    return s * sum(sizes) + sum(sizes[:r]) + j


def union_inputs(seed, n_sites, sizes, dead=(), sunk=()):
    """well_conditioned() over the union; the members `sunk` get plantCAccountingDelta = -500: wood + delta stays far below
    zero whatever the update does, so they keep their forecast"""
    pools, planes, fake = well_conditioned(seed, n_sites, sum(sizes), dead)
    pools[list(sunk), DELTA] = -500.0
    fake[:, :13] = pools
    return pools, planes, fake


def run_shards(base, n_sites, sizes, prec, pools, planes, ops, analysed, obs, sd, infl=None, dead=(), order=None, tamper=None):
    """the union's pools [n_sites x sum(sizes)][13] and planes cut into len(sizes) batches; every batch's moments; the blocks
    stacked (in `order`; tamper = (block, site, count) overwrites one count); every batch's analysis -> dict.  Asserted on the
    way: shard_moments leaves every batch bit-identical."""
    k = len(sizes)
    mask = np.zeros(pools.shape[0], dtype=bool)
    mask[list(dead)] = True
    pools_r = shr.split(pools, n_sites, sizes)
    dead_r = [np.flatnonzero(m) for m in shr.split(mask, n_sites, sizes)]
    batches, devs, st0s, prm0s, rings0s, moments = [], [], [], [], [], []
    for r in range(k):
        b, st0 = crafted(base, n_sites, sizes[r], prec, pools_r[r], dead_r[r])
        mine = [np.ascontiguousarray(shr.split(p.T, n_sites, sizes)[r].T) for p in planes]
        batches.append(b)
        devs.append(upload(mine, prec == sa.F32_MIXED) if planes else None)
        st0s.append(st0)
        prm0s.append(b.get_params())
        rings0s.append(b.get_rings())
    for r, b in enumerate(batches):
        moments.append(b.enkf_shard_moments(ops, analysed, planes=devs[r]))
        np.testing.assert_array_equal(bits(b.get_state()), bits(st0s[r]))
        np.testing.assert_array_equal(bits(b.get_params()), bits(prm0s[r]))
        np.testing.assert_array_equal(bits(b.get_rings()), bits(rings0s[r]))
    gathered = torch.stack([moments[r] for r in (order or range(k))]).contiguous()
    if tamper is not None:
        gathered[tamper[0], tamper[1], 0] = tamper[2]
    infos = []
    for r, b in enumerate(batches):
        info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
        b.enkf_analysis_sharded(gathered, obs, sd, ops, analysed, planes=devs[r], inflation=infl, info_out=info)
        infos.append(info.cpu().numpy())
    st1s = [b.get_state() for b in batches]
    for r, b in enumerate(batches):
        np.testing.assert_array_equal(bits(b.get_params()), bits(prm0s[r]))      # all parameters
        np.testing.assert_array_equal(bits(b.get_rings()), bits(rings0s[r]))
        b.close()
    return dict(st0=shr.interleave(st0s, n_sites), st1=shr.interleave(st1s, n_sites), prm0=shr.interleave(prm0s, n_sites),
                st0s=st0s, st1s=st1s, infos=infos, moments=[m.cpu().numpy() for m in moments])


def check_union(r, n_sites, ops, slots, obs, sd, planes, infl=None, site_ok=None, bound=1e-10):
    """the shards' results in the union's layout against the member-space reference over the union; site_info; everything the
    analysis must not touch bit for bit -> the reference's info"""
    st0 = r["st0"]
    ok = np.ones(n_sites) if site_ok is None else np.asarray(site_ok)
    want, want_info = er.analysis(st0, st0[:, 29], ok, n_sites, op_tuples(ops), slots, obs, sd, infl, planes or None, r["prm0"])
    sites = np.flatnonzero(ok)
    for info in r["infos"]:
        np.testing.assert_array_equal(info[sites, :3], want_info[sites, :3])
        np.testing.assert_array_equal(info[:, :3], r["infos"][0][:, :3])
    np.testing.assert_array_equal(sum(info[:, 3] for info in r["infos"])[sites], want_info[sites, 3])
    within(r["st1"], want, st0, n_sites, slots, bound=bound)
    other = [k for k in range(32) if k not in slots]
    np.testing.assert_array_equal(bits(r["st1"][:, other]), bits(st0[:, other]))
    code = r["infos"][0][:, 0]
    untouched = np.repeat(code != 1, st0.shape[0] // n_sites) | (st0[:, 29] != 0)
    np.testing.assert_array_equal(bits(r["st1"][untouched]), bits(st0[untouched]))
    return want_info


def ops_for(n_obs):
    return {1: [sa.enkf_plane("nee")], 4: ops4(), 16: ops16()}[n_obs]


def pools_for(n):
    names = {1: ["plantLeafC"], 7: ANALYSED, 13: POOLS13}[n]
    return names, [sa.POOLS.index(p) for p in names]


# (sizes, n_sites, n_obs, analysed pools, precision, inflates): every M_r of {1, 2, 63, 64, 65, 255, 256, 257, 300}
UNION_CASES = [((64,), 1, 1, 1, sa.F64, False),
               ((63, 257), 3, 4, 7, sa.F64, True),
               ((1, 300, 65), 3, 16, 13, sa.F64, True),
               ((256, 255), 1, 4, 13, sa.F32_MIXED, True),
               ((2, 64, 1), 3, 4, 1, sa.F32_MIXED, False),
               ((300,), 3, 16, 13, sa.F32_MIXED, True),
               ((65, 2, 256), 1, 1, 13, sa.F64, False)]


@pytest.mark.parametrize("k", range(len(UNION_CASES)), ids=["x".join(map(str, c[0])) + f"-s{c[1]}-o{c[2]}-a{c[3]}" for c in UNION_CASES])
def test_the_shards_against_the_union(base, k):
    """a float32 plane under the PLANE operator in the fp32-mixed batches; lambda > 1; with three sites a NaN observation at
    site 0 and site 1 all NaN; a dead member in the first and the last shard; one member under the biomass rule"""
    sizes, n_sites, n_obs, n_pools, prec, inflates = UNION_CASES[k]
    last = len(sizes) - 1
    dead = [ucol(n_sites - 1, last, sizes[last] - 1, sizes)] + ([ucol(0, 0, 5, sizes)] if sizes[0] > 5 else [])
    big = int(np.argmax(sizes))
    sunk = [ucol(0, big, 3, sizes)]
    pools, planes, fake = union_inputs(40 + k, n_sites, sizes, dead, sunk)
    ops = ops_for(n_obs)
    analysed, slots = pools_for(n_pools)
    three = n_sites == 3
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(k), nan_sites=(1,) if three else (),
                      nan_obs=((0, n_obs - 1),) if three and n_obs > 1 else ())
    infl = 1.0 + 0.05 * ((np.arange(n_sites) + 1) % 3) if inflates else None
    r = run_shards(base, n_sites, sizes, prec, pools, planes, ops, analysed, obs, sd, infl=infl, dead=dead)
    info = check_union(r, n_sites, ops, slots, obs, sd, planes, infl)
    assert info[0, 0] == 1 and info[0, 3] == 1 and r["infos"][big][0, 3] == 1          # the sunk member, in its own shard
    assert info[:, 2].sum() == n_sites * sum(sizes) - len(dead)
    if three:
        assert list(info[:, 0]) == [1, -1, 1] and info[0, 1] == max(n_obs - 1, 1)
    assert np.abs(r["st1"][:, slots] - r["st0"][:, slots]).max() > 0


@pytest.mark.parametrize("n_sites,M", [(3, 300), (1, 8192)])
def test_world_one_agrees_with_the_block_and_sites_calls(base, n_sites, M):
    """one shard is a per-site filter of its own, for any member count: 8192 members are beyond the block call's 4096"""
    dead = [7, n_sites * M - 2]
    pools, planes, fake = union_inputs(60, n_sites, (M,), dead, sunk=[11])
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(6), nan_obs=((0, 2),))
    infl = np.full(n_sites, 1.08)
    r = run_shards(base, n_sites, (M,), sa.F64, pools, planes, ops, ANALYSED, obs, sd, infl=infl, dead=dead)
    check_union(r, n_sites, ops, SLOTS, obs, sd, planes, infl)
    rs = run_sites(base, n_sites, M, sa.F64, "auto", pools, planes, ops, ANALYSED, obs, sd, infl=infl, dead=dead)
    within(r["st1"], rs["st1"], r["st0"], n_sites)
    np.testing.assert_array_equal(r["infos"][0], rs["info"])
    if M <= 4096:
        b, st0 = crafted(base, n_sites, M, sa.F64, pools, dead)
        loc = b.enkf_localization(*empty(n_sites), len(ops))
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device=DEV)
        b.enkf_analysis_block(loc, obs, sd, ops, ANALYSED, planes=upload(planes), inflation=infl, info_out=info)
        within(r["st1"], b.get_state(), st0, n_sites)
        np.testing.assert_array_equal(r["infos"][0], info.cpu().numpy())
        b.close()


DEGENERATE = ["an empty shard at one site", "a shard with one live member", "a union of one and one", "a union of one"]


@pytest.mark.parametrize("what", DEGENERATE)
def test_degenerate_shards(base, what):
    n_sites = 2
    if what in DEGENERATE[:2]:
        sizes = (64, 3)
        dead = [ucol(1, 1, j, sizes) for j in range(3)] if what == DEGENERATE[0] else [ucol(0, 1, 0, sizes), ucol(0, 1, 2, sizes)]
    else:
        sizes = (2, 2)
        dead = [ucol(0, 0, 1, sizes), ucol(0, 1, 1, sizes)] + ([ucol(0, 0, 0, sizes)] if what == DEGENERATE[3] else [])
    pools, planes, fake = union_inputs(70, n_sites, sizes, dead)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(7))
    r = run_shards(base, n_sites, sizes, sa.F64, pools, planes, ops, ANALYSED, obs, sd, dead=dead)
    info = check_union(r, n_sites, ops, SLOTS, obs, sd, planes)
    W = shr.moment_words(len(ANALYSED), len(ops))
    assert all(m.shape == (n_sites, W) for m in r["moments"])
    if what == DEGENERATE[0]:
        assert (r["moments"][1][1] == 0).all() and r["moments"][1][0, 0] == 3
        np.testing.assert_array_equal(bits(r["st1s"][1][3:]), bits(r["st0s"][1][3:]))
        assert list(info[:, 0]) == [1, 1] and list(info[:, 2]) == [67, 64]
    elif what == DEGENERATE[1]:
        assert r["moments"][1][0, 0] == 1 and (r["moments"][1][0, 2 + len(ANALYSED) + len(ops):] == 0).all()
        assert np.abs(r["st1s"][1][1, SLOTS] - r["st0s"][1][1, SLOTS]).max() > 0     # its one live member is analysed
        assert list(info[:, 2]) == [65, 67]
    elif what == DEGENERATE[2]:
        assert list(info[:, 0]) == [1, 1] and list(info[:, 2]) == [2, 4]
        assert np.abs(r["st1"][[0, 2]][:, SLOTS] - r["st0"][[0, 2]][:, SLOTS]).max() > 0
    else:
        assert list(info[:, 0]) == [0, 1] and list(info[:, 2]) == [1, 4]
        for st1, st0 in zip(r["st1s"], r["st0s"]):
            np.testing.assert_array_equal(bits(st1[:2]), bits(st0[:2]))


def test_the_moment_block_is_what_the_header_states(base):
    """count, reserved zero, the shard's means, the centred products [V][n_obs] not divided, against numpy to rounding"""
    n_sites, sizes = 2, (300,)
    dead = [4, 299, 300]
    pools, planes, fake = union_inputs(75, n_sites, sizes, dead)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(8))
    r = run_shards(base, n_sites, sizes, sa.F64, pools, planes, ops, ANALYSED, obs, sd, dead=dead)
    nA, p = len(SLOTS), len(ops)
    for s in range(n_sites):
        cols = np.arange(s * 300, (s + 1) * 300)
        live = cols[r["st0"][cols, 29] == 0]
        fc = r["st0"][live, :13]
        H = np.stack([er.predicted(op, fc, [q[:, live] for q in planes], None) for op in op_tuples(ops)], 1)
        n, mean, Cm = shr.shard_moments(np.concatenate([fc[:, SLOTS], H], 1), nA)
        blk = r["moments"][0][s]
        assert blk[0] == n == len(live) and blk[1] == 0
        np.testing.assert_allclose(blk[2:2 + nA + p], mean, rtol=1e-13)
        np.testing.assert_allclose(blk[2 + nA + p:].reshape(nA + p, p), Cm, rtol=1e-11, atol=1e-11 * np.abs(Cm).max())


def test_repeatable_and_the_order_of_the_blocks(base):
    n_sites, sizes = 3, (65, 257, 64)
    dead = [3, 700]
    pools, planes, fake = union_inputs(80, n_sites, sizes, dead)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(9), nan_obs=((2, 1),))
    infl = np.array([1.0, 1.1, 1.03])
    runs = [run_shards(base, n_sites, sizes, sa.F64, pools, planes, ops, ANALYSED, obs, sd, infl=infl, dead=dead, order=o)
            for o in (None, None, (2, 0, 1))]
    for r in runs:
        check_union(r, n_sites, ops, SLOTS, obs, sd, planes, infl)      # (every shard reports the same site_info[:, :3])
    np.testing.assert_array_equal(bits(runs[1]["st1"]), bits(runs[0]["st1"]))
    for a, b in zip(runs[1]["moments"], runs[0]["moments"]):
        np.testing.assert_array_equal(bits(a), bits(b))
    for a, b in zip(runs[1]["infos"], runs[0]["infos"]):
        np.testing.assert_array_equal(a, b)
    within(runs[2]["st1"], runs[0]["st1"], runs[0]["st0"], n_sites)


BAD_INPUTS = ["obs inf", "sd 0", "sd negative", "lambda below 1", "count nan", "count negative", "count 2.5", "count 1e9"]


@pytest.mark.parametrize("what", BAD_INPUTS)
def test_bad_input_gives_code_minus_two_on_every_shard(base, what):
    n_sites, sizes = 3, (64, 65)
    pools, planes, fake = union_inputs(85, n_sites, sizes)
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(10))
    infl = np.full(n_sites, 1.05)
    tamper = None
    if what == "obs inf":
        obs[1, 2] = np.inf
    elif what == "sd 0":
        sd[1, 0] = 0.0
    elif what == "sd negative":
        sd[1, 3] = -1.0
    elif what == "lambda below 1":
        infl[1] = 0.5
    else:
        tamper = (1, 1, {"count nan": np.nan, "count negative": -1.0, "count 2.5": 2.5, "count 1e9": 1e9}[what])
    r = run_shards(base, n_sites, sizes, sa.F64, pools, planes, ops, ANALYSED, obs, sd, infl=infl, tamper=tamper)
    # (a torn block is no input of the reference: it sees the site as one whose plan failed, and the site is left out of the
    # comparison of site_info)
    check_union(r, n_sites, ops, SLOTS, obs, sd, planes, infl, site_ok=[1, 0, 1] if tamper else None)
    M = sum(sizes)
    for info, st1, st0, m in zip(r["infos"], r["st1s"], r["st0s"], sizes):
        assert list(info[:, 0]) == [1, -2, 1] and info[1, 1] == 0 and info[1, 3] == 0
        np.testing.assert_array_equal(bits(st1[m:2 * m]), bits(st0[m:2 * m]))
    assert np.abs(r["st1"][:M, SLOTS] - r["st0"][:M, SLOTS]).max() > 0


def test_the_synchronous_form_refuses_with_the_site_named(base):
    n_sites, M = 3, 64
    pools, planes, fake = union_inputs(86, n_sites, (M,))
    ops = ops4()
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(11))
    b, st0 = crafted(base, n_sites, M, sa.F64, pools)
    dev = upload(planes)
    gathered = b.enkf_shard_moments(ops, ANALYSED, planes=dev).view(1, n_sites, -1).clone()
    torn = gathered.clone()
    torn[0, 2, 0] = 2.5
    bad_sd = sd.copy()
    bad_sd[1, 0] = -1.0
    for g, e_sd, site in ((torn, sd, "site 2"), (gathered, bad_sd, "site 1")):
        with pytest.raises(sa.SipnetError) as e:
            b.enkf_analysis_sharded(g, obs, e_sd, ops, ANALYSED, planes=dev)
        assert e.value.code == _lib.ERR_BAD_ARGUMENT and site in str(e.value) and "nothing was written" in str(e.value)
        np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    b.enkf_analysis_sharded(gathered, obs, sd, ops, ANALYSED, planes=dev)         # ... and analyses good input
    st1 = b.get_state()
    b.close()
    want, _ = er.analysis(st0, st0[:, 29], np.ones(n_sites), n_sites, op_tuples(ops), SLOTS, obs, sd, None, planes, None)
    within(st1, want, st0, n_sites)


def test_refusals(base):
    n_sites, M = 2, 64
    pools, _, _ = union_inputs(87, n_sites, (M,))
    b, st0 = crafted(base, n_sites, M, sa.F64, pools)
    L, h = b.L, b.h
    wood = sa.enkf_pools(["plantWoodC"])
    arr = (_lib.EnkfObs * 1)(wood)
    obs = torch.full((n_sites, 1), 100.0, dtype=torch.float64, device=DEV)
    sd = torch.ones((n_sites, 1), dtype=torch.float64, device=DEV)
    W = b.enkf_moment_words([wood], ["plantWoodC"])
    assert W == 6
    mom = torch.zeros((1, n_sites, W), dtype=torch.float64, device=DEV)
    BAD = _lib.ERR_BAD_ARGUMENT

    def moments(m=mom, n_obs=1, mask=1, ops=arr):
        return L.sipnet_batch_enkf_shard_moments(h, n_obs, ops, mask, None, 0, 0, 0, m.data_ptr() if m is not None else None,
                                                 b._stream())

    def apply(world=1, g=mom, o=obs, s=sd, n_obs=1, mask=1):
        return L.sipnet_batch_enkf_analysis_sharded(h, n_obs, arr, mask, None, 0, 0, 0, o.data_ptr() if o is not None else None,
                                                    s.data_ptr() if s is not None else None, None, world,
                                                    g.data_ptr() if g is not None else None, None, b._stream())

    assert moments(m=None) == BAD and b"d_moments" in L.sipnet_last_error()
    assert moments(n_obs=0) == BAD and moments(n_obs=17) == BAD and moments(mask=0) == BAD and moments(mask=1 << 13) == BAD
    assert moments(ops=None) == BAD
    assert moments() == _lib.OK
    assert apply(world=0) == BAD and b"world" in L.sipnet_last_error()
    assert apply(world=65) == BAD and apply(world=-1) == BAD
    assert apply(g=None) == BAD and b"d_gathered" in L.sipnet_last_error()
    assert apply(o=None) == BAD and apply(s=None) == BAD and apply(n_obs=0) == BAD and apply(mask=0) == BAD
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))
    assert apply() == _lib.OK
    assert np.abs(b.get_state()[:, 0] - st0[:, 0]).max() > 0
    with pytest.raises(ValueError):
        b.enkf_analysis_sharded(mom[:, :, :5].contiguous(), obs, sd, [wood], ["plantWoodC"])
    with pytest.raises(ValueError):
        b.enkf_shard_moments([wood], ["plantWoodC"], out=torch.zeros(3, dtype=torch.float64, device=DEV))
    # a batch connected across ranks is refused, as by the other analyses
    b.close()
    b, _ = crafted(base, 1, M, sa.F64, pools[:M])
    h = b.h
    b.pf_connect([b.pf_publish(with_params=True)], 0)
    assert moments() == BAD and b"connected" in L.sipnet_last_error()
    assert apply() == BAD and b"connected" in L.sipnet_last_error()
    b.close()


# ---- the conditioning set -------------------------------------------------------------------------------------------------
CONDITIONING = shr.conditioning_set()
SHARD_CUTS = ((0.5,), (0.2, 0.55))            # the 64 members in 2 and in 3 shards
ROW_SLOTS = [3, 4, 5, 8, 9, 10, 11]           # pools that neither are analysed (LAD_SLOTS) nor feed the biomass rule


def normalised(case):
    sd = np.sqrt(case["R"])
    return dict(case, R=sd * sd)              # (what a kernel forms from the sd it is given)


def ten_rows(case):
    return dict(case, H=case["H"][:, :10], y=case["y"][:10], R=case["R"][:10], p=10, name=case["name"] + "-rows10")


def ten_row_state(case):
    """the case's X in the analysed slots, rows 0..6 in ROW_SLOTS, rows 7..9 in the three float64 planes"""
    n = case["X"].shape[0]
    pools = np.full((n, 13), 1000.0)
    pools[:, LAD_SLOTS] = case["X"]
    pools[:, ROW_SLOTS] = case["H"][:, :7]
    planes = [np.ascontiguousarray(case["H"][:, 7 + k][None, :]) for k in range(3)]
    ops = [sa.enkf_pools([POOLS13[k]]) for k in ROW_SLOTS] + [sa.enkf_plane(v) for v in ("nee", "gpp", "et")]
    return pools, planes, case["y"].reshape(1, 10), np.sqrt(case["R"]).reshape(1, 10), ops


@pytest.mark.parametrize("case", CONDITIONING, ids=[c["name"] for c in CONDITIONING])
def test_conditioning_set_in_two_and_three_shards(base, case):
    """error against the extended-precision update of the union <= max(1e-10, 4 x own_error(merged_chain64 cut alike, case))"""
    case = normalised(case)
    if case["p"] == 4:
        pools, obs, sd, ops = ladder_state(case, 1, 4)
        planes = []
    else:
        case = ten_rows(case)
        pools, planes, obs, sd, ops = ten_row_state(case)
    n = case["X"].shape[0]
    for fractions in SHARD_CUTS:
        edges = [0] + shr.cuts_at(n, fractions) + [n]
        sizes = tuple(int(b - a) for a, b in zip(edges[:-1], edges[1:]))
        bound = max(xr.FLOOR, xr.FACTOR * shr.own_error(case, fractions))
        assert bound <= xr.CAP
        r = run_shards(base, 1, sizes, sa.F64, pools, planes, ops, LAD_ANALYSED, obs, sd)
        want, kept, _ = ladder_truth(case, r["st0"], 1, sd[0])
        worst = ladder_worst(r["st1"], want, r["st0"], 1, bound)
        print(f"LADDER sharded {sizes} {case['name']} error {worst * bound:.3e} bound {bound:.3e} ratio {worst:.3f}")
        assert kept == 0
        for info in r["infos"]:
            assert list(info[0, :3]) == [1, case["p"], n] and info[0, 3] == 0


# ---- ranks that are processes ----------------------------------------------------------------------------------------------
CHILD = os.path.join(helpers.REPO, "tests", "enkf_sharded_ranks.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("collective", ["group", "direct"])
def test_ranks_that_are_processes_rehearsed_on_one_gpu(tmp_path, collective):
    """dist.enkf_analysis_sharded in fresh child processes (tests/enkf_sharded_ranks.py).  group: two processes on this one GPU,
    the all-gather over the process group (gloo, through host copies).  direct: the all-gather through the engine's own RCCL
    communicator on the batch's stream -- one rank, since RCCL refuses two ranks on one device.  Every rank's result against the
    member-space reference over the union."""
    world = 2 if collective == "group" else 1
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), CHILD, "--collective", collective, "--out", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=helpers.REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = [np.load(str(tmp_path / f"rank{k}.npz")) for k in range(world)]
    n_sites = int(got[0]["n_sites"])
    res = dict(st0=shr.interleave([g["st0"] for g in got], n_sites), st1=shr.interleave([g["st1"] for g in got], n_sites),
               prm0=shr.interleave([g["prm0"] for g in got], n_sites), infos=[g["info"] for g in got])
    from tests.enkf_sharded_ranks import inputs
    sizes, pools, planes, ops, obs, sd, infl, dead = inputs(world)
    info = check_union(res, n_sites, ops, SLOTS, obs, sd, planes, infl)
    assert (info[:, 0] == 1).all() and info[:, 2].sum() == n_sites * sum(sizes) - len(dead)
    for g in got:
        assert int(g["gathered_world"]) == world
