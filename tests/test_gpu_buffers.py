"""The owners of device and pinned-host memory (csrc/dev_buf.h) on the GPU, through sipnet_debug_live_bytes: the bytes that the
library's own objects hold, process-wide.  Everything comes back when the owners are closed, a block that has grown keeps the
results and is neither shrunk nor allocated twice, and a batch that cannot be created leaves nothing behind.  Small shapes
throughout: 2 sites, 64 to 256 members, 48 to 500 steps."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, dist as sd_, synth
from sipnet_amd.node import Node
from tests.enkf_gpu_common import ANALYSED, BASE, DEV, crafted, observe
from tests.test_gpu_enkf_edges import PARAMS4, complete, ops4, params_of, two_series, upload, well_conditioned

pytestmark = pytest.mark.gpu

FLAGS = sa.flags_from()


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, FLAGS)[0]


@functools.lru_cache(maxsize=None)
def forcing(n_steps, site=0):
    return synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(n_steps, site=site)))


def live():
    """(device, pinned) bytes held, once nothing unreachable is left to close itself later and no thread scratch is counted"""
    gc.collect()
    sa.lib().sipnet_pf_release_scratch()
    return sa.debug_live_bytes()


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).view(np.uint8)


# ---- 1. everything comes back -------------------------------------------------------------------------------------------
def batch_cycle(members):
    b = sa.Batch(FLAGS, 2, 256, sa.F64, fast_math=True)
    for s in range(2):
        b.set_climate(s, forcing(96, s))
        b.set_params(s, members)
    b.setup()
    planes, _ = b.run()
    b.setup()
    b.run(full=True)
    b.setup()
    b.run_stats()
    b.setup()
    b.run_sums(0, 96, 48)
    b.enable_diagnostics(True)
    b.setup()
    b.run()
    assert b.get_diagnostics()["n_clamp_warn"].shape == (512,)
    b.enable_diagnostics(False)
    # every site a filter of its own, on the planes of the first run
    obs = planes[0].double().sum(0).view(2, 256).median(1).values.cpu().numpy()
    b.setup()
    b.run(planes=planes)
    b.pf_analysis_sites(planes[0], obs, [1.0, 1.0], [0.3, 0.6], with_params=True)
    assert sa.debug_live_bytes()[0] > 0 and sa.debug_live_bytes()[1] > 0
    b.close()


def filter_cycle(members):
    # one filter in one batch, its particles carrying their parameters
    b1 = sa.Batch(FLAGS, 1, 256, sa.F64, fast_math=True)
    b1.set_climate(0, forcing(96))
    b1.set_params(0, members)
    b1.setup()
    p1, _ = b1.run()
    obs = float(p1[0].sum(0).median())
    sd_.pf_analysis(b1, p1[0], obs, 1.0, 0.3, with_params=True, diagnostics=False)
    # the batch-less entry points: the host thread's scratch
    anc = sd_.pf_systematic_ancestors(b1.pf_log_weights(p1[0], obs, 1.0), 0.3)
    sd_.pf_exchange_plan(anc, 256, 1, 0)
    b1.close()
    # a filter connected to a world of itself: the parameter bank, the peer tables, the one-launch analysis
    b2 = sa.Batch(FLAGS, 1, 256, sa.F32_MIXED, kernel=sa.KERNEL_ONE_WAVE)
    b2.set_climate(0, forcing(96))
    b2.set_params(0, members)
    b2.setup()
    p2, _ = b2.run(0, 48)
    d = b2.pf_publish(with_params=True)
    b2.pf_connect([d] * 2, 1)
    g = torch.empty((2, b2.pf_block_len()), dtype=torch.float64, device=b2.device)
    b2.pf_local_weights(p2[0], float(p2[0].double().sum(0).median()), 1.0, g[1])
    g[0] = g[1]
    anc = torch.empty(256, dtype=torch.int32, device=b2.device)
    tot = torch.zeros(1, dtype=torch.int64, device=b2.device)
    for _ in range(2):
        b2.pf_resample_peers(g, 0.5, anc, tot)
        b2.run(0, 48, planes=p2)
    torch.cuda.synchronize()
    assert int(tot[0]) > 0
    b2.close()


def enkf_cycle(base):
    n_sites, M = 2, 64
    pools, planes, fake = well_conditioned(91, n_sites, M)
    ops, params = ops4(), params_of(PARAMS4[:2])
    obs, sd = observe(fake, planes, None, n_sites, ops, np.random.default_rng(5))
    b, _ = crafted(base, n_sites, M, sa.F64, pools)
    dev = upload(planes)
    info = torch.full((n_sites, 4), -9, dtype=torch.int32, device=DEV)
    b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=dev, info_out=info)
    assert (info[:, 0] == 1).all()
    b.enkf_analysis_joint(obs, sd, ops, ANALYSED, params, planes=dev)
    series = [upload([z], f32=z.dtype == np.float32)[0] for z in two_series(np.random.default_rng(6), n_sites, M, fake)]
    b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, series, params, planes=dev)
    ptr, nbr, rho = complete(n_sites, 0.5)
    loc = b.enkf_localization(ptr, nbr, rho, len(ops))
    b.enkf_analysis_local(loc, obs, sd, ops, ANALYSED, planes=dev)
    b.enkf_analysis_block(loc, obs, sd, ops, ANALYSED, planes=dev)
    gathered = b.enkf_shard_moments(ops, ANALYSED, planes=dev).view(1, n_sites, -1).clone()
    b.enkf_analysis_sharded(gathered, obs, sd, ops, ANALYSED, planes=dev)
    b.close()                                                           # (closes the localization first)


def node_cycle(members):
    nd = Node(FLAGS, 2, 128, devices=[0, 0], fast_math=True)
    for s in range(2):
        nd.set_climate(s, forcing(96, s))
    nd.set_params(None, members[:128])
    nd.setup()
    nd.run(0, 96)
    nd.gather_stats()
    nd.setup()
    nd.run_gathering(0, 96, 2)
    nd.sync()
    nd.setup()
    nd.run_gathering_reduced(0, 96, 2, "sums", 48)
    nd.sync()
    nd.close()


def test_everything_comes_back_when_the_owners_are_closed(base):
    members = synth.perturbed_params(base, 256)
    first = live()
    for round_ in range(2):                                             # (a second round must not creep either)
        batch_cycle(members)
        filter_cycle(members)
        enkf_cycle(base)
        node_cycle(members)
        now = live()
        print(f"round {round_}: live (device, pinned) bytes {now}, at the start {first}")
        assert now == first


# ---- 2. a block that has grown keeps the results -----------------------------------------------------------------------
def batch_outputs(b, members, n_steps):
    for s in range(2):
        b.set_climate(s, forcing(n_steps, s))
        b.set_params(s, members)
    b.setup()
    planes, _ = b.run()
    b.setup()
    planes2, stats = b.run_stats()
    assert torch.equal(planes, planes2)
    torch.cuda.synchronize()
    return bits(planes), bits(stats)


@pytest.mark.parametrize("prec,fast", [(sa.F64, True), (sa.F64, False), (sa.F32_MIXED, None)], ids=["f64-fast", "f64-strict", "f32"])
def test_a_batch_that_regrows_keeps_its_results(base, prec, fast):
    members = synth.perturbed_params(base, 64)
    b = sa.Batch(FLAGS, 2, 64, prec, fast_math=fast)
    held = []
    for n_steps in (96, 500, 96):
        got = batch_outputs(b, members, n_steps)
        held.append(sa.debug_live_bytes())
        fresh = sa.Batch(FLAGS, 2, 64, prec, fast_math=fast)
        want = batch_outputs(fresh, members, n_steps)
        fresh.close()
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    b.close()
    print("live (device, pinned) bytes after the runs of 96, 500, 96 steps:", held)
    assert held[1][0] > held[0][0] and held[1][1] > held[0][1]           # (the longer forcing needed more)
    assert held[2] == held[1]                                            # grow-only: no shrink, no second block


def make_node(members):
    nd = Node(FLAGS, 2, 128, devices=[0, 0], fast_math=True)
    for s in range(2):
        nd.set_climate(s, forcing(96, s))
    nd.set_params(None, members)
    return nd


def node_run(nd, n_steps):
    nd.setup()
    nd.run(0, n_steps)
    planes = nd.member_planes()
    return bits(planes), bits(nd.gather_stats())


def test_a_node_that_regrows_keeps_its_results(base):
    members = synth.perturbed_params(base, 128)
    nd = make_node(members)
    want = {}
    held = []
    for n_steps in (48, 96, 48):
        got = node_run(nd, n_steps)
        held.append(sa.debug_live_bytes())
        if n_steps not in want:
            fresh = make_node(members)
            want[n_steps] = node_run(fresh, n_steps)
            fresh.close()
            assert sa.debug_live_bytes() == held[-1]
        for g, w in zip(got, want[n_steps]):
            np.testing.assert_array_equal(g, w)
    nd.close()
    print("live (device, pinned) bytes after the runs of 48, 96, 48 steps:", held)
    assert held[1][0] > held[0][0]
    assert held[2] == held[1]


def node_gathering(nd, n_steps):
    nd.setup()
    nd.run_gathering(0, n_steps, 2)
    return [bits(nd.gathered_member_planes(k)) for k in range(nd.n)]


def node_reduced(nd, n_steps):
    nd.setup()
    nd.run_gathering_reduced(0, n_steps, 2, "sums", 24)
    return [bits(nd.gathered_reduced_member_rows(k)) for k in range(nd.n)]


@pytest.mark.parametrize("order", ["sums first", "planes first"])
def test_gathered_planes_do_not_depend_on_which_form_ran_first(base, order):
    members = synth.perturbed_params(base, 128)
    want, want_sums = {}, {}
    for n_steps in (48, 96):                                             # a fresh node for each length
        fresh = make_node(members)
        want[n_steps] = node_gathering(fresh, n_steps)
        fresh.close()
        fresh = make_node(members)
        want_sums[n_steps] = node_reduced(fresh, n_steps)
        fresh.close()
    nd = make_node(members)
    held = []
    for n_steps in (48, 96, 48):
        for form in (("sums", "planes") if order == "sums first" else ("planes", "sums")):
            got = node_reduced(nd, n_steps) if form == "sums" else node_gathering(nd, n_steps)
            for g, w in zip(got, (want_sums if form == "sums" else want)[n_steps]):
                np.testing.assert_array_equal(g, w)
        held.append(sa.debug_live_bytes())
    nd.close()
    print(f"{order}: live (device, pinned) bytes after 48, 96, 48 steps:", held)
    assert held[1][0] > held[0][0]
    assert held[2] == held[1]


# ---- 3. a batch that cannot be created leaves nothing behind ------------------------------------------------------------
def test_a_refused_allocation_leaves_nothing_and_the_next_batch_runs(base, oracle):
    total = torch.cuda.get_device_properties(0).total_memory
    n_members = total // (sa.RING_SLOTS * 8) + 1                         # ncol * 250 * 8 bytes of ring exceed the device
    assert n_members < 2 ** 31 and n_members * sa.RING_SLOTS * 8 > total
    before = live()
    h = C.c_void_p()
    rc = sa.lib().sipnet_batch_create((C.c_int32 * 12)(*FLAGS), 1, int(n_members), sa.F64, 0, C.byref(h))
    assert rc == _lib.ERR_NO_DEVICE, (rc, sa.lib().sipnet_last_error())
    assert sa.lib().sipnet_last_error().startswith(b"sipnet_batch_create: ")
    assert not h.value
    assert sa.debug_live_bytes() == before
    members = synth.perturbed_params(base, 64)
    clim = forcing(96)
    b = sa.Batch(FLAGS, 1, 64, sa.F64, fast_math=False)
    b.set_climate(0, clim)
    b.set_params(0, members)
    b.setup()
    planes, _ = b.run()
    got = planes.cpu().numpy()
    b.close()
    want, _, _ = oracle.run_block(FLAGS, members, clim)
    assert np.abs(got - want).max() < 1e-9                                # (the strict kernel against the CPU oracle, as smoke())
    assert live() == before
