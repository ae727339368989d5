"""What the C host's node object refuses (sipnet_node_*, csrc/node.cpp and its parts): the return code and the whole text
of sipnet_last_error() -- or, where a call leaves without a text, that the text of the refusal before it still stands --
for creation, the setters, the run calls, the calls that need a certain kind of run before them, the particle filter's
calls, and shards or segments that do not exist.  Then what the node remembers of its last run, across a plain run, a
gathering run, a reduced one and a plain one again on ONE node, every result against ONE batch bit for bit.
Two sites x 8 members x 48 records on two shards of device 0 (event-ordered copies) and on one shard (RCCL, one rank)."""
import ctypes as C
import os

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd._lib import SHARD_MEMBERS, SHARD_SITES
from sipnet_amd.node import Node
from tests import helpers

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
S, M, T, K = 2, 8, 48, 10
BAD, NO_DEVICE = _lib.ERR_BAD_ARGUMENT, _lib.ERR_NO_DEVICE
F32, SUMS = 1, 2


def last():
    return sa.lib().sipnet_last_error().decode()


def refused(rc, code, text):
    assert rc == code and last() == text, (rc, last())


def refused_silently(call, code=BAD):
    """the call leaves with `code` and sets no text of its own"""
    sa.lib().sipnet_node_run(None, 0, 1)
    before = last()
    assert before == "sipnet_node_run: bad argument"
    assert call() == code and last() == before, last()


@pytest.fixture(scope="module")
def inputs():
    base = sa.read_params(BASE, sa.flags_from())[0]
    clims = [synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T, site=s))) for s in range(S)]
    return clims, synth.perturbed_params(base, M, seed=5)


@pytest.fixture(scope="module")
def one_batch(inputs):
    """fast -> (planes [3][T][S][M], statistics [3][T][S][2], sums over groups of K steps in step order) of ONE batch"""
    clims, members = inputs
    out = {}
    for fast in (True, False):
        b = sa.Batch(sa.flags_from(), S, M, sa.F64, fast_math=fast)
        for s in range(S):
            b.set_climate(s, clims[s])
            b.set_params(s, members)
        b.setup()
        planes, stats = b.run_stats(0, T)
        want = planes.cpu().numpy().reshape(3, T, S, M)
        sums = np.zeros((3, (T + K - 1) // K, S, M))
        for t in range(T):
            sums[:, t // K] += want[:, t]
        out[fast] = want, stats.cpu().numpy(), sums
        b.close()
    return out


def make_node(inputs, devices=(0, 0), shard=SHARD_MEMBERS, n_sites=S, precision=sa.F64, fast=True):
    clims, members = inputs
    nd = Node(sa.flags_from(), n_sites, M, precision=precision, devices=list(devices), shard=shard,
              fast_math=fast if precision == sa.F64 else None)
    for s in range(n_sites):
        nd.set_climate(s, clims[s])
    nd.set_params(None, members)
    nd.setup()
    return nd


# ---- creation ----------------------------------------------------------------------------------------------------------
def create(flags="ok", n_sites=S, n_members=M, devices=(0, 0), n_devices=None, mode=SHARD_MEMBERS, sharded=True):
    L = sa.lib()
    fl = (C.c_int32 * 12)(*sa.flags_from()) if flags == "ok" else None
    dv = (C.c_int32 * max(len(devices), 1))(*devices)
    h = C.c_void_p()
    n = len(devices) if n_devices is None else n_devices
    if sharded:
        rc = L.sipnet_node_create_sharded(fl, n_sites, n_members, sa.F64, dv, n, mode, C.byref(h))
    else:
        rc = L.sipnet_node_create(fl, n_sites, n_members, sa.F64, dv, n, C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_create_refuses():
    bad = "%s: bad argument (needs at least one member -- or, sharding sites, one site -- per device)"
    refused(create(flags=None), BAD, bad % "sipnet_node_create_sharded")
    refused(create(flags=None, devices=(0,), sharded=False), BAD, bad % "sipnet_node_create")
    refused(create(n_devices=0), BAD, bad % "sipnet_node_create_sharded")
    refused(create(devices=(0,) * 65), BAD, bad % "sipnet_node_create_sharded")
    refused(create(n_members=1), BAD, bad % "sipnet_node_create_sharded")                        # fewer members than devices
    refused(create(devices=(0, 0, 0), mode=SHARD_SITES), BAD, bad % "sipnet_node_create_sharded")   # two sites, three devices
    refused(create(mode=2), BAD, bad % "sipnet_node_create_sharded")
    have = sa.lib().sipnet_device_count()
    no = "%s: no usable HIP device %d (this engine has no CPU path)"
    refused(create(devices=(0, have)), NO_DEVICE, no % ("sipnet_node_create_sharded", have))
    refused(create(devices=(have,), sharded=False), NO_DEVICE, no % ("sipnet_node_create", have))
    refused(create(devices=(0, 0), sharded=False), BAD, "sipnet_node_create: a device is listed twice")


# ---- setters, run calls, calls out of order --------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", [SHARD_MEMBERS, SHARD_SITES], ids=["members", "sites"])
def test_setters_refuse(inputs, shard):
    clims, members = inputs
    L = sa.lib()
    nd = make_node(inputs, shard=shard)
    c = clims[0]
    ev = (_lib.Event * 1)()
    for h, sites in ((nd.h, (-1, S)), (None, (0,))):
        for site in sites:
            refused(L.sipnet_node_set_climate(h, site, c.n_steps, c.data.ctypes.data, c.year.ctypes.data, c.day.ctypes.data), BAD,
                    "sipnet_node_set_climate: bad argument")
            refused(L.sipnet_node_set_events(h, site, 0, ev), BAD, "sipnet_node_set_events: bad argument")
            # (site -1 is SIPNET_ALL_SITES there)
            refused(L.sipnet_node_set_params(h, site - 1 if site < 0 else site, 0, M, members.ctypes.data), BAD, "sipnet_node_set_params: bad argument")
    for first, count, raw in ((1, M, members.ctypes.data), (0, 0, members.ctypes.data), (0, M, None)):
        refused(L.sipnet_node_set_params(nd.h, 0, first, count, raw), BAD, "sipnet_node_set_params: bad argument")
    refused_silently(lambda: L.sipnet_node_set_math(None, 1))
    refused_silently(lambda: L.sipnet_node_set_kernel(None, 0, 0))
    refused_silently(lambda: L.sipnet_node_setup(None))
    refused_silently(lambda: L.sipnet_node_sync(None))
    refused_silently(lambda: L.sipnet_node_get_status(None, None))
    refused_silently(lambda: L.sipnet_node_get_status(nd.h, None))
    nd.close()


def test_run_calls_refuse_and_gathers_want_a_plain_run(inputs):
    L = sa.lib()
    nd = make_node(inputs)
    stats = "sipnet_node_gather_stats: nothing has run (sipnet_node_run_gathering leaves no statistics)"
    planes = "sipnet_node_gather_planes: nothing has run (after sipnet_node_run_gathering the planes are gathered already)"
    for h in (nd.h, None):                                             # before any run, and no node at all
        refused(L.sipnet_node_gather_stats(h, None), BAD, stats)
        refused(L.sipnet_node_gather_planes(h), BAD, planes)
    for h, n_steps in ((nd.h, 0), (nd.h, -3), (None, T)):
        refused(L.sipnet_node_run(h, 0, n_steps), BAD, "sipnet_node_run: bad argument")
        refused(L.sipnet_node_forecast(h, 0, n_steps), BAD, "sipnet_node_run: bad argument")
    form = "sipnet_node_run_gathering_reduced: form must be SIPNET_GATHER_F32 or SIPNET_GATHER_SUMS"
    groups = "sipnet_node_run_gathering_reduced: sum_steps > 0 and at most one segment per group of steps"
    for h, step0, n_steps, n_seg in ((nd.h, 0, T, 0), (nd.h, 0, T, T + 1), (nd.h, -1, T, 2), (nd.h, 0, 0, 1), (None, 0, T, 2)):
        refused(L.sipnet_node_run_gathering(h, step0, n_steps, n_seg), BAD, "sipnet_node_run_gathering: bad argument")
        refused(L.sipnet_node_run_gathering_reduced(h, step0, n_steps, n_seg, SUMS, K), BAD, "sipnet_node_run_gathering: bad argument")
        refused(L.sipnet_node_run_gathering_reduced(h, step0, n_steps, n_seg, 0, K), BAD, form)    # (the form comes first)
    refused(L.sipnet_node_run_gathering_reduced(nd.h, 0, T, 2, 3, K), BAD, form)
    refused(L.sipnet_node_run_gathering_reduced(nd.h, 0, T, 2, SUMS, 0), BAD, groups)
    refused(L.sipnet_node_run_gathering_reduced(nd.h, 0, T, 2, SUMS, -1), BAD, groups)
    refused(L.sipnet_node_run_gathering_reduced(nd.h, 0, T, 6, SUMS, K), BAD, groups)              # five groups of ten
    assert L.sipnet_node_n_segments(nd.h) == 0 and L.sipnet_node_n_segments(None) == 0
    assert L.sipnet_node_reduced_in_kernel(nd.h) == 0 and L.sipnet_node_reduced_in_kernel(None) == 0
    nd.run_gathering(0, T, 2)                                          # after a gathering run
    refused(L.sipnet_node_gather_stats(nd.h, None), BAD, stats)
    refused(L.sipnet_node_gather_planes(nd.h), BAD, planes)
    nd.close()
    mixed = make_node(inputs, precision=sa.F32_MIXED)
    refused(L.sipnet_node_run_gathering_reduced(mixed.h, 0, T, 2, F32, 0), BAD,
            "sipnet_node_run_gathering_reduced: the planes of an fp32-mixed node are floats already (sipnet_node_run_gathering)")
    mixed.close()


def test_filter_calls_refuse(inputs):
    L = sa.lib()
    connect = "sipnet_node_pf_connect: a filter needs ONE site, its particles sharded as members over at most 16 devices"
    arm = "sipnet_node_pf_arm: needs sipnet_node_pf_connect and sigma > 0"
    analysis = "sipnet_node_pf_analysis: needs sipnet_node_pf_connect and a forecast (sipnet_node_forecast / _run)"
    refused(L.sipnet_node_pf_connect(None, 1), BAD, connect)
    for shard, n_sites in ((SHARD_MEMBERS, 2), (SHARD_SITES, 2), (SHARD_SITES, 1)):
        nd = make_node(inputs, devices=(0, 0) if n_sites == 2 else (0,), shard=shard, n_sites=n_sites)
        refused(L.sipnet_node_pf_connect(nd.h, 1), BAD, connect)
        nd.close()
    nd = make_node(inputs, n_sites=1)
    nd.forecast(0, T)
    for h in (nd.h, None):                                             # not connected
        refused(L.sipnet_node_pf_arm(h, 1.0, 1.0), BAD, arm)
        refused(L.sipnet_node_pf_analysis(h, 0, 1.0, 1.0, 0.5), BAD, analysis)
        refused_silently(lambda: L.sipnet_node_pf_check(h, None))
    assert L.sipnet_node_pf_block_len(nd.h) == 0 and L.sipnet_node_pf_block_len(None) == 0
    nd.pf_connect(True)
    assert L.sipnet_node_pf_block_len(nd.h) > 0
    for sigma in (0.0, -1.0, float("nan")):
        refused(L.sipnet_node_pf_arm(nd.h, 1.0, sigma), BAD, arm)
    for variable in (-1, 3):
        refused(L.sipnet_node_pf_analysis(nd.h, variable, 1.0, 1.0, 0.5), BAD, analysis)
    nd.setup()
    nd.run_gathering(0, T, 2)
    refused(L.sipnet_node_pf_analysis(nd.h, 0, 1.0, 1.0, 0.5), BAD,
            "sipnet_node_pf_analysis: the last run was sipnet_node_run_gathering (segmented planes); forecast with "
            "sipnet_node_forecast / sipnet_node_run")
    nd.close()
    fresh = make_node(inputs, n_sites=1)                               # connected, nothing has run
    fresh.pf_connect(True)
    refused(L.sipnet_node_pf_analysis(fresh.h, 0, 1.0, 1.0, 0.5), BAD, analysis)
    fresh.close()


# ---- shards and segments that do not exist -----------------------------------------------------------------------------
def test_shards_and_segments_out_of_range(inputs):
    L = sa.lib()
    nd = make_node(inputs)
    a, c = C.c_int32(-7), C.c_int32(-7)
    i3 = [C.c_int32(-7) for _ in range(3)]
    nd.run_gathering_reduced(0, T, 2, "sums", K)
    for h, ks in ((nd.h, (-1, nd.n)), (None, (0,))):
        for k in ks:
            for f in ("batch", "stream", "planes", "stats", "gathered_stats", "gathered_planes", "pf_ancestors"):
                assert getattr(L, "sipnet_node_" + f)(h, k) is None, f
            refused_silently(lambda: L.sipnet_node_member_range(h, k, C.byref(a), C.byref(c)))
            refused_silently(lambda: L.sipnet_node_site_range(h, k, C.byref(a), C.byref(c)))
            assert L.sipnet_node_gathered_segment(h, k, 0, C.byref(a), C.byref(c)) is None
            assert L.sipnet_node_gathered_reduced(h, k, 0, *[C.byref(x) for x in i3]) is None
    for k in range(nd.n):
        for f in ("batch", "stream", "planes"):
            assert getattr(L, "sipnet_node_" + f)(nd.h, k) is not None, f
        assert L.sipnet_node_member_range(nd.h, k, None, None) == 0 and L.sipnet_node_site_range(nd.h, k, None, None) == 0
        assert L.sipnet_node_gathered_reduced(nd.h, k, 1, None, None, None) is not None
        for segment in (-1, 2, 3):                                     # two segments: before, at and past the count
            assert L.sipnet_node_gathered_reduced(nd.h, k, segment, *[C.byref(x) for x in i3]) is None
            assert L.sipnet_node_gathered_segment(nd.h, k, segment, C.byref(a), C.byref(c)) is None
    nd.setup()
    nd.run_gathering(0, T, 3)
    for k in range(nd.n):
        assert L.sipnet_node_gathered_segment(nd.h, k, 2, None, None) is not None
        for segment in (-1, 3, 4):
            assert L.sipnet_node_gathered_segment(nd.h, k, segment, C.byref(a), C.byref(c)) is None
        for segment in (-1, 0, 3):                                     # the planes themselves travelled: nothing reduced
            assert L.sipnet_node_gathered_reduced(nd.h, k, segment, *[C.byref(x) for x in i3]) is None
    nd.setup()
    nd.run(0, T)                                                       # a plain run: no segments at all
    for k in range(nd.n):
        assert L.sipnet_node_gathered_segment(nd.h, k, 0, C.byref(a), C.byref(c)) is None
        assert L.sipnet_node_gathered_reduced(nd.h, k, 0, *[C.byref(x) for x in i3]) is None
    assert [x.value for x in [a, c] + i3] == [-7] * 5                  # a refused call writes nothing
    nd.close()


# ---- what the node remembers of its last run -------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,shard,fast", [((0, 0), SHARD_MEMBERS, True), ((0, 0), SHARD_SITES, True), ((0,), SHARD_MEMBERS, True),
                                                ((0, 0), SHARD_MEMBERS, False)],
                         ids=["members-2-shards", "sites-2-shards", "rccl-one-rank", "strict-2-shards"])
def test_the_last_run_across_calls_on_one_node(inputs, one_batch, devices, shard, fast):
    L = sa.lib()
    want, want_stats, want_sums = one_batch[fast]
    nd = make_node(inputs, devices=devices, shard=shard, fast=fast)
    in_kernel = int(all(L.sipnet_batch_sums_in_kernel(L.sipnet_node_batch(nd.h, k)) for k in range(nd.n)))
    assert in_kernel == int(fast)

    def plain_run():
        nd.setup()
        nd.run(0, T)
        assert L.sipnet_node_n_segments(nd.h) == 0 and L.sipnet_node_reduced_in_kernel(nd.h) == 0
        got = nd.gather_stats()
        if shard == SHARD_SITES or nd.n == 1:
            np.testing.assert_array_equal(got, want_stats)
        else:                                                          # (the shards' sums added up: another order of additions)
            np.testing.assert_allclose(got, want_stats, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(nd.member_planes(), want)
        nd.gather_planes()
        nd.sync()
        for k in range(nd.n):
            gp = nd.gathered_planes(k)
            for q in range(nd.n):
                (m0, mc), (s0, sc) = nd.member_range(q), nd.site_range(q)
                np.testing.assert_array_equal(gp[q][:, :, :sc * mc].reshape(3, T, sc, mc), want[:, :, s0:s0 + sc, m0:m0 + mc])
                assert (gp[q][:, :, sc * mc:] == 0).all()

    plain_run()
    nd.setup()
    nd.run_gathering(0, T, 3)
    assert L.sipnet_node_n_segments(nd.h) == 3 and L.sipnet_node_reduced_in_kernel(nd.h) == 0
    for k in range(nd.n):
        np.testing.assert_array_equal(nd.gathered_member_planes(k), want)
    assert L.sipnet_node_run_gathering(nd.h, 0, T, 0) == BAD           # a refused call changes nothing of it
    assert L.sipnet_node_n_segments(nd.h) == 3
    nd.setup()
    nd.run_gathering_reduced(0, T, 2, "sums", K)
    assert L.sipnet_node_n_segments(nd.h) == 2 and L.sipnet_node_reduced_in_kernel(nd.h) == in_kernel
    for k in range(nd.n):
        got = nd.gathered_reduced_member_rows(k)
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want_sums)
    nd.setup()
    nd.run_gathering_reduced(0, T, 4, "f32")
    assert L.sipnet_node_n_segments(nd.h) == 4 and L.sipnet_node_reduced_in_kernel(nd.h) == 0
    for k in range(nd.n):
        got = nd.gathered_reduced_member_rows(k)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want.astype(np.float32))
    plain_run()
    assert (nd.status() == 0).all()
    nd.close()
