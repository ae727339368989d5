"""What the particle filter's peer path refuses (pf.hip: sipnet_batch_pf_connect, sipnet_batch_resample,
sipnet_batch_pf_resample_peers): the error code, a piece of the message, and that a refused call leaves state, rings and
parameters bit for bit as they were.  After a refused connect the batch is not connected (sipnet_batch_pf_info: world 1) and
a publish + connect + exchange gives the ancestors and the state of a batch that never saw the refusal.  Every batch gives
its device and pinned bytes back (sipnet_debug_live_bytes).  All refusals are host-side argument checks: none launches a
kernel on the bad input.  One site x 256 members, fp64, a 48-step forecast."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd._lib import PfPeer
from tests import helpers

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
DEV = "cuda"
T, N = 48, 256
BAD = _lib.ERR_BAD_ARGUMENT


@pytest.fixture(scope="module")
def inputs():
    base = sa.read_params(BASE, sa.flags_from())[0]
    clim = synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(2 * T)))
    return clim, synth.perturbed_params(base, N, seed=17)


def live():
    gc.collect()
    sa.lib().sipnet_pf_release_scratch()
    return sa.debug_live_bytes()


@pytest.fixture
def forecast(inputs):
    """-> a function that makes a batch after its 48-step forecast, (batch, planes); on the way out every batch made is
    closed and the library holds the bytes it held before the first was made"""
    before = live()
    made = []

    def make():
        clim, members = inputs
        b = sa.Batch(sa.flags_from(), 1, N, sa.F64, fast_math=True)
        made.append(b)
        b.set_climate(0, clim)
        b.set_params(0, members)
        b.setup()
        planes, _ = b.run(0, T)
        return b, planes

    yield make
    for b in made:
        b.close()
    assert live() == before


def snapshot(b):
    return [x.copy().view(np.uint8) for x in (b.get_state(), b.get_rings(), b.get_params())]


def assert_untouched(b, before):
    for got, want in zip(snapshot(b), before):
        np.testing.assert_array_equal(got, want)


def weights_block(b, planes):
    """the gathered buffer of a world of two whose ranks are both this batch; rank 0's weights raised, so that it holds more
    than half of the total and some of rank 1's particles (the upper half of the draw) take their ancestors from it"""
    tot = planes[0].double().sum(0)
    obs, sigma = float(tot.median()), float(tot.std()) * 0.5 + 1e-12
    g = torch.empty((2, b.pf_block_len()), dtype=torch.float64, device=DEV)
    b.pf_local_weights(planes[0], obs, sigma, g[1])
    g[0] = g[1] + 0.35
    return g


def exchange(b, planes):
    """publish, connect to a world of two (this batch twice, as rank 1), one exchange -> ancestors, state bytes"""
    d = b.pf_publish(with_params=True)
    b.pf_connect([d] * 2, 1)
    assert b.pf_info()["world"] == 2
    anc = b.pf_resample_peers(weights_block(b, planes), 0.29).cpu().numpy()
    return anc, b.get_state().view(np.uint8)


@pytest.fixture(scope="module")
def never_refused(inputs):
    clim, members = inputs
    b = sa.Batch(sa.flags_from(), 1, N, sa.F64, fast_math=True)
    b.set_climate(0, clim)
    b.set_params(0, members)
    b.setup()
    planes, _ = b.run(0, T)
    want = exchange(b, planes)
    b.close()
    assert len(np.unique(want[0])) < N and (want[0] // N == 0).any() and (want[0] // N == 1).any()
    return want


def refused(call, code, text):
    with pytest.raises(sa.SipnetError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


def assert_connects_as_if_never_refused(b, planes, never_refused):
    assert b.pf_info()["world"] == 1
    anc, state = exchange(b, planes)
    np.testing.assert_array_equal(anc, never_refused[0])
    np.testing.assert_array_equal(state, never_refused[1])


def test_connect_with_a_descriptor_from_before_a_resampling(forecast, never_refused):
    b, planes = forecast()
    d = b.pf_publish(with_params=True)
    b.resample(torch.arange(N, dtype=torch.int32, device=DEV))         # (every column its own ancestor: the buffers swap)
    before = snapshot(b)
    refused(lambda: b.pf_connect([d] * 2, 1), BAD, "not what this batch published")
    assert_untouched(b, before)
    assert_connects_as_if_never_refused(b, planes, never_refused)


@pytest.mark.parametrize("field", ["precision", "with_params"])
def test_connect_with_a_peer_of_another_precision_or_parameter_mode(forecast, never_refused, field):
    b, planes = forecast()
    d = b.pf_publish(with_params=True)
    b.pf_connect([d] * 2, 1)                                           # (a connection that the refused call takes down)
    assert b.pf_info()["world"] == 2
    d = b.pf_publish(with_params=True)
    other = PfPeer.from_buffer_copy(d)
    setattr(other, field, 1 - getattr(other, field))
    before = snapshot(b)
    refused(lambda: b.pf_connect([bytes(other), d], 1), BAD, "another precision")
    assert_untouched(b, before)
    assert_connects_as_if_never_refused(b, planes, never_refused)


@pytest.mark.parametrize("world,rank", [(0, 0), (17, 0), (1, 1), (2, 2)])
def test_connect_with_a_world_or_rank_out_of_range(forecast, never_refused, world, rank):
    b, planes = forecast()
    d = b.pf_publish(with_params=True)
    arr = (PfPeer * 17)(*[PfPeer.from_buffer_copy(d) for _ in range(17)])
    before = snapshot(b)
    assert b.L.sipnet_batch_pf_connect(b.h, world, rank, arr) == BAD
    assert b"sipnet_batch_pf_connect: bad argument" in b.L.sipnet_last_error()
    assert_untouched(b, before)
    assert_connects_as_if_never_refused(b, planes, never_refused)


def test_resample_without_parameters_on_a_batch_connected_with_a_bank(forecast):
    b, _ = forecast()
    d = b.pf_publish(with_params=True)
    b.pf_connect([d] * 2, 1)
    assert b.pf_info()["params_by_index"] == 1
    before = snapshot(b)
    refused(lambda: b.resample(torch.arange(N, dtype=torch.int32, device=DEV), with_params=False), BAD, "resample with_params")
    assert_untouched(b, before)
    assert b.pf_info()["world"] == 2 and b.pf_info()["params_by_index"] == 1


@pytest.mark.parametrize("with_params", [False, True])
def test_resample_with_a_negative_block_size(forecast, with_params):
    b, _ = forecast()
    recv = torch.zeros((b.L.sipnet_batch_member_words(b.h, int(with_params)), 4), dtype=torch.float64, device=DEV)
    before = snapshot(b)
    refused(lambda: b.resample(torch.arange(N, dtype=torch.int32, device=DEV), recv, (4, -1), with_params), BAD,
            "negative block size")
    assert_untouched(b, before)


@pytest.mark.parametrize("with_params", [False, True])
def test_resample_with_columns_announced_and_no_buffer(forecast, with_params):
    b, _ = forecast()
    before = snapshot(b)
    refused(lambda: b.resample(torch.arange(N, dtype=torch.int32, device=DEV), None, (3,), with_params), BAD,
            "no buffer given")
    assert_untouched(b, before)


def test_resample_peers_after_new_parameters_on_a_connected_batch(forecast, inputs):
    b, planes = forecast()
    d = b.pf_publish(with_params=True)
    b.pf_connect([d] * 2, 1)
    g = weights_block(b, planes)
    before = snapshot(b)
    b.set_params(0, inputs[1])                                          # (the same values: the rows convert to the same bits)
    refused(lambda: b.pf_resample_peers(g, 0.29), BAD, "connect again")
    assert_untouched(b, before)
    assert b.pf_info()["params_by_index"] == 0                         # (the bank is gone ...)
    d = b.pf_publish(with_params=True)                                 # (... and a new connection brings a new one)
    b.pf_connect([d] * 2, 1)
    b.pf_resample_peers(g, 0.29)
    assert b.pf_info()["params_by_index"] == 1 and b.pf_info()["cycles"] == 1
