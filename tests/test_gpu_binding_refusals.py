"""What the Python binding itself refuses or keeps (sipnet_amd/batch.py, dist.py, node.py), before or around the library call:
the ValueErrors of plane_quantiles, of the EnKF analyses' shared argument marshalling (through enkf_analysis_sites), of
enkf_analysis_smooth, enkf_shard_moments and enkf_analysis_sharded; out= tensors written in place; the joint analysis and the
smoother without series agreeing bit for bit when the two inflations differ (the argument order of both calls); the gathered
buffers that dist.pf_analysis_peers and dist.enkf_analysis_sharded keep on the batch; Node's assembled planes and per-shard
state against a Batch.  2 sites x 4 members, 8 steps, fp64: a per-site vector (2), a per-column vector (8) and a series of
ncol < ld columns all differ in length (the connected particle filter takes one site only: 1 site x 8 members there)."""
import os

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import dist as sd
from sipnet_amd import synth
from sipnet_amd._lib import NSTATE, RING_SLOTS
from sipnet_amd.node import Node
from tests import helpers

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
DEV = "cuda"
S, M, T = 2, 4, 8
NCOL = S * M
ANALYSED = ["plantWoodC", "plantLeafC", "soilC"]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.fixture(scope="module")
def inputs():
    base = sa.read_params(BASE, sa.flags_from())[0]
    clims = [synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T, site=s))) for s in range(S)]
    return clims, synth.perturbed_params(base, M, seed=3)


def set_up(inputs):
    clims, members = inputs
    b = sa.Batch(sa.flags_from(), S, M, sa.F64, fast_math=True)
    for s in range(S):
        b.set_climate(s, clims[s])
    b.set_params(None, members)
    b.setup()
    return b


def fresh(inputs):
    """a batch after its 8-step forecast -> (batch, planes)"""
    b = set_up(inputs)
    planes, _ = b.run(0, T)
    return b, planes


@pytest.fixture(scope="module")
def shared(inputs):
    """the one batch of the refusals: none of them changes it"""
    b, planes = fresh(inputs)
    yield b, planes
    b.close()


def wood_obs(b):
    """above-ground wood observed 1 % above each site's mean -> (operators, obs [S][1], sd [S][1])"""
    wood = b.get_state()[:, 0].reshape(S, M)
    mean = wood.mean(1, keepdims=True)
    return [sa.enkf_pools(["plantWoodC"])], mean * 1.01, wood.std(1, keepdims=True) + 1e-3 * mean


# ---- plane_quantiles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("series", [lambda: torch.zeros((T, 2 * NCOL), dtype=torch.float64, device=DEV)[:, ::2],
                                    lambda: torch.zeros(NCOL, dtype=torch.float64, device=DEV),
                                    lambda: torch.zeros((T, NCOL - 1), dtype=torch.float64, device=DEV)],
                         ids=["non-contiguous", "1-d", "ld<ncol"])
def test_plane_quantiles_refuses_a_series_it_cannot_read(shared, series):
    b, _ = shared
    with pytest.raises(ValueError) as e:
        b.plane_quantiles(series(), [0.5])
    assert "plane_quantiles" in str(e.value) and "series" in str(e.value)


def test_plane_quantiles_refuses_obs_of_the_wrong_count(shared):
    b, planes = shared
    with pytest.raises(ValueError) as e:
        b.plane_quantiles(planes[0], [0.5], obs=np.zeros(T * S - 1))
    assert "plane_quantiles" in str(e.value) and "obs" in str(e.value)


def test_plane_quantiles_refuses_an_out_count_of_the_wrong_dtype(shared):
    b, planes = shared
    first = b.plane_quantiles(planes[0], [0.25, 0.75])
    with pytest.raises(ValueError) as e:
        b.plane_quantiles(planes[0], [0.25, 0.75], out=(first.quant, first.count.to(torch.int64), None, None))
    assert "plane_quantiles" in str(e.value) and "count" in str(e.value)


def test_plane_quantiles_writes_into_the_out_of_an_earlier_call(shared):
    b, planes = shared
    obs = planes[0].reshape(T, S, M).mean(2)
    want = b.plane_quantiles(planes[0], [0.25, 0.5, 0.75], obs=obs, path=1)
    assert want.crps is not None and want.rank is not None and want.path == 1
    out = b.plane_quantiles(planes[0] + 1.0, [0.25, 0.5, 0.75], obs=obs, path=1)       # (other values, to be overwritten)
    assert not torch.equal(out.quant, want.quant)
    got = b.plane_quantiles(planes[0], [0.25, 0.5, 0.75], obs=obs, path=1, out=out)
    for name in ("quant", "count", "crps", "rank"):
        assert getattr(got, name) is getattr(out, name), name
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.path == want.path


# ---- the EnKF analyses' shared arguments, through enkf_analysis_sites ---------------------------------------------------------
def test_enkf_arguments_of_the_wrong_count_dtype_or_layout_are_value_errors(shared):
    b, planes = shared
    ops, obs, sd_ = wood_obs(b)
    st0 = b.get_state()

    def refused(word, obs=obs, sd_=sd_, **kw):
        with pytest.raises(ValueError) as e:
            b.enkf_analysis_sites(obs, sd_, ops, ANALYSED, **kw)
        assert "enkf_analysis_sites" in str(e.value) and word in str(e.value), str(e.value)

    refused("obs", obs=np.zeros((S, 2)))
    refused("inflation", inflation=[1.0] * (S + 1))
    refused("planes differ", planes=[planes[0], planes[1].float(), None])
    refused("unit column stride", planes=[planes[0][:, ::2], None, None])
    refused("info_out", info_out=torch.zeros((S, 4), dtype=torch.int64, device=DEV))
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))


def test_joint_and_smoother_without_series_agree_bit_for_bit_when_the_inflations_differ(inputs):
    """inflation 1 on the pools, 1.5 on the parameter: the two values swapped would inflate the pools and change the state"""
    results = []
    for smooth in (False, True):
        b, planes = fresh(inputs)
        ops, obs, sd_ = wood_obs(b)
        st0, prm0 = b.get_state(), b.get_params()
        params = [sa.enkf_param("aMax", *synth.PERTURB["aMax"][:2])]
        kw = dict(planes=planes, inflation=np.full(S, 1.0), param_inflation=np.full(S, 1.5))
        if smooth:
            assert b.enkf_analysis_smooth(obs, sd_, ops, ANALYSED, [], params, **kw) == []
        else:
            b.enkf_analysis_joint(obs, sd_, ops, ANALYSED, params, **kw)
        st1, prm1 = b.get_state(), b.get_params()
        b.close()
        assert (st1 != st0).any() and (prm1 != prm0).any()
        results.append((bits(st1), bits(prm1)))
    np.testing.assert_array_equal(results[1][0], results[0][0])
    np.testing.assert_array_equal(results[1][1], results[0][1])


def test_smoother_refuses_a_pair_of_two_dtypes_and_a_series_narrower_than_the_batch(shared):
    b, planes = shared
    ops, obs, sd_ = wood_obs(b)
    st0 = b.get_state()
    with pytest.raises(ValueError) as e:
        b.enkf_analysis_smooth(obs, sd_, ops, ANALYSED, [(planes[0], planes[0].float())])
    assert "enkf_analysis_smooth" in str(e.value) and "series 0" in str(e.value)
    with pytest.raises(ValueError) as e:
        b.enkf_analysis_smooth(obs, sd_, ops, ANALYSED, [torch.zeros((T, NCOL - 1), dtype=torch.float64, device=DEV)])
    assert "enkf_analysis_smooth" in str(e.value) and "columns" in str(e.value)
    np.testing.assert_array_equal(bits(b.get_state()), bits(st0))


def test_sharded_moments_and_analysis_refuse_buffers_of_the_wrong_size(shared):
    b, _ = shared
    ops, obs, sd_ = wood_obs(b)
    W = b.enkf_moment_words(ops, ANALYSED)
    with pytest.raises(ValueError) as e:
        b.enkf_shard_moments(ops, ANALYSED, out=torch.zeros(S * W - 1, dtype=torch.float64, device=DEV))
    assert "enkf_shard_moments" in str(e.value) and "out" in str(e.value)
    with pytest.raises(ValueError) as e:
        b.enkf_analysis_sharded(torch.zeros((1, S, W + 1), dtype=torch.float64, device=DEV), obs, sd_, ops, ANALYSED)
    assert "enkf_analysis_sharded" in str(e.value) and "gathered" in str(e.value)


# ---- the buffers dist keeps on the batch (world 1, no group: no collective) ------------------------------------------------------
def test_pf_analysis_peers_keeps_its_gathered_buffer_and_a_connect_resets_it(inputs):
    """(a connected filter's particles are one site's: the same 8 columns as 1 site x 8 members)"""
    clims, members = inputs
    b = sa.Batch(sa.flags_from(), 1, NCOL, sa.F64, fast_math=True)
    b.set_climate(0, clims[0])
    b.set_params(0, np.concatenate([members, members[::-1] * 1.0]))
    b.setup()
    planes, _ = b.run(0, T)
    tot = planes[0].sum(0)
    obs, sigma = float(tot.median()), float(tot.std()) * 1.5 + 1e-12
    sd.pf_connect_peers(b)
    assert b._pf_gathered is None
    anc, g1 = sd.pf_analysis_peers(b, planes[0], obs, sigma, 0.5)
    assert g1 is b._pf_gathered and tuple(g1.shape) == (1, b.pf_block_len()) and anc.numel() == NCOL
    _, g2 = sd.pf_analysis_peers(b, planes[0], obs, sigma, 0.5)
    assert g2 is g1 and b._pf_gathered is g1
    sd.pf_arm_peers(b, obs, sigma)
    assert b._pf_gathered is g1
    b.pf_connect([b.pf_publish(with_params=True)], 0)
    assert b._pf_gathered is None
    b.close()


def test_enkf_analysis_sharded_keeps_its_gathered_buffer(inputs):
    b, planes = fresh(inputs)
    ops, obs, sd_ = wood_obs(b)
    st0 = b.get_state()
    g1 = sd.enkf_analysis_sharded(b, obs, sd_, ops, ANALYSED, planes=planes)
    assert g1 is b._enkf_gathered and tuple(g1.shape) == (1, S, b.enkf_moment_words(ops, ANALYSED))
    assert (b.get_state() != st0).any()
    g2 = sd.enkf_analysis_sharded(b, obs, sd_, ops, ANALYSED, planes=planes)
    assert g2 is g1 and b._enkf_gathered is g1
    b.close()


# ---- Node on one device against a Batch -------------------------------------------------------------------------------------
def test_node_planes_and_shard_state_equal_the_batch(inputs):
    clims, members = inputs
    b = set_up(inputs)                              # (the node's history: set up once, one run with statistics)
    planes, _ = b.run_stats(0, T)
    nd = Node(sa.flags_from(), S, M, devices=[0], fast_math=True)
    for s in range(S):
        nd.set_climate(s, clims[s])
    nd.set_params(None, members)
    nd.setup()
    nd.run(0, T)
    np.testing.assert_array_equal(nd.member_planes(), planes.cpu().numpy().reshape(3, T, S, M))
    st, rings = nd.shard_state(0), nd.shard_rings(0)
    assert st.shape == (NCOL, NSTATE) and rings.shape == (NCOL, RING_SLOTS)
    np.testing.assert_array_equal(bits(st), bits(b.get_state()))
    # (ring slots no step has written yet are uninitialised memory: slot 0 and the 8 inserts)
    np.testing.assert_array_equal(bits(rings[:, :T + 1]), bits(b.get_rings()[:, :T + 1]))
    nd.close()
    b.close()
