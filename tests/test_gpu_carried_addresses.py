"""The carbon wave's regular-tile step with CARRIED addresses (coop_wave_carbon.inc, `Carried`: the one-chunk LDS-ring kernel of
fp64 batches with the default physics, stepCoopKernel<double, true, true, false> -- c10k's, c2's and c2x16's launch).  What the
step used to derive from t and the slot numbers -- which of a mailbox's two slots, the two ring slots, the posted sequence
number -- is carried from step to step as per-lane LDS addresses and re-seeded at the top of every regular tile; the ring's
wrap is a wave-uniform test.  Everything here is bit for bit against runs the change does not touch: the same batch with the
regular tiles switched off (SIPNET_KOPT_NO_REGULAR_TILES: the general step) and the forced ring-in-HBM kernel.

Shape: 1 site x 65 members (a full chunk and a chunk with one live lane), 1 300 half-hourly steps of the synthetic forcing:
the 250-slot ring wraps five times, and since 250 mod 16 = 10 the wrap falls on another step of a tile each time."""
import os

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from tests import helpers

pytestmark = pytest.mark.gpu
BASE = os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param")
KERNEL = "stepCoopKernel<double, true, true, false>"
M, T = 65, 1300
TOL_F64 = 1e-9          # the bar of tests/test_gpu_configs.py
WHOLE = ((0, T),)
# a first launch that ends at an odd step inside a tile, a one-step launch, a launch that begins inside a tile
SPLIT = ((0, 333), (333, 334), (334, T))
BUILDS = [("product", 0), ("bounded", sa.KOPT_BOUNDED_WAITS)]


@pytest.fixture(scope="module")
def flags():
    return sa.flags_from()


@pytest.fixture(scope="module")
def clim():
    return synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T)))


@pytest.fixture(scope="module")
def members(flags):
    return synth.perturbed_params(sa.read_params(BASE, flags)[0], M)


@pytest.fixture(scope="module")
def starving(members):
    """member 3 of the full chunk loses its roots at step 617, the tenth step of a regular tile (the ring is full from step
    240 on: two evictions a step); its 63 neighbours and the second chunk live on"""
    m = members.copy()
    m[3, pi("plantWoodInit")] *= 5e-5
    return m


def run(flags, clim, members, kernel, options, launches):
    """-> planes[3][T][M], state, rings, the launched kernel's name.  A wait of the bounded build that ran out of polls
    raises (SIPNET_ERR_INTERNAL)."""
    b = sa.Batch(flags, 1, members.shape[0], sa.F64, fast_math=True, kernel=kernel, kernel_options=options)
    b.set_climate(0, clim)
    b.set_params(0, members)
    b.setup()
    planes, _ = b.alloc_outputs(T)
    planes.fill_(float("nan"))
    for a, z in launches:
        b.run(a, z - a, planes=planes[:, a:z])
    out = (planes.cpu().numpy(), b.get_state(), b.get_rings(), b.last_launch()["kernel"])
    b.close()
    return out


@pytest.fixture(scope="module")
def references(flags, clim, members):
    """the whole run by two paths this kernel's regular-tile step has no part in, computed once"""
    general = run(flags, clim, members, sa.KERNEL_COOP_LDS, sa.KOPT_NO_REGULAR_TILES, WHOLE)
    hbm = run(flags, clim, members, sa.KERNEL_COOP_HBM, 0, WHOLE)
    assert general[3] == KERNEL and hbm[3] == "stepCoopKernel<double, true, false, false>"
    for k in range(3):          # (the standing rule: the same bits on every path)
        np.testing.assert_array_equal(general[k], hbm[k])
    assert np.isfinite(general[0]).all()
    return general, hbm


def same(got, want, what):
    for k, name in enumerate(("planes", "final state (totNee among it)", "rings")):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, name))


@pytest.mark.parametrize("name,options", BUILDS, ids=[b[0] for b in BUILDS])
def test_whole_run_equals_the_general_step_and_the_hbm_ring_kernel(name, options, flags, clim, members, references):
    got = run(flags, clim, members, sa.KERNEL_COOP_LDS, options, WHOLE)
    assert got[3] == KERNEL
    same(got, references[0], "regular tiles off")
    same(got, references[1], "ring in HBM")


@pytest.mark.parametrize("name,options", BUILDS, ids=[b[0] for b in BUILDS])
def test_split_launches_reseed_the_carried_values(name, options, flags, clim, members, references):
    """parities, the sequence number and the slot addresses are seeded from t and the tile's record at ANY tBegin"""
    got = run(flags, clim, members, sa.KERNEL_COOP_LDS, options, SPLIT)
    assert got[3] == KERNEL
    same(got, references[0], "split at 333 | 334")


def test_a_member_dying_inside_a_regular_tile(oracle, flags, clim, starving):
    """the dying step and the general steps behind it take t, the ring slots and the alive word from the carried values"""
    _, rec, _ = oracle.run_member(flags, starving[3], clim, None)
    died = int(np.nonzero(rec[:, 20] + rec[:, 21] == 0.0)[0][0])
    assert 300 < died < T - 200 and died % 16 not in (0, 15), died       # in the middle of a tile, the ring long full
    got = run(flags, clim, starving, sa.KERNEL_COOP_LDS, 0, WHOLE)
    gen = run(flags, clim, starving, sa.KERNEL_COOP_LDS, sa.KOPT_NO_REGULAR_TILES, WHOLE)
    assert got[3] == KERNEL
    same(got, gen, "regular tiles off")
    assert int(got[1][3, 30]) == died
    pick = np.r_[0:8, 60:65]
    want, _, so = oracle.run_block(flags, starving[pick], clim)
    assert (so == 0).all()
    d = np.abs(got[0][:, :, pick] - want).max(axis=(1, 2))
    print("member 3 died at step %d: max|dNEE| %.3e |dGPP| %.3e |dET| %.3e" % (died, d[0], d[1], d[2]))
    assert d.max() < TOL_F64


def test_eight_members_against_the_oracle(oracle, flags, clim, members, references):
    got = run(flags, clim, members, sa.KERNEL_COOP_LDS, 0, WHOLE)
    pick = np.r_[0:4, 61:65]                       # both chunks, the lone live lane of the second among them
    want, _, so = oracle.run_block(flags, members[pick], clim)
    assert (so == 0).all()
    d = np.abs(got[0][:, :, pick] - want).max(axis=(1, 2))
    print("max|dNEE| %.3e |dGPP| %.3e |dET| %.3e" % (d[0], d[1], d[2]))
    assert d.max() < TOL_F64
    assert want[1].max() > 0.01 and (want[1] == 0).any()         # photosynthesis by day, none by night: both paths of the step
