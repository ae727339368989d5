"""The ensemble statistics -- per (step, site) the sum and the sum of squares over the members -- at their size, alignment
and chunk edges, against the exact sums (tests/stats_reference.py: math.fsum over error-free terms) and the bounds any order
of double additions stays within.

A  Batch.reduce_plane (reducePlaneKernel) on crafted planes: every member count next to a branch of the kernel (a
   wavefront, the 16-byte loads' tails, the four-accumulator loop from 386 doubles / 772 floats), one and three sites
   (an odd count puts sites 1 and 2 off the 16-byte alignment), padded rows full of NaN, a plane that begins one element
   into its allocation: integer-valued data exactly, normal data within the bounds.
B  special values: equal values, zeros of both signs, denormals, a large mean, squares that overflow, infinities, a NaN
   in one site only.
C  a site's numbers do not depend on its neighbours or on the call; exactly rows x n_sites x 2 doubles are written.
D  2^26 + 5 cells: past the launch's former limit of 2^32 threads in the grid's x dimension.
E  Batch.run_stats where the launch itself sums (coop_stats.inc, finishStatsKernel): 1, 7, 8, 9, 16 and 17 chunks per
   site with full, ragged and nearly empty last chunks; one launch, launches cut off the tiles and the staged halves, a
   padded pitch, planes one element off alignment.
F  the three reduction passes behind the one-wavefront and strict kernels at the same edges.

Every case prints `stats-ratio <path>: <worst error / bound of the sums> <of the sums of squares>` before it asserts."""
import functools
import os

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from tests import helpers
from tests import stats_reference as sr
from tests.regime_gpu_common import COOP, FLAG_SETS, batch, bits, family_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.float64, torch.float32]
DTYPE_IDS = ["f64", "f32"]


def bare(n_sites, M, prec=sa.F64):
    """a batch that was created and nothing else: all that reduce_plane needs"""
    return sa.Batch(sa.flags_from(), n_sites, M, prec)


def widened(host, dtype):
    """what the device reads of host through a tensor of dtype, as doubles"""
    return np.asarray(host, dtype=np.float64).astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)


def on_device(host, dtype, pad=0, offset=0):
    """host [rows][ncol] -> a contiguous device tensor [rows][ncol + pad] of dtype that begins `offset` elements into its
    allocation; the padding (and the elements in front) full of NaN, so that any read of them shows"""
    host = np.asarray(host, dtype=np.float64)
    rows, ncol = host.shape
    flat = torch.full((rows * (ncol + pad) + offset,), NAN, dtype=dtype, device=DEV)
    plane = flat[offset:].view(rows, ncol + pad)
    plane[:, :ncol] = torch.tensor(host, dtype=dtype, device=DEV)
    assert plane.is_contiguous() and plane.data_ptr() == flat.data_ptr() + offset * flat.element_size()
    return plane


def report(path, r):
    """print the worst ratios of r [..][2] and require them inside the bounds"""
    r1, r2 = float(r[..., 0].max()), float(r[..., 1].max())
    print(f"stats-ratio {path}: {r1:.4f} {r2:.4f}")
    assert r1 <= 1.0 and r2 <= 1.0, (path, r1, r2)


# ---- A: reduce_plane on crafted planes --------------------------------------------------------------------------------------
MEMBERS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 386, 387, 511, 512, 513, 767, 768, 771, 772, 773,
           1023, 1024, 1025, 4097]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("M", MEMBERS)
def test_reduce_plane_at_every_size_pitch_and_alignment(M, dtype):
    """integer-valued data (|x| <= 2^20: every partial sum, of squares too, is an integer below 2^53, exact in any order):
    equality; normal data x 3 - 1 with ties: inside the bounds.  With padding, Batch.reduce_plane takes the pitch from the
    tensor and sums the first ncol columns of each row"""
    rng = np.random.default_rng(4000 + M)
    ROWS, SITES = 5, 3
    ints = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(ROWS, SITES * M)).astype(np.float64)
    ints[0, :min(M, 4)] = 2.0 ** 20                                   # (the largest value is there)
    real = rng.standard_normal((ROWS, SITES * M)) * 3.0 - 1.0
    real[:, ::5] = real[:, :1]                                        # ties
    real = widened(real, dtype)
    worst = np.zeros(2)
    for n_sites in (1, 3):
        b = bare(n_sites, M)
        for rows in (1, 5):
            xi, xr = ints[:rows, :n_sites * M], real[:rows, :n_sites * M]
            want = sr.plane_stats(xi, n_sites, M)
            bounds = sr.stats_bounds(xr, n_sites, M)
            for pad in (0, 1, 3, 7):
                for offset in (0, 1):
                    what = (M, n_sites, rows, pad, offset)
                    got = b.reduce_plane(on_device(xi, dtype, pad, offset)).cpu().numpy()
                    assert got.shape == want.shape and np.array_equal(got, want), what
                    got = b.reduce_plane(on_device(xr, dtype, pad, offset)).cpu().numpy()
                    r = sr.ratios(got, xr, n_sites, M, bounds)
                    worst = np.maximum(worst, r.reshape(-1, 2).max(axis=0))
                    assert (r <= 1.0).all(), (what, r.max())
        b.close()
    report(f"reduce-kernel {DTYPE_IDS[DTYPES.index(dtype)]} M={M}", worst[None, :])


def test_the_c_abi_takes_a_pitch_of_its_own():
    """sipnet_batch_reduce_plane with an ld the tensor's shape does not show: every other row of a plane, by twice its pitch"""
    import ctypes as C
    n_sites, M, rows = 3, 130, 4
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2 * rows, n_sites * M + 3)) * 3.0 - 1.0
    plane = torch.tensor(x, dtype=torch.float64, device=DEV)
    stats = torch.full((rows, n_sites, 2), -7.0, dtype=torch.float64, device=DEV)
    b = bare(n_sites, M)
    rc = sa.lib().sipnet_batch_reduce_plane(b.h, C.c_void_p(plane.data_ptr()), 0, rows, 2 * plane.shape[1], C.c_void_p(stats.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, sa.lib().sipnet_last_error()
    report("reduce-kernel f64 every other row", sr.ratios(stats.cpu().numpy(), x[::2], n_sites, M))
    b.close()


def test_the_binding_refuses_what_it_cannot_pass_on():
    b = bare(2, 8)
    good = torch.zeros((3, 16), dtype=torch.float64, device=DEV)
    stats = torch.full((3, 2, 2), -7.0, dtype=torch.float64, device=DEV)
    bad = {"a host tensor": good.cpu(), "an integer tensor": good.to(torch.int64), "a half tensor": good.to(torch.float16),
           "columns with a stride": torch.zeros((3, 32), dtype=torch.float64, device=DEV)[:, ::2],
           "rows that are a slice of wider ones": torch.zeros((3, 20), dtype=torch.float64, device=DEV)[:, :16],
           "fewer than ncol columns": good[:, :15].contiguous(), "one dimension": good.reshape(-1), "no tensor": good.cpu().numpy()}
    for name, plane in bad.items():
        with pytest.raises(ValueError, match="reduce_plane"):
            b.reduce_plane(plane, stats)
    with pytest.raises(ValueError, match="reduce_plane"):
        b.reduce_plane(good, stats[:2])
    torch.cuda.synchronize()
    assert (stats == -7.0).all()
    planes = torch.zeros((3, 4, 16), dtype=torch.float64, device=DEV)
    bad = {"a host tensor": planes.cpu(), "floats for a batch of doubles": planes.float(), "two planes": planes[:2],
           "columns with a stride": torch.zeros((3, 4, 32), dtype=torch.float64, device=DEV)[:, :, ::2],
           "rows that are a slice of wider ones": torch.zeros((3, 4, 20), dtype=torch.float64, device=DEV)[:, :, :16],
           "fewer than ncol columns": planes[:, :, :15].contiguous(), "fewer rows than steps": planes[:, :3]}
    for name, p in bad.items():
        with pytest.raises(ValueError, match="run_stats"):                   # (raised before the batch is looked at: it is not set up)
            b.run_stats(0, 4, planes=p)
    b.close()


# ---- B: special values ------------------------------------------------------------------------------------------------------
def special_plane(name, rng, M, dtype):
    """-> [1][3 M] doubles (None: the element type cannot hold the case)"""
    f32 = dtype == torch.float32
    n = 3 * M
    x = rng.standard_normal(n) * 3.0 - 1.0
    if name == "all_equal":
        x[:] = 0.1
    elif name == "zeros_of_both_signs":
        x = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    elif name == "denormals":
        x = (2.0 ** -149 if f32 else 5e-324) * (1.0 + np.arange(n) % 1000)
    elif name == "large_mean":
        x = 1e6 + 1e-3 * rng.standard_normal(n)
    elif name == "squares_overflow":
        if f32:
            return None
        x = np.where(rng.random(n) < 0.5, 1e160, -1e160)
    elif name == "inf_in_one_site":
        x[M + 5] = np.inf
    elif name == "both_infinities_in_one_site":
        x[M + 5], x[2 * M - 1] = np.inf, -np.inf
    elif name == "nan_in_site_1_only":
        x[2 * M - 1] = np.nan
    else:
        raise KeyError(name)
    return widened(x, dtype)[None, :]


SPECIALS = ["all_equal", "zeros_of_both_signs", "denormals", "large_mean", "squares_overflow", "inf_in_one_site",
            "both_infinities_in_one_site", "nan_in_site_1_only"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", SPECIALS)
def test_reduce_plane_of_special_values(name, dtype):
    """M = 67: every site ragged, sites 1 and 2 off alignment (element by element); M = 776: aligned rows, the
    four-accumulator loop and its tail in both element types.  The affected cells equal the reference as values (a NaN
    equals a NaN), every other cell stays within its bound"""
    inf = np.inf
    for M in (67, 776):
        x = special_plane(name, np.random.default_rng(77 + M), M, dtype)
        if x is None:
            assert name == "squares_overflow"                              # (1e160 is no float: the double plane carries the case)
            return
        b = bare(3, M)
        got = b.reduce_plane(on_device(x, dtype)).cpu().numpy()
        b.close()
        want = sr.plane_stats(x, 3, M)
        if name == "inf_in_one_site":
            assert tuple(want[0, 1]) == (inf, inf) and np.isfinite(want[0, [0, 2]]).all()
        elif name == "both_infinities_in_one_site":
            assert np.isnan(want[0, 1, 0]) and want[0, 1, 1] == inf and np.isfinite(want[0, [0, 2]]).all()
        elif name == "nan_in_site_1_only":
            assert np.isnan(want[0, 1]).all() and np.isfinite(want[0, [0, 2]]).all()
        elif name == "squares_overflow":
            assert (want[0, :, 1] == inf).all() and np.isfinite(want[0, :, 0]).all()
        elif name == "zeros_of_both_signs":
            assert (want == 0.0).all()
        elif name == "denormals":
            assert (want[0, :, 0] > 0.0).all() and ((want[0, :, 1] == 0.0).all() if dtype == torch.float64 else (want[0, :, 1] > 0.0).all())
        special = ~np.isfinite(want)
        assert np.array_equal(got[special], want[special], equal_nan=True), (name, M, got, want)
        report(f"reduce-kernel {DTYPE_IDS[DTYPES.index(dtype)]} {name} M={M}", sr.ratios(got, x, 3, M))


# ---- C: isolation and repetition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("M", [65, 776])
def test_a_site_depends_on_nothing_but_its_own_values(M, dtype):
    rng = np.random.default_rng(M)
    rows, S = 5, 3
    x = rng.standard_normal((rows, S * M)) * 3.0 - 1.0
    y = x.copy()
    y[:, :M] = rng.standard_normal((rows, M)) * 1e3                    # the neighbours change, one of them to a NaN
    y[:, 2 * M:] = -x[:, 2 * M:]
    y[2, 2 * M] = np.nan
    b = bare(S, M)
    # a statistics block in the middle of a larger buffer: exactly rows x n_sites x 2 doubles are rewritten
    buf = torch.full((rows * S * 2 + 16,), -7.0, dtype=torch.float64, device=DEV)
    block = buf[8:-8].view(rows, S, 2)
    px = on_device(x, dtype, pad=3)
    out = b.reduce_plane(px, block)
    assert out.data_ptr() == block.data_ptr()
    first = buf.clone()
    assert (first[:8] == -7.0).all() and (first[-8:] == -7.0).all() and int((first != -7.0).sum()) == rows * S * 2
    again = b.reduce_plane(px)                                         # the same call, another block
    assert torch.equal(bits(again), bits(block))
    other = b.reduce_plane(on_device(y, dtype, pad=3))
    assert torch.equal(bits(other[:, 1]), bits(block[:, 1]))
    assert not torch.equal(bits(other[:, 0]), bits(block[:, 0])) and not torch.equal(bits(other[:, 2]), bits(block[:, 2]))
    b.close()


# ---- D: the large grid ----------------------------------------------------------------------------------------------------------
def test_reduce_plane_of_more_cells_than_one_grid_row_of_wavefronts():
    """n_steps * n_sites = 2^26 + 5 one-member cells of a float plane (256 MiB): a wavefront per cell in the grid's x
    dimension would need 2^32 + 320 threads there.  Every cell's sums are its value and its square as doubles, exactly"""
    n = 2 ** 26 + 5
    g = torch.Generator(device=DEV)
    g.manual_seed(26)
    x = torch.randn((n, 1), dtype=torch.float32, device=DEV, generator=g)
    b = bare(1, 1, sa.F32_MIXED)
    stats = b.reduce_plane(x)
    b.close()
    assert stats.shape == (n, 1, 2)
    xd = x[:, 0].double()
    assert torch.equal(stats[:, 0, 0], xd)
    assert torch.equal(stats[:, 0, 1], xd * xd)                        # (24 significant bits squared: exact in a double)
    assert float(xd[-5:].abs().min()) > 0.0 and float(stats[-1, 0, 1]) > 0.0


# ---- E, F: run_stats ------------------------------------------------------------------------------------------------------------
T = 53                                                                 # three tiles of 16 and 5 steps
CUTS = [0, 1, 2, 19, 35, T]                                            # a one-step launch, one inside a tile, ones off the tiles and the staged halves
DATA = os.path.join(helpers.REPO, "sipnet_amd", "data")


@functools.lru_cache(maxsize=None)
def clims(n_sites):
    return [synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T, site=s))) for s in range(n_sites)]


@functools.lru_cache(maxsize=None)
def base_of(flagset):
    flags = sa.flags_from(**FLAG_SETS[flagset])
    return flags, sa.read_params(os.path.join(DATA, "base_forest.param" if flagset == "default" else "allflags_forest.param"), flags)[0]


def chunk_sizes(c):
    return [64 * c, 64 * c - 1, 64 * (c - 1) + 2, 64 * (c - 1) + 1]


def planes_like(b, pad=0, offset=0):
    """zero-filled planes [3][T][ncol + pad] that begin `offset` elements into their allocation; the padding full of NaN"""
    ld = b.ncol + pad
    flat = torch.zeros((3 * T * ld + offset,), dtype=b.out_dtype, device=b.device)
    planes = flat[offset:].view(3, T, ld)
    planes[:, :, b.ncol:] = NAN
    return planes


def run_stats_every_way(tag, family, flagset, prec, kernel, options, n_sites, M, strict=False, edited=False):
    """one batch of n_sites x M, run plainly and with statistics in one launch, once more, in launches cut at CUTS, with a
    padded pitch and with planes one element off alignment.  edited: at site 0 one member never runs and one starves"""
    flags, base = base_of(flagset)
    members = synth.perturbed_params(base, M, seed=40 + M)
    b = batch(flags, clims(n_sites), members, prec, kernel, options, strict=strict)
    if edited:
        ed = members.copy()
        ed[min(5, M - 1), pi("leafAllocation")] = 0.9                    # never runs (status 3)
        ed[min(5, M - 1), pi("woodAllocation")] = 0.9
        if M > 9:
            ed[9, pi("plantWoodInit")] = 1e-4                            # starves
            ed[9, pi("laiInit")] = 1e-4
        b.set_params(0, ed)
        b.setup()
    S, ncol = n_sites, n_sites * M
    plain = planes_like(b)
    b.run(0, T, planes=plain)
    status = b.get_status()
    ran = torch.as_tensor(status == 0, device=plain.device)
    assert bool(ran.all()) != edited, status[status != 0]

    def launch(pad=0, offset=0, cuts=(0, T)):
        b.setup()
        planes = planes_like(b, pad, offset)
        stats = torch.full((3, T, S, 2), NAN, dtype=torch.float64, device=b.device)
        for a, z in zip(cuts[:-1], cuts[1:]):
            _, st = b.run_stats(a, z - a, planes=planes[:, a:z])
            stats[:, a:z] = st
        name = b.last_launch()["kernel"]
        assert family_ok(family, flagset, name) and ("double" if prec == sa.F64 else "float") in name, (tag, name)
        assert np.array_equal(b.get_status(), status), tag
        assert torch.isnan(planes[:, :, ncol:]).all(), tag                # the padding: never written
        assert torch.equal(bits(planes[:, :, :ncol][:, :, ran]), bits(plain[:, :, ran])), tag + ": planes"
        return planes[:, :, :ncol], stats

    single, again, cut = launch(), launch(), launch(cuts=CUTS)
    padded, shifted = launch(pad=2), launch(offset=1)
    b.close()
    assert torch.equal(bits(again[1]), bits(single[1])), tag + ": a repeated launch"
    # a row's sums do not depend on where the launches were cut, and the chunks are added in index order.  (What a member
    # that never runs leaves in its columns does depend on the cuts, tests/test_gpu_sums.py: its site is left out here and
    # held to the planes as read back below)
    first = 1 if edited else 0
    assert torch.equal(bits(cut[1][:, :, first:]), bits(single[1][:, :, first:])), tag + ": cut launches"
    worst = np.zeros(2)
    bounds = None
    for planes, stats in (single, cut, padded, shifted):
        x = planes.double().cpu().numpy().reshape(3 * T, ncol)
        if bounds is None or edited:
            bounds = sr.stats_bounds(x, S, M)
        r = sr.ratios(stats.cpu().numpy().reshape(3 * T, S, 2), x, S, M, bounds)
        worst = np.maximum(worst, r.reshape(-1, 2).max(axis=0))
    return worst


CHUNKS = [(c, 1) for c in (1, 7, 8, 9, 16, 17)] + [(c, 3) for c in (1, 8, 9)]
PRECS = [(sa.F64, "f64"), (sa.F32_MIXED, "f32")]


@pytest.mark.parametrize("c,n_sites", CHUNKS, ids=[f"c{c}x{s}" for c, s in CHUNKS])
@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("family", sorted(COOP))
def test_run_stats_where_the_launch_sums(family, prec, pname, c, n_sites):
    """the cooperative kernels with SIPNET_KOPT_STATS_IN_KERNEL: the one-chunk layouts' factor / light wave reads the stored
    tiles (16-byte loads where the chunk is full and everything aligned, else element by element), the two- and four-chunk
    layouts' light wave the staged halves; finishStatsKernel adds c chunks per site, eight at a time and a tail"""
    worst = np.zeros(2)
    for M in chunk_sizes(c):
        edited = (c, n_sites) == (8, 3) and M == 64 * c - 1
        tag = f"{family} {pname} c={c} sites={n_sites} M={M}"
        worst = np.maximum(worst, run_stats_every_way(tag, family, "default", prec, COOP[family], sa.KOPT_STATS_IN_KERNEL, n_sites, M,
                                                      edited=edited))
    report(f"in-launch {family} {pname} c={c} sites={n_sites}", worst[None, :])


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("family", ["coop_lds", "coop_pair"])
def test_run_stats_of_the_optional_physics_instantiations(family, prec, pname):
    """stepCoopX...: growth respiration, leaf water, litter pool on, the moisture effect off; three sites of 64 * 2 + 9"""
    M = 64 * 2 + 9
    worst = run_stats_every_way(f"{family} russell_3 {pname} M={M}", family, "russell_3", prec, COOP[family], sa.KOPT_STATS_IN_KERNEL, 3, M)
    report(f"in-launch {family} russell_3 {pname} c=3 sites=3", worst[None, :])


THREE_PASS = [("one_wave", sa.KERNEL_ONE_WAVE, sa.F64, False), ("one_wave", sa.KERNEL_ONE_WAVE, sa.F32_MIXED, False),
              ("strict", sa.KERNEL_STRICT, sa.F64, True)]


@pytest.mark.parametrize("family,kernel,prec,strict", THREE_PASS, ids=["one_wave_f64", "one_wave_f32", "strict_f64"])
def test_run_stats_by_the_three_passes(family, kernel, prec, strict):
    """the kernels that do not sum in their launch are followed by three reducePlaneKernel passes: nine chunks per site, the
    last one holding one member (odd rows: sites 1 and 2 off alignment) and full"""
    worst = np.zeros(2)
    for M in (64 * 8 + 1, 64 * 9):
        tag = f"{family} {'f64' if prec == sa.F64 else 'f32'} sites=3 M={M}"
        worst = np.maximum(worst, run_stats_every_way(tag, family, "default", prec, kernel, 0, 3, M, strict=strict))
    report(f"three-pass {family} {'f64' if prec == sa.F64 else 'f32'} c=9 sites=3", worst[None, :])
