"""The step kernels on members far from the one perturbed forest (tests/parameter_regimes.py): every ranged parameter
uniform over its range, with general and with plain exponents; the base with one or two parameters at a bound; hand-set
exact values (pools at 0, Q10s at 1 and one ulp above, fractions at 0 and 1, the last valid allocation and the first
invalid one, the four clamps of the parameter conversion ...) at lanes 0, 63, 64, 127 and in the ragged chunk; and
ensembles around three crop parameter files.  tests/test_parameter_regimes.py shows on the CPU that the oracle is well
conditioned on exactly these members, so the bounds here are the fuzzer's (tools/fuzz_gpu.py), unchanged:

  fp64        every plane value within 1e-9 of the plane maximum (floor 1e-3), pools within 1e-8 (floor 1e-2), the
              oracle's status, and its clamp / balance counters from the families that report them
  fp32-mixed  everything finite, the share of values off by more than 1e-4 of the plane maximum below 2e-3, time sums
              within 2e-3, pools within 5e-3 (floor 1.0)

Members whose oracle planes are not finite (the reference is undefined there: tests/test_parameter_regimes.py caps them
at 5 % of a set) have their VALUES unjudged; their status and every neighbour in their wavefront are judged.  The members
parameter_regimes.f32_excluded names (at most two per regime; tests/test_parameter_regimes.py holds the reasons to what
the oracle does) are left out of the fp32-mixed comparison of values only.  One year of the
synthetic climate, one site unless stated, a forced kernel whose name is asserted; the oracle runs once per (regime,
flag set).

What a throughput kernel leaves in the planes and rings of a member that never runs (status 3: it is advanced like its
neighbours) means nothing, depends on the layout and on where the launches were cut, and is compared nowhere; the
strict-order kernel leaves such a member's columns untouched.  Sums and statistics are the sums of whatever is there.

Achieved on an MI355X (worst over the families; fp64: planes, pools | fp32-mixed: max, share over 1e-4, time sums, pools):
  wide, wide_plain   default, ncycle, russell_3   5.2e-14, 2.1e-11 (strict: 5.7e-16, 4.2e-12) | 1.8e-6, 0, 8.8e-7, 1.6e-3
  corners            default, ncycle, russell_3   4.8e-14, 5.8e-11 (strict: 3.3e-16, 6.3e-13) | 5.1e-7, 0, 7.2e-7, 9.8e-4
  edges              default, russell_3           7.7e-14, 1.6e-11 (strict: 1.0e-15, 1.8e-12) | 9.9e-7, 0, 3.6e-7, 6.6e-4
  edges              ncycle                       5.3e-12, 1.6e-11 (the fAnoxia 1 member: the oracle's own one-ulp figure)
                                                  | 4.4e-7, 0, 3.5e-7, 2.9e-4; with the fAnoxia 1 member judged: 2.4e-3,
                                                  1.8e-3, 2.3e-3, 5.3e-2 -- what the CPU yardstick predicts of it
  crop_1, 2, 3       their flag sets              5.3e-14, 1.6e-11 (strict: 8.9e-16, 2.4e-12) | 1.7e-6, 0, 3.8e-7, 1.3e-4
  counters: equal everywhere (clamp warnings: wide 2, corners 6, edges 13 166 in one member, crop 0; balance warnings 0)
  sums: cooperative kernels bit for bit over the year, skipped members' columns included; one-wavefront kernel over 205
  steps within 6.3e-11 of a member's largest sum (fp32-mixed; fp64: equal), its state within 1.2e-9; statistics within
  4.1e-16 of the largest; every bit identity holds"""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd.config import param_index as pi
from tests import parameter_regimes as pr
from tests.regime_gpu_common import COOP, KERNELS, batch, bits, family_ok, host_sums, judge, outputs, same

pytestmark = pytest.mark.gpu
DEFAULT_REGIMES = ["wide", "wide_plain", "corners", "edges", "crop_1", "crop_2", "crop_3"]
# rows of the converted block (convertParamsKernel)
RATE_ROWS = ["baseVegResp", "litterBreakdownRate", "baseSoilResp", "woodTurnoverRate", "leafTurnoverRate", "fineRootTurnoverRate",
             "coarseRootTurnoverRate", "baseCoarseRootResp", "baseFineRootResp"]
TINY = 1e-6


class Reference:
    """the oracle's planes, final records, status and counters per (regime, flag set), computed once"""

    def __init__(self, oracle):
        self.oracle, self.cache, self.counters, self.clims, self.sets = oracle, {}, {}, {}, {}

    def clim(self, site=0):
        if site not in self.clims:
            self.clims[site] = pr.clim(site)
        return self.clims[site]

    def members(self, regime, flagset="default"):
        if (regime, flagset) not in self.sets:
            self.sets[regime, flagset] = pr.members(regime, flagset)
        return self.sets[regime, flagset]

    def run(self, regime, flagset="default"):
        """-> planes, final, status, lost (members whose oracle planes or pools are not finite)"""
        key = (regime, flagset)
        if key not in self.cache:
            want, final, st = self.oracle.run_block(pr.flags(flagset), self.members(regime, flagset), self.clim())
            lost = ~(np.isfinite(want).all(axis=(0, 1)) & np.isfinite(final).all(axis=1)) & (st == 0)
            self.cache[key] = (want, final, st, lost)
        return self.cache[key]

    def diag(self, regime):
        if regime not in self.counters:
            members, clim, flags = self.members(regime), self.clim(), pr.flags("default")
            out = [self.oracle.run_member(flags, members[m], clim, want_rec=False)[2] for m in range(members.shape[0])]
            self.counters[regime] = (np.array([d.n_clamp_warn for d in out]), np.array([d.n_balance_warn for d in out]))
        return self.counters[regime]


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def plain_exponents(name):
    """the PlainExp argument of a throughput kernel's name (the second one)"""
    return name.split("<", 1)[1].split(",")[1].strip(" >") == "true"


def run_case(ref, regime, flagset, family, prec):
    flags, members, clim = pr.flags(flagset), ref.members(regime, flagset), ref.clim()
    want, final, st, lost = ref.run(regime, flagset)
    b = batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict")
    planes = torch.zeros((3, clim.n_steps, members.shape[0]), dtype=b.out_dtype, device=b.device)
    b.run(planes=planes)
    name = b.last_launch()["kernel"]
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, flagset, name) and ("double" if prec == sa.F64 else "float") in name, (family, name)
    if family != "strict":
        assert plain_exponents(name) == (regime == "wide_plain"), name
    unjudged = lost.copy()
    if prec == sa.F32_MIXED:
        unjudged[pr.f32_excluded(regime, flagset)] = True
    judge(f"{regime} {flagset} {name}", prec, got, state, status, want, final, st, unjudged)
    return name


FAMILIES = [("strict", sa.F64)] + [(f, p) for f in ("one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", FAMILIES, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in FAMILIES])
@pytest.mark.parametrize("regime", DEFAULT_REGIMES)
def test_every_kernel_family_on_every_regime(regime, family, prec, ref):
    run_case(ref, regime, "default", family, prec)


OPTIONAL = [("ncycle", "coop_ncycle"), ("ncycle", "coop_ncycle_pair"), ("ncycle", "one_wave"),
            ("russell_3", "coop_lds"), ("russell_3", "coop_pair"), ("russell_3", "one_wave")]
CROP_OF = {"ncycle": "crop_2", "russell_3": "crop_3"}             # the crop file whose own flags these are


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("flagset,family", OPTIONAL, ids=[a + "-" + b for a, b in OPTIONAL])
@pytest.mark.parametrize("regime", ["wide", "corners", "edges", "crop"])
def test_optional_physics_and_nitrogen_kernels(regime, flagset, family, prec, ref):
    run_case(ref, CROP_OF[flagset] if regime == "crop" else regime, flagset, family, prec)


@pytest.mark.parametrize("regime", ["wide", "corners", "edges", "crop"])
def test_optional_physics_four_chunk_layout(regime, ref):
    """stepCoopXQuadKernel: the fp32-mixed build only (the engine refuses the fp64 one)"""
    run_case(ref, "crop_3" if regime == "crop" else regime, "russell_3", "coop_quad", sa.F32_MIXED)


@pytest.mark.parametrize("family", ["strict", "one_wave", "coop_lds", "coop_hbm", "coop_pair"])      # (no full-state build of the four-chunk layout)
@pytest.mark.parametrize("regime", DEFAULT_REGIMES)
def test_clamp_and_balance_counters_match_the_oracles(regime, family, ref):
    members, clim = ref.members(regime), ref.clim()
    _, _, st, lost = ref.run(regime)
    clamp, balance = ref.diag(regime)
    b = batch(pr.flags("default"), [clim], members, sa.F64, KERNELS[family], strict=family == "strict", diagnostics=True)
    b.run()
    name = b.last_launch()["kernel"]
    d = b.get_diagnostics()
    b.close()
    assert family_ok(family, "default", name), name
    ok = (st == 0) & ~lost
    print(f"{regime} {name}: clamp warnings {int(clamp[ok].sum())} (most {int(clamp[ok].max())}), balance warnings {int(balance[ok].sum())}")
    assert np.array_equal(d["n_clamp_warn"][ok], clamp[ok]) and np.array_equal(d["n_balance_warn"][ok], balance[ok])


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("regime", DEFAULT_REGIMES)
def test_layouts_tile_paths_and_plan_builders_give_the_same_bits(regime, prec, ref):
    """the identities the suite holds on the perturbed forest, on these members: the four cooperative layouts agree bit
    for bit, regular tiles switched off (SIPNET_KOPT_NO_REGULAR_TILES) change nothing -- an edge member decides which
    path its 63 neighbours take -- and neither does who built the plan"""
    flags, members, clim = pr.flags("default"), ref.members(regime), ref.clim()
    first = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS), zeroed=True)
    for name, kernel in COOP.items():
        for opt in (0, sa.KOPT_NO_REGULAR_TILES):
            if (kernel, opt) != (sa.KERNEL_COOP_LDS, 0):
                same(first, outputs(batch(flags, [clim], members, prec, kernel, opt), zeroed=True), f"{name} options {opt}", ran_only=True)
    dev = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_DEVICE_PLAN), zeroed=True)
    host = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_HOST_PLAN), zeroed=True)
    assert dev[3]["plan_device_sites"] == 1 and host[3]["plan_device_sites"] == 0
    same(dev, host, "device plan against host plan", ran_only=True)
    same(first, host, "default against host plan", ran_only=True)


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("flagset,kernel", [("ncycle", sa.KERNEL_COOP_NCYCLE), ("ncycle", sa.KERNEL_COOP_NCYCLE_PAIR),
                                            ("russell_3", sa.KERNEL_COOP_LDS), ("russell_3", sa.KERNEL_COOP_PAIR)],
                         ids=["ncycle", "ncycle_pair", "x_lds", "x_pair"])
def test_regular_tiles_off_change_nothing_under_the_optional_flags(flagset, kernel, prec, ref):
    """... and on `edges` under the other two flag sets, where members 127 and 132 (soilInit 0, litterInit 0) turn
    non-finite inside a full chunk under the nitrogen cycle"""
    flags, members, clim = pr.flags(flagset), ref.members("edges", flagset), ref.clim()
    first = outputs(batch(flags, [clim], members, prec, kernel), zeroed=True)
    same(first, outputs(batch(flags, [clim], members, prec, kernel, sa.KOPT_NO_REGULAR_TILES), zeroed=True), "regular tiles off", ran_only=True)


SUM_KERNELS = [(f, p) for f in ("one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", SUM_KERNELS, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in SUM_KERNELS])
@pytest.mark.parametrize("regime", ["wide", "edges"])
def test_sums_in_the_launch_equal_the_planes_summed_in_step_order(regime, family, prec, ref):
    """sipnet_batch_run_sums over days, next to members that never run (edges: lanes 63 and 64) inside full chunks: the
    same batch's planes added up in step order, every column as read back -- a throughput kernel advances a member that
    never runs like its neighbours, and what it leaves in that member's column means nothing, but the sums are the sums of
    it.  Bit for bit on the cooperative kernels, over the year.  The one-wavefront kernel's summing build and its
    plane-storing build fuse a few products differently, so they agree to the arithmetic's last bits, by the criterion
    and over the 205 steps of tests/test_gpu_sums.py (a rounding that enters the carried state grows with the length
    of the run: over a year the two builds drift apart by 3e-12 of a member's largest daily sum in fp64 and by 3.5e-3
    in fp32-mixed, which says nothing about either)"""
    flags, members, clim = pr.flags("default"), ref.members(regime), ref.clim()
    if family == "one_wave":
        clim = clim.slice(0, 48 * 4 + 13)
    T, K = clim.n_steps, 48
    plain = outputs(batch(flags, [clim], members, prec, KERNELS[family]), zeroed=True)
    b = batch(flags, [clim], members, prec, KERNELS[family])
    assert b.sums_in_kernel()
    sums = torch.zeros((3, (T + K - 1) // K, members.shape[0]), dtype=torch.float64, device=b.device)
    b.run_sums(0, T, K, out=sums)
    name, got, state, status = b.last_launch()["kernel"], sums.cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert "Sums" in name and ("Fast" in name) == (family == "one_wave"), name
    want = host_sums(plain[0].double().cpu().numpy(), K)
    assert np.array_equal(status, plain[4]) and (status != 0).sum() == (2 if regime == "edges" else 0)
    ran = status == 0
    top = np.abs(want).max(axis=1, keepdims=True)                       # per plane and member
    worst = (np.abs(got - want) / np.maximum(top, 1e-300)).max()
    top_state = np.maximum(np.abs(plain[1]), np.abs(state))
    worst_state = (np.abs(state - plain[1])[ran] / np.maximum(top_state[ran], 1e-300)).max()
    print(f"{regime} {name}: sums against the planes added in step order: {worst:.2e} of the member's largest sum, state {worst_state:.2e}")
    if family == "one_wave":
        tol = dict(rtol=1e-6, atol=1e-8) if prec == sa.F32_MIXED else dict(rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(got, want, **tol)
        np.testing.assert_allclose(state[ran], plain[1][ran], rtol=1e-13 if prec == sa.F64 else 1e-5, atol=1e-300 if prec == sa.F64 else 1e-7)
    else:
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(state[ran], plain[1][ran])


STAT_KERNELS = [(f, p) for f in ("one_wave", "coop_lds", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", STAT_KERNELS, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in STAT_KERNELS])
@pytest.mark.parametrize("regime", ["wide", "edges"])
def test_run_stats_equals_the_sums_over_the_planes(regime, family, prec, ref):
    """sipnet_batch_run_stats (the cooperative kernels' light wave: SIPNET_KOPT_STATS_IN_KERNEL; reduction passes behind
    the one-wavefront kernel): the sums and sums of squares over the very planes the launch wrote, by the criterion of
    tests/test_gpu_batch.py -- with members that never run inside full chunks: whatever the launch left in their columns
    (zeros, or what a throughput kernel leaves there) is in the planes as read back, and in the statistics"""
    flags, members, clim = pr.flags("default"), ref.members(regime), ref.clim()
    T, M = clim.n_steps, members.shape[0]
    plain = outputs(batch(flags, [clim], members, prec, KERNELS[family]), zeroed=True)
    b = batch(flags, [clim], members, prec, KERNELS[family], sa.KOPT_STATS_IN_KERNEL if family.startswith("coop") else 0)
    planes = torch.zeros((3, T, M), dtype=b.out_dtype, device=b.device)
    _, stats = b.run_stats(0, T, planes=planes)
    name, status = b.last_launch()["kernel"], b.get_status()
    b.close()
    assert family_ok(family, "default", name), name
    ran = torch.as_tensor(status == 0, device=planes.device)
    assert torch.equal(bits(planes[:, :, ran]), bits(plain[0][:, :, ran])), name
    p, got = planes.double().cpu().numpy(), stats.cpu().numpy()[:, :, 0]
    assert np.array_equal(status, plain[4]) and (status != 0).sum() == (2 if regime == "edges" else 0)
    s1, s2 = p.sum(-1), (p * p).sum(-1)
    e1 = np.abs(got[..., 0] - s1).max() / max(np.abs(p).sum(-1).max(), 1.0)
    e2 = np.abs(got[..., 1] - s2).max() / max(s2.max(), 1.0)
    print(f"{regime} {name}: statistics against the planes: sums {e1:.2e}, sums of squares {e2:.2e} of the largest")
    assert np.isfinite(got).all() and e1 < 1e-12 and e2 < 1e-12, name


CUT_KERNELS = [("strict", sa.F64), ("one_wave", sa.F64), ("coop_lds", sa.F64), ("coop_hbm", sa.F64), ("coop_pair", sa.F64),
               ("coop_quad", sa.F64), ("one_wave", sa.F32_MIXED), ("coop_lds", sa.F32_MIXED), ("coop_quad", sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", CUT_KERNELS, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in CUT_KERNELS])
def test_a_run_cut_off_tile_boundaries_equals_the_uncut_run(family, prec, ref):
    flags, members, clim = pr.flags("default"), ref.members("edges"), ref.clim()
    whole = outputs(batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict"), zeroed=True)
    cut = outputs(batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict"),
                  cuts=[0, 1, 23, 4001, 9999, clim.n_steps], zeroed=True)
    assert family_ok(family, "default", whole[3]["kernel"]) and whole[3]["kernel"] == cut[3]["kernel"]
    same(whole, cut, "cut at 1, 23, 4001, 9999", ran_only=True)


MULTI = [("auto", sa.KERNEL_AUTO), ("one_wave", sa.KERNEL_ONE_WAVE), ("coop_pair", sa.KERNEL_COOP_PAIR), ("coop_quad", sa.KERNEL_COOP_QUAD)]


def sites_batch(flags, clims, sets, prec, kernel):
    b = sa.Batch(flags, len(clims), sets[0].shape[0], prec, fast_math=True if prec == sa.F64 else None, kernel=kernel)
    for s, (c, m) in enumerate(zip(clims, sets)):
        b.set_climate(s, c)
        b.set_params(s, m)
    b.setup()
    return b


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("family,kernel", MULTI, ids=[m[0] for m in MULTI])
def test_three_sites_three_regimes_in_one_batch(family, kernel, prec, ref):
    """`wide`, the first 133 corners and `edges` side by side, each site under a climate of its own: planes and state
    equal the three one-site batches bit for bit"""
    flags = pr.flags("default")
    sets = [ref.members("wide"), ref.members("corners")[:133], ref.members("edges")]
    clims = [ref.clim(s) for s in range(3)]
    M = 133
    planes, state, rings, li, status = outputs(sites_batch(flags, clims, sets, prec, kernel), zeroed=True)
    assert family == "auto" or family_ok(family, "default", li["kernel"]), li["kernel"]
    for s in range(3):
        one = outputs(sites_batch(flags, [clims[s]], [sets[s]], prec, kernel), zeroed=True)
        assert one[3]["kernel"] == li["kernel"]
        assert np.array_equal(status[s * M:(s + 1) * M], one[4]), f"site {s}: status"
        ran = one[4] == 0                                   # (what a member that never runs leaves behind means nothing)
        cols = s * M + np.flatnonzero(ran)
        assert torch.equal(bits(planes[:, :, torch.as_tensor(cols, device=planes.device)]),
                           bits(one[0][:, :, torch.as_tensor(ran, device=planes.device)])), f"site {s}: planes"
        assert np.array_equal(state[cols], one[1][ran], equal_nan=True), f"site {s}: state"
        assert np.array_equal(rings[cols], one[2][ran], equal_nan=True), f"site {s}: rings"
    assert (status != 0).sum() == 4                         # corners 83 and 85, edges 63 and 64


def converted(raw, flags):
    """convertParamsKernel restated: raw rows [M][80] in file units -> the converted block's rows"""
    out = raw.copy()
    col = lambda n: raw[:, pi(n)]
    out[:, 47] = 1 - col("leafAllocation") - col("woodAllocation") - col("fineRootAllocation")       # coarseRootAllocation
    for n in RATE_ROWS:
        out[:, pi(n)] = col(n) / 365.0
    out[:, 9] = col("psnTOpt") + (col("psnTOpt") - col("psnTMin"))                                   # psnTMax
    f = col("fAnoxia")
    out[:, pi("fAnoxia")] = np.where(f <= 0.0, TINY, np.where(f >= 1.0, 1.0 - TINY, f))
    a = col("anaerobicDecompRate")
    out[:, pi("anaerobicDecompRate")] = np.where(a <= 0.0, TINY, np.where(a > 1.0, 1.0, a))
    gdd, soil_phenol = flags[sa.FLAG_NAMES.index("gdd")], flags[sa.FLAG_NAMES.index("soilPhenol")]
    if not gdd:                                             # the throughput kernels' leaf-on threshold rides in this row
        out[:, pi("gddLeafOn")] = col("soilTempLeafOn") if soil_phenol else np.where(col("leafOnDay") > 0, col("leafOnDay"), 1e300)
    return out


@pytest.mark.parametrize("flagset,regime", [("default", "corners"), ("ncycle", "corners"), ("ncycle", "edges"), ("no_gdd", "corners")])
def test_get_params_of_the_corners_in_both_units(flagset, regime, ref):
    """Batch.get_params(): the converted block against a numpy restatement of convertParamsKernel, bit for bit -- under
    the nitrogen-cycle flags on `edges` too, whose members sit on the four clamps.  In file units: every row that the
    conversion copies is the raw row bit for bit, the per-year rates are (raw / 365) * 365 bit for bit -- the raw value
    to one ulp, which is what a division and a multiplication leave -- and the derived and clamped rows are the
    converted ones (the criterion of tests/test_gpu_enkf_joint.py, made exact against the RAW rows wherever the
    conversion loses nothing)"""
    if flagset == "no_gdd":
        flags, members = sa.flags_from(gdd=0), ref.members(regime, "default")
    else:
        flags, members = pr.flags(flagset), ref.members(regime, flagset)
    b = sa.Batch(flags, 1, members.shape[0], sa.F64, fast_math=True)
    b.set_climate(0, ref.clim().slice(0, 48))
    b.set_params(0, members)
    b.setup()
    conv, file_units = b.get_params(), b.get_params(file_units=True)
    b.close()
    want = converted(members, flags)
    u8 = lambda x: np.ascontiguousarray(x).view(np.uint8)
    np.testing.assert_array_equal(u8(conv), u8(want))
    rates = [pi(n) for n in RATE_ROWS]
    changed = rates + [9, 47, pi("fAnoxia"), pi("anaerobicDecompRate"), pi("gddLeafOn")]
    copied = [k for k in range(80) if k not in changed]
    np.testing.assert_array_equal(u8(file_units[:, copied]), u8(members[:, copied]))
    np.testing.assert_array_equal(u8(file_units[:, rates]), u8(members[:, rates] / 365.0 * 365.0))
    assert (np.abs(file_units[:, rates] - members[:, rates]) <= np.spacing(np.abs(members[:, rates]))).all()
    rest = [k for k in changed if k not in rates]
    np.testing.assert_array_equal(u8(file_units[:, rest]), u8(conv[:, rest]))
    if flagset == "ncycle" and regime == "edges":
        assert set(np.unique(conv[:, pi("fAnoxia")])) >= {TINY, 1.0 - TINY} and set(np.unique(conv[:, pi("anaerobicDecompRate")])) >= {TINY, 1.0}
