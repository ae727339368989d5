"""The step kernels on forcing outside the one synthetic climate (tests/forcing_regimes.py): a polar year, an arid
year, a year of whole degrees around 0 C, four files of other step lengths -- one changing its length twice inside
tiles -- and an in-memory year whose zeros are +-1e-300 / +-5e-324.  tests/test_forcing_regimes.py shows on the CPU that
the oracle is well conditioned on exactly these inputs and members, so the bounds here are the fuzzer's
(tools/fuzz_gpu.py), unchanged:

  fp64        every plane value within 1e-9 of the plane maximum (floor 1e-3), pools within 1e-8 (floor 1e-2), the
              oracle's status, and its clamp / balance counters from the families that report them
  fp32-mixed  everything finite, the share of values off by more than 1e-4 of the plane maximum below 2e-3, time sums
              within 2e-3, pools within 5e-3 (floor 1.0)

133 members: synth.perturbed_params(base, 130, scale=3.0) -- two chunks and a ragged third -- plus the fuzzer's three
hard members.  The oracle runs once per regime and flag set."""
import os

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd.config import param_index as pi
from tests import forcing_regimes as fr
from tests import helpers
from tests.regime_gpu_common import COOP, FLAG_SETS, batch, family_ok, judge, outputs, same

pytestmark = pytest.mark.gpu
DATA = os.path.join(helpers.REPO, "sipnet_amd", "data")
REGIMES = list(fr.FILE_REGIMES) + ["tiny"]
class Reference:
    """the oracle's planes, final records, status and counters per (regime, flag set), computed once"""

    def __init__(self, oracle):
        self.oracle, self.cache, self.counters = oracle, {}, {}

    def flags(self, flagset):
        return sa.flags_from(**FLAG_SETS[flagset])

    def members(self, flagset):
        key = ("members", flagset)
        if key not in self.cache:
            path = os.path.join(DATA, "base_forest.param" if flagset == "default" else "allflags_forest.param")
            self.cache[key] = fr.hard_members(sa.read_params(path, self.flags(flagset))[0])
        return self.cache[key]

    def clim(self, regime, flagset="default"):
        key = ("clim", regime)
        if key not in self.cache:
            self.cache[key] = fr.clim(regime)
        return self.cache[key]

    def run(self, regime, flagset="default"):
        key = (regime, flagset)
        if key not in self.cache:
            self.cache[key] = self.oracle.run_block(self.flags(flagset), self.members(flagset), self.clim(regime))
        return self.cache[key]

    def diag(self, regime):
        if regime not in self.counters:
            members, clim, flags = self.members("default"), self.clim(regime), self.flags("default")
            out = [self.oracle.run_member(flags, members[m], clim, want_rec=False)[2] for m in range(members.shape[0])]
            self.counters[regime] = (np.array([d.n_clamp_warn for d in out]), np.array([d.n_balance_warn for d in out]))
        return self.counters[regime]


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def run_case(ref, regime, flagset, family, prec):
    flags, members, clim = ref.flags(flagset), ref.members(flagset), ref.clim(regime)
    want, final, st = ref.run(regime, flagset)
    kernel = {"strict": sa.KERNEL_AUTO, "one_wave": sa.KERNEL_ONE_WAVE, "coop_ncycle": sa.KERNEL_COOP_NCYCLE,
              "coop_ncycle_pair": sa.KERNEL_COOP_NCYCLE_PAIR, **COOP}[family]
    b = batch(flags, [clim], members, prec, kernel, strict=family == "strict")
    planes, _ = b.run()
    name = b.last_launch()["kernel"]
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, flagset, name) and ("double" if prec == sa.F64 else "float") in name, (family, name)
    judge(f"{regime} {flagset} {name}", prec, got, state, status, want, final, st)
    return name


FAMILIES = [("strict", sa.F64)] + [(f, p) for f in ("one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", FAMILIES, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in FAMILIES])
@pytest.mark.parametrize("regime", REGIMES)
def test_every_kernel_family_on_every_regime(regime, family, prec, ref):
    run_case(ref, regime, "default", family, prec)


@pytest.mark.parametrize("family", ["strict", "one_wave", "coop_lds", "coop_hbm", "coop_pair"])      # (no full-state build of the four-chunk layout)
@pytest.mark.parametrize("regime", REGIMES)
def test_clamp_and_balance_counters_match_the_oracles(regime, family, ref):
    flags, members, clim = ref.flags("default"), ref.members("default"), ref.clim(regime)
    _, _, st = ref.run(regime)
    clamp, balance = ref.diag(regime)
    b = batch(flags, [clim], members, sa.F64, COOP.get(family, sa.KERNEL_ONE_WAVE if family == "one_wave" else sa.KERNEL_AUTO),
              strict=family == "strict", diagnostics=True)
    b.run()
    name = b.last_launch()["kernel"]
    d = b.get_diagnostics()
    b.close()
    assert family_ok(family, "default", name), name
    ok = st == 0
    print(f"{regime} {name}: clamp warnings {int(clamp.sum())} (most {int(clamp.max())}), balance warnings {int(balance.sum())}")
    assert np.array_equal(d["n_clamp_warn"][ok], clamp[ok]) and np.array_equal(d["n_balance_warn"][ok], balance[ok])


OPTIONAL = [("ncycle", "coop_ncycle"), ("ncycle", "coop_ncycle_pair"), ("ncycle", "one_wave"),
            ("russell_3", "coop_lds"), ("russell_3", "coop_hbm"), ("russell_3", "coop_pair"), ("russell_3", "one_wave")]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("flagset,family", OPTIONAL, ids=[a + "-" + b for a, b in OPTIONAL])
@pytest.mark.parametrize("regime", ["polar", "arid", "lengths_alternating"])
def test_optional_physics_and_nitrogen_kernels(regime, flagset, family, prec, ref):
    run_case(ref, regime, flagset, family, prec)


@pytest.mark.parametrize("regime", ["polar", "arid", "lengths_alternating"])
def test_optional_physics_four_chunk_layout(regime, ref):
    """stepCoopXQuadKernel: the fp32-mixed build only (the engine refuses the fp64 one)"""
    run_case(ref, regime, "russell_3", "coop_quad", sa.F32_MIXED)


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("regime", REGIMES)
def test_layouts_tile_paths_and_plan_builders_give_the_same_bits(regime, prec, ref):
    """the identities the suite holds on the synthetic climate, on these inputs: the four cooperative layouts agree bit for
    bit, regular tiles switched off (SIPNET_KOPT_NO_REGULAR_TILES) change nothing, and neither does who built the plan"""
    flags, members, clim = ref.flags("default"), ref.members("default"), ref.clim(regime)
    first = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS))
    assert first[3]["plan_device_sites"] in (0, 1)
    for name, kernel in COOP.items():
        for opt in (0, sa.KOPT_NO_REGULAR_TILES):
            if (kernel, opt) != (sa.KERNEL_COOP_LDS, 0):
                same(first, outputs(batch(flags, [clim], members, prec, kernel, opt)), f"{name} options {opt}")
    dev = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_DEVICE_PLAN))
    host = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_HOST_PLAN))
    assert dev[3]["plan_device_sites"] == 1 and host[3]["plan_device_sites"] == 0          # (every step >= 0.0202 days: eligible)
    same(dev, host, "device plan against host plan")
    same(first, host, "default against host plan")


SWITCH_KERNELS = [("strict", sa.F64), ("one_wave", sa.F64), ("coop_lds", sa.F64), ("coop_hbm", sa.F64), ("coop_pair", sa.F64),
                  ("coop_quad", sa.F64), ("one_wave", sa.F32_MIXED), ("coop_lds", sa.F32_MIXED), ("coop_quad", sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", SWITCH_KERNELS, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in SWITCH_KERNELS])
def test_a_run_cut_around_the_length_switches_equals_the_uncut_run(family, prec, ref):
    flags, members, clim = ref.flags("default"), ref.members("default"), ref.clim("lengths_switching")
    a, z = fr.SWITCH_STEPS
    kernel = COOP.get(family, sa.KERNEL_ONE_WAVE if family == "one_wave" else sa.KERNEL_AUTO)
    whole = outputs(batch(flags, [clim], members, prec, kernel, strict=family == "strict"))
    cut = outputs(batch(flags, [clim], members, prec, kernel, strict=family == "strict"),
                  cuts=[0, a - 1, a, a + 1, z - 1, z, z + 1, clim.n_steps])
    assert family_ok(family, "default", whole[3]["kernel"]) and whole[3]["kernel"] == cut[3]["kernel"]
    same(whole, cut, "cut at the switches")


MULTI = [("auto", sa.KERNEL_AUTO), ("one_wave", sa.KERNEL_ONE_WAVE), ("coop_hbm", sa.KERNEL_COOP_HBM), ("coop_pair", sa.KERNEL_COOP_PAIR),
         ("coop_quad", sa.KERNEL_COOP_QUAD)]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("family,kernel", MULTI, ids=[m[0] for m in MULTI])
def test_three_sites_three_regimes_three_lengths(family, kernel, prec, ref):
    """a polar year, the 3-hour file and the switching file side by side in one batch: every site against the oracle over
    ITS forcing (rows past a shorter site's last record are not written)"""
    regimes = ["polar", "lengths_3h", "lengths_switching"]
    flags, members = ref.flags("default"), ref.members("default")
    clims = [ref.clim(r) for r in regimes]
    M = members.shape[0]
    b = batch(flags, clims, members, prec, kernel)
    planes, _ = b.run()
    name = b.last_launch()["kernel"]
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family == "auto" or family_ok(family, "default", name), name
    for s, r in enumerate(regimes):
        want, final, st = ref.run(r)
        cols = slice(s * M, (s + 1) * M)
        judge(f"site {s} {r} {name}", prec, got[:, :clims[s].n_steps, cols], state[cols], status[cols], want, final, st)


@pytest.mark.parametrize("family,prec", FAMILIES, ids=[f + ("_f64" if p == sa.F64 else "_f32") for f, p in FAMILIES])
def test_a_dry_soil_under_a_vanishing_vpd_divides_zero_by_a_denormal(family, prec, ref, oracle):
    """what the test of fdiv on its own found (tests/test_gpu_fast_math.py): moisture()'s removable / potTrans is taken by a
    reciprocal, which overflows for 0 < potTrans < 2^-1024 (fp32-mixed: for a denormal float), and with removable = 0 the
    quotient came back NaN where the reference's is 0 -- and was not selected away, because removable < potTrans holds.
    fr.tiny_vpd() with fr.dry_members() reaches it at the first step; the plan builders now floor the record's VPD (plan.h,
    kVpdFloor), which keeps the divisor in the range and changes no result."""
    flags = ref.flags("default")
    members = fr.dry_members(sa.read_params(os.path.join(DATA, "base_forest.param"), flags)[0])
    clim = fr.tiny_vpd()
    want, final, st = oracle.run_block(flags, members, clim)
    kernel = {"strict": sa.KERNEL_AUTO, "one_wave": sa.KERNEL_ONE_WAVE, **COOP}[family]
    b = batch(flags, [clim], members, prec, kernel, strict=family == "strict")
    planes, _ = b.run()
    name = b.last_launch()["kernel"]
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, "default", name), name
    ok = st == 0
    assert np.isfinite(got[:, :, ok]).all(), f"{name}: {int((~np.isfinite(got[:, :, ok])).any(axis=(0, 1)).sum())} members not finite"
    judge(f"tiny_vpd, dry members, {name}", prec, got, state, status, want, final, st)


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("plan", [sa.KOPT_HOST_PLAN, sa.KOPT_DEVICE_PLAN], ids=["host_plan", "device_plan"])
def test_both_plan_builders_floor_a_vanishing_vpd(plan, prec, oracle, ref):
    """the same input through the host's and the device's plan builder: the same bits, and the regime bounds"""
    flags = ref.flags("default")
    members = fr.dry_members(sa.read_params(os.path.join(DATA, "base_forest.param"), flags)[0])
    clim = fr.tiny_vpd()
    want, final, st = oracle.run_block(flags, members, clim)
    b = batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, plan)
    planes, _ = b.run()
    li = b.last_launch()
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert li["plan_device_sites"] == (1 if plan == sa.KOPT_DEVICE_PLAN else 0), li
    judge(f"tiny_vpd, plan option {plan}, {li['kernel']}", prec, got, state, status, want, final, st)
    other = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_HOST_PLAN + sa.KOPT_DEVICE_PLAN - plan))
    same(outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, plan)), other, "one plan builder against the other")


@pytest.mark.parametrize("plan", [sa.KOPT_HOST_PLAN, sa.KOPT_DEVICE_PLAN], ids=["host_plan", "device_plan"])
@pytest.mark.parametrize("family", ["one_wave", "coop_lds", "coop_quad"])
def test_a_soil_just_below_a_frozen_threshold_of_zero_is_frozen_in_fp32_mixed(family, plan, ref, oracle):
    """what `tiny` found: an fp32-mixed batch's plan narrowed a soil temperature of -1e-300 (or -5e-324) to -0.0f, and the
    kernels' `tsoil < frozenSoilThreshold` then said "not frozen" to every member whose threshold is 0 -- the parameter
    file's own value -- where the oracle says "frozen": transpiration and foliar respiration of those steps without the
    frozen-soil factors (NEE off by 0.38 of the plane maximum, its time sum by 1e-2, for 6 of the 133 members of the
    regime tests).  The narrowing keeps the sign class now (+-FLT_MIN), in both plan builders.  Here EVERY member has the
    threshold 0, over the sixty spring days in which `tiny`'s soil crosses it: the fuzzer's fp32-mixed criteria."""
    flags = ref.flags("default")
    members = ref.members("default").copy()
    members[:, pi("frozenSoilThreshold")] = 0.0
    clim = ref.clim("tiny").slice(90 * 48, 150 * 48)
    below = (clim.data[:, 2] < 0) & (clim.data[:, 2] > -1e-200)
    assert below.sum() > 50 and (clim.data[below, 3] > 0).sum() > 20           # ... some of them by day
    want, final, st = oracle.run_block(flags, members, clim)
    b = batch(flags, [clim], members, sa.F32_MIXED, COOP.get(family, sa.KERNEL_ONE_WAVE), plan)
    planes, _ = b.run()
    li = b.last_launch()
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, "default", li["kernel"]) and li["plan_device_sites"] == (1 if plan == sa.KOPT_DEVICE_PLAN else 0), li
    judge(f"threshold 0, soil just below it, {li['kernel']}", sa.F32_MIXED, got, state, status, want, final, st)
