"""The step kernels on event schedules beyond one event a day (tests/event_regimes.py): several events on one record, events
on the first and the last record, on 21 consecutive records (the nitrogen-cycle layout's two-slot event mailbox), on both sides
of tile boundaries and on every tile position a day's first record can have, a tillage modifier that snaps to zero, stacks and
comes back in a second year, events on the year's first record, and four sites with four different lists.
tests/test_event_regimes.py shows on the CPU that the oracle runs all 133 members on every schedule and flag set, equals the
real reference there bit for bit, and is well conditioned in the event amounts, so the bounds here are the fuzzer's
(tools/fuzz_gpu.py, tests/regime_gpu_common.judge), unchanged, and no member is left out.

133 members (tests/event_regimes.members: two chunks and a ragged third), 400 to 7 200 records.  The oracle runs once per
(forcing, schedule, flag set)."""
import numpy as np
import pytest
import torch

import sipnet_amd as sa
from tests import event_regimes as er
from tests.regime_gpu_common import COOP, KERNELS, batch, bits, family_ok, host_sums, judge, outputs, same

pytestmark = pytest.mark.gpu
SCHEDULES = list(er.SCHEDULES)
ON_DAILY = [("daily2y", s) for s in SCHEDULES]
TILE_POSITIONS = [(f, s) for f in er.FORCINGS[1:] for s in er.ANY_FORCING]


class Reference:
    """the oracle's planes, final records, status and counters per (forcing, schedule, flag set), computed once"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def members(self, flagset):
        return self.get(("members", flagset), lambda: er.members(flagset))

    def clim(self, forcing):
        return self.get(("clim", forcing), lambda: er.clim(forcing))

    def events(self, forcing, schedule):
        return self.get(("events", forcing, schedule), lambda: er.SCHEDULES[schedule](self.clim(forcing)))

    def run(self, forcing, schedule, flagset="default"):
        return self.get((forcing, schedule, flagset), lambda: self.oracle.run_block(
            er.flags(flagset), self.members(flagset), self.clim(forcing), self.events(forcing, schedule)))

    def diag(self, schedule, flagset):
        def make():
            members, clim, ev = self.members(flagset), self.clim("daily2y"), self.events("daily2y", schedule)
            out = [self.oracle.run_member(er.flags(flagset), members[m], clim, ev, want_rec=False)[2] for m in range(members.shape[0])]
            return np.array([d.n_clamp_warn for d in out]), np.array([d.n_balance_warn for d in out])
        return self.get(("diag", schedule, flagset), make)

    def sites(self, flagset, M):
        """per_site(): -> (clims, events, members, [the oracle's run of every site])"""
        def make():
            clims, events = er.per_site()
            members = self.members(flagset)
            members = members if M == members.shape[0] else np.concatenate([members[:M - 3], members[-3:]])      # (the hard members stay)
            return clims, events, members, [self.oracle.run_block(er.flags(flagset), members, c, e) for c, e in zip(clims, events)]
        return self.get(("sites", flagset, M), make)


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


def ids(pairs):
    return [f + ("_f64" if p == sa.F64 else "_f32") for f, p in pairs]


def run_case(ref, forcing, schedule, flagset, family, prec):
    flags, members, clim, ev = er.flags(flagset), ref.members(flagset), ref.clim(forcing), ref.events(forcing, schedule)
    want, final, st = ref.run(forcing, schedule, flagset)
    assert (st == 0).all()                                      # (the condition tests/test_event_regimes.py holds)
    b = batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict", events=[ev])
    planes, _ = b.run()
    name = b.last_launch()["kernel"]
    got, state, status = planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, flagset, name) and ("double" if prec == sa.F64 else "float") in name, (family, name)
    judge(f"{forcing} {schedule} {flagset} {name}", prec, got, state, status, want, final, st)


FAMILIES = [("strict", sa.F64)] + [(f, p) for f in ("one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", FAMILIES, ids=ids(FAMILIES))
@pytest.mark.parametrize("forcing,schedule", ON_DAILY + TILE_POSITIONS, ids=[f + "-" + s for f, s in ON_DAILY + TILE_POSITIONS])
def test_every_kernel_family_on_every_schedule(forcing, schedule, family, prec, ref):
    run_case(ref, forcing, schedule, "default", family, prec)


OPTIONAL = [("ncycle", "coop_ncycle"), ("ncycle", "coop_ncycle_pair"), ("ncycle", "one_wave"),
            ("russell_3", "coop_lds"), ("russell_3", "coop_hbm"), ("russell_3", "coop_pair"), ("russell_3", "one_wave")]
OPTIONAL_SCHEDULES = ["same_record", "consecutive", "year_edge", "tillage"]


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("flagset,family", OPTIONAL, ids=[a + "-" + b for a, b in OPTIONAL])
@pytest.mark.parametrize("schedule", OPTIONAL_SCHEDULES)
def test_optional_physics_and_nitrogen_kernels(schedule, flagset, family, prec, ref):
    """`consecutive` on coop_ncycle and coop_ncycle_pair: 21 records in a row hand the soil side of an event to the soil wave
    through the two slots of mailEvent"""
    run_case(ref, "daily2y", schedule, flagset, family, prec)


@pytest.mark.parametrize("schedule", OPTIONAL_SCHEDULES)
def test_optional_physics_four_chunk_layout(schedule, ref):
    """stepCoopXQuadKernel: the fp32-mixed build only (the engine refuses the fp64 one)"""
    run_case(ref, "daily2y", schedule, "russell_3", "coop_quad", sa.F32_MIXED)


PER_SITE = [("auto", "default", sa.KERNEL_AUTO), ("one_wave", "default", sa.KERNEL_ONE_WAVE), ("coop_hbm", "default", sa.KERNEL_COOP_HBM),
            ("coop_pair", "default", sa.KERNEL_COOP_PAIR), ("coop_quad", "default", sa.KERNEL_COOP_QUAD),
            ("coop_ncycle_pair", "ncycle", sa.KERNEL_COOP_NCYCLE_PAIR)]


@pytest.mark.parametrize("M", [64, 133])
@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("family,flagset,kernel", PER_SITE, ids=[p[0] for p in PER_SITE])
def test_four_sites_with_four_event_lists(family, flagset, kernel, prec, M, ref):
    """every site against the oracle over ITS forcing and ITS events (with the same list on every site a wrong events base
    fetches the right bytes); M = 64: a workgroup of the two- and four-chunk layouts holds chunks of different sites.  Then
    the same batch with the sites in reverse order: every site's planes, pools and rings bit-equal to the first order's"""
    clims, events, members, runs = ref.sites(flagset, M)
    flags, S = er.flags(flagset), len(clims)
    first = outputs(batch(flags, clims, members, prec, kernel, events=events))
    name = first[3]["kernel"]
    assert family == "auto" or family_ok(family, flagset, name), name
    got = first[0].double().cpu().numpy()
    for s in range(S):
        want, final, st = runs[s]
        cols = slice(s * M, (s + 1) * M)
        judge(f"site {s} of {S}, M {M}, {name}", prec, got[:, :clims[s].n_steps, cols], first[1][cols], first[4][cols], want, final, st)
    back = outputs(batch(flags, clims[::-1], members, prec, kernel, events=events[::-1]))
    assert back[3]["kernel"] == name
    for s in range(S):
        a, z, n = slice(s * M, (s + 1) * M), slice((S - 1 - s) * M, (S - s) * M), clims[s].n_steps
        assert torch.equal(bits(first[0][:, :n, a]), bits(back[0][:, :n, z])), f"site {s}: planes"
        assert np.array_equal(first[1][a], back[1][z], equal_nan=True) and np.array_equal(first[2][a], back[2][z], equal_nan=True), f"site {s}: state"
        assert np.array_equal(first[4][a], back[4][z])


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_layouts_tile_paths_and_plan_builders_give_the_same_bits(schedule, prec, ref):
    """the four cooperative layouts agree bit for bit, regular tiles switched off (SIPNET_KOPT_NO_REGULAR_TILES) change nothing
    -- `tile_edges` is the case that matters: a tile is regular only without events -- and neither does who built the plan"""
    flags, members, clim, ev = er.flags("default"), ref.members("default"), ref.clim("daily2y"), [ref.events("daily2y", schedule)]
    first = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, events=ev))
    for name, kernel in COOP.items():
        for opt in (0, sa.KOPT_NO_REGULAR_TILES):
            if (kernel, opt) != (sa.KERNEL_COOP_LDS, 0):
                same(first, outputs(batch(flags, [clim], members, prec, kernel, opt, events=ev)), f"{name} options {opt}")
    dev = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_DEVICE_PLAN, events=ev))
    host = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_LDS, sa.KOPT_HOST_PLAN, events=ev))
    assert dev[3]["plan_device_sites"] == 1 and host[3]["plan_device_sites"] == 0
    same(dev, host, "device plan against host plan")
    same(first, host, "default against host plan")


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", ["coop_ncycle", "coop_ncycle_pair"])
@pytest.mark.parametrize("schedule", ["consecutive", "tile_edges"])
def test_the_nitrogen_cycle_layouts_agree_and_regular_tiles_off_change_nothing(schedule, kernel, prec, ref):
    flags, members, clim, ev = er.flags("ncycle"), ref.members("ncycle"), ref.clim("daily2y"), [ref.events("daily2y", schedule)]
    first = outputs(batch(flags, [clim], members, prec, sa.KERNEL_COOP_NCYCLE, events=ev))
    same(first, outputs(batch(flags, [clim], members, prec, KERNELS[kernel], sa.KOPT_NO_REGULAR_TILES, events=ev)), f"{kernel}, regular tiles off")


def cuts_of(clim, schedule, events):
    """t - 1, t, t + 1 around every event record; `tillage`: inside the decays too"""
    at = set(er.records_of(clim, events).tolist())
    if schedule == "tillage":
        d = er.TILLAGE_DAYS
        at |= {d["three_weeks"] + 10, d["three_weeks"] + 20, d["first"] + 15, d["third"] + 60, d["second_year"] + 2}
    T = clim.n_steps
    return sorted({0, T} | {t + k for t in at for k in (-1, 0, 1) if 0 < t + k < T})


SWITCH_KERNELS = [("strict", sa.F64), ("one_wave", sa.F64), ("coop_lds", sa.F64), ("coop_hbm", sa.F64), ("coop_pair", sa.F64),
                  ("coop_quad", sa.F64), ("one_wave", sa.F32_MIXED), ("coop_lds", sa.F32_MIXED), ("coop_quad", sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", SWITCH_KERNELS, ids=ids(SWITCH_KERNELS))
@pytest.mark.parametrize("schedule", ["consecutive", "tile_edges", "tillage"])
def test_a_run_cut_around_every_event_record_equals_the_uncut_run(schedule, family, prec, ref):
    flags, members, clim, ev = er.flags("default"), ref.members("default"), ref.clim("daily2y"), ref.events("daily2y", schedule)
    cuts = cuts_of(clim, schedule, ev)
    assert len(cuts) >= 15
    whole = outputs(batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict", events=[ev]))
    cut = outputs(batch(flags, [clim], members, prec, KERNELS[family], strict=family == "strict", events=[ev]), cuts=cuts)
    assert family_ok(family, "default", whole[3]["kernel"]) and whole[3]["kernel"] == cut[3]["kernel"]
    same(whole, cut, f"{len(cuts) - 1} launches")


@pytest.mark.parametrize("family,prec", [("coop_ncycle", sa.F64), ("coop_ncycle_pair", sa.F64), ("coop_ncycle", sa.F32_MIXED)],
                         ids=["coop_ncycle_f64", "coop_ncycle_pair_f64", "coop_ncycle_f32"])
def test_the_event_mailbox_survives_a_launch_cut_at_every_record(family, prec, ref):
    """`consecutive` under the nitrogen cycle: a launch starts with seqEvent = tBegin - 1 and t & 1 picks the slot, so cuts on
    odd and even records alike, between records that both carry events"""
    flags, members, clim, ev = er.flags("ncycle"), ref.members("ncycle"), ref.clim("daily2y"), ref.events("daily2y", "consecutive")
    cuts = cuts_of(clim, "consecutive", ev)
    whole = outputs(batch(flags, [clim], members, prec, KERNELS[family], events=[ev]))
    cut = outputs(batch(flags, [clim], members, prec, KERNELS[family], events=[ev]), cuts=cuts)
    assert family_ok(family, "ncycle", whole[3]["kernel"]) and whole[3]["kernel"] == cut[3]["kernel"]
    same(whole, cut, f"{len(cuts) - 1} launches")


SUM_KERNELS = [(f, p) for f in ("one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad") for p in (sa.F64, sa.F32_MIXED)]


@pytest.mark.parametrize("family,prec", SUM_KERNELS, ids=ids(SUM_KERNELS))
def test_sums_over_groups_of_seven_equal_the_planes_summed_in_step_order(family, prec, ref):
    """sipnet_batch_run_sums on `consecutive`: weeks that hold no event, one, and seven.  Bit for bit on the cooperative
    kernels; the one-wavefront kernel's summing build fuses a few products differently from its plane-storing build, so there
    by the criterion and over the 205 records of tests/test_gpu_sums.py (the events fall on records 60 to 80)"""
    flags, members, clim, ev = er.flags("default"), ref.members("default"), ref.clim("daily2y"), ref.events("daily2y", "consecutive")
    if family == "one_wave":
        clim = clim.slice(0, 205)
    T, K = clim.n_steps, 7
    plain = outputs(batch(flags, [clim], members, prec, KERNELS[family], events=[ev]))
    b = batch(flags, [clim], members, prec, KERNELS[family], events=[ev])
    assert b.sums_in_kernel()
    sums = torch.zeros((3, (T + K - 1) // K, members.shape[0]), dtype=torch.float64, device=b.device)
    b.run_sums(0, T, K, out=sums)
    name, got, state, status = b.last_launch()["kernel"], sums.cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert "Sums" in name and ("Fast" in name) == (family == "one_wave"), name
    want = host_sums(plain[0].double().cpu().numpy(), K)
    assert (status == 0).all() and (plain[4] == 0).all()
    if family == "one_wave":
        tol = dict(rtol=1e-6, atol=1e-8) if prec == sa.F32_MIXED else dict(rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(got, want, **tol)
        np.testing.assert_allclose(state, plain[1], rtol=1e-13 if prec == sa.F64 else 1e-5, atol=1e-300 if prec == sa.F64 else 1e-7)
    else:
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(state, plain[1])


def counters_case(ref, schedule, flagset, family):
    flags, members, clim, ev = er.flags(flagset), ref.members(flagset), ref.clim("daily2y"), ref.events("daily2y", schedule)
    _, _, st = ref.run("daily2y", schedule, flagset)
    clamp, balance = ref.diag(schedule, flagset)
    b = batch(flags, [clim], members, sa.F64, KERNELS[family], strict=family == "strict", diagnostics=True, events=[ev])
    b.run()
    name = b.last_launch()["kernel"]
    d = b.get_diagnostics()
    b.close()
    assert family_ok(family, flagset, name) or (family == "coop_ncycle" and name.startswith("stepCoopNFullKernel<")), name
    print(f"{schedule} {flagset} {name}: clamp warnings {int(clamp.sum())} (most {int(clamp.max())}), balance warnings {int(balance.sum())}")
    assert (st == 0).all()
    assert np.array_equal(d["n_clamp_warn"], clamp) and np.array_equal(d["n_balance_warn"], balance)


@pytest.mark.parametrize("family", ["strict", "one_wave", "coop_lds", "coop_hbm", "coop_pair"])      # (no full-state build of the four-chunk layout)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_clamp_and_balance_counters_match_the_oracles(schedule, family, ref):
    """the balance check is what reads evInC / evOutC (and, below, evInN / evOutN): a planting, a fertiliser or a harvest that
    one of them misses is a balance warning the oracle does not have"""
    counters_case(ref, schedule, "default", family)


@pytest.mark.parametrize("schedule", ["same_record", "year_edge"])
def test_clamp_and_balance_counters_under_the_nitrogen_cycle(schedule, ref):
    counters_case(ref, schedule, "ncycle", "coop_ncycle")


EVENTS_OUT = [("default", "strict"), ("default", "coop_lds"), ("ncycle", "strict"), ("ncycle", "coop_ncycle")]


@pytest.mark.parametrize("flagset,family", EVENTS_OUT, ids=[a + "-" + b for a, b in EVENTS_OUT])
@pytest.mark.parametrize("schedule", ["same_record", "consecutive", "year_edge"])
def test_events_out_from_the_full_records_equals_the_oracles_file(schedule, flagset, family, ref, oracle, tmp_path):
    """events.out of one (deciduous) member regenerated from the batch's full records, from the strict kernel and from a
    throughput kernel's full-state build, against the file the oracle writes for that member, byte for byte: a record with
    several events has several lines, in input order, the computed leaf-on last"""
    m = 1
    flags, members, clim, ev = er.flags(flagset), ref.members(flagset), ref.clim("daily2y"), ref.events("daily2y", schedule)
    b = batch(flags, [clim], members, sa.F64, KERNELS[family], strict=family == "strict", diagnostics=family != "strict", events=[ev])
    init_pools = b.get_state()[m, :13]
    _, rec = b.run(full=True, want_planes=False)
    name = b.last_launch()["kernel"]
    rec = rec.cpu().numpy()[:, :, m]
    b.close()
    assert name.startswith({"strict": "stepKernel<", "coop_lds": "stepCoopKernel<", "coop_ncycle": "stepCoopNFullKernel<"}[family]), name
    got_path, want_path = str(tmp_path / "got.out"), str(tmp_path / "want.out")
    sa.write_events_out(got_path, flags, members[m], clim, ev, rec, init_pools)
    assert oracle.run_member(flags, members[m], clim, ev, events_out=want_path)[0] == 0
    got, want = open(got_path, "rb").read(), open(want_path, "rb").read()
    per_day = {}
    for ln in want.decode().splitlines():
        per_day[tuple(ln.split()[:2])] = per_day.get(tuple(ln.split()[:2]), 0) + 1
    assert len(want.splitlines()) >= len(ev) - 3 and (max(per_day.values()) >= 6 or schedule == "consecutive")
    if got != want:
        a, g = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(a), len(g))) if a[i] != g[i]]
        print(name, len(a), len(g), bad[:3], a[bad[0]] if bad else "", g[bad[0]] if bad else "")
    assert got == want
