"""The event schedules of tests/event_regimes.py, without a GPU: that each schedule IS what it claims (records with several
events, the tile positions hit, the tillage modifier's snap to zero, its stacking and its second year, events on the year's
first record), that the oracle runs every member of the GPU tests on every schedule and flag set (a condition: no GPU test may
leave a member out), that the oracle equals the REAL reference's step loop on these schedules bit for bit
(tests/golden/ref_event_records.npz, written by tools/make_golden.py event_records()), and the conditioning yardstick of
tests/test_oracle_edits.py: the continuous event amounts one ulp toward zero, the exact constants 0 and 1 and the irrigation
method held; planes within 1e-12 of the plane maximum (floor 1e-3), the twelve pools within 1e-12 (floor 1e-2).  A schedule
that fails it is narrowed; the GPU bound is never widened for it.

The thirteenth pool slot, plantCAccountingDelta, is a difference of carbon totals; it is anywhere between 1e-2 gC and, under
the nitrogen cycle, 7e2 gC here, next to totals of up to 2e4 gC, so a figure relative to itself says little: it is held in
absolute terms, within 1e-12 of the member's total carbon -- the quantity whose rounding it inherits, and the bound the other
pools have.

The reference's reader refuses leaf-on / leaf-off events next to a computed phenology (events.c:251-261), and all three flag
sets compute it: the pin to the reference runs every schedule without those two types (the five others, on the same records).
The oracle's leaf events on records shared with other events are held by tests/test_events_infrastructure.py and by what
the GPU tests compare (the strict kernel is a second restatement).  The fixture also holds the warning lines the reference
printed: under the nitrogen cycle its own nitrogen balance check fails on every record with a harvest (0.0098 gN for the
suite's harvest), and the oracle's counter says the same.

The default parameter file's forest is evergreen; every second member of that flag set is made deciduous
(tests/event_regimes.members), or a leaf event would move nothing there.

Measured, worst over the six schedules (amounts one ulp toward zero: planes | twelve pools | plantCAccountingDelta, absolute and
of the total carbon; then planes and pools with the amounts moved by a float's ulp, the fp32-mixed runs' context):
  default     2.3e-15 | 1.4e-14 | 4.5e-12 gC, 2.0e-16 | 2.6e-7, 9.0e-7
  ncycle      9.8e-15 | 7.8e-13 | 5.0e-12 gC, 6.0e-15 | 9.0e-8, 1.6e-5
  russell_3   7.9e-15 | 2.6e-13 | 6.9e-12 gC, 1.2e-15 | 9.4e-8, 2.3e-7
Narrowed: nothing."""
import collections
import os

import numpy as np
import pytest

import sipnet_amd as sa
from tests import event_regimes as er
from tests import helpers

TILL_MOD = 34                  # record column (include/sipnet_amd.h)
CARBON = [14, 15, 16, 18, 20, 21]      # plantWoodC plantLeafC soilC litterC coarseRootC fineRootC
SCHEDULES = list(er.SCHEDULES)
FLAG_SETS = list(er.FLAG_SETS)


@pytest.fixture(scope="module")
def daily():
    return er.clim("daily2y")


@pytest.fixture(scope="module")
def runs(oracle, daily):
    """(schedule, flag set) -> (events, planes, final, status) of the oracle on daily2y, computed once"""
    cache = {}

    def get(schedule, flagset):
        if (schedule, flagset) not in cache:
            ev = er.SCHEDULES[schedule](daily)
            cache[schedule, flagset] = (ev,) + tuple(oracle.run_block(er.flags(flagset), er.members(flagset), daily, ev))
        return cache[schedule, flagset]
    return get


def positions(c, events):
    return set((er.records_of(c, events) % er.TILE).tolist())


def test_daily2y_is_two_years_of_one_record_a_day(daily, tmp_path):
    assert daily.n_steps == 730 and np.all(daily.data[:, 0] == 1.0)
    assert np.array_equal(daily.year, np.repeat([2021, 2022], 365)) and np.array_equal(daily.day, np.tile(np.arange(1, 366), 2))
    assert np.array_equal(er.day_starts(daily), np.arange(730))
    path = str(tmp_path / "daily2y.clim")                    # ... and survives a file
    sa.synth.write_clim(path, er.daily2y_raw())
    got = sa.read_clim(path)
    assert np.array_equal(got.data, daily.data) and np.array_equal(got.year, daily.year) and np.array_equal(got.day, daily.day)


def test_same_record_puts_several_events_on_one_record(daily):
    ev = er.same_record(daily)
    per_record = collections.Counter(er.records_of(daily, ev).tolist())
    assert per_record == {20: 8, 45: 2, 70: 9, 100: 2}
    on = lambda t: [e for e, r in zip(ev, er.records_of(daily, ev)) if r == t]
    assert sorted(e.type for e in on(20)) == [0, 1, 2, 2, 3, 4, 5, 6] and {int(e.p[1]) for e in on(20) if e.type == er.IRRIG} == {0, 1}
    assert [e.p[0] for e in on(45)] == [0.3, 0.4] and all(e.type == er.TILL for e in on(45))
    assert [int(e.p[1]) for e in on(70)] == [0, 1] * 4 + [0] and all(e.type == er.IRRIG for e in on(70))
    assert [e.type for e in on(100)] == [er.HARVEST, er.PLANT] and list(on(100)[0].p) == [1.0, 1.0, 0.0, 0.0]


def test_first_last_consecutive_tile_edges_and_year_edge_sit_where_they_claim(daily):
    rec = lambda name: er.records_of(daily, er.SCHEDULES[name](daily))
    assert collections.Counter(rec("first_last").tolist()) == {0: 7, 729: 7}
    ev = er.consecutive(daily)
    assert np.array_equal(rec("consecutive"), np.arange(60, 81)) and [e.type for e in ev] == list(range(7)) * 3
    assert rec("consecutive")[0] % er.TILE != 0                                  # the mailbox's run starts inside a tile
    edges = rec("tile_edges")
    assert tuple(edges) == er.TILE_EDGE_DAYS and sorted(set((edges % 16).tolist())) == [0, 1, 15]
    assert set((edges // 16).tolist()) == {0, 1, 2, 4, 5, 6}                     # tile 3, and all from 7 on, left alone
    for last in (15, 31, 95):                                                    # the last record of a tile and the first of the next
        assert last % 16 == 15 and last in edges and last + 1 in edges
    assert 47 in edges and 48 not in edges and 64 in edges and 63 not in edges   # ... and each on its own
    ye = rec("year_edge")
    assert collections.Counter(ye.tolist()) == {364: 7, 365: 7}
    assert daily.year[365] != daily.year[364] and daily.year[364] == daily.year[363]


def test_the_tile_position_forcings_put_a_days_first_record_where_they_claim():
    c3, a, b = er.clim("lengths_3h"), er.clim("hh150_from1"), er.clim("hh150_from15")
    assert set((er.day_starts(c3) % 16).tolist()) == {0, 8}
    assert set((er.day_starts(a)[1:] % 16).tolist()) == {15} and set((er.day_starts(b)[1:] % 16).tolist()) == {1}
    assert a.n_steps == 150 * 48 - 1 and b.n_steps == 150 * 48 - 15 and len(er.day_starts(a)) == 150
    for name in er.ANY_FORCING:
        assert positions(c3, er.SCHEDULES[name](c3)) == {0, 8}, name
        assert positions(a, er.SCHEDULES[name](a)) == {15} and positions(b, er.SCHEDULES[name](b)) == {1}, name
    assert len(er.tillage(a)) == 5 and len(er.tillage(er.clim("daily2y"))) == 6  # (no second year in 150 days)


def test_per_site_has_four_lengths_and_four_lists():
    clims, events = er.per_site()
    assert tuple(c.n_steps for c in clims) == er.PER_SITE_LENGTHS == (730, 730, 400, 611)
    assert [len(e) for e in events] == [21, 0, 21, 40]
    assert not np.array_equal(clims[0].data, clims[1].data)                      # (other seeds too)
    for c, ev in zip(clims, events):
        assert len(ev) == 0 or er.records_of(c, ev).max() < c.n_steps
    assert np.array_equal(er.records_of(clims[2], events[2]), np.arange(160, 181))
    assert [int(e.p[1]) for e in events[3]] == [0, 1] * 20 and np.all(np.diff(er.records_of(clims[3], events[3])) == 15)
    keys = [[(e.type, e.year, e.day, tuple(e.p)) for e in ev] for ev in events]
    assert all(keys[i] != keys[j] for i in range(4) for j in range(i))


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_tillage_reaches_the_snap_to_zero_the_stack_and_the_second_year(flagset, oracle, daily):
    ev = er.tillage(daily)
    st, rec, _ = oracle.run_member(er.flags(flagset), er.members(flagset)[0], daily, ev)
    till, d = rec[:, TILL_MOD], er.TILLAGE_DAYS
    assert st == 0 and (till[:d["one_step"] + 1] == 0).all()                     # 0.005: gone after its own step's decay
    assert 0.005 * np.exp(-1 / 30.0) < 0.01
    # 0.02 falls below 0.01 with its 21st decay: 20 records carry it, the tillage's own included
    n = int(np.argmax(0.02 * np.exp(-np.arange(1, 60) / 30.0) < 0.01)) + 1
    t0 = d["three_weeks"]
    assert n == 21 and (till[t0:t0 + n - 1] > 0).all() and (till[t0 + n - 1:d["first"]] == 0).all()
    assert till[t0] == 0.02 * np.exp(-1 / 30.0)
    # the stack: 0.3 on what thirty days left of 0.6, then 0.4 on both
    assert 0.3 < till[d["second"] - 1] / np.exp(-1 / 30.0) + 0.3 < 0.6 and 0.5 < till[d["second"]] < 0.52
    assert till[d["third"]] > 0.6 and till[d["third"]] > till[d["first"]]
    t2 = d["second_year"]
    assert daily.year[t2] == 2022 and (till[t2 - 60:t2] == 0).all() and (till[d["third"]:t2 - 60] > 0).any()
    assert (till[t2:t2 + 2] > 0.01).all() and (till[t2 + 2:] == 0).all()         # 0.011: above the threshold for two decays


@pytest.mark.parametrize("flagset", FLAG_SETS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_oracle_runs_every_member_on_every_schedule(schedule, flagset, runs):
    _, planes, final, status = runs(schedule, flagset)
    assert (status == 0).sum() == 133 == len(status)
    assert np.isfinite(planes).all() and np.isfinite(final).all()


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_oracle_runs_every_member_on_the_other_forcings_and_on_every_site(flagset, oracle):
    flags, members = er.flags(flagset), er.members(flagset)
    cases = [(er.clim(f), er.SCHEDULES[s](er.clim(f))) for f in er.FORCINGS[1:] for s in er.ANY_FORCING] + list(zip(*er.per_site()))
    for c, ev in cases:
        planes, final, status = oracle.run_block(flags, members, c, ev)
        assert (status == 0).all() and np.isfinite(planes).all() and np.isfinite(final).all()


@pytest.mark.parametrize("flagset", FLAG_SETS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_oracle_equals_the_reference_step_loop_on_every_schedule(schedule, flagset, oracle, daily):
    ref = np.load(os.path.join(helpers.GOLDEN, "ref_event_records.npz"))
    idx, want = ref[f"{schedule}_idx"], ref[f"{schedule}_{flagset}"]
    events = [e for e in er.SCHEDULES[schedule](daily) if e.type not in (er.LEAFON, er.LEAFOFF)]
    at = er.records_of(daily, events)
    assert len(events) >= 6 and all(t + k in idx for t in at for k in range(-3, 4) if 0 <= t + k < 730)
    assert set(range(0, 730, 7)) <= set(idx.tolist()) and idx[-1] == 729 and want.shape == (2, len(idx), 36)
    for k, m in enumerate(ref["members"]):
        st, rec, diag = oracle.run_member(er.flags(flagset), er.members(flagset)[m], daily, events)
        assert st == 0
        # the reference's own clamp and balance warning lines: what reads the event input / output terms of the balance
        assert [diag.n_clamp_warn, diag.n_balance_warn] == ref[f"{schedule}_{flagset}_warnings"][:, k].tolist()
        assert rec[idx].tobytes() == want[k].tobytes(), (schedule, flagset, int(m), np.flatnonzero((rec[idx] != want[k]).any(axis=1))[:5])
        assert not np.array_equal(rec[at.max()], oracle.run_member(er.flags(flagset), er.members(flagset)[m], daily)[1][at.max()])


def test_the_oracle_writes_one_line_per_event_of_a_record_in_input_order(oracle, daily, tmp_path):
    ev = er.same_record(daily)
    path = str(tmp_path / "events.out")
    assert oracle.run_member(er.flags("default"), er.members()[1], daily, ev, events_out=path)[0] == 0         # (a deciduous member)
    lines = [ln.split() for ln in open(path).read().splitlines()]
    day21 = [ln[2] for ln in lines if ln[:2] == ["2021", "21"]]
    # (the leaf-on line is written after the step's fluxes, sipnet.c:1230-1247: last of its record)
    assert day21 == ["fert", "harv", "irrig", "irrig", "plant", "till", "leafoff", "leafon"]
    assert [ln[2] for ln in lines if ln[:2] == ["2021", "71"]] == ["irrig"] * 9
    soil = [ln[3].split(",")[0] for ln in lines if ln[:2] == ["2021", "71"]]
    assert soil[0] != soil[1] and soil[0::2] == [soil[0]] * 5 and soil[1::2] == [soil[1]] * 4      # the two methods alternate


def float_ulp_toward_zero(x):
    return x - np.sign(x) * float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("flagset", FLAG_SETS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_conditioning_yardstick_of_the_event_amounts(schedule, flagset, oracle, daily, runs):
    ev, want, final, st = runs(schedule, flagset)
    flags, members = er.flags(flagset), er.members(flagset)
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-3)

    def figures(step):
        ev2 = er.moved(ev, step)
        n_moved = sum(a.p[i] != b.p[i] for a, b in zip(ev, ev2) for i in range(4))
        got, final2, st2 = oracle.run_block(flags, members, daily, ev2)
        assert np.array_equal(st, st2)
        planes = (np.abs(got - want) / scale).max()
        pools = (np.abs(final2[:, 14:26] - final[:, 14:26]) / np.maximum(np.abs(final[:, 14:26]), 1e-2)).max()
        delta = np.abs(final2[:, 26] - final[:, 26])
        return n_moved, planes, pools, delta.max(), (delta / final[:, CARBON].sum(axis=1)).max()
    n_moved, planes, pools, delta, delta_rel = figures(lambda x: np.nextafter(x, 0.0))
    _, planes32, pools32, _, _ = figures(float_ulp_toward_zero)
    print(f"{schedule} {flagset}: {n_moved} amounts one ulp toward zero: planes {planes:.2e} of the plane maximum, twelve pools {pools:.2e}, "
          f"plantCAccountingDelta {delta:.2e} gC = {delta_rel:.2e} of the total carbon (largest |delta| {np.abs(final[:, 26]).max():.2e}); "
          f"a float's ulp: planes {planes32:.2e}, pools {pools32:.2e}")
    held = sum(1 for e in ev for i in range(er.N_PARAMS[e.type]) if (e.type == er.IRRIG and i == 1) or e.p[i] in (0.0, 1.0))
    assert n_moved == sum(er.N_PARAMS[e.type] for e in ev) - held and n_moved >= 6
    assert (final[:, CARBON].sum(axis=1) > 1.0).all()
    assert planes <= 1e-12 and pools <= 1e-12 and delta_rel <= 1e-12
