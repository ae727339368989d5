"""sipo_run_block_edits (oracle/sipnet_oracle.c): the oracle's run with pools and parameters overwritten between steps,
pinned without a GPU -- against records of the REAL reference step loop with `envi` overwritten at the same steps
(tests/golden/ref_edit_records.npz, written by tools/make_golden.py through oracle/ref_harness.c), against
sipo_run_block's bits, and against the plain run of another member.  Then the edit sets of tests/state_edits.py, which
tests/test_gpu_state_edits.py puts on the kernels: that each set is what it claims, that leaf-on falls between the first and
the last edit, and the conditioning yardstick of tests/test_parameter_regimes.py under the same rule -- the continuous edited
values (scaled and restored pools, 12 x leafCSpWt, 2 x soilWHC) one ulp toward zero, the exact constants 0 and 30 and the
deltas placed on the alive threshold held; planes within 1e-12 of the plane maximum (floor 1e-3), final pools within 1e-12 (floor 1e-2).  An edit set
that fails it is narrowed or dropped; the GPU bound is never widened for it.

An edit that leaves a member dead at the head of the next step resets its running mean of NPP in these sequences, as
include/sipnet_amd.h defines it and tests/test_gpu_state_edits.py applies it (edit_ring_reset, pinned to the reference's own
resetMeanTracker by the fixture's second record set).

Measured (the edited values one ulp toward zero: planes | final pools | the planes figure scaled to a float's ulp):
  default     6.5e-16 | 2.4e-14 | 3.5e-7
  ncycle      1.2e-15 | 3.6e-14 | 6.6e-7
  russell_3   7.3e-16 | 5.1e-14 | 3.9e-7
Narrowed: litterC = 0 is not dealt under the nitrogen cycle -- the reference divides by the empty pool there (litterC /
litterN = 0, rLitter / 0 = 0 / 0) and all 14 such members' planes were NaN from the step after the edit."""
import os

import numpy as np
import pytest

import sipnet_amd as sa
from sipnet_amd.config import param_index as pi
from tests import helpers
from tests import parameter_regimes as pr
from tests import state_edits as se

FLAG_SETS = list(pr.FLAG_SETS)


@pytest.mark.parametrize("case_name", ["niwot", "russell_2", "russell_3"])
def test_oracle_with_edits_equals_the_reference_step_loop_exactly(case_name, oracle, tmp_path):
    ref = np.load(os.path.join(helpers.GOLDEN, "ref_edit_records.npz"))
    case = helpers.load_smoke_case(case_name, str(tmp_path))
    n = 2000
    clim = case["clim"].slice(0, n)
    end = (int(case["clim"].year[n]), int(case["clim"].day[n]))
    events = [e for e in case["events"] if (e.year, e.day) < end]           # (the forcing was cut for the reference too)
    steps, pools, idx = ref[f"{case_name}_steps"], ref[f"{case_name}_pools"], ref[f"{case_name}_idx"]
    assert len(steps) == 3 and pools.shape == (3, 13) and (pools[0, [0, 6, 7]] == 0).all() and (pools[1, [0, 6, 7]] > 0).all()
    if case_name == "russell_2":                              # the second edit falls on the record of the first fertiliser event
        assert case["flags"][0] and (events[0].year, events[0].day) == (int(clim.year[steps[1]]), int(clim.day[steps[1]]))
        assert int(clim.day[steps[1] - 1]) != int(clim.day[steps[1]])
    _, final, st, diag, rec = oracle.run_block_edits(case["flags"], case["params"][None], clim, steps, pools[:, None, :],
                                                     events=events, rec_member=0)
    assert st[0] == 0
    assert np.array_equal(rec[idx], ref[f"{case_name}_rec"])
    assert np.array_equal(final[0], rec[-1]) and idx[-1] == n - 1
    # emptied at the head of a step: dead from there on, without a death step
    assert rec[steps[0], 14] == 0.0 and rec[steps[0], 1] == 0.0 and rec[steps[1], 14] > 1.0 and diag[0].died_at_step == -1
    # ... and with the running mean reset at the emptying, as the reference's death step resets it
    rec2 = oracle.run_block_edits(case["flags"], case["params"][None], clim, steps, pools[:, None, :], events=events, rec_member=0,
                                  ring_reset=[[1], [0], [0]])[4]
    assert np.array_equal(rec2[idx], ref[f"{case_name}_rec_reset"]) and rec2[steps[0], 32] == 0.0 and rec[steps[0], 32] != 0.0
    plain = oracle.run_member(case["flags"], case["params"], clim, events)[1]
    assert np.array_equal(plain[:steps[0]], rec[:steps[0]]) and not np.array_equal(plain[steps[0]], rec[steps[0]])


@pytest.fixture(scope="module")
def forest():
    return {f: (se.members(f), se.clim()) for f in FLAG_SETS}


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_an_all_nan_table_and_an_empty_one_give_run_blocks_bits(flagset, oracle, forest):
    members, clim = forest[flagset]
    members, clim = members[:40], clim.slice(0, 700)
    want = oracle.run_block(se.flags(flagset), members, clim)
    nan = np.full((3, 40, 13), np.nan)
    for steps, pools, prm in (((0, 333, 699), nan, None), ((0, 333, 699), nan, np.full((3, 40, 80), np.nan)), ((), nan[:0], None)):
        got = oracle.run_block_edits(se.flags(flagset), members, clim, steps, pools, prm)
        for g, w in zip(got[:3], want):
            assert g.tobytes() == w.tobytes()
    # refusals: steps out of order or out of range
    for steps in ((5, 5, 9), (9, 5, 700), (-1, 5, 9)):
        L, vp = oracle.lib, lambda a: a.ctypes.data_as(helpers.C.c_void_p)
        s32 = np.array(steps, dtype=np.int32)
        fl = (helpers.C.c_int * 12)(*se.flags(flagset))
        rc = L.sipo_run_block_edits(fl, vp(members), 0, 40, 40, 700, vp(clim.data), vp(clim.year), vp(clim.day), 0, None, None,
                                    None, None, None, None, 3, vp(s32), vp(nan), None, None, None, None)
        assert rc == 3


def setup_pools(raw, flags):
    """setupMember's expressions (sipnet.c:1858-1951) in numpy: the 13 pools a member starts with"""
    col = lambda n: raw[:, pi(n)]
    litter, ncycle = flags[sa.FLAG_NAMES.index("litterPool")], flags[sa.FLAG_NAMES.index("nitrogenCycle")]
    p = np.zeros((raw.shape[0], 13))
    p[:, se.WOOD] = (1 - col("coarseRootFrac") - col("fineRootFrac")) * col("plantWoodInit")
    p[:, se.LEAF] = col("laiInit") * col("leafCSpWt")
    p[:, se.LITTER] = col("litterInit") if litter else 0.0
    p[:, se.SOILC] = col("soilInit")
    p[:, se.COARSE] = col("coarseRootFrac") * col("plantWoodInit")
    p[:, se.FINE] = col("fineRootFrac") * col("plantWoodInit")
    p[:, se.WATER] = np.maximum(col("soilWFracInit") * col("soilWHC"), 0.0)
    p[:, se.SNOW] = col("snowInit")
    if ncycle:
        p[:, se.MIN_N], p[:, se.ORG_N] = col("mineralNInit"), col("soilOrgNInit")
        p[:, se.LITTER_N], p[:, se.STORAGE_N] = col("litterOrgNInit"), col("plantStorageNInit")
    return p


INITS = ["plantWoodInit", "laiInit", "litterInit", "soilInit", "soilWFracInit", "snowInit", "mineralNInit", "soilOrgNInit",
         "litterOrgNInit", "plantStorageNInit", "coarseRootFrac", "fineRootFrac"]


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_member_bs_initial_pools_written_into_member_a_at_step_0_give_bs_run(flagset, oracle, forest):
    """B is A with other *Init parameters (and root fractions, which only the setup reads): A with B's pools laid over
    it before the first step IS B, bit for bit -- planes, final record, status"""
    a, clim = forest[flagset]
    a, clim = a[:24].copy(), clim.slice(0, 600)
    flags = se.flags(flagset)
    rng = np.random.default_rng(3)
    b = a.copy()
    for n in INITS:
        b[:, pi(n)] = a[:, pi(n)] * rng.uniform(0.5, 1.5, 24) + (0.2 if n in ("laiInit", "snowInit") else 0.0)
    b[:, pi("soilWFracInit")] = rng.uniform(0.0, 1.0, 24)
    b[:, pi("coarseRootFrac")], b[:, pi("fineRootFrac")] = rng.uniform(0.05, 0.3, 24), rng.uniform(0.05, 0.3, 24)
    want = oracle.run_block(flags, b, clim)
    pools = setup_pools(b, flags)
    # (what survives of A's own setup is the tracker's first soil wetness, which nothing reads before it is rewritten)
    got = oracle.run_block_edits(flags, a, clim, (0,), pools[None])
    assert (want[2] == 0).all() and not np.array_equal(oracle.run_block(flags, a, clim)[0], want[0])
    for g, w in zip(got[:3], want):
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_edit_sets_are_what_they_claim(flagset, forest):
    members, _ = forest[flagset]
    kinds, deal = se.kinds(flagset), se.lane_kinds(flagset)
    assert se.M == 200 == len(deal) and [deal[m] for m in (0, 63, 64, 127, 128, 199)] == ["emptied", "just_dying", "just_surviving"] * 2
    assert ("litter_0" in kinds) == (flagset == "russell_3") and ("min_n_0" in kinds) == ("storage_n_0" in kinds) == (flagset == "ncycle")
    for w in range(4):                                        # every wavefront: dying and living lanes, every kind but in the ragged one
        lanes = deal[64 * w:64 * (w + 1)]
        assert {"just_dying", "untouched", "scale"} <= set(lanes) or w == 3
        assert w == 3 or set(lanes) == set(kinds)
    sharp = {"just_dying", "just_surviving", "emptied"}
    assert sharp & set(deal[192:]) and set(deal[192:]) - sharp            # the ragged chunk of 8 too
    assert se.lane_kinds(flagset, 400)[200:] == deal
    rng = np.random.default_rng(1)
    state = rng.uniform(0.5, 2000.0, (200, 32))
    memo, cur = {}, state
    for ci in range(3):
        new = se.apply(flagset, ci, cur, members, memo)
        assert new[:, 13:].tobytes() == cur[:, 13:].tobytes() and new is not cur
        assert np.isfinite(new).all() and (new[:, [k for k in range(13) if k != se.DELTA]] >= 0).all()
        for c, kind in enumerate(deal):
            changed = set(np.flatnonzero(new[c, :13] != cur[c, :13]).tolist())
            if kind == "untouched":
                assert not changed
            elif kind == "scale":
                f = se.factors(ci, 200)[c]
                assert 0.25 <= f <= 4.0 and changed == set(se.CARBON) and np.array_equal(new[c, list(se.CARBON)], cur[c, list(se.CARBON)] * f)
            elif kind == "emptied":
                assert (ci == 0 and changed == {se.WOOD, se.COARSE, se.FINE} and (new[c, [se.WOOD, se.COARSE, se.FINE]] == 0).all()) or \
                    (ci == 1 and not changed) or (ci == 2 and np.array_equal(new[c, :13], state[c, :13]))
            elif kind in ("just_dying", "just_surviving"):
                assert changed == ({se.DELTA} if ci == c % 3 else set())
                if changed:
                    s = new[c, se.WOOD] + new[c, se.DELTA]
                    up, down = new[c, se.WOOD] + np.nextafter(new[c, se.DELTA], np.inf), new[c, se.WOOD] + np.nextafter(new[c, se.DELTA], -np.inf)
                    assert (s > se.TINY and not down > se.TINY) if kind == "just_surviving" else (not s > se.TINY and up > se.TINY)
            else:
                slot, cut, value = {"leaf_0": (se.LEAF, 2, 0.0), "leaf_12": (se.LEAF, 0, 12.0 * members[c, pi("leafCSpWt")]),
                                    "water_0": (se.WATER, 1, 0.0), "water_2whc": (se.WATER, 2, 2.0 * members[c, pi("soilWHC")]),
                                    "snow_0": (se.SNOW, 0, 0.0), "snow_30": (se.SNOW, 2, 30.0), "litter_0": (se.LITTER, 1, 0.0),
                                    "min_n_0": (se.MIN_N, 1, 0.0), "storage_n_0": (se.STORAGE_N, 0, 0.0)}[kind]
                assert changed == ({slot} if ci == cut else set()) and (ci != cut or new[c, slot] == value)
        tab = se.table(cur, new)
        touched = (new[:, :13] != cur[:, :13]).any(axis=1)
        assert np.isnan(tab[~touched]).all() and np.array_equal(tab[touched], new[touched, :13]) and touched.sum() >= 15
        cur = new


def oracle_sequence(oracle, flagset, members, clim, move=None):
    """the three edits applied to the oracle's own state at the cuts, as tests/test_gpu_state_edits.py applies them to a
    batch's: an edit that leaves a member dead at the head of the next step resets its running mean too
    -> (tables [3][M][13], planes, final, status, diag); move(table, ci) alters a table before it is used (the
    conditioning yardstick)"""
    flags, memo, tables, resets = se.flags(flagset), {}, [], []
    for ci, cut in enumerate(se.CUTS):
        _, final, st, _ = oracle.run_block_edits(flags, members, clim.slice(0, cut), se.CUTS[:ci], np.array(tables).reshape(ci, se.M, 13),
                                                 ring_reset=np.array(resets).reshape(ci, se.M))
        state = np.zeros((se.M, 32))
        state[:, :13] = final[:, 14:27]
        new = se.apply(flagset, ci, state, members, memo)                     # (the two rows `apply` reads are rows the conversion copies)
        tab = se.table(state, new)
        tables.append(tab if move is None else move(tab, ci))
        resets.append(~se.alive(new[:, :13]) & se.alive(state[:, :13]))
    return (np.array(tables),) + oracle.run_block_edits(flags, members, clim, se.CUTS, np.array(tables), ring_reset=np.array(resets))


@pytest.fixture(scope="module")
def sequences(oracle, forest):
    cache = {}

    def get(flagset):
        if flagset not in cache:
            cache[flagset] = oracle_sequence(oracle, flagset, *forest[flagset])
        return cache[flagset]
    return get


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_leaf_on_falls_between_the_first_and_the_last_edit(flagset, oracle, forest, sequences):
    members, clim = forest[flagset]
    assert clim.n_steps == se.T and 39 < se.T / 48 < 41 and clim.day[se.CUTS[0]] != clim.day[se.CUTS[0] - 1] and clim.day[se.CUTS[1] - 1] != clim.day[se.CUTS[1] - 2]
    on = []
    for m in range(0, se.M, 9):
        st, _, dbg = oracle.run_member_debug(se.flags(flagset), members[m], clim)
        assert st == 0 and dbg[0, 67] == 0 and dbg[-1, 67] == 1
        on.append(int(np.argmax(dbg[:, 67] == 1)))
    assert se.CUTS[0] < min(on) and max(on) < se.CUTS[2] and min(on) < se.CUTS[1] < max(on)
    # ... and in the edited run the edits do what they are for
    tables, planes, final, st, diag = sequences(flagset)
    deal = np.array(se.lane_kinds(flagset))
    assert (st == 0).all() and np.isfinite(planes).all() and np.isfinite(final).all()
    died = np.array([d.died_at_step for d in diag])
    print(f"{flagset}: leaf-on at steps {min(on)}..{max(on)}; death steps of the just-surviving members {sorted(set(died[deal == 'just_surviving']))}, "
          f"of the others {sorted(set(died[deal != 'just_surviving']))}")
    # (dead at the head of a step is no death step; a member emptied or put under the threshold is back as soon as its
    # allocation has made 1e-6 gC of wood and roots, and may then die a recorded death)
    assert (final[deal == "emptied", 14] > 1.0).all()         # restored


@pytest.mark.parametrize("flagset", FLAG_SETS)
def test_conditioning_yardstick_of_the_edit_sets(flagset, oracle, forest, sequences):
    members, clim = forest[flagset]
    tables, want, final, st, _ = sequences(flagset)
    deal = np.array(se.lane_kinds(flagset))
    moving = np.isin(deal, se.CONTINUOUS)

    def move(tab, ci):
        out = tab.copy()
        out[moving] = np.nextafter(tab[moving], 0.0)
        return np.where(tab == 0.0, tab, out)                 # (a hand-set 0 stays 0)
    moved_tables, got, final2, st2, _ = oracle_sequence(oracle, flagset, members, clim, move)
    n_moved = int((moved_tables != tables)[~np.isnan(tables)].sum())
    assert n_moved >= 3 * 5 * int((deal == "scale").sum()) and np.array_equal(st, st2)
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-3)
    per_member = (np.abs(got - want) / scale).max(axis=(0, 1))
    pools = (np.abs(final2[:, 14:27] - final[:, 14:27]) / np.maximum(np.abs(final[:, 14:27]), 1e-2)).max(axis=1)
    as_f32 = per_member.max() * (np.finfo(np.float32).eps / np.finfo(np.float64).eps)
    print(f"{flagset}: {n_moved} edited values one ulp toward zero: planes {per_member.max():.2e} of the plane maximum (member {per_member.argmax()}, "
          f"{deal[per_member.argmax()]}), final pools {pools.max():.2e} (member {pools.argmax()}, {deal[pools.argmax()]}); scaled to fp32 {as_f32:.2e}")
    for kind in se.CONTINUOUS:
        print(f"    {kind}: planes {per_member[deal == kind].max():.2e}, pools {pools[deal == kind].max():.2e}")
    assert per_member[moving].max() > 0 and (per_member[~moving] == 0).all()
    assert per_member.max() <= 1e-12 and pools.max() <= 1e-12
    assert as_f32 <= 1e-4                                     # no member joins an fp32-mixed exclusion list
