"""The record-writing ("Full") builds of the step kernels beyond one temperate spring window: the 44-column record, the
accumulators of the restart schema and the planes of the same launch, in fp64 and in fp32-mixed, on the windows
tests/record_windows.py picks from the oracle (tests/test_record_windows.py holds each window to what it is there for):

  A  melt, switch, thaw: a record launch between lean launches of one year -- the Full build takes over the state a lean
     launch left (possibly inside the regular-tile path) and hands its own to the next lean launch
  B  12-hour and 0.6 / 0.4-day steps, the whole run with the record
  C  the yearly accumulators (state slots 20..26) across a new year, SIPNET_KOPT_FULL_STATE, the record around the new year
  D  eight sites of three lengths (the XCD-grouped chunk mapping of the two-chunk launches), launches cut at 7 and 64, a record
     pitch ld = ncol + 5 with a sentinel in the pad columns and in the rows past a site's end
  E  melt once more with the other plain-exponent instantiation of every cooperative family

Bounds (the fuzzer's record criterion, tools/fuzz_gpu.py, as in tests/test_gpu_state_edits.py; not tuned):
  fp64        each of the 36 columns within 1e-9 of the largest value the member's column takes in the whole run (floor 1e-3)
  fp32-mixed  the worst figure below 5e-3, or below 5e-2 with fewer than 1e-4 of the values over 5e-3
The whole run's planes and final pools by regime_gpu_common.judge, unchanged.  The event-log columns 36..43 against the
strict-order kernel cut the same way: rtol 1e-9, atol 1e-12 and deaths on the same steps in fp64; fp32-mixed, which may take
a phenology threshold a step apart, by each member's sum of a column over the window (5e-3 of the largest sum of the column,
floor 1e-3) and by who dies.  Accumulators: fp64 rtol 1e-9, atol 1e-9; fp32-mixed judge's pool bound (5e-3, floor 1.0), and
yearlyNee / totNee, sums that cancel, within 2e-3 of the oracle's sum of |NEE| over the same steps plus 1.
No member is left out of any comparison: record_windows' one-ulp figure names none on melt and thaw.

Achieved on an MI355X (a slice of the families: strict, coop_lds fp32-mixed, the two-chunk nitrogen layouts fp64, one_wave on
`everything` in both precisions, all of D; fp64: record, planes, pools | fp32-mixed: record, share over 5e-3, planes max, pools):
  melt      1.7e-13, 3.5e-14, 3.9e-11 (strict: 1.5e-14, 9.6e-16, 1.1e-11) | 1.2e-5, 0, 4.8e-7, 1.8e-4
  switch    8.6e-14, 2.8e-14, 1.3e-11 (strict: 1.7e-14, 2.4e-16, 4.0e-12) | 8.8e-6, 0, 3.7e-7, 4.8e-4
  thaw      2.5e-14, 3.2e-14, 1.9e-11 (strict: 9.4e-16, 1.1e-15, 2.4e-12) | 1.4e-6, 0, 7.0e-7, 3.5e-4
  halfday   7.0e-11 (nUptake under `everything`), 4.2e-14, 5.5e-12 (strict: 1.5e-13, 6.2e-16, 1.0e-11) | 2.4e-4 (woodCreation),
            0, 6.2e-7, 5.0e-4; event log 1.8e-12 off the strict kernel's, 133 members leaf on and off under the three
            optional flag sets, none under `default` (base_forest.param: leafGrowth 0, fracLeafFall 0)
  newyear   accumulators 5.8e-15 (largest difference 1.2e-13), record 1.9e-14 | 5.9e-7, totNee / yearlyNee 1.4e-7 of the sum of
            |NEE|, record 5.3e-7
  eight sites, ld = ncol + 5: 1.8e-13 | 1.0e-6; the sentinel intact in the pad columns and past every site's end
  event log of the windows: equal to the strict kernel's to 2.8e-14 (fp32-mixed: window sums to 1.7e-7)"""
import functools

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd._lib import check, ptr
from sipnet_amd.config import param_index as pi
from tests import record_windows as rw
from tests.regime_gpu_common import batch, judge
from tests.test_gpu_configs import _scenario

pytestmark = pytest.mark.gpu
F64, F32 = sa.F64, sa.F32_MIXED
KERNEL_OF = {"strict": (sa.KERNEL_AUTO, 0), "one_wave": (sa.KERNEL_ONE_WAVE, 0), "runtime_flags": (sa.KERNEL_ONE_WAVE, sa.KOPT_RUNTIME_FLAGS),
             "coop_lds": (sa.KERNEL_COOP_LDS, 0), "coop_hbm": (sa.KERNEL_COOP_HBM, 0), "coop_pair": (sa.KERNEL_COOP_PAIR, 0),
             "coop_ncycle": (sa.KERNEL_COOP_NCYCLE, 0), "coop_ncycle_pair": (sa.KERNEL_COOP_NCYCLE_PAIR, 0)}
FAMILIES = {"default": ["strict", "one_wave", "runtime_flags", "coop_lds", "coop_hbm", "coop_pair"],
            "russell_3": ["one_wave", "coop_lds", "coop_hbm", "coop_pair"],
            "ncycle": ["one_wave", "coop_ncycle", "coop_ncycle_pair"],
            "everything": ["one_wave", "coop_ncycle", "coop_ncycle_pair"]}
RUNS = [(fs, fam, p) for fs, fams in FAMILIES.items() for fam in fams for p in (F64, F32) if not (fam == "strict" and p == F32)]
ident = lambda c: "-".join(str(x) if not isinstance(x, int) else ("f64" if x == F64 else "f32") for x in c)


def record_kernel(flagset, family, prec, plain):
    """the name last_launch() gives the record launch of this family (step_kernel.hip, step_fast.hip, step_coop.hip)"""
    r, pe = "double" if prec == F64 else "float", "true" if plain else "false"
    x = {"default": "", "russell_3": "X"}.get(flagset)
    if family == "strict":
        return "stepKernel<Cfg<double, false, true, true>>"
    if family in ("one_wave", "runtime_flags"):
        mode = 0 if (flagset, family) == ("default", "one_wave") else 2 if flagset == "ncycle" else 1
        return f"stepFastKernel<{r}, {pe}, {mode}, 1, true>"
    if family in ("coop_lds", "coop_hbm"):
        return f"stepCoop{x}Kernel<{r}, {pe}, {'true' if family == 'coop_lds' else 'false'}, true>"
    if family == "coop_pair":
        return f"stepCoop{x}PairKernel<{r}, {pe}, true>"
    nx = "NX" if flagset == "everything" else "N"
    return f"stepCoop{nx}{'Pair' if family == 'coop_ncycle_pair' else ''}FullKernel<{r}, {pe}>"


def check_record_kernel(name, flagset, family, prec, plain):
    assert name == record_kernel(flagset, family, prec, plain), (name, record_kernel(flagset, family, prec, plain))
    assert ("double" if prec == F64 else "float") in name
    if flagset in ("default", "russell_3") and family != "strict":
        assert name.split(",")[-1].strip(" >") == "true", name                 # Full: the last template argument


@pytest.fixture(scope="module")
def ref(oracle):
    return rw.Reference(oracle)


@pytest.fixture(scope="module")
def strict_log():
    """the event-log columns 36..43 of the window from a strict-order batch cut the same way, once per window; with
    phenology=True the batch's final phenology bits too (state slot 27: 1 didLeafGrowth | 2 didLeafFall)"""
    cache = {}

    def get(w, flipped, cuts, options=0, phenology=False):
        key = (w.case, w.flagset, flipped)
        if key not in cache:
            run = cut_run(w, "strict", F64, cuts, options)
            cache[key] = (run["rec"][:, 36:], run["state"][:, 27].astype(int))
        return cache[key] if phenology else cache[key][0]
    return get


def cut_run(w, family, prec, cuts, options=0):
    """cuts: (first step, end, with the record) per launch; one of them has the record -> planes [3][T][M] as doubles and as
    the batch wrote them, rec [b - a][44][M], state, status, names per launch"""
    kernel, opts = KERNEL_OF[family]
    b = batch(w.flags, [w.clim], w.members, prec, kernel, opts | options, strict=family == "strict")
    M = w.members.shape[0]
    planes = torch.zeros((3, w.T, M), dtype=b.out_dtype, device=b.device)
    rec = torch.full((w.b - w.a, sa.NREC, M), np.nan, dtype=torch.float64, device=b.device)
    names = []
    for x, z, full in cuts:
        assert not full or (x, z) == (w.a, w.b)
        b.run(x, z - x, planes=planes[:, x:z], rec=rec if full else None)
        names.append(b.last_launch()["kernel"])
    out = dict(raw=planes.cpu().numpy(), planes=planes.double().cpu().numpy(), rec=rec.cpu().numpy(), state=b.get_state(),
               status=b.get_status(), names=names, record_name=names[[c[2] for c in cuts].index(True)])
    b.close()
    return out


def window_cuts(w):
    return [c for c in ((0, w.a, False), (w.a, w.b, True), (w.b, w.T, False)) if c[1] > c[0]]


def judge_record(tag, prec, w, got):
    """the 36 output columns of the window against the oracle's, every member"""
    assert got.shape == w.rows.shape and (w.status == 0).all()
    rel = np.abs(got - w.rows) / w.scale()[None]
    keep = np.ones(rel.shape[2], dtype=bool) if prec == F64 else ~w.f32_excluded()
    rel = rel[:, :, keep]
    worst, over = float(np.nanmax(rel)), float((rel > 5e-3).mean())
    t, c, m = np.unravel_index(np.nanargmax(rel), rel.shape)
    print(f"{tag}: record columns {worst:.2e} of the column maximum (step {w.a + t}, column {c}, member {np.flatnonzero(keep)[m]}: got "
          f"{got[t, c, np.flatnonzero(keep)[m]]!r}, the oracle {w.rows[t, c, np.flatnonzero(keep)[m]]!r}), share over 5e-3: {over:.2e}")
    assert np.isfinite(got).all(), tag
    assert worst < 1e-9 if prec == F64 else (worst < 5e-3 or (worst < 5e-2 and over < 1e-4)), tag


def judge_event_log(tag, prec, got, want):
    """columns 36..43 against the strict-order kernel's"""
    assert np.isfinite(got).all() and got.shape == want.shape
    if prec == F64:
        print(f"{tag}: event log {np.abs(got - want).max():.2e} off the strict kernel's, {int(want[:, 7].sum())} deaths, "
              f"{int((want[:, 0] > 0).any(axis=0).sum())} members leaf on, {int((want[:, 2] > 0).any(axis=0).sum())} leaf off")
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
        assert np.array_equal(got[:, 7], want[:, 7])                            # deaths on the same steps
    else:
        sums_g, sums_w = got.sum(axis=0), want.sum(axis=0)                      # [8][M]
        rel = np.abs(sums_g - sums_w) / np.maximum(np.abs(sums_w).max(axis=1, keepdims=True), 1e-3)
        print(f"{tag}: event log, sums over the window {rel[:7].max():.2e} of the column's largest sum off the strict kernel's")
        assert rel[:7].max() < 5e-3, tag
        assert np.array_equal(sums_g[7] > 0, sums_w[7] > 0), tag               # who dies


def same_as_planes(prec, run, w):
    """the planes of the record launch are bit for bit the record's columns 0..2 (fp32-mixed: narrowed to the planes' floats)"""
    for k in range(3):
        col = run["rec"][:, k]
        assert np.array_equal(run["raw"][k, w.a:w.b], col if prec == F64 else col.astype(np.float32)), k


def whole_run_reference(w):
    """planes, final records and status as run_block gives them, from a window that covers the whole run"""
    assert (w.a, w.b) == (0, w.T)
    return np.ascontiguousarray(w.rows[:, :3].transpose(1, 0, 2)), w.last.T, w.status


# ---- A: a record launch between lean launches -----------------------------------------------------------------------------------
A_CASES = [(case,) + r for case in ("melt", "switch", "thaw") for r in RUNS]


def run_window(ref, strict_log, case, flagset, family, prec, flipped=False):
    w = ref.window(case, flagset, flipped)
    want, final, st = ref.planes(case, flagset, flipped)
    cuts = window_cuts(w)
    run = cut_run(w, family, prec, cuts)
    plain = (flagset == "default") != flipped
    check_record_kernel(run["record_name"], flagset, family, prec, plain)
    if family != "strict":
        lean = [n for n, c in zip(run["names"], cuts) if not c[2]]
        assert all(("Full" not in n) if family.startswith("coop_ncycle") else n.endswith("false>") for n in lean) and run["record_name"] not in lean, run["names"]
    tag = f"{case} {flagset} {run['record_name']}"
    judge_record(tag, prec, w, run["rec"][:, :36])
    judge(tag, prec, run["planes"], run["state"], run["status"], want, final, st, w.f32_excluded() if prec == F32 else None)
    same_as_planes(prec, run, w)
    judge_event_log(tag, prec, run["rec"][:, 36:], strict_log(w, flipped, cuts))
    return run


@pytest.mark.parametrize("case,flagset,family,prec", A_CASES, ids=[ident(c) for c in A_CASES])
def test_a_record_window_inside_a_lean_year(case, flagset, family, prec, ref, strict_log):
    run_window(ref, strict_log, case, flagset, family, prec)


# ---- B: 12-hour and alternating steps, the whole run with the record ----------------------------------------------------------
B_CASES = [(case,) + r for case in ("halfday_12h", "halfday_alternating") for r in RUNS]


@pytest.mark.parametrize("case,flagset,family,prec", B_CASES, ids=[ident(c) for c in B_CASES])
def test_half_day_steps_with_the_record(case, flagset, family, prec, ref, strict_log):
    w = ref.window(case, flagset)
    cuts = [(0, w.T, True)]
    run = cut_run(w, family, prec, cuts)
    check_record_kernel(run["record_name"], flagset, family, prec, flagset == "default")
    tag = f"{case} {flagset} {run['record_name']}"
    judge_record(tag, prec, w, run["rec"][:, :36])
    judge(tag, prec, run["planes"], run["state"], run["status"], *whole_run_reference(w))
    same_as_planes(prec, run, w)
    # leaf-on and leaf-off each happen for at least half of the members: by the strict kernel's phenology bits at the end
    # of the year, and -- where the parameter file gives the two events an amount (base_forest.param has leafGrowth 0 and
    # fracLeafFall 0: `default` logs 0 on any forcing) -- by the amounts in columns 36 and 38
    log, bits = strict_log(w, False, cuts, phenology=True)
    M = log.shape[2]
    assert ((bits & 1) != 0).sum() * 2 >= M and ((bits & 2) != 0).sum() * 2 >= M, bits
    if flagset != "default":
        assert (log[:, 0] > 0).any(axis=0).sum() * 2 >= M and (log[:, 2] > 0).any(axis=0).sum() * 2 >= M
    judge_event_log(tag, prec, run["rec"][:, 36:], log)


# ---- C: the accumulators across a new year ---------------------------------------------------------------------------------------
def oracle_accumulators(w):
    """state slots 14..26 [M][13] from the oracle's last record and debug row (include/sipnet_amd.h)"""
    want = np.zeros((w.members.shape[0], 13))
    want[:, 0], want[:, 5] = w.last[35], w.last[3]                # totGpp, totNee
    want[:, 1:5] = w.debug[63:67].T                               # totRtot, totRa, totRh, totNpp
    want[:, 6:13] = w.debug[56:63].T                              # yearly{Gpp, Rtot, Ra, Rh, Npp, Nee, Litter}
    return want


@pytest.mark.parametrize("flagset,family,prec", RUNS, ids=[ident(c) for c in RUNS])
def test_accumulators_across_the_new_year(flagset, family, prec, ref, strict_log):
    w = ref.window("newyear", flagset)
    cuts = window_cuts(w)
    assert [c[:2] for c in cuts] == [(0, 473), (473, 487), (487, 960)]
    run = cut_run(w, family, prec, cuts, sa.KOPT_FULL_STATE)
    check_record_kernel(run["record_name"], flagset, family, prec, flagset == "default")
    assert family == "strict" or run["names"] == [run["record_name"]] * 3, run["names"]     # full state: the same build without the record
    tag = f"newyear {flagset} {run['record_name']}"
    want, got = oracle_accumulators(w), run["state"][:, 14:27]
    nee = [5, 11]                                                              # totNee, yearlyNee: sums that cancel
    other = [k for k in range(13) if k not in nee]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    nee_rel = np.abs(got[:, nee] - want[:, nee]) / (w.abs_nee.T + 1.0)
    print(f"{tag}: accumulators {rel[:, other].max():.2e} (floor 1.0), totNee / yearlyNee {nee_rel.max():.2e} of the sum of |NEE|; "
          f"largest |difference| {np.abs(got - want).max():.2e}")
    assert (want[:, 7] > 0).all() and (want[:, 7] < want[:, 1]).all()          # yearlyRtot was reset, and has grown again
    if prec == F64:
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
    else:
        assert rel[:, other].max() < 5e-3 and nee_rel.max() < 2e-3, tag
    judge_record(tag, prec, w, run["rec"][:, :36])
    want_planes, final, st = ref.planes("newyear", flagset)
    judge(tag, prec, run["planes"], run["state"], run["status"], want_planes, final, st)
    same_as_planes(prec, run, w)
    judge_event_log(tag, prec, run["rec"][:, 36:], strict_log(w, False, cuts, sa.KOPT_FULL_STATE))


# ---- D: several sites, ragged ends, a padded pitch -------------------------------------------------------------------------------
D_FAMILIES = [("default", "coop_lds"), ("default", "coop_hbm"), ("default", "coop_pair"), ("default", "one_wave"), ("ncycle", "coop_ncycle_pair")]
D_CASES = [(fs, fam, p) for fs, fam in D_FAMILIES for p in (F64, F32)]
D_SITES, D_MEMBERS, D_STEPS, D_PAD, SENTINEL = 8, 70, 107, 5, -7777.0
D_LENGTHS = [(107, 78, 107 - 16)[s % 3] for s in range(D_SITES)]
D_CUTS = (0, 7, 64, 107)


@functools.lru_cache(maxsize=None)
def sites_scenario(flagset):
    """the first 107 steps of the events scenario; every site its own 70 members of the 150, member 5 never alive"""
    base = rw.members(flagset)[0]
    clim, ev, members = _scenario(base, lethal=True)
    per_site = []
    for s in range(D_SITES):
        m = members[10 * s:10 * s + D_MEMBERS].copy()
        m[5, pi("plantWoodInit")] = 0.0
        per_site.append(m)
    return clim.slice(0, D_STEPS), ev, per_site


@pytest.mark.parametrize("flagset,family,prec", D_CASES, ids=[ident(c) for c in D_CASES])
def test_eight_ragged_sites_and_a_padded_record_pitch(flagset, family, prec, oracle):
    clim, ev, per_site = sites_scenario(flagset)
    flags, (kernel, opts) = rw.flags(flagset), KERNEL_OF[family]
    ncol = D_SITES * D_MEMBERS
    ld = ncol + D_PAD
    b = sa.Batch(flags, D_SITES, D_MEMBERS, prec, fast_math=True if prec == F64 else None, kernel=kernel, kernel_options=opts)
    for s in range(D_SITES):
        b.set_events(s, ev)
        b.set_climate(s, clim.slice(0, D_LENGTHS[s]))
        b.set_params(s, per_site[s])
    b.setup()
    assert b.n_steps == D_STEPS and [b.site_n_steps(s) for s in range(D_SITES)] == D_LENGTHS
    planes = torch.full((3, D_STEPS, ld), SENTINEL, dtype=b.out_dtype, device=b.device)
    rec = torch.full((D_STEPS, sa.NREC, ld), SENTINEL, dtype=torch.float64, device=b.device)
    for x, z in zip(D_CUTS[:-1], D_CUTS[1:]):
        check(b.L.sipnet_batch_run(b.h, x, z - x, ptr(planes[0, x:]), ptr(planes[1, x:]), ptr(planes[2, x:]), ptr(rec[x:]), ld,
                                   b._stream()), "run")
        li = b.last_launch()
        check_record_kernel(li["kernel"], flagset, family, prec, flagset == "default")
        chunks = D_SITES * ((D_MEMBERS + 63) // 64)
        if family in ("coop_pair", "coop_ncycle_pair"):
            assert D_SITES % 8 == 0 and li["grid"] == 8 * ((chunks // 8 + 1) // 2), li       # the XCD-grouped mapping's grid
        else:
            assert li["grid"] == chunks, li
    got, pl, status = rec.cpu().numpy(), planes.double().cpu().numpy(), b.get_status()
    b.close()
    assert (status == 0).all()
    # the sentinel survives in the pad columns and in every row past a site's end, and nowhere else
    assert (got[:, :, ncol:] == SENTINEL).all() and (pl[:, :, ncol:] == SENTINEL).all()
    worst = 0.0
    rels = []
    for s in range(D_SITES):
        cols, n = slice(s * D_MEMBERS, (s + 1) * D_MEMBERS), D_LENGTHS[s]
        assert (got[n:, :, cols] == SENTINEL).all() and (pl[:, n:, cols] == SENTINEL).all(), s
        assert (got[:n, :, cols] != SENTINEL).all() and (pl[:, :n, cols] != SENTINEL).all(), s
        for m in range(D_MEMBERS):                              # (every member: the one never alive and the ragged chunk's last among them)
            st, want, _ = oracle.run_member(flags, per_site[s][m], clim.slice(0, n), ev)
            assert st == 0
            rels.append((np.abs(got[:n, :36, s * D_MEMBERS + m] - want) / np.maximum(np.abs(want).max(axis=0), 1e-3)).ravel())
        assert np.array_equal(pl[:, :n, cols], got[:n, :3, cols].transpose(1, 0, 2) if prec == F64
                              else got[:n, :3, cols].transpose(1, 0, 2).astype(np.float32).astype(np.float64)), s
    rel = np.concatenate(rels)
    worst, over = float(rel.max()), float((rel > 5e-3).mean())
    print(f"{flagset} {li['kernel']}, eight sites, ld = ncol + {D_PAD}: record columns {worst:.2e} of the column maximum, share over 5e-3: {over:.2e}")
    assert worst < 1e-9 if prec == F64 else (worst < 5e-3 or (worst < 5e-2 and over < 1e-4))


# ---- E: the other exponent instantiation -----------------------------------------------------------------------------------------
E_CASES = [(fs, fam) for fs, fams in FAMILIES.items() for fam in fams if fam.startswith("coop")]


@pytest.mark.parametrize("flagset,family", E_CASES, ids=[a + "-" + b for a, b in E_CASES])
def test_melt_with_the_other_exponent_instantiation(flagset, family, ref, strict_log):
    run = run_window(ref, strict_log, "melt", flagset, family, F64, flipped=True)
    assert run["record_name"] != record_kernel(flagset, family, F64, flagset == "default")
