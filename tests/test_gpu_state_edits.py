"""Forecasts from states the step kernels did not compute themselves, against the oracle's run with the same overwrites
(sipo_run_block_edits, pinned to the real reference's step loop by tests/test_oracle_edits.py): pools edited by hand between
launches (tests/state_edits.py: scaled, emptied and restored, leaf carbon 0 in the growing season, soil water above
capacity, snow in May, mineral N 0, stands put one ulp under and over the alive threshold -- dealt round-robin so that dying
and living lanes share every wavefront, at a cut on a 16-step tile, one step after a midnight, and in mid-morning), the states
the five EnKF analyses leave (the joint one with its parameter rows), and resampled particles.  The bounds are
regime_gpu_common.judge's -- the fuzzer's -- unchanged, in both precisions; tests/test_oracle_edits.py shows that the oracle
does not amplify a one-ulp move of these edits (<= 1.2e-15 of the plane maximum, 5.1e-14 of a pool).

Achieved on an MI355X (hand edits, worst over the families; fp64: planes, pools | fp32-mixed: max, share over 1e-4, time sums, pools):
  default     3.1e-14, 9.2e-12 (strict: 4.3e-16, 7.0e-13) | 3.3e-6, 0, 2.5e-7, 3.3e-6
  ncycle      7.7e-14, 1.0e-12 (strict: 9.9e-16, 5.1e-14) | 1.6e-6, 0, 2.1e-7, 1.6e-6
  russell_3   4.6e-14, 1.5e-12 (strict: 5.0e-16, 2.4e-14) | 9.5e-7, 0, 2.4e-7, 1.3e-6
  death steps: equal to the oracle's in fp64 (28 members of `default`, 13 of them after an edit had killed them; 13 of each
  other set); records at the edit steps and the step after 2.8e-13 of the column maximum (fp32-mixed 1.1e-6)
  analysed states, the five analyses x auto and the four layouts: 9.0e-15, 1.1e-14 | 1.9e-7, 0, 5.1e-8, 1.5e-7
  resampled particles (190 ancestors of 200): 7.2e-14, 1.3e-11 | 5.8e-7, 0, 1.4e-7, 3.2e-6; the nitrogen-cycle layouts (186):
  5.2e-14, 1.3e-12 | 4.2e-7, 0, 1.8e-7, 1.7e-6

Pools that leave a member DEAD AT THE HEAD of the next step (`emptied`, `just_dying`) are where engine and reference part
unless the caller follows include/sipnet_amd.h (sipnet_batch_set_state): every death the model itself produces is a death
step, which resets the running mean of NPP, and the engine takes any dead step as the start of a new ring epoch; the
reference, handed such pools from outside, has no death step, skips the dead steps' inserts and carries its old ring on -- a
ring that stood still, which a ring indexed by step cannot hold.  The header therefore defines such an edit as a death: the
caller writes 0 into slot 13 (the ring sum) and the index of the next step into slot 28 (ring_valid_from) with the pools,
and the oracle is told to reset the member's mean at that edit by the reference's own resetMeanTracker
(edit_ring_reset; pinned to the reference's step loop in tests/test_oracle_edits.py).  With that, every member is judged
against the oracle over the whole window.

fp32-mixed leaves out of the value comparison what tests/test_gpu_parameter_regimes.py leaves out: members whose oracle
planes are not finite (none here), and members whose one-ulp figure scaled to a float's ulp exceeds 1e-4 (none here:
tests/test_oracle_edits.py asserts it); emptied pools are covered by judge's pool floor of 1.0 in that precision.  Of
died_at_step it compares WHO dies, not the step: fp32 fluxes may carry a pool across the alive threshold a step apart from
fp64 (the reason the fuzzer judges fp32-mixed planes by the share of outliers); fp64 is held to the oracle's step.

pf_analysis with_params=False needs a member's state copied between oracle members, which the oracle's entry does not do:
out of scope.

Lean cooperative launches of the hand-edit tests, of the resampled-particle tests and of the plane runs the sums are compared
with run the build with bounded hand-over waits (KOPT_BOUNDED_WAITS): a protocol fault would end as SIPNET_ERR_INTERNAL.  The
product build of every cooperative layout runs in the identity and analysed-state tests only -- and where a record or
in-kernel sums are asked for, which the lean-only bounded build cannot give."""
import functools

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import dist, synth
from tests import parameter_regimes as pr
from tests import state_edits as se
from tests.enkf_gpu_common import ANALYSED, grid, observe, operators, site_clim
from tests.regime_gpu_common import COOP, KERNELS, batch, bits, family_ok, host_sums, judge

pytestmark = pytest.mark.gpu
F64, F32 = sa.F64, sa.F32_MIXED
RUNS = {"default": ["strict", "one_wave", "coop_lds", "coop_hbm", "coop_pair", "coop_quad"],
        "ncycle": ["strict", "one_wave", "coop_ncycle", "coop_ncycle_pair"],
        "russell_3": ["strict", "one_wave", "coop_lds", "coop_hbm", "coop_pair"]}
HAND = [(fs, fam, p) for fs, fams in RUNS.items() for fam in fams for p in (F64, F32) if not (fam == "strict" and p == F32)]
HAND.append(("russell_3", "coop_quad", F32))                  # (optional physics at four chunks: the fp32-mixed build only)
ident = lambda c: "-".join([c[0], c[1], "f64" if c[2] == F64 else "f32"])


@functools.lru_cache(maxsize=None)
def forest(flagset):
    return se.members(flagset), se.clim()


def options(family):
    return sa.KOPT_BOUNDED_WAITS if family.startswith("coop") else 0


def edited_run(flagset, family, prec, cuts=se.CUTS, T=se.T, opts=0, full=False, sums=0):
    """run to each cut, get_state -> edit -> set_state, continue.  -> dict(planes or sums, rec, state, status, names, tables,
    dead [cuts][M]: the members the edit left dead at the head of the next step)"""
    members, clim = forest(flagset)
    b = batch(se.flags(flagset), [clim.slice(0, T)], members, prec, KERNELS[family], opts, strict=family == "strict")
    conv = b.get_params()
    planes, rec = b.alloc_outputs(T, full)
    planes.zero_()
    memo, tables, dead, names, parts = {}, [], [], [], []
    for ci, (a, z) in enumerate(zip((0,) + tuple(cuts), tuple(cuts) + (T,))):
        if sums:
            parts.append(b.run_sums(a, z - a, sums))
        else:
            b.run(a, z - a, planes=planes[:, a:z], rec=rec[a:z] if full else None)
        names.append(b.last_launch()["kernel"])
        if ci < len(cuts):
            st = b.get_state()
            new = se.apply(flagset, ci, st, conv, memo)
            gone = ~se.alive(new[:, :13]) & se.alive(st[:, :13])       # (dead by this edit, not by a death step before it)
            new[gone, 13], new[gone, 28] = 0.0, float(cuts[ci])   # the header's contract: such an edit is a death, the ring starts over
            b.set_state(new)
            tables.append(se.table(st, new))
            dead.append(gone)
    if sums:
        planes = torch.cat(parts, dim=1)
    out = dict(planes=planes.double().cpu().numpy(), rec=rec.cpu().numpy() if full else None, state=b.get_state(), status=b.get_status(),
               names=names, tables=np.array(tables), dead=np.array(dead).astype(np.int32))
    b.close()
    return out


@pytest.mark.parametrize("flagset,family,prec", HAND, ids=[ident(c) for c in HAND])
def test_hand_edits_against_the_oracle(flagset, family, prec, oracle):
    members, clim = forest(flagset)
    run = edited_run(flagset, family, prec, opts=options(family))
    for name in run["names"]:
        assert family_ok(family, flagset, name) and ("double" if prec == F64 else "float") in name, (family, name)
    want, final, st, diag = oracle.run_block_edits(se.flags(flagset), members, clim, se.CUTS, run["tables"], ring_reset=run["dead"])
    assert np.isfinite(want).all() and np.isfinite(final).all() and (st == 0).all()
    deal = np.array(se.lane_kinds(flagset))
    killed = run["dead"].any(axis=0)
    assert set(deal[killed]) == {"emptied", "just_dying"} and killed.sum() == np.isin(deal, ["emptied", "just_dying"]).sum()
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-3)
    rel = np.abs(run["planes"] - want) / scale
    died_o, died_g = np.array([d.died_at_step for d in diag]), run["state"][:, 30].astype(int)
    for kind in se.kinds(flagset):
        print(f"    {kind}: planes {rel[:, :, deal == kind].max():.2e}")
        for m in np.flatnonzero((deal == kind) & (rel.max(axis=(0, 1)) > 1e-4))[:3]:        # where a disagreement starts
            t = int(np.argmax(rel[:, :, m].max(axis=0) > 1e-4))
            print(f"        member {m}: first off by > 1e-4 at step {t} (got {run['planes'][:, t, m]}, oracle {want[:, t, m]}); death step "
                  f"{died_g[m]}, the oracle's {died_o[m]}; killed by the edits at {[int(c) for c, g in zip(se.CUTS, run['dead']) if g[m]]}")
    judge(f"{flagset} {run['names'][-1]}", prec, run["planes"], run["state"], run["status"], want, final, st)
    # died_at_step (state slot 30) against the oracle's diag
    print(f"    death steps recorded by the oracle: {int((died_o >= 0).sum())} members, {int((died_o[killed] >= 0).sum())} of them killed by an edit before")
    if prec == F64:
        assert np.array_equal(died_g, died_o)
    else:                                                     # (fp32 fluxes may cross a threshold a step apart: who dies is compared)
        assert np.array_equal(died_g >= 0, died_o >= 0)


# (the four-chunk layout has no full-state build: no record to ask for; the two-chunk nitrogen-cycle layout has one,
# stepCoopNPairFullKernel)
RECORDS = [("default", "strict", F64), ("default", "one_wave", F64), ("default", "coop_lds", F64), ("default", "coop_hbm", F32),
           ("default", "coop_pair", F64), ("ncycle", "coop_ncycle", F64), ("ncycle", "coop_ncycle_pair", F64), ("default", "coop_pair", F32)]


@pytest.mark.parametrize("flagset,family,prec", RECORDS, ids=[ident(c) for c in RECORDS])
def test_records_at_the_edit_steps_against_the_oracles(flagset, family, prec, oracle):
    """the 36 record columns at each edit step and the step after, by the fuzzer's record criterion (tools/fuzz_gpu.py): each
    column within 1e-9 of the largest value the member's column takes in the run (floor 1e-3); fp32-mixed within 5e-3, or
    within 5e-2 with fewer than 1e-4 of the values over 5e-3"""
    members, clim = forest(flagset)
    run = edited_run(flagset, family, prec, full=True)
    full_n = {"coop_ncycle": "stepCoopNFullKernel<", "coop_ncycle_pair": "stepCoopNPairFullKernel<"}
    assert all(family_ok(family, flagset, n) or (family in full_n and n.startswith(full_n[family])) for n in run["names"]), run["names"]
    steps = [c + k for c in se.CUTS for k in (0, 1)]
    worst, over, n = 0.0, 0, 0
    for m in range(se.M):
        _, _, st, _, rec = oracle.run_block_edits(se.flags(flagset), members, clim, se.CUTS, run["tables"], rec_member=m,
                                                  ring_reset=run["dead"])
        assert st[m] == 0 == run["status"][m]
        rel = np.abs(run["rec"][steps, :36, m] - rec[steps]) / np.maximum(np.abs(rec).max(axis=0), 1e-3)
        worst, over, n = max(worst, float(rel.max())), over + int((rel > 5e-3).sum()), n + rel.size
    print(f"{flagset} {run['names'][-1]}: record columns at the edit steps and the step after: {worst:.2e} of the column maximum, {over} of {n} over 5e-3")
    assert worst < 1e-9 if prec == F64 else (worst < 5e-3 or (worst < 5e-2 and over / n < 1e-4))


SUMS = [("default", "one_wave", F64), ("default", "one_wave", F32), ("default", "coop_lds", F64), ("default", "coop_hbm", F64),
        ("default", "coop_pair", F32), ("default", "coop_quad", F64), ("ncycle", "coop_ncycle", F64), ("ncycle", "coop_ncycle_pair", F32)]


@pytest.mark.parametrize("flagset,family,prec", SUMS, ids=[ident(c) for c in SUMS])
def test_sums_of_the_edited_run_equal_its_planes_added_in_step_order(flagset, family, prec):
    """the same sequence through sipnet_batch_run_sums, cuts at multiples of the group of 7: bit for bit on the cooperative
    kernels, state included; the one-wavefront kernel's summing build by the criterion and over the 205 steps of
    tests/test_gpu_parameter_regimes.py (its two builds round a few products differently, and the difference grows with
    the run).  The planes come from the bounded-wait build (a lean launch), the sums from the product build (the bounded
    build has no summing instantiation)"""
    cuts, T = ((49, 98, 147), 205) if family == "one_wave" else (se.SUM_CUTS, se.T)
    plain = edited_run(flagset, family, prec, cuts, T, opts=options(family))
    summed = edited_run(flagset, family, prec, cuts, T, sums=se.SUM_GROUP)
    assert all("Sums" in n and ("Fast" in n) == (family == "one_wave") for n in summed["names"]), summed["names"]
    want, got = host_sums(plain["planes"], se.SUM_GROUP), summed["planes"]
    assert (plain["status"] == 0).all() and (summed["status"] == 0).all()
    top = np.abs(want).max(axis=1, keepdims=True)
    print(f"{summed['names'][-1]}: sums against the planes added in step order: {(np.abs(got - want) / np.maximum(top, 1e-300)).max():.2e} of the member's largest sum")
    if family == "one_wave":
        np.testing.assert_allclose(got, want, **(dict(rtol=1e-6, atol=1e-8) if prec == F32 else dict(rtol=1e-13, atol=1e-16)))
        np.testing.assert_allclose(summed["state"], plain["state"], rtol=1e-13 if prec == F64 else 1e-5, atol=1e-300 if prec == F64 else 1e-7)
    else:
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(summed["state"], plain["state"])


IDENTITY = [("default", f, p, o) for f in ("strict", "one_wave") + tuple(COOP) for p in (F64, F32) for o in (0, sa.KOPT_NO_REGULAR_TILES)
            if not (f == "strict" and p == F32) and not (o and not f.startswith("coop"))]
IDENTITY += [("ncycle", f, p, o) for f in ("coop_ncycle", "coop_ncycle_pair") for p in (F64, F32) for o in (0, sa.KOPT_NO_REGULAR_TILES)]


@pytest.mark.parametrize("flagset,family,prec,opts", IDENTITY, ids=[ident(c) + ("-no_tiles" if c[3] else "") for c in IDENTITY])
def test_state_and_rings_written_back_as_read_change_nothing(flagset, family, prec, opts):
    members, clim = forest(flagset)
    out = []
    for write_back in (None, True):                           # the uncut run, then the run cut and written back at every cut
        b = batch(se.flags(flagset), [clim], members, prec, KERNELS[family], opts, strict=family == "strict")
        planes = torch.zeros((3, se.T, se.M), dtype=b.out_dtype, device=b.device)
        cuts = se.CUTS if write_back else ()
        for a, z in zip((0,) + cuts, cuts + (se.T,)):
            if write_back and a:
                b.set_state(b.get_state())
                b.set_rings(b.get_rings())
            b.run(a, z - a, planes=planes[:, a:z])
        out.append((planes, b.get_state(), b.get_rings(), b.last_launch()["kernel"], b.get_status()))
        b.close()
    assert family_ok(family, flagset, out[0][3]) and out[0][3] == out[1][3] and (out[0][4] == 0).all()
    assert torch.equal(bits(out[0][0]), bits(out[1][0])), "planes"
    assert out[0][1].tobytes() == out[1][1].tobytes() and out[0][2].tobytes() == out[1][2].tobytes()


ANALYSES = ["sites", "block", "local", "smooth", "joint"]
JOINT_PARAMS = ["aMax", "halfSatPar", "vegRespQ10", "soilWHC", "psnTOpt", "psnTMin"]
LAYOUTS = [("auto", sa.KERNEL_AUTO)] + list(COOP.items())


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("layout,kernel", LAYOUTS, ids=[n for n, _ in LAYOUTS])
@pytest.mark.parametrize("analysis", ANALYSES)
def test_forecast_from_an_analysed_state_against_the_oracle(analysis, layout, kernel, prec, oracle):
    """forecast 96 steps, the analysis on the device, forecast on: the oracle gets the analysed slots as an edit before step
    96 -- and the converted rows the joint analysis rewrote, the derived psnTMax among them"""
    n_sites, M, T, T1 = 2, se.M, site_clim(0).n_steps, 96
    flags = sa.flags_from()
    members = synth.perturbed_params(pr.base("default"), n_sites * M, seed=9)
    b = sa.Batch(flags, n_sites, M, prec, fast_math=True if prec == F64 else None, kernel=kernel)
    for s in range(n_sites):
        b.set_climate(s, site_clim(s))
        b.set_params(s, members[s * M:(s + 1) * M])
    b.setup()
    planes = torch.zeros((3, T, n_sites * M), dtype=b.out_dtype, device=b.device)
    b.run(0, T1, planes=planes[:, :T1])
    st0, prm0 = b.get_state(), b.get_params()
    window = planes[:, :T1].contiguous()
    ops = operators()
    obs, sd = observe(st0, [p.cpu().numpy() for p in window], prm0, n_sites, ops, np.random.default_rng(4))
    if analysis == "sites":
        b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=window)
    elif analysis == "smooth":
        b.enkf_analysis_smooth(obs, sd, ops, ANALYSED, [window.clone()], planes=window)
    elif analysis == "joint":
        b.enkf_analysis_joint(obs, sd, ops, ANALYSED, [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in JOINT_PARAMS], planes=window)
    else:
        loc = b.enkf_localization(*sa.gaspari_cohn(*grid(n_sites), 60.0), len(ops))
        (b.enkf_analysis_local if analysis == "local" else b.enkf_analysis_block)(loc, obs, sd, ops, ANALYSED, planes=window)
    st1, prm1 = b.get_state(), b.get_params(file_units=False)
    assert (st1[:, :13] != st0[:, :13]).any() and st1[:, 13:].tobytes() == st0[:, 13:].tobytes()
    assert (prm1 != prm0).any() == (analysis == "joint")
    b.run(T1, T - T1, planes=planes[:, T1:])
    name, got, state, status = b.last_launch()["kernel"], planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert layout == "auto" or family_ok(layout, "default", name), name
    edit_prm = np.where(prm1 == prm0, np.nan, prm1) if analysis == "joint" else None
    for s in range(n_sites):
        sl = slice(s * M, (s + 1) * M)
        want, final, st, _ = oracle.run_block_edits(flags, members[sl], site_clim(s), (T1,), se.table(st0[sl], st1[sl])[None],
                                                    None if edit_prm is None else edit_prm[sl][None])
        judge(f"{analysis} {name} site {s}", prec, got[:, :, sl], state[sl], status[sl], want, final, st)


PF = [(fs, f, p) for fs, fams in (("default", RUNS["default"]), ("ncycle", ["coop_ncycle", "coop_ncycle_pair"])) for f in fams
      for p in (F64, F32) if not (f == "strict" and p == F32)]


@pytest.mark.parametrize("entry", ["pf_analysis", "pf_resample_sites"])
@pytest.mark.parametrize("flagset,family,prec", PF, ids=[ident(c) for c in PF])
def test_resampled_particles_continue_like_the_oracles_run_of_their_ancestors(flagset, family, prec, entry, oracle):
    """with_params=True: after the resampling column j IS member ancestors[j] -- pools, ring and parameters -- so its
    forecast is the oracle's plain, continuous run of that member.  Every kernel family; the cooperative launches (lean)
    on the bounded-wait build"""
    members, clim = forest(flagset)
    T1 = 96 * 5 + 7
    b = batch(se.flags(flagset), [clim], members, prec, KERNELS[family], options(family), strict=family == "strict")
    planes = torch.zeros((3, se.T, se.M), dtype=b.out_dtype, device=b.device)
    b.run(0, T1, planes=planes[:, :T1])
    nee = planes[0, :T1].contiguous()
    total = nee.double().sum(0)
    obs, sigma = float(total.median()), 2.0 * float(total.std()) + 1e-12          # mild weights: many ancestors survive
    if entry == "pf_analysis":
        anc, _ = dist.pf_analysis(b, nee, obs, sigma, u0=0.43, with_params=True)
    else:
        anc = b.pf_resample_sites(b.pf_log_weights(nee, obs, sigma), [0.43], with_params=True)
    anc = anc.cpu().numpy().astype(int)
    assert 0.4 * se.M < len(np.unique(anc)) < se.M
    b.run(T1, se.T - T1, planes=planes[:, T1:])
    name, got, state, status = b.last_launch()["kernel"], planes.double().cpu().numpy(), b.get_state(), b.get_status()
    b.close()
    assert family_ok(family, flagset, name), name
    want, final, st = oracle.run_block(se.flags(flagset), members, clim)
    want = np.concatenate([want[:, :T1], want[:, T1:, anc]], axis=1)
    judge(f"{entry} {name}: {len(np.unique(anc))} ancestors", prec, got, state, status, want, final[anc], st[anc])
