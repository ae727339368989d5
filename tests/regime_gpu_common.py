"""What tests/test_gpu_forcing_regimes.py, tests/test_gpu_parameter_regimes.py and tests/test_gpu_state_edits.py share: the flag sets and forced kernels,
a batch set up in one call, the fuzzer's criteria (tools/fuzz_gpu.py) with the achieved figures printed first, the check
that the forced kernel ran, and the bit-for-bit comparison of two batches' outputs."""
import numpy as np
import torch

import sipnet_amd as sa

NCYCLE_FLAGS = dict(litterPool=1, anaerobic=1, nitrogenCycle=1)
RUSSELL_3 = dict(growthResp=1, leafWater=1, litterPool=1, waterHResp=0)
FLAG_SETS = {"default": {}, "ncycle": NCYCLE_FLAGS, "russell_3": RUSSELL_3}
COOP = {"coop_lds": sa.KERNEL_COOP_LDS, "coop_hbm": sa.KERNEL_COOP_HBM, "coop_pair": sa.KERNEL_COOP_PAIR, "coop_quad": sa.KERNEL_COOP_QUAD}
KERNELS = {"strict": sa.KERNEL_AUTO, "one_wave": sa.KERNEL_ONE_WAVE, "coop_ncycle": sa.KERNEL_COOP_NCYCLE,
           "coop_ncycle_pair": sa.KERNEL_COOP_NCYCLE_PAIR, **COOP}


def family_ok(family, flagset, name):
    """did the forced kernel run?  (last_launch()'s name: 'stepCoopKernel<double, true, true, false>' ...)"""
    head, args = name.split("<", 1)
    args = [a.strip(" >") for a in args.split(",")]
    x = {"default": "", "russell_3": "X", "ncycle": "N"}[flagset]
    if family == "strict":
        return head == "stepKernel"
    if family == "one_wave":
        return head == "stepFastKernel" and (flagset != "default" or args[2] == "0")      # (0: the flags compiled in)
    if family in ("coop_lds", "coop_hbm"):
        return head == "stepCoop" + x + "Kernel" and args[2] == ("true" if family == "coop_lds" else "false")
    return head == {"coop_pair": "stepCoop" + x + "PairKernel", "coop_quad": "stepCoop" + x + "QuadKernel",
                    "coop_ncycle": "stepCoopNKernel", "coop_ncycle_pair": "stepCoopNPairKernel"}[family]


def batch(flags, clims, members, prec, kernel, options=0, strict=False, diagnostics=False, events=None):
    """events: None, or every site's list of sa.Event"""
    b = sa.Batch(flags, len(clims), members.shape[0], prec, fast_math=(not strict) if prec == sa.F64 else None,
                 kernel=kernel, kernel_options=options)
    for s, c in enumerate(clims):
        if events is not None:
            b.set_events(s, events[s])
        b.set_climate(s, c)
    b.set_params(None, members)
    if diagnostics:
        b.enable_diagnostics()
    b.setup()
    return b


def judge(tag, prec, got, state, status, want, final, st, unjudged=None):
    """the fuzzer's criteria (tools/fuzz_gpu.py), with the achieved figures printed first.  unjudged: members whose
    VALUES are left out (the oracle's own are undefined); their status is judged like everyone's"""
    ok = st == 0
    assert np.array_equal(np.asarray(status) != 0, ~ok) and (np.asarray(status)[ok] == 0).all(), (tag, status, st)
    if unjudged is not None:
        ok = ok & ~np.asarray(unjudged, dtype=bool)
    got, want = got[:, :, ok], want[:, :, ok]
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-3)
    rel = np.abs(got - want) / scale
    pfloor = 1.0 if prec == sa.F32_MIXED else 1e-2
    perr = (np.abs(state[ok, :13] - final[ok, 14:27]) / np.maximum(np.abs(final[ok, 14:27]), pfloor)).max()
    if prec == sa.F64:
        print(f"{tag}: planes {np.nanmax(rel):.2e} of the plane maximum, pools {perr:.2e}")
        assert np.isfinite(got).all(), tag
        assert rel.max() < 1e-9 and perr < 1e-8, tag
    else:
        share = float((rel > 1e-4).mean())
        sums = (np.abs(got.sum(1) - want.sum(1)) / (np.abs(want).sum(1) + 1.0)).max()
        print(f"{tag}: fp32 max {np.nanmax(rel):.2e}, share off by > 1e-4 of the plane maximum {share:.2e}, time sums {sums:.2e}, "
              f"pools {perr:.2e}")
        assert np.isfinite(got).all() and np.isfinite(state[ok, :13]).all(), tag
        assert share < 2e-3 and sums < 2e-3 and perr < 5e-3, tag


def host_sums(planes, k):
    """planes [3][T][ncol] -> [3][ceil(T / k)][ncol], added in step order like the kernel"""
    T = planes.shape[1]
    out = np.zeros((3, (T + k - 1) // k, planes.shape[2]))
    for t in range(T):
        out[:, t // k] += planes[:, t]
    return out


def bits(x):
    return x.contiguous().view(torch.uint8)


def outputs(b, cuts=None, zeroed=False):
    """zeroed: planes filled with zeros first (a member that never runs leaves its columns as they are)"""
    T = b.n_steps
    planes, _ = b.alloc_outputs(T)
    if zeroed:
        planes.zero_()
    cuts = [0, T] if cuts is None else cuts
    for a, z in zip(cuts[:-1], cuts[1:]):
        b.run(a, z - a, planes=planes[:, a:z])
    out = (planes, b.get_state(), b.get_rings(), b.last_launch(), b.get_status())
    b.close()
    return out


def same(x, y, what, ran_only=False):
    """ran_only: only the members whose status is 0 -- what a throughput kernel leaves in the planes and rings of a
    member that never runs means nothing and depends on the layout and on where the launches were cut
    (tests/test_gpu_sums.py); that it never runs is compared"""
    if ran_only:
        assert np.array_equal(x[4], y[4]), what + ": status"
        ran = torch.as_tensor(x[4] == 0, device=x[0].device)
        assert torch.equal(bits(x[0][:, :, ran]), bits(y[0][:, :, ran])), what + ": planes"
        assert np.array_equal(x[1][x[4] == 0], y[1][x[4] == 0], equal_nan=True), what + ": state"
        assert np.array_equal(x[2][x[4] == 0], y[2][x[4] == 0], equal_nan=True), what + ": rings"
        return
    assert torch.equal(bits(x[0]), bits(y[0])), what + ": planes"
    assert np.array_equal(x[1], y[1], equal_nan=True), what + ": state"
    assert np.array_equal(x[2], y[2], equal_nan=True), what + ": rings"
