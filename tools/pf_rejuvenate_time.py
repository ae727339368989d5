#!/usr/bin/env python3
"""dev (GPU box): Batch.pf_rejuvenate (sipnet_batch_pf_rejuvenate) next to its two yardsticks in the same process and on the
same shape: Batch.pf_resample_sites (with_params, totals on the device), the step of the cycle it follows, and a torch device
copy of the rows it touches (the listed parameter rows and the masked state rows, read once and written once).
Lines: shape x precision x (4 or 16 listed parameters) x (without or with the pools of 0x10FF: eight and
plantCAccountingDelta); 1024 x 256 is the shape of the one-workgroup-per-site path.  Columns: the call on a
batch whose parameters are NOT behind an index (every column has its own rows already); the cycle resample -> rejuvenate,
where every call follows an indexed resampling and so first gives every duplicate its own rows (materializeParams: a gather
of all 80 rows); that gather's share = cycle - resample - rejuvenate; the copy; the ratios.  shrink, pool_sd and the totals
are device tensors, info_out is given: nothing is synchronised.  HIP events around `calls` calls, enough of them for a quarter
of a second, after 3 warm-up calls; the median of `reps` repetitions and their range, ms per call.
usage: pf_rejuvenate_time.py [--reps R] [--out FILE] [--shapes 256x1024,64x4096,1x131072,1024x256]"""
import argparse

import numpy as np
import torch

import enkf_time_common as tc
from enkf_time_common import sa, synth
from quantiles_time import timed

NAMES = ["aMax", "psnTMin", "psnTOpt", "dVpdSlope", "halfSatPar", "baseVegResp", "baseFolRespFrac", "baseFineRootResp",
         "baseCoarseRootResp", "vegRespQ10", "fineRootQ10", "coarseRootQ10", "frozenSoilThreshold", "woodTurnoverRate",
         "leafTurnoverRate", "wueConst"]
POOLS8 = 0x10FF


def fmt(t):
    return "%8.4f (%.4f .. %.4f)" % t[:3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="256x1024,64x4096,1x131072,1024x256")
    args = ap.parse_args()
    base, shapes = tc.start("pf_rejuvenate_time.py", args.shapes)
    lines = ["# Batch.pf_rejuvenate next to Batch.pf_resample_sites (with_params) and a torch copy of the touched rows;",
             "# ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls" % args.reps,
             "# path: g one workgroup per site (sites of at most 256 members), s per-chunk launches; split_forced: path g's shapes on path s, median ms"]
    print("\n".join(lines), flush=True)
    tc.emit(lines, "%-11s %-4s %-4s %-5s %-4s %28s %12s %28s %28s %11s %28s %9s %7s" % (
        "shape", "prec", "prm", "pools", "path", "rejuvenate_ms", "split_forced", "resample_sites_ms", "resample+rejuvenate_ms", "gather_ms",
        "copy_rows_ms", "x_resamp", "x_copy"))
    pools = [sa.POOLS[p] for p in range(13) if POOLS8 >> p & 1]
    for n_sites, M in shapes:
        for prec, label in ((sa.F32_MIXED, "f32"), (sa.F64, "f64")):
            if (n_sites, M) != shapes[0] and prec == sa.F32_MIXED:
                continue                  # (both precisions at the first shape; the pass reads no ring, so they differ little)
            b, _ = tc.make(base, n_sites, M, prec)
            ncol = n_sites * M
            gen = torch.Generator(device="cuda").manual_seed(3)
            logw = torch.randn(ncol, dtype=torch.float64, device="cuda", generator=gen)
            u0 = torch.full((n_sites,), 0.37, dtype=torch.float64, device="cuda")
            total = torch.zeros(n_sites, dtype=torch.int64, device="cuda")
            info = torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda")
            shrink = torch.full((n_sites,), sa.liu_west_shrink(0.98), dtype=torch.float64, device="cuda")
            st = b.get_state()
            sd = np.abs(st[:, :13]).reshape(n_sites, M, 13).mean(1) * 0.01
            sd = torch.tensor(np.where(sd > 0, sd, 0.01), dtype=torch.float64, device="cuda")

            def resample():
                b.pf_resample_sites(logw, u0, with_params=True, total_out=total)
            t_res = timed(resample, args.reps)
            draw = [0]
            for n_prm in (4, 16):
                params = [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in NAMES[:n_prm]]
                for with_pools in (False, True):
                    def rejuvenate():
                        draw[0] += 1
                        b.pf_rejuvenate(params, shrink, pools if with_pools else None, sd if with_pools else None, seed=1,
                                        draw=draw[0], site_total=total, info_out=info)

                    def cycle():
                        resample()
                        rejuvenate()
                    rejuvenate()          # (not indexed from here on)
                    t_rej = timed(rejuvenate, args.reps)
                    path = "g" if b.pf_info()["fused"] else "s"
                    assert int(info[:, 0].min().item()) == 1
                    # where the library takes one workgroup per site (sites of one chunk): the per-chunk launches forced
                    t_other = None
                    if path == "g":
                        b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                        t_other = timed(rejuvenate, args.reps)
                        assert b.pf_info()["fused"] == 0
                        b.set_kernel(sa.KERNEL_AUTO, 0)
                    t_cyc = timed(cycle, args.reps)
                    n_rows = n_prm + (9 if with_pools else 0)
                    src = torch.randn((n_rows, ncol), dtype=torch.float64, device="cuda", generator=gen)
                    dst = torch.empty_like(src)
                    t_cp = timed(lambda: dst.copy_(src), args.reps)
                    tc.emit(lines, "%-11s %-4s %-4d %-5s %-4s %28s %12s %28s %28s %11.4f %28s %9.2f %7.2f" % (
                        "%dx%d" % (n_sites, M), label, n_prm, "8+1" if with_pools else "-", path, fmt(t_rej),
                        "%10.4f" % t_other[0] if t_other else "-", fmt(t_res), fmt(t_cyc),
                        t_cyc[0] - t_res[0] - t_rej[0], fmt(t_cp), t_rej[0] / t_res[0], t_rej[0] / t_cp[0]))
                    del src, dst
            b.close()
            torch.cuda.empty_cache()
    tc.emit(lines, "# gather_ms = resample+rejuvenate - resample_sites - rejuvenate: what giving every duplicate its own rows costs (80 rows gathered)")
    tc.emit(lines, "# x_resamp = rejuvenate / resample_sites, x_copy = rejuvenate / copy_rows (the rows it touches: prm + 9 state rows with pools)")
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
