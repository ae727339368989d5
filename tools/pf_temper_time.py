#!/usr/bin/env python3
"""dev (GPU box): Batch.pf_temper_sites (sipnet_batch_pf_temper_sites) next to its two yardsticks in the same process and on
the same shape: one Batch.pf_resample_sites (totals and ESS on the device), and the loop a caller needed before this call
existed, 8 x 15 pf_resample_sites as ESS probes (beta a device tensor, nothing synchronised -- the host bisection that
would steer them is not even counted).
Lines: shape x (without or with carried log-weights, d_base).  Columns: the call on the path the library takes (g one
workgroup per site, s launches per chunk and stage); where that is g, the per-chunk launches forced; one resampling; the 120
probes; the ratios.  The log-likelihoods are -0.5 chi^2-like with a scale that puts every site's root inside (0, 1), the
target half the members, so every site runs all eight rounds (code 1).  ess_target, delta_max, base and the outputs are
device tensors, info_out is given: nothing is synchronised.  HIP events around `calls` calls, enough of them for a quarter
of a second, after 3 warm-up calls; the median of `reps` repetitions and their range, ms per call.
usage: pf_temper_time.py [--reps R] [--out FILE] [--shapes 256x1024,64x4096,1x131072]"""
import argparse

import torch

import enkf_time_common as tc
from enkf_time_common import sa
from quantiles_time import timed


def fmt(t):
    return "%8.4f (%.4f .. %.4f)" % t[:3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="256x1024,64x4096,1x131072")
    args = ap.parse_args()
    base, shapes = tc.start("pf_temper_time.py", args.shapes)
    lines = ["# Batch.pf_temper_sites next to one Batch.pf_resample_sites and to 8 x 15 of them as ESS probes;",
             "# ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls" % args.reps,
             "# path: g one workgroup per site, s launches per chunk and stage; split_forced: path g's shapes on path s, median ms"]
    print("\n".join(lines), flush=True)
    tc.emit(lines, "%-11s %-5s %-4s %28s %12s %28s %28s %9s %9s" % (
        "shape", "base", "path", "temper_ms", "split_forced", "resample_sites_ms", "120_probes_ms", "x_resamp", "x_probes"))
    for n_sites, M in shapes:
        b, _ = tc.make(base, n_sites, M, sa.F64)
        ncol = n_sites * M
        gen = torch.Generator(device="cuda").manual_seed(5)
        z = torch.randn((3, ncol), dtype=torch.float64, device="cuda", generator=gen)
        loglik = -0.5 * 30.0 * (z * z).sum(0)
        carried = -0.5 * torch.randn(ncol, dtype=torch.float64, device="cuda", generator=gen) ** 2
        u0 = torch.full((n_sites,), 0.37, dtype=torch.float64, device="cuda")
        beta = torch.full((n_sites,), 0.02, dtype=torch.float64, device="cuda")
        total = torch.zeros(n_sites, dtype=torch.int64, device="cuda")
        ess = torch.zeros(n_sites, dtype=torch.float64, device="cuda")
        info = torch.zeros((n_sites, 2), dtype=torch.int32, device="cuda")
        dmax = torch.ones(n_sites, dtype=torch.float64, device="cuda")
        out = torch.empty(ncol, dtype=torch.float64, device="cuda")

        def resample():
            b.pf_resample_sites(loglik, u0, beta=beta, total_out=total, ess_out=ess)

        def probes():
            for _ in range(sa.TEMPER_ROUNDS * (sa.TEMPER_SECTIONS - 1)):
                resample()
        t_res = timed(resample, args.reps)
        t_probe = timed(probes, args.reps)
        for with_base in (False, True):
            target = torch.full((n_sites,), (0.3 if with_base else 0.5) * M, dtype=torch.float64, device="cuda")

            def temper():
                b.pf_temper_sites(loglik, target, base=carried if with_base else None, delta_max=dmax, out=out, info_out=info)
            b.set_kernel(sa.KERNEL_AUTO, 0)
            t_tmp = timed(temper, args.reps)
            path = "g" if b.pf_info()["fused"] else "s"
            assert int(info[:, 0].min().item()) == 1 and int(info[:, 0].max().item()) == 1
            t_other = None
            if path == "g":
                b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                t_other = timed(temper, args.reps)
                assert b.pf_info()["fused"] == 0
                b.set_kernel(sa.KERNEL_AUTO, 0)
            tc.emit(lines, "%-11s %-5s %-4s %28s %12s %28s %28s %9.2f %9.3f" % (
                "%dx%d" % (n_sites, M), "yes" if with_base else "-", path, fmt(t_tmp), "%10.4f" % t_other[0] if t_other else "-",
                fmt(t_res), fmt(t_probe), t_tmp[0] / t_res[0], t_tmp[0] / t_probe[0]))
        b.close()
        torch.cuda.empty_cache()
    tc.emit(lines, "# x_resamp = temper / resample_sites, x_probes = temper / the 120 probes (8 rounds x 15 candidates)")
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
