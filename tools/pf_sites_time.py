#!/usr/bin/env python3
"""dev (GPU box): the many-site particle-filter analysis (sipnet_batch_pf_analysis_sites: per-site weights, draws and
ancestors + the resampling gather) against the one-site call (sipnet_batch_pf_analysis) over ONE site holding the same
number of particles.  48-step planes; per shape and precision: the path the library picks (one workgroup per site when
sites have at most 4096 particles and are at least as many as the CUs, else three launches), one workgroup per site forced
(the batch is told the device has one CU; sites of at most 4096 particles only), the three-launch path forced
(SIPNET_KOPT_PF_MULTI_LAUNCH), and the reference.  HIP events around `calls` calls after a warm-up, median over `reps`
repetitions, ms per call.
usage: pf_sites_time.py [--calls K] [--reps R] [--out FILE] [--shapes 32x1024,256x1024,...]"""
import torch

import enkf_time_common as tc
from enkf_time_common import sa


def main():
    args = tc.arguments(50, 7, "32x1024,256x1024,16x8192,2x65536,64x4096").parse_args()
    base, shapes = tc.start("pf_sites_time.py", args.shapes)
    lines = ["# sipnet_batch_pf_analysis_sites vs sipnet_batch_pf_analysis over one site of the same particles; 48-step planes,",
             "# with_params (the parameter index is gathered), d_site_total / d_total given (no host synchronisation);",
             "# ms per call (weights + ancestors + gather), median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# default = what sipnet_batch_pf_analysis_sites picks (path: group = one workgroup per site, split = three launches);",
             "# ratio = default / onesite",
             "%-10s %-9s %9s %11s %6s %11s %11s %11s %8s" % ("shape", "precision", "particles", "default_ms", "path", "group_ms",
                                                          "split_ms", "onesite_ms", "ratio")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            n = n_sites * M
            res = {}
            for key in ("default", "group", "split"):
                if key == "group" and M > 4096:
                    res[key] = float("nan")
                    continue
                b, planes = tc.make(base, n_sites, M, prec)
                nee = planes[0]
                if key == "group":
                    b.debug_set_num_cus(1)
                elif key == "split":
                    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                tot = nee.double().sum(0).reshape(n_sites, M)
                obs = tot.median(dim=1).values.contiguous()
                sig = (tot.std(dim=1) * 1.5 + 1e-12).contiguous()
                u0 = torch.rand(n_sites, dtype=torch.float64, device=nee.device)
                total = torch.zeros(n_sites, dtype=torch.int64, device=nee.device)
                res[key] = tc.median_ms(lambda: b.pf_analysis_sites(nee, obs, sig, u0, True, total), args.calls, args.reps)
                assert int(total.min().item()) > 0
                if key == "default":
                    path = "group" if b.pf_info()["fused"] else "split"
                b.close()
            b, planes = tc.make(base, 1, n, prec)
            nee = planes[0]
            tot = nee.double().sum(0)
            obs1, sig1 = float(tot.median()), float(tot.std()) * 1.5 + 1e-12
            total = torch.zeros(1, dtype=torch.int64, device=nee.device)
            res["one"] = tc.median_ms(lambda: b.pf_analysis_local(nee, obs1, sig1, 0.5, True, total), args.calls, args.reps)
            b.close()
            line = "%-10s %-9s %9d %11.4f %6s %11.4f %11.4f %11.4f %8.2f" % (
                "%dx%d" % (n_sites, M), pname, n, res["default"], path, res["group"], res["split"], res["one"],
                res["default"] / res["one"])
            tc.emit(lines, line)
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
