#!/usr/bin/env python3
"""dev (GPU box): the many-site ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_sites) against the many-site
particle filter (sipnet_batch_pf_analysis_sites, with its gather) on the same batch.  48-step planes; 4 operators (LAI,
above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation).  Per shape and precision: the path the library picks, one workgroup per site forced (the batch is told the
device has one CU; sites of at most 4096 members only), the per-chunk launches forced (SIPNET_KOPT_PF_MULTI_LAUNCH), and the
particle filter.  HIP events around `calls` calls after a warm-up, median over `reps` repetitions, ms per call.
usage: enkf_sites_time.py [--calls K] [--reps R] [--out FILE] [--shapes 32x1024,256x1024,...]"""
import torch

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa


def main():
    args = tc.arguments(50, 7, "32x1024,256x1024,16x8192,2x65536,64x4096").parse_args()
    base, shapes = tc.start("enkf_sites_time.py", args.shapes)
    lines = ["# sipnet_batch_enkf_analysis_sites (4 operators: LAI, wood, soil wetness, NEE sum; 7 analysed pools) vs",
             "# sipnet_batch_pf_analysis_sites (with_params, with the gather) on the same batch; 48-step planes, no host synchronisation;",
             "# ms per call, median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# default = what sipnet_batch_enkf_analysis_sites picks (path: group = one workgroup per site, split = per-chunk launches);",
             "# ratio = default / pf_sites",
             "%-10s %-9s %9s %11s %6s %11s %11s %11s %8s" % ("shape", "precision", "members", "default_ms", "path", "group_ms",
                                                          "split_ms", "pf_sites_ms", "ratio")]
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
                if key == "group":
                    b.debug_set_num_cus(1)
                elif key == "split":
                    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                obs_d, sd_d, infl, info = tc.observations(b, planes, n_sites, M)
                res[key] = tc.median_ms(lambda: b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                      info_out=info), args.calls, args.reps)
                assert int(info[:, 0].min().item()) == 1, info
                if key == "default":
                    path = "group" if b.pf_info()["fused"] else "split"
                    nee = planes[0]
                    tot = nee.double().sum(0).reshape(n_sites, M)
                    po = tot.median(dim=1).values.contiguous()
                    sig = (tot.std(dim=1) * 1.5 + 1e-12).contiguous()
                    u0 = torch.rand(n_sites, dtype=torch.float64, device=nee.device)
                    total = torch.zeros(n_sites, dtype=torch.int64, device=nee.device)
                    res["pf"] = tc.median_ms(lambda: b.pf_analysis_sites(nee, po, sig, u0, True, total), args.calls, args.reps)
                b.close()
            line = "%-10s %-9s %9d %11.4f %6s %11.4f %11.4f %11.4f %8.2f" % (
                "%dx%d" % (n_sites, M), pname, n, res["default"], path, res["group"], res["split"], res["pf"],
                res["default"] / res["pf"])
            tc.emit(lines, line)
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
