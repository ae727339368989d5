#!/usr/bin/env python3
"""dev (GPU box): the block-local ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_block) against the serial
localized one (sipnet_batch_enkf_analysis_local) and the per-site one (sipnet_batch_enkf_analysis_sites), all three on the same
batch in the same process.  The shapes, operators and radii of tools/enkf_local_time.py: sites on a 2-D grid (0.25 degree
spacing, 32 or 16 wide), Gaspari-Cohn tapers at two half-widths (about 8 and about 24 neighbours per site); 48-step planes;
4 operators (LAI, above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation).  Per shape, precision and radius: the largest row count of a site, where the block kernel kept its matrices,
ms per call of the three, and the ratios.  HIP events around `calls` calls after a warm-up, median over `reps` repetitions.
usage: enkf_block_time.py [--calls K] [--reps R] [--out FILE] [--shapes 512x256,256x1024] [--radii 20,37] [--no-serial]"""
import numpy as np
import torch

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa


def main():
    ap = tc.arguments(20, 5, "512x256,256x1024")
    ap.add_argument("--radii", default="20,37")
    ap.add_argument("--no-serial", action="store_true", help="skip enkf_analysis_local (a kernel trace of the block call)")
    args = ap.parse_args()
    base, shapes = tc.start("enkf_block_time.py", args.shapes)
    radii = [float(r) for r in args.radii.split(",")]
    lines = ["# sipnet_batch_enkf_analysis_block vs sipnet_batch_enkf_analysis_local (the serial localized filter) and",
             "# sipnet_batch_enkf_analysis_sites on the same batch in the same process (4 operators: LAI, wood, soil wetness, NEE",
             "# sum; 7 analysed pools); 48-step planes, no host synchronisation; sites on a 0.25 degree grid, Gaspari-Cohn",
             "# half-width radius_km; ms per call, median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# max_rows = the largest n_obs x (1 + in-neighbours); matrices = where the block kernel keeps a target's",
             "# covariance and transform; serial/block = local_ms / block_ms; block/sites = block_ms / sites_ms",
             "%-10s %-9s %9s %9s %8s %8s %9s %10s %10s %10s %12s %11s" % (
                 "shape", "precision", "radius_km", "mean_nbrs", "max_rows", "matrices", "n_levels", "block_ms", "local_ms",
                 "sites_ms", "serial/block", "block/sites")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            b, planes = tc.make(base, n_sites, M, prec)
            st = b.get_state()
            # a third of the sites unobserved: reached only
            obs_d, sd_d, infl, info = tc.observations(b, planes, n_sites, M, unobserved=slice(1, None, 3))
            rows = torch.zeros((n_sites, 2), dtype=torch.int32, device="cuda")
            sites_ms = tc.median_ms(lambda: b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                  info_out=info), args.calls, args.reps)
            for radius in [None] + radii:
                ptr, nbr, rho = tc.lists(n_sites, radius)
                loc = b.enkf_localization(ptr, nbr, rho, len(OPS))
                b.set_state(st)
                block_ms = tc.median_ms(lambda: b.enkf_analysis_block(loc, obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                      info_out=info, rows_out=rows), args.calls, args.reps)
                where = "LDS" if b.pf_info()["fused"] else "global"
                assert int(info[:, 0].min().item()) >= -1, info
                assert int(rows[:, 1].max().item()) == 0 and int(rows[:, 0].max().item()) <= loc.max_rows, rows
                local_ms = float("nan")
                if not args.no_serial:
                    b.set_state(st)
                    local_ms = tc.median_ms(lambda: b.enkf_analysis_local(loc, obs_d, sd_d, OPS, ANALYSED, planes=planes,
                                                                          inflation=infl, info_out=info), args.calls, args.reps)
                line = "%-10s %-9s %9s %9.1f %8d %8s %9d %10.4f %10.4f %10.4f %12.1f %11.2f" % (
                    "%dx%d" % (n_sites, M), pname, "empty" if radius is None else "%g" % radius, np.diff(ptr).mean(),
                    loc.max_rows, where, loc.n_levels, block_ms, local_ms, sites_ms, local_ms / block_ms, block_ms / sites_ms)
                tc.emit(lines, line)
                loc.close()
            b.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
