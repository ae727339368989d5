#!/usr/bin/env python3
"""dev (GPU box): the localized multi-site ensemble Kalman filter (sipnet_batch_enkf_analysis_local) against the per-site
one (sipnet_batch_enkf_analysis_sites) on the same batch.  Sites on a 2-D grid (0.25 degree spacing, 32 or 16 wide),
Gaspari-Cohn tapers at two half-widths (about 8 and about 24 neighbours per site); 48-step planes; 4 operators (LAI,
above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation).  Per shape, precision and radius: n_levels (one launch each), ms per call, us per level; then the empty
lists against enkf_analysis_sites.  HIP events around `calls` calls after a warm-up, median over `reps` repetitions.
usage: enkf_local_time.py [--calls K] [--reps R] [--out FILE] [--shapes 512x256,256x1024] [--radii 20,37]"""
import numpy as np

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa


def main():
    ap = tc.arguments(20, 5, "512x256,256x1024")
    ap.add_argument("--radii", default="20,37")
    args = ap.parse_args()
    base, shapes = tc.start("enkf_local_time.py", args.shapes)
    radii = [float(r) for r in args.radii.split(",")]
    lines = ["# sipnet_batch_enkf_analysis_local (4 operators: LAI, wood, soil wetness, NEE sum; 7 analysed pools) vs",
             "# sipnet_batch_enkf_analysis_sites on the same batch; 48-step planes, no host synchronisation; sites on a 0.25 degree",
             "# grid, Gaspari-Cohn half-width radius_km; ms per call, median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# radius 'empty' = no neighbours (bit-identical to enkf_analysis_sites); us_per_level = local_ms / n_levels;",
             "# ratio = local_ms / sites_ms",
             "%-10s %-9s %9s %9s %8s %10s %12s %10s %7s" % ("shape", "precision", "radius_km", "mean_nbrs", "n_levels",
                                                         "local_ms", "us_per_level", "sites_ms", "ratio")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            b, planes = tc.make(base, n_sites, M, prec)
            st = b.get_state()
            # a third of the sites unobserved: reached only
            obs_d, sd_d, infl, info = tc.observations(b, planes, n_sites, M, unobserved=slice(1, None, 3))
            sites_ms = tc.median_ms(lambda: b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                  info_out=info), args.calls, args.reps)
            for radius in [None] + radii:
                ptr, nbr, rho = tc.lists(n_sites, radius)
                loc = b.enkf_localization(ptr, nbr, rho, len(OPS))
                b.set_state(st)
                ms = tc.median_ms(lambda: b.enkf_analysis_local(loc, obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                info_out=info), args.calls, args.reps)
                assert int(info[:, 0].min().item()) >= -1, info
                line = "%-10s %-9s %9s %9.1f %8d %10.4f %12.2f %10.4f %7.2f" % (
                    "%dx%d" % (n_sites, M), pname, "empty" if radius is None else "%g" % radius, np.diff(ptr).mean(),
                    loc.n_levels, ms, 1000.0 * ms / loc.n_levels, sites_ms, ms / sites_ms)
                tc.emit(lines, line)
                loc.close()
            b.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
