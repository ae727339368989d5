#!/usr/bin/env python3
"""dev (GPU box): the block-local ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_block) against the serial
localized one (sipnet_batch_enkf_analysis_local) and the per-site one (sipnet_batch_enkf_analysis_sites), all three on the same
batch in the same process.  The shapes, operators and radii of tools/enkf_local_time.py: sites on a 2-D grid (0.25 degree
spacing, 32 or 16 wide), Gaspari-Cohn tapers at two half-widths (about 8 and about 24 neighbours per site); 48-step planes;
4 operators (LAI, above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation).  Per shape, precision and radius: the largest row count of a site, where the block kernel kept its matrices,
ms per call of the three, and the ratios.  HIP events around `calls` calls after a warm-up, median over `reps` repetitions.
usage: enkf_block_time.py [--calls K] [--reps R] [--out FILE] [--shapes 512x256,256x1024] [--radii 20,37] [--no-serial]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sipnet_amd as sa  # noqa: E402
from sipnet_amd import synth  # noqa: E402

T = 48
ANALYSED = ["plantWoodC", "plantLeafC", "soilC", "soilWater", "coarseRootC", "fineRootC", "plantCAccountingDelta"]
OPS = [sa.enkf_pools(["plantLeafC"], divide_by="leafCSpWt"), sa.enkf_pools(["plantWoodC", "plantCAccountingDelta"]),
       sa.enkf_pools(["soilWater"], divide_by="soilWHC"), sa.enkf_plane("nee")]


def make(base, n_sites, M, prec):
    b = sa.Batch(sa.flags_from(), n_sites, M, prec, fast_math=True)
    for s in range(n_sites):
        b.set_climate(s, synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T, site=s))))
        b.set_params(s, synth.perturbed_params(base, M, seed=s))
    b.setup()
    planes, _ = b.run(0, T)
    return b, planes


def median_ms(fn, calls, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return float(np.median(out))


def grid(n_sites):
    width = 32 if n_sites >= 512 else 16
    r, c = np.divmod(np.arange(n_sites), width)
    return 40.0 + 0.25 * r, -90.0 + 0.25 * c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="512x256,256x1024")
    ap.add_argument("--radii", default="20,37")
    ap.add_argument("--no-serial", action="store_true", help="skip enkf_analysis_local (a kernel trace of the block call)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("enkf_block_time.py needs a HIP device")
    base, _ = sa.read_params(os.path.join(REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
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
            b, planes = make(base, n_sites, M, prec)
            st = b.get_state()
            lai = st[:, 1] / 80.0
            obs = np.stack([lai, st[:, 0] + st[:, 12], st[:, 3] / 10.0,
                            planes[0].double().sum(0).cpu().numpy()], 1).reshape(n_sites, M, 4).mean(1)
            sd = np.abs(obs) * 0.1 + 1e-3
            obs[1::3] = np.nan                                   # a third of the sites unobserved: reached only
            obs_d = torch.tensor(obs, dtype=torch.float64, device="cuda")
            sd_d = torch.tensor(sd, dtype=torch.float64, device="cuda")
            infl = torch.full((n_sites,), 1.02, dtype=torch.float64, device="cuda")
            info = torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda")
            rows = torch.zeros((n_sites, 2), dtype=torch.int32, device="cuda")
            sites_ms = median_ms(lambda: b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                               info_out=info), args.calls, args.reps)
            lat, lon = grid(n_sites)
            for radius in [None] + radii:
                if radius is None:
                    ptr, nbr, rho = np.zeros(n_sites + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)
                else:
                    ptr, nbr, rho = sa.gaspari_cohn(lat, lon, radius)
                loc = b.enkf_localization(ptr, nbr, rho, len(OPS))
                b.set_state(st)
                block_ms = median_ms(lambda: b.enkf_analysis_block(loc, obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
                                                                   info_out=info, rows_out=rows), args.calls, args.reps)
                where = "LDS" if b.pf_info()["fused"] else "global"
                assert int(info[:, 0].min().item()) >= -1, info
                assert int(rows[:, 1].max().item()) == 0 and int(rows[:, 0].max().item()) <= loc.max_rows, rows
                local_ms = float("nan")
                if not args.no_serial:
                    b.set_state(st)
                    local_ms = median_ms(lambda: b.enkf_analysis_local(loc, obs_d, sd_d, OPS, ANALYSED, planes=planes,
                                                                       inflation=infl, info_out=info), args.calls, args.reps)
                line = "%-10s %-9s %9s %9.1f %8d %8s %9d %10.4f %10.4f %10.4f %12.1f %11.2f" % (
                    "%dx%d" % (n_sites, M), pname, "empty" if radius is None else "%g" % radius, np.diff(ptr).mean(),
                    loc.max_rows, where, loc.n_levels, block_ms, local_ms, sites_ms, local_ms / block_ms, block_ms / sites_ms)
                print(line, flush=True)
                lines.append(line)
                loc.close()
            b.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
