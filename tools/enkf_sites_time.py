#!/usr/bin/env python3
"""dev (GPU box): the many-site ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_sites) against the many-site
particle filter (sipnet_batch_pf_analysis_sites, with its gather) on the same batch.  48-step planes; 4 operators (LAI,
above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation).  Per shape and precision: the path the library picks, one workgroup per site forced (the batch is told the
device has one CU; sites of at most 4096 members only), the per-chunk launches forced (SIPNET_KOPT_PF_MULTI_LAUNCH), and the
particle filter.  HIP events around `calls` calls after a warm-up, median over `reps` repetitions, ms per call.
usage: enkf_sites_time.py [--calls K] [--reps R] [--out FILE] [--shapes 32x1024,256x1024,...]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="32x1024,256x1024,16x8192,2x65536,64x4096")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("enkf_sites_time.py needs a HIP device")
    base, _ = sa.read_params(os.path.join(REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
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
                b, planes = make(base, n_sites, M, prec)
                if key == "group":
                    b.debug_set_num_cus(1)
                elif key == "split":
                    b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                st = b.get_state()
                lai = st[:, 1] / 80.0
                obs = np.stack([lai, st[:, 0] + st[:, 12], st[:, 3] / 10.0,
                                planes[0].double().sum(0).cpu().numpy()], 1).reshape(n_sites, M, 4).mean(1)
                sd = np.abs(obs) * 0.1 + 1e-3
                obs_d = torch.tensor(obs, dtype=torch.float64, device="cuda")
                sd_d = torch.tensor(sd, dtype=torch.float64, device="cuda")
                infl = torch.full((n_sites,), 1.02, dtype=torch.float64, device="cuda")
                info = torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda")
                res[key] = median_ms(lambda: b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl,
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
                    res["pf"] = median_ms(lambda: b.pf_analysis_sites(nee, po, sig, u0, True, total), args.calls, args.reps)
                b.close()
            line = "%-10s %-9s %9d %11.4f %6s %11.4f %11.4f %11.4f %8.2f" % (
                "%dx%d" % (n_sites, M), pname, n, res["default"], path, res["group"], res["split"], res["pf"],
                res["default"] / res["pf"])
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
