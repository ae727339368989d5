#!/usr/bin/env python3
"""dev (GPU box): the joint state-parameter analysis (sipnet_batch_enkf_analysis_joint) with 0, 4 and 16 analysed parameters
against the per-site analysis (sipnet_batch_enkf_analysis_sites) on the same batch in the same process, the two alternating:
sites, joint 0, sites again, joint 4, joint 16.  The shapes and settings of enkf_sites_time.py: 48-step planes; 4 operators
(LAI, above-ground wood, soil wetness, the NEE sum), 7 analysed pools, inflation 1.02, d_site_info given (no host
synchronisation); per shape and precision the path the library picks, one workgroup per site forced (sites of at most 4096
members only) and the per-chunk launches forced.  HIP events around `calls` calls after a warm-up, median over `reps`
repetitions, ms per call.  noise = the spread between the per-site call's two medians; joint0 - sites must not exceed it (the
shared kernels were extended, not changed); per_param = (joint16 - joint0) / 16 is reported, not bounded.
usage: enkf_joint_time.py [--calls K] [--reps R] [--out FILE] [--shapes 32x1024,256x1024,...]"""
import torch

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa

NAMES = ["aMax", "halfSatPar", "vegRespQ10", "soilWHC", "psnTOpt", "psnTMin", "baseVegResp", "leafTurnoverRate", "dVpdSlope",
         "baseFolRespFrac", "fineRootQ10", "coarseRootQ10", "frozenSoilThreshold", "woodTurnoverRate", "wueConst",
         "fineRootTurnoverRate"]


def main():
    args = tc.arguments(50, 7, "32x1024,256x1024,16x8192,2x65536,64x4096,1024x256,2048x128,1x4194304").parse_args()
    base, shapes = tc.start("enkf_joint_time.py", args.shapes)
    params = [sa.enkf_param(n, *tc.synth.PERTURB[n][:2]) for n in NAMES]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = ["# sipnet_batch_enkf_analysis_joint with 0, 4 and 16 analysed parameters vs sipnet_batch_enkf_analysis_sites on the same",
             "# batch, alternating (sites_a, joint0, sites_b, joint4, joint16); 4 operators, 7 analysed pools, inflation 1.02, 48-step",
             "# planes, no host synchronisation; ms per call, median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# path: default = what the library picks (group = one workgroup per site, split = per-chunk launches), or forced;",
             "# noise = |sites_a - sites_b|; excess0 = joint0 - min(sites_a, sites_b) (must not exceed noise); per_param = (joint16 - joint0) / 16",
             "%-10s %-9s %-14s %9s %9s %9s %9s %9s %9s %9s %10s" % ("shape", "precision", "path", "sites_a", "joint0", "sites_b",
                                                                  "joint4", "joint16", "noise", "excess0", "per_param")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            b, planes = tc.make(base, n_sites, M, prec)
            obs_d, sd_d, infl, info = tc.observations(b, planes, n_sites, M)

            def sites():
                b.enkf_analysis_sites(obs_d, sd_d, OPS, ANALYSED, planes=planes, inflation=infl, info_out=info)

            def joint(k):
                return lambda: b.enkf_analysis_joint(obs_d, sd_d, OPS, ANALYSED, params[:k], planes=planes, inflation=infl,
                                                     info_out=info)

            for key in ("default", "group", "split"):
                if key == "group" and M > 4096:
                    continue
                b.debug_set_num_cus(1 if key == "group" else cus)
                b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH if key == "split" else 0)
                ms = []
                for fn in (sites, joint(0), sites, joint(4), joint(16)):
                    ms.append(tc.median_ms(fn, args.calls, args.reps))
                    assert int(info[:, 0].min().item()) == 1, info
                path = key if key != "default" else "default:" + ("group" if b.pf_info()["fused"] else "split")
                noise, excess = abs(ms[0] - ms[2]), ms[1] - min(ms[0], ms[2])
                tc.emit(lines, "%-10s %-9s %-14s %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %10.5f" % (
                    "%dx%d" % (n_sites, M), pname, path, ms[0], ms[1], ms[2], ms[3], ms[4], noise, excess, (ms[4] - ms[1]) / 16))
            b.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
