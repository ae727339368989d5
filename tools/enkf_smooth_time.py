#!/usr/bin/env python3
"""dev (GPU box): the ensemble Kalman smoother's series stage (sipnet_batch_enkf_analysis_smooth) against the joint call with
n_params = 0 (sipnet_batch_enkf_analysis_joint) on the same batch in the same process, alternating: joint, smooth with the
three 48-row planes, smooth with three 365-row double series (a year of daily sums), joint again; then a device-to-device copy
(dst.copy_(src)) of the same series, the traffic floor the stage is to be read against.  The series are smoothed out of place,
so every call sees the same values and moves the copy's bytes.  The shapes of enkf_sites_time.py with at most 4 096 members
per site, its settings (4 operators, 7 analysed pools, inflation 1.02, d_site_info given: no host synchronisation); per shape
and precision the anomalies staged in LDS (the default) and read from the scratch block (SIPNET_KOPT_PF_MULTI_LAUNCH, which
also puts the pool analysis on its per-chunk launches: the joint call is timed under the same option).  HIP events around
`calls` calls after a warm-up, median over `reps` repetitions, ms per call.  noise = the spread of the joint call's two
medians; added = smooth - min(joint); GB/s = the series' bytes read + written over added; x_copy = added / copy.
usage: enkf_smooth_time.py [--calls K] [--reps R] [--out FILE] [--shapes 32x1024,256x1024,...]"""
import torch

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa

DAYS = 365


def main():
    args = tc.arguments(20, 5, "32x1024,256x1024,64x4096,1024x256,2048x128").parse_args()
    base, shapes = tc.start("enkf_smooth_time.py", args.shapes)
    lines = ["# sipnet_batch_enkf_analysis_smooth vs sipnet_batch_enkf_analysis_joint (n_params = 0) on the same batch, alternating",
             "# (joint_a, smooth48 = the three 48-row planes, smooth365 = three 365-row double series, joint_b), out of place;",
             "# 4 operators, 7 analysed pools, inflation 1.02, no host synchronisation; ms per call, median of %d x %d calls after"
             % (args.reps, args.calls),
             "# 5 warm-up calls; form: lds = the anomalies staged in LDS, scratch = read from the scratch block (per-chunk pool path);",
             "# noise = |joint_a - joint_b|; add = smooth - min(joint); GB/s = series bytes (read + write) / add; copy = dst.copy_(src) of",
             "# the same series; x = add / copy",
             "%-10s %-9s %-8s %8s %8s %8s %8s %8s %8s %8s %7s %8s %8s %8s %7s" % (
                 "shape", "precision", "form", "joint_a", "smooth48", "smth365", "joint_b", "noise", "add48", "copy48", "x48",
                 "add365", "copy365", "GB/s365", "x365")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            if M > 4096:
                continue
            b, planes = tc.make(base, n_sites, M, prec)
            obs_d, sd_d, infl, info = tc.observations(b, planes, n_sites, M)
            out48 = torch.empty_like(planes)
            gen = torch.Generator(device="cuda").manual_seed(1)
            year = torch.randn((3, DAYS, b.ncol), dtype=torch.float64, device="cuda", generator=gen)
            out365 = torch.empty_like(year)
            bytes365 = 2 * year.numel() * year.element_size()

            def joint():
                b.enkf_analysis_joint(obs_d, sd_d, OPS, ANALYSED, [], planes=planes, inflation=infl, info_out=info)

            def smooth(src, dst):
                return lambda: b.enkf_analysis_smooth(obs_d, sd_d, OPS, ANALYSED, [(src, dst)], planes=planes, inflation=infl,
                                                      info_out=info)

            for form in ("lds", "scratch"):
                b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH if form == "scratch" else 0)
                ms = []
                for fn in (joint, smooth(planes, out48), smooth(year, out365), joint):
                    ms.append(tc.median_ms(fn, args.calls, args.reps))
                    assert int(info[:, 0].min().item()) == 1, info
                c48 = tc.median_ms(lambda: out48.copy_(planes), args.calls, args.reps)
                c365 = tc.median_ms(lambda: out365.copy_(year), args.calls, args.reps)
                lo = min(ms[0], ms[3])
                a48, a365 = ms[1] - lo, ms[2] - lo
                tc.emit(lines, "%-10s %-9s %-8s %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %7.2f %8.4f %8.4f %8.0f %7.2f" % (
                    "%dx%d" % (n_sites, M), pname, form, ms[0], ms[1], ms[2], ms[3], abs(ms[0] - ms[3]), a48, c48, a48 / c48,
                    a365, c365, bytes365 / (a365 * 1e6), a365 / c365))
            b.close()
            del year, out365, out48
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
