#!/usr/bin/env python3
"""dev (GPU box): the EnKF analysis of an ensemble sharded by member (sipnet_batch_enkf_shard_moments +
sipnet_batch_enkf_analysis_sharded) against sipnet_batch_enkf_analysis_sites on the same batch.  48-step planes; 7 analysed
pools; 4 operators (LAI, above-ground wood, soil wetness, the NEE sum) or 16 (those, nine more sums of pools, the GPP, ET and
halved NEE sums); observations at the ensemble means, sd 10 %, inflation 1.02, d_site_info given (no host synchronisation).
Per shape, precision and operator count: with world = 1 the moments call, the analysis call and their sum, then the per-site
call; then the same union cut into 8 shards of 1/8 the members -- ONE shard's two calls, fed a buffer of 8 blocks, on the one
device (a rehearsal: on a node the 8 shards run side by side and an all-gather of the blocks stands between the two calls;
its bytes are listed, its time is not measured here).  HIP events around `calls` calls after a warm-up, median over `reps`
repetitions, ms per call.
usage: enkf_sharded_time.py [--calls K] [--reps R] [--out FILE] [--shapes 1x131072,256x1024]"""
import torch

import enkf_time_common as tc
from enkf_time_common import ANALYSED, OPS, sa

POOLS13 = list(sa.POOLS[:13])
OPS16 = OPS + [sa.enkf_pools([POOLS13[k], POOLS13[(5 * k + 1) % 13]], scale=(1.0, 0.5, 0.25)[k % 3]) for k in range(9)] + [
    sa.enkf_plane("gpp"), sa.enkf_plane("et"), sa.enkf_plane("nee", scale=0.5)]


def observed(b, planes, ops, n_sites, world=1):
    """the moments (their h means are the observations), sd, inflation, info and the buffer of `world` blocks (this batch's
    block in every slot)"""
    mom = b.enkf_shard_moments(ops, ANALYSED, planes=planes)
    nA = len(ANALYSED)
    obs = mom[:, 2 + nA:2 + nA + len(ops)].contiguous()
    sd = obs.abs() * 0.1 + 1e-3
    infl = torch.full((n_sites,), 1.02, dtype=torch.float64, device="cuda")
    info = torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda")
    gathered = mom.unsqueeze(0).repeat(world, 1, 1).contiguous()
    return obs, sd, infl, info, gathered


def pair(base, n_sites, M, prec, ops, world, calls, reps, sites_too):
    """-> (moments ms, analysis ms, per-site call ms or None) of one batch of n_sites x M fed `world` blocks"""
    b, planes = tc.make(base, n_sites, M, prec)
    obs, sd, infl, info, gathered = observed(b, planes, ops, n_sites, world)
    out = gathered[0]
    t_mom = tc.median_ms(lambda: b.enkf_shard_moments(ops, ANALYSED, planes=planes, out=out), calls, reps)
    t_app = tc.median_ms(lambda: b.enkf_analysis_sharded(gathered, obs, sd, ops, ANALYSED, planes=planes, inflation=infl,
                                                         info_out=info), calls, reps)
    assert int(info[:, 0].min().item()) == 1 and int(info[:, 2].min().item()) == world * M, info
    t_sites = None
    if sites_too:
        t_sites = tc.median_ms(lambda: b.enkf_analysis_sites(obs, sd, ops, ANALYSED, planes=planes, inflation=infl,
                                                             info_out=info), calls, reps)
        assert int(info[:, 0].min().item()) == 1, info
    b.close()
    return t_mom, t_app, t_sites


def main():
    args = tc.arguments(50, 7, "1x131072,256x1024").parse_args()
    base, shapes = tc.start("enkf_sharded_time.py", args.shapes)
    lines = ["# sipnet_batch_enkf_shard_moments + sipnet_batch_enkf_analysis_sharded vs sipnet_batch_enkf_analysis_sites on the same",
             "# batch; 7 analysed pools, 4 or 16 operators, inflation 1.02, 48-step planes, no host synchronisation;",
             "# ms per call, median of %d x %d calls after 5 warm-up calls" % (args.reps, args.calls),
             "# world 1: moments, analysis, their sum, the per-site call; ratio = sum / sites",
             "# world 8: ONE shard of 1/8 the members, its two calls fed 8 blocks, on the one device (a rehearsal); gather_B = the",
             "# bytes one rank receives in the all-gather (8 x n_sites x W x 8), block_B = what it sends",
             "%-10s %-9s %5s %10s %11s %9s %9s %7s %12s %11s %9s %9s %9s" % (
                 "shape", "precision", "n_obs", "moments_ms", "analysis_ms", "sum_ms", "sites_ms", "ratio", "s8_moments", "s8_analysis",
                 "s8_sum", "block_B", "gather_B")]
    print("\n".join(lines), flush=True)
    for prec, pname in ((sa.F32_MIXED, "f32mixed"), (sa.F64, "f64")):
        for n_sites, M in shapes:
            for ops in (OPS, OPS16):
                t_mom, t_app, t_sites = pair(base, n_sites, M, prec, ops, 1, args.calls, args.reps, True)
                s_mom, s_app, _ = pair(base, n_sites, M // 8, prec, ops, 8, args.calls, args.reps, False)
                W = 2 + (len(ANALYSED) + len(ops)) * (1 + len(ops))
                tc.emit(lines, "%-10s %-9s %5d %10.4f %11.4f %9.4f %9.4f %7.2f %12.4f %11.4f %9.4f %9d %9d" % (
                    "%dx%d" % (n_sites, M), pname, len(ops), t_mom, t_app, t_mom + t_app, t_sites, (t_mom + t_app) / t_sites,
                    s_mom, s_app, s_mom + s_app, n_sites * W * 8, 8 * n_sites * W * 8))
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
