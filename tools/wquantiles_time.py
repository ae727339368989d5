#!/usr/bin/env python3
"""dev (GPU box): Batch.plane_quantiles_weighted (sipnet_batch_plane_quantiles_weighted) next to Batch.plane_quantiles and
Batch.reduce_plane (the streaming floor: the same bytes read once, no ordering) over the same arrays.
Shapes: the daily sums of 256 sites x 1 024 members x 365 days, fp64 (both calls sort); one fp64 plane of 1 site x 10 240
members x a year of half-hourly steps (above the weighted sort path's 8 192 members: the weighted call selects, the unweighted
one still sorts); 1 site x 65 536 members of floats x 512 rows (both select).  q = (0.025, 0.5, 0.975), live members only;
without scores, and with the moments, the ranks and -- on the sort path -- the CRPS.  The log-weights are seeded normal
numbers times 2 (nearly every member weighs something); the series are seeded normal numbers.  The three calls are timed in
turn inside every repetition (so that a drift of the machine meets all of them): HIP events around `calls` calls, enough of them
for a quarter of a second, after 3 warm-up calls each; the median of `reps` repetitions and their range, ms per call; GB/s = the
array's bytes / the weighted call's median.
usage: wquantiles_time.py [--reps R] [--out FILE] [--shapes sums,year,wide] [--rows-scale F]"""
import argparse
import math
import os

import numpy as np
import torch

import enkf_time_common as tc
from enkf_time_common import sa

Q = (0.025, 0.5, 0.975)
SHAPES = {   # name: (n_sites, members, rows, dtype)
    "sums": (256, 1024, 365, torch.float64),
    "year": (1, 10240, 17520, torch.float64),
    "wide": (1, 65536, 512, torch.float32),
}


def timed_in_turn(fns, reps):
    """-> per function (median, least, most) ms per call, the functions taking turns inside every repetition"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        calls.append(int(min(200, max(3, math.ceil(250.0 / max(e0.elapsed_time(e1), 1e-3))))))
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0.record()
            for _ in range(calls[k]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / calls[k])
    return [(float(np.median(o)), float(min(o)), float(max(o))) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="sums,year,wide")
    ap.add_argument("--rows-scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wquantiles_time.py needs a HIP device")
    base, _ = sa.read_params(os.path.join(tc.REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    lines = ["# Batch.plane_quantiles_weighted, q = (0.025, 0.5, 0.975), live members only, next to Batch.plane_quantiles and",
             "# Batch.reduce_plane over the same array, the three in turn inside every repetition; scores: the weighted call also gives",
             "# the moments; ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls; GB/s = array" % args.reps,
             "# bytes / the weighted call's median",
             "%-5s %-14s %-7s %-6s %-19s %-15s %9s %26s %8s %26s %24s %8s %9s" % (
                 "name", "sites x members", "rows", "dtype", "paths (w / plain)", "scores", "array_MB", "weighted_ms", "GB/s",
                 "plane_quantiles_ms", "reduce_plane_ms", "x_plain", "x_reduce")]
    print("\n".join(lines), flush=True)
    for name in args.shapes.split(","):
        n_sites, M, rows, dtype = SHAPES[name]
        rows = max(1, int(rows * args.rows_scale))
        b, _ = tc.make(base, n_sites, M, sa.F64 if dtype == torch.float64 else sa.F32_MIXED)
        gen = torch.Generator(device="cuda").manual_seed(7)
        series = torch.randn((rows, n_sites * M), dtype=dtype, device="cuda", generator=gen)
        obs = torch.randn((rows, n_sites), dtype=torch.float64, device="cuda", generator=gen) * 0.01
        logw = torch.randn((n_sites * M,), dtype=torch.float64, device="cuda", generator=gen) * 2.0
        nbytes = series.numel() * series.element_size()
        stats = torch.empty((rows, n_sites, 2), dtype=torch.float64, device="cuda")
        for scores in (False, True):
            y = obs if scores else None
            plain = b.plane_quantiles(series, Q, obs=y)
            res = b.plane_quantiles_weighted(series, logw, Q, obs=y, want_moments=scores)
            assert int(res.site_weight[:, 2].abs().max().item()) == 0 and not bool(torch.isnan(res.quant).any().item())
            t_w, t_p, t_r = timed_in_turn([lambda: b.plane_quantiles_weighted(series, logw, Q, obs=y, want_moments=scores),
                                           lambda: b.plane_quantiles(series, Q, obs=y, out=plain),
                                           lambda: b.reduce_plane(series, stats)], args.reps)
            path = lambda p: "sort" if p == 1 else "selection"
            what = ("moments+rank" + ("+crps" if res.crps is not None else "")) if scores else "none"
            fmt = lambda t: "%9.4f (%.4f .. %.4f)" % t
            tc.emit(lines, "%-5s %-14s %-7d %-6s %-19s %-15s %9.1f %26s %8.1f %26s %24s %8.2f %9.2f" % (
                name, "%d x %d" % (n_sites, M), rows, "f64" if dtype == torch.float64 else "f32",
                path(res.path) + " / " + path(plain.path), what, nbytes / 1e6, fmt(t_w), nbytes / 1e6 / t_w[0], fmt(t_p), fmt(t_r),
                t_w[0] / t_p[0], t_w[0] / t_r[0]))
        b.close()
        del series
        torch.cuda.empty_cache()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
