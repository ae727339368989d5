#!/usr/bin/env python3
"""dev (GPU box): Batch.plane_quantiles (sipnet_batch_plane_quantiles) next to two yardsticks over the same array:
Batch.reduce_plane (the streaming floor: the same bytes read once, no ordering) and what a user does today without leaving the
device, torch.sort along the member axis plus the gathers and the interpolation (all members, no liveness, no scores).
Shapes: one fp64 plane of 1 site x 10 240 members x a year of half-hourly steps (the sort path, 16 384 keys a cell); the daily
sums of 256 sites x 1 024 members x 365 days, fp64 (the sort path, 1 024 keys a cell); 1 site x 65 536 members of floats x
512 rows (the selection path).  q = (0.025, 0.5, 0.975), live members only, without scores and with them (ranks and the CRPS;
the selection path: ranks).  The batch is set up from the synthetic climate; the series are seeded normal numbers (the sort
network does the same work whatever the values).  HIP events around `calls` calls, enough of them for a quarter of a second,
after 3 warm-up calls; the median of `reps` repetitions and their range, ms per call; GB/s = the array's bytes / the median.
usage: quantiles_time.py [--reps R] [--out FILE] [--shapes year,sums,wide] [--rows-scale F]"""
import argparse
import math
import os

import numpy as np
import torch

import enkf_time_common as tc
from enkf_time_common import sa

Q = (0.025, 0.5, 0.975)
SHAPES = {   # name: (n_sites, members, rows, dtype, path)
    "year": (1, 10240, 17520, torch.float64, 0),
    "sums": (256, 1024, 365, torch.float64, 0),
    "wide": (1, 65536, 512, torch.float32, 0),
}


def timed(fn, reps):
    """-> (median, least, most) ms per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    calls = int(min(200, max(3, math.ceil(250.0 / max(e0.elapsed_time(e1), 1e-3)))))
    out = []
    for _ in range(reps):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return float(np.median(out)), float(min(out)), float(max(out)), calls


def torch_route(series, rows, n_sites, M):
    lo, g = sa.quantile_positions(M, Q)
    lo_t = torch.tensor(lo.astype(np.int64), device="cuda")
    hi_t = torch.clamp(lo_t + 1, max=M - 1)
    g_t = torch.tensor(g, dtype=torch.float64, device="cuda")

    def fn():
        xs, _ = torch.sort(series[:, :n_sites * M].view(rows, n_sites, M), dim=2)
        a, b = xs[:, :, lo_t].double(), xs[:, :, hi_t].double()
        return a + g_t * (b - a)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="year,sums,wide")
    ap.add_argument("--rows-scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quantiles_time.py needs a HIP device")
    base, _ = sa.read_params(os.path.join(tc.REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    lines = ["# Batch.plane_quantiles, q = (0.025, 0.5, 0.975), live members only, next to Batch.reduce_plane (the same bytes, no",
             "# ordering) and torch.sort along the members + gathers + interpolation (all members, no scores) over the same array;",
             "# ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls; GB/s = array bytes / median" % args.reps,
             "%-5s %-14s %-7s %-6s %-9s %6s %9s %22s %8s %20s %20s %9s %9s" % (
                 "name", "sites x members", "rows", "dtype", "path", "scores", "array_MB", "quantiles_ms", "GB/s", "reduce_plane_ms",
                 "torch_sort_ms", "x_reduce", "x_torch")]
    print("\n".join(lines), flush=True)
    for name in args.shapes.split(","):
        n_sites, M, rows, dtype, path = SHAPES[name]
        rows = max(1, int(rows * args.rows_scale))
        b, _ = tc.make(base, n_sites, M, sa.F64 if dtype == torch.float64 else sa.F32_MIXED)
        gen = torch.Generator(device="cuda").manual_seed(7)
        series = torch.randn((rows, n_sites * M), dtype=dtype, device="cuda", generator=gen)
        obs = torch.randn((rows, n_sites), dtype=torch.float64, device="cuda", generator=gen) * 0.01
        nbytes = series.numel() * series.element_size()
        stats = torch.empty((rows, n_sites, 2), dtype=torch.float64, device="cuda")
        t_red = timed(lambda: b.reduce_plane(series, stats), args.reps)
        t_sort = timed(torch_route(series, rows, n_sites, M), args.reps)
        for scores in (False, True):
            res = b.plane_quantiles(series, Q, obs=obs if scores else None, path=path)
            t_q = timed(lambda: b.plane_quantiles(series, Q, obs=obs if scores else None, path=path, out=res), args.reps)
            # (the result is what the torch route gives, where that route's two roundings of the interpolation agree)
            want = torch_route(series, rows, n_sites, M)()
            assert int(res.count.min().item()) == M and torch.allclose(res.quant.permute(1, 2, 0), want, rtol=1e-12, atol=1e-300)
            fmt = lambda t: "%9.4f (%.4f .. %.4f)" % t[:3]
            tc.emit(lines, "%-5s %-14s %-7d %-6s %-9s %6s %9.1f %22s %8.1f %20s %20s %9.2f %9.2f" % (
                name, "%d x %d" % (n_sites, M), rows, "f64" if dtype == torch.float64 else "f32",
                "sort" if res.path == 1 else "selection", ("rank+crps" if res.crps is not None else "rank") if scores else "none",
                nbytes / 1e6, fmt(t_q), nbytes / 1e6 / t_q[0], fmt(t_red), fmt(t_sort), t_q[0] / t_red[0], t_q[0] / t_sort[0]))
        b.close()
        del series
        torch.cuda.empty_cache()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
