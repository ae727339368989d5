#!/usr/bin/env python3
"""dev (GPU box): Batch.series_loglik (sipnet_batch_series_loglik) next to Batch.reduce_plane over the same array (the project's
yardstick for "the same bytes, read once"), and Batch.pf_resample_sites next to Batch.pf_analysis_sites.
Lines: one fp64 plane of 1 site x 10 240 members x a year of half-hourly steps against 17 520 observations, no gaps
("year"); the same with every second day missing ("gaps": the reads that are left are half the array); the daily sums of 256
sites x 1 024 members x 365 days, NEE (Gauss) and ET (Laplace) together ("sums": two arrays, reduce_plane over both); 1 site x
65 536 members of floats x 512 rows ("wide").  With the constants, every output but the per-term sums; path: the library's
choice.  The series are seeded normal numbers, the observations the members' mean plus noise.  HIP events around `calls`
calls, enough of them for a quarter of a second, after 3 warm-up calls; the median of `reps` repetitions and their range, ms
per call; GB/s = the bytes of the rows that are read / the median.
The resampling: 256 sites x 1 024 particles, fp32-mixed and fp64; pf_analysis_sites on a one-step plane (its log-weights
cost one row) next to pf_resample_sites on the log-weights it left, without and with the effective sample size and the keep
rule (ess_min = M / 2).
usage: series_loglik_time.py [--reps R] [--out FILE] [--shapes year,gaps,sums,wide,resample] [--rows-scale F]"""
import argparse
import os

import numpy as np
import torch

import enkf_time_common as tc
from enkf_time_common import sa
from quantiles_time import timed

SHAPES = {   # name: (n_sites, members, rows, dtype, terms, every second day missing)
    "year": (1, 10240, 17520, torch.float64, 1, False),
    "gaps": (1, 10240, 17520, torch.float64, 1, True),
    "sums": (256, 1024, 365, torch.float64, 2, False),
    "wide": (1, 65536, 512, torch.float32, 1, False),
}


def fmt(t):
    return "%9.4f (%.4f .. %.4f)" % t[:3]


def series_lines(lines, base, names, reps, rows_scale):
    tc.emit(lines, "%-5s %-14s %-7s %-6s %-5s %-5s %9s %9s %22s %8s %22s %9s" % (
        "name", "sites x members", "rows", "dtype", "terms", "path", "array_MB", "read_MB", "series_loglik_ms", "GB/s", "reduce_plane_ms",
        "x_reduce"))
    for name in names:
        n_sites, M, rows, dtype, n_terms, half = SHAPES[name]
        rows = max(1, int(rows * rows_scale))
        b, _ = tc.make(base, n_sites, M, sa.F64 if dtype == torch.float64 else sa.F32_MIXED)
        gen = torch.Generator(device="cuda").manual_seed(7)
        arrays = [torch.randn((rows, n_sites * M), dtype=dtype, device="cuda", generator=gen) for _ in range(n_terms)]
        terms, used = [], 0
        for k, x in enumerate(arrays):
            mean = x.double().view(rows, n_sites, M).mean(2).t().contiguous()
            obs = mean + 0.3 * torch.randn((n_sites, rows), dtype=torch.float64, device="cuda", generator=gen)
            if half:
                obs[:, (torch.arange(rows, device="cuda") // 48) % 2 == 1] = float("nan")
            used += int((~torch.isnan(obs[0])).sum().item())
            sd = torch.full((n_sites, rows), 1.5, dtype=torch.float64, device="cuda")
            terms.append(sa.loglik_term(x, obs, sd, kind=sa.LOGLIK_LAPLACE if k else sa.LOGLIK_GAUSS))
        nbytes = sum(x.numel() * x.element_size() for x in arrays)
        read = used * n_sites * M * arrays[0].element_size()
        stats = torch.empty((rows, n_sites, 2), dtype=torch.float64, device="cuda")
        out = torch.empty(b.ncol, dtype=torch.float64, device="cuda")
        used_out = torch.empty((n_sites, n_terms), dtype=torch.int32, device="cuda")
        info = torch.empty((n_sites, 2), dtype=torch.int32, device="cuda")

        def reduce_all():
            for x in arrays:
                b.reduce_plane(x, stats)

        def loglik(path=0):
            return b.series_loglik(terms, out=out, used_out=used_out, info_out=info, path=path)
        t_red = timed(reduce_all, reps)
        one = loglik(1).clone()
        assert torch.equal(one.view(torch.int64), loglik(2).view(torch.int64)) and int(info[:, 1].min().item()) == used
        chunks = n_sites * ((M + 255) // 256)
        tiles = n_terms * ((rows + 255) // 256)
        ran = 2 if (tiles > 1 and chunks < 2 * torch.cuda.get_device_properties(0).multi_processor_count) else 1   # (the library's rule)
        for path in (0, 3 - ran):
            t = timed(lambda: loglik(path), reps)
            tc.emit(lines, "%-5s %-14s %-7d %-6s %-5d %-5s %9.1f %9.1f %22s %8.1f %22s %9.2f" % (
                name, "%d x %d" % (n_sites, M), rows, "f64" if dtype == torch.float64 else "f32", n_terms,
                "%d%s" % (ran if path == 0 else path, "" if path == 0 else "*"), nbytes / 1e6, read / 1e6, fmt(t), read / 1e6 / t[0], fmt(t_red),
                t[0] / t_red[0]))
        b.close()
        del arrays, terms
        torch.cuda.empty_cache()
    tc.emit(lines, "# path: the one the library chose; N*: the other one, forced")


def resample_lines(lines, base, reps):
    n_sites, M = 256, 1024
    tc.emit(lines, "# the resampling at %d x %d, with_params, totals on the device: pf_analysis_sites on a ONE-step plane | pf_resample_sites on its" % (n_sites, M))
    tc.emit(lines, "# log-weights | the same with ess_out and ess_min = M / 2 (fresh log-weights copied in before every call, the copy timed alone)")
    tc.emit(lines, "%-5s %22s %22s %22s %22s" % ("prec", "pf_analysis_sites_ms", "pf_resample_sites_ms", "with_ess_keep_ms", "logw_copy_ms"))
    for prec, label in ((sa.F32_MIXED, "f32"), (sa.F64, "f64")):
        b, planes = tc.make(base, n_sites, M, prec)
        plane = planes[0][:1].contiguous()
        tot = plane.double().view(n_sites, M)
        obs, sig = tot.median(1).values, tot.std(1) * 0.7
        u0 = torch.full((n_sites,), 0.37, dtype=torch.float64, device="cuda")
        total = torch.zeros(n_sites, dtype=torch.int64, device="cuda")
        ess = torch.zeros(n_sites, dtype=torch.float64, device="cuda")
        ess_min = torch.full((n_sites,), M / 2.0, dtype=torch.float64, device="cuda")
        t_a = timed(lambda: b.pf_analysis_sites(plane, obs, sig, u0, with_params=True, total_out=total), reps)
        _, logw = b.pf_analysis_sites(plane, obs, sig, u0, with_params=True, total_out=total)
        work = logw.clone()
        t_r = timed(lambda: b.pf_resample_sites(logw, u0, with_params=True, total_out=total), reps)

        def cycle():
            work.copy_(logw)
            b.pf_resample_sites(work, u0, ess_min=ess_min, with_params=True, total_out=total, ess_out=ess)
        t_k = timed(cycle, reps)
        t_c = timed(lambda: work.copy_(logw), reps)
        tc.emit(lines, "%-5s %22s %22s %22s %22s" % (label, fmt(t_a), fmt(t_r), fmt(t_k), fmt(t_c)))
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="year,gaps,sums,wide,resample")
    ap.add_argument("--rows-scale", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("series_loglik_time.py needs a HIP device")
    base, _ = sa.read_params(os.path.join(tc.REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    names = args.shapes.split(",")
    lines = ["# Batch.series_loglik (normalised, used_out and info_out given) next to Batch.reduce_plane over the same array(s);",
             "# ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls; GB/s = bytes of the rows read / median" % args.reps]
    print("\n".join(lines), flush=True)
    series_lines(lines, base, [n for n in names if n in SHAPES], args.reps, args.rows_scale)
    if "resample" in names:
        resample_lines(lines, base, args.reps)
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
