#!/usr/bin/env python3
"""dev (GPU box): the Metropolis move over members, Batch.mcmc_propose and Batch.mcmc_accept (sipnet_batch_mcmc_propose /
_accept), next to its two yardsticks in the same process and on the same shape: Batch.pf_rejuvenate over the same listed rows
(no pools; the approximate move this one stands beside) and a torch device copy of the rows the proposal touches (the listed
rows read and written, the saved rows written: 2 n rows copied).
Lines: shape x (1, 4 or 16 listed parameters); 1024 x 256 is the shape of the one-workgroup-per-site path.  Columns: the
proposal of one half; the pair proposal + accept with random log-posteriors (about half the proposals are put back) and the
accept's share = pair - proposal; where the library takes one workgroup per site, the proposal on the per-chunk launches
forced; the rejuvenation; the copy; the ratios.  gamma, jitter,
shrink and the log-posteriors are device tensors, info_out is given: nothing is synchronised.  HIP events around `calls` calls,
enough of them for a quarter of a second, after 3 warm-up calls; the median of `reps` repetitions and their range, ms per call.
usage: mcmc_move_time.py [--reps R] [--out FILE] [--shapes 256x1024,64x4096,1x131072,1024x256]"""
import argparse

import torch

import enkf_time_common as tc
from enkf_time_common import sa, synth
from pf_rejuvenate_time import NAMES, fmt
from quantiles_time import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="256x1024,64x4096,1x131072,1024x256")
    args = ap.parse_args()
    base, shapes = tc.start("mcmc_move_time.py", args.shapes)
    lines = ["# Batch.mcmc_propose and Batch.mcmc_accept next to Batch.pf_rejuvenate over the same rows and a torch copy of the touched rows;",
             "# ms per call: median (least .. most) of %d repetitions of `calls` calls after 3 warm-up calls" % args.reps,
             "# path: g one workgroup per site (sites of at most 256 members), s per-chunk launches; split_forced: path g's shapes on path s, median ms"]
    print("\n".join(lines), flush=True)
    tc.emit(lines, "%-11s %-4s %-4s %-4s %28s %12s %28s %10s %28s %28s %8s %7s" % (
        "shape", "prec", "prm", "path", "propose_ms", "split_forced", "propose+accept_ms", "accept_ms", "rejuvenate_ms", "copy_rows_ms",
        "x_rejuv", "x_copy"))
    for n_sites, M in shapes:
        b, _ = tc.make(base, n_sites, M, sa.F64)
        ncol = n_sites * M
        gen = torch.Generator(device="cuda").manual_seed(3)
        info = torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda")
        jitter = torch.full((n_sites,), 1e-3, dtype=torch.float64, device="cuda")
        shrink = torch.full((n_sites,), sa.liu_west_shrink(0.98), dtype=torch.float64, device="cuda")
        moved = torch.zeros(ncol, dtype=torch.int32, device="cuda")
        cur = torch.randn(ncol, dtype=torch.float64, device="cuda", generator=gen)
        new = torch.randn(ncol, dtype=torch.float64, device="cuda", generator=gen)
        draw = [0]
        for n_prm in (1, 4, 16):
            params = [sa.enkf_param(n, *synth.PERTURB[n][:2]) for n in NAMES[:n_prm]]
            gamma = torch.full((n_sites,), float(sa.demc_gamma(n_prm)), dtype=torch.float64, device="cuda")
            saved = torch.zeros((n_prm, ncol), dtype=torch.float64, device="cuda")

            def propose():
                draw[0] += 1
                b.mcmc_propose(params, gamma, jitter, half=draw[0] & 1, seed=1, draw=draw[0], saved=saved, moved=moved, info_out=info)

            def pair():
                propose()
                cur.copy_(new.roll(1))      # (fresh log-posteriors: an accept that kept new would accept nothing more)
                b.mcmc_accept(params, saved, moved, new, cur, seed=1, draw=draw[0], info_out=info)

            def refresh():
                cur.copy_(new.roll(1))

            def rejuvenate():
                draw[0] += 1
                b.pf_rejuvenate(params, shrink, seed=1, draw=draw[0], info_out=info)

            t_pro = timed(propose, args.reps)
            path = "g" if b.pf_info()["fused"] else "s"
            assert int(info[:, 0].min().item()) == 1 and int(info[:, 1].sum().item()) > 0
            t_other = None
            if path == "g":
                b.set_kernel(sa.KERNEL_AUTO, sa.KOPT_PF_MULTI_LAUNCH)
                t_other = timed(propose, args.reps)
                assert b.pf_info()["fused"] == 0
                b.set_kernel(sa.KERNEL_AUTO, 0)
            t_pair = timed(pair, args.reps)
            assert 0 < int(info[:, 2].sum().item()) < int(info[:, 1].sum().item())
            t_fresh = timed(refresh, args.reps)
            t_rej = timed(rejuvenate, args.reps)
            src = torch.randn((2 * n_prm, ncol), dtype=torch.float64, device="cuda", generator=gen)
            dst = torch.empty_like(src)
            t_cp = timed(lambda: dst.copy_(src), args.reps)
            tc.emit(lines, "%-11s %-4s %-4d %-4s %28s %12s %28s %10.4f %28s %28s %8.2f %7.2f" % (
                "%dx%d" % (n_sites, M), "f64", n_prm, path, fmt(t_pro), "%10.4f" % t_other[0] if t_other else "-", fmt(t_pair),
                t_pair[0] - t_pro[0] - t_fresh[0], fmt(t_rej), fmt(t_cp), t_pro[0] / t_rej[0], t_pro[0] / t_cp[0]))
            del src, dst
        b.close()
        torch.cuda.empty_cache()
    tc.emit(lines, "# accept_ms = propose+accept - propose - the copy that refreshes the log-posteriors between pairs")
    tc.emit(lines, "# x_rejuv = propose / rejuvenate (the same rows, no pools), x_copy = propose / copy_rows (2 n rows: the listed rows and the saved rows)")
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
