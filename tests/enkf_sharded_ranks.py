"""One rank of tests/test_gpu_enkf_sharded.py::test_ranks_that_are_processes_rehearsed_on_one_gpu, started by
torch.distributed.run: its shard of a crafted union as a batch on device 0, sipnet_amd.dist.enkf_analysis_sharded, and its
state before and after written to --out/rank<k>.npz.  --collective group: the process group (gloo among several ranks on the
one GPU, through host copies); direct: a DirectComm of the engine's own (one rank)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SITES = 3
SIZES = {1: (200,), 2: (130, 70)}


def inputs(world):
    """the union every rank crafts alike -> (sizes, pools, planes, operators, obs, sd, inflation, dead columns)"""
    from tests.enkf_gpu_common import observe
    from tests.test_gpu_enkf_edges import ops4, well_conditioned
    sizes = SIZES[world]
    dead = [9, N_SITES * sum(sizes) - 1]
    pools, planes, fake = well_conditioned(90, N_SITES, sum(sizes), dead)
    ops = ops4()
    obs, sd = observe(fake, planes, None, N_SITES, ops, np.random.default_rng(12), nan_obs=((1, 0),))
    return sizes, pools, planes, ops, obs, sd, np.array([1.0, 1.05, 1.1]), dead


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collective", choices=["group", "direct"], required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    import sipnet_amd as sa
    from sipnet_amd import dist as sd_
    from tests import enkf_sharded_reference as shr
    from tests.enkf_gpu_common import ANALYSED, BASE, DEV, crafted
    from tests.test_gpu_enkf_edges import upload
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    if args.collective == "group":
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sizes, pools, planes, ops, obs, sd, infl, dead = inputs(world)
    mask = np.zeros(pools.shape[0], dtype=bool)
    mask[dead] = True
    base = sa.read_params(BASE, sa.flags_from())[0]
    b, st0 = crafted(base, N_SITES, sizes[rank], sa.F64, shr.split(pools, N_SITES, sizes)[rank],
                     np.flatnonzero(shr.split(mask, N_SITES, sizes)[rank]))
    dev = upload([np.ascontiguousarray(shr.split(p.T, N_SITES, sizes)[rank].T) for p in planes])
    prm0 = b.get_params()
    comm = sd_.DirectComm(rank, world, 0) if args.collective == "direct" else None
    info = torch.zeros((N_SITES, 4), dtype=torch.int32, device=DEV)
    gathered = sd_.enkf_analysis_sharded(b, obs, sd, ops, ANALYSED, planes=dev, inflation=infl, rank=rank, world=world,
                                         group=None if comm is not None else dist.group.WORLD, collectives=comm, info_out=info)
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), st0=st0, st1=b.get_state(), prm0=prm0, info=info.cpu().numpy(),
             n_sites=N_SITES, gathered_world=gathered.shape[0])
    if comm is not None:
        comm.close()
    b.close()
    if args.collective == "group":
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
