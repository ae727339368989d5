"""dev (GPU box): what the timing tools of the many-site analyses share (pf_sites_time.py, enkf_sites_time.py,
enkf_local_time.py, enkf_block_time.py): the batch with its 48-step planes, the median of HIP-event timings, the ensemble
Kalman filter's operators, analysed pools and synthetic observations, the grid of sites, and the tail that writes --out."""
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


def arguments(calls, reps, shapes):
    """the parser of --calls, --reps, --out and --shapes with the tool's defaults"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=calls)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=shapes)
    return ap


def start(tool, shapes):
    """the base parameters and the shapes [(n_sites, M)] of "32x1024,..."; exits without a HIP device"""
    if not torch.cuda.is_available():
        sys.exit(tool + " needs a HIP device")
    base, _ = sa.read_params(os.path.join(REPO, "sipnet_amd", "data", "base_forest.param"), sa.flags_from())
    return base, [tuple(int(v) for v in s.split("x")) for s in shapes.split(",")]


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


def observations(b, planes, n_sites, M, unobserved=None):
    """on the device: every operator's observation at the site's ensemble mean, sd 10 %, inflation 1.02, and an info array;
    `unobserved`: a slice of sites without observations (reached only)"""
    st = b.get_state()
    lai = st[:, 1] / 80.0
    obs = np.stack([lai, st[:, 0] + st[:, 12], st[:, 3] / 10.0,
                    planes[0].double().sum(0).cpu().numpy()], 1).reshape(n_sites, M, 4).mean(1)
    sd = np.abs(obs) * 0.1 + 1e-3
    if unobserved is not None:
        obs[unobserved] = np.nan
    return (torch.tensor(obs, dtype=torch.float64, device="cuda"), torch.tensor(sd, dtype=torch.float64, device="cuda"),
            torch.full((n_sites,), 1.02, dtype=torch.float64, device="cuda"),
            torch.zeros((n_sites, 4), dtype=torch.int32, device="cuda"))


def grid(n_sites):
    """sites on a 0.25 degree grid, 32 or 16 wide"""
    width = 32 if n_sites >= 512 else 16
    r, c = np.divmod(np.arange(n_sites), width)
    return 40.0 + 0.25 * r, -90.0 + 0.25 * c


def lists(n_sites, radius):
    """the Gaspari-Cohn lists of the grid at half-width `radius` km; None: no neighbours"""
    if radius is None:
        return np.zeros(n_sites + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)
    return sa.gaspari_cohn(*grid(n_sites), radius)


def emit(lines, text):
    print(text, flush=True)
    lines.append(text)


def write_out(lines, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
