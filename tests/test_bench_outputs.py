"""bench.py's plain line and --dump-outputs: the arrays the timed path computed in its last step, sampled with a
fixed seed when they are large, identical from run to run, and equal to the oracle on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers

BENCH = os.path.join(helpers.REPO, "bench.py")


def test_dump_outputs_keeps_a_seeded_sample_under_the_budget(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)
    planes = torch.randn(3, 200, 1000, dtype=torch.float64)
    anc = torch.arange(5000, dtype=torch.int64)
    outs = [(v, planes[i], 1) for i, v in enumerate(("nee", "gpp", "et"))] + [("ancestors", anc, 0)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    total = 0
    for name in ("nee", "gpp", "et", "ancestors"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 400_000
    nee = np.load(tmp_path / "a" / "nee.npy")
    assert nee.shape == (200, 62)                   # 100 000 B per array / (200 steps x 8 B) member columns
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(1000, 62, replace=False))
    np.testing.assert_array_equal(nee, planes[0].numpy()[:, idx])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "ancestors.npy"), np.arange(5000, dtype=np.float64))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_what_the_oracle_computes(tmp_path):
    import sipnet_amd as sa
    from sipnet_amd import synth
    M, T, K = 256, 480, 2
    lines = []
    for d in ("one", "two"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "c2", "--members", str(M), "--nsteps", str(T),
                            "--steps", str(K), "--warmup", "1", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300, cwd=helpers.REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        out = [x for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(out) == 1, r.stdout[-3000:]
        lines.append(json.loads(out[0]))
    for j in lines:
        assert j["metric"] == "ensemble-site-timesteps/sec" and j["unit"] == "ensemble-site-timesteps/s"
        assert j["higher_is_better"] is True and j["dtype"] == "f64" and j["steps"] == K
        assert j["full"] is False and "roofline" not in j and "parity" not in j and "cpu_baseline" not in j
        assert j["value"] == pytest.approx(M * T / (j["ms_per_step"] * 1e-3), rel=1e-9)
    flags = sa.flags_from()
    base, _ = sa.read_params(os.path.join(helpers.REPO, "sipnet_amd", "data", "base_forest.param"), flags)
    clim = synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(T)))
    members = synth.perturbed_params(base, M, seed=synth.SEED_PARAMS)
    want, _, _ = helpers.load_oracle().run_block(flags, members, clim)
    for v, name in enumerate(("nee", "gpp", "et")):
        a, b = np.load(tmp_path / "one" / f"{name}.npy"), np.load(tmp_path / "two" / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == (T, M)     # small enough to be written whole
        assert np.array_equal(a, b)
        assert float(np.abs(a - want[v]).max()) < 1e-9, name
