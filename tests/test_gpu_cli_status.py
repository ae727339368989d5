"""The CLI when a member does not run (status != 0), and the single-variable outputs: every run mode reports a
failing run exactly once, by its global name, exits with its status, and leaves the other runs' outputs untouched.
russell_4 (no events, soil phenology: the default-physics kernels) cut to 100 records -- neither a multiple of 16 nor
of 8 -- with a three-member table whose last row has leafAllocation 0.9: the allocation fractions no longer add to less
than one, the batch API's status 3."""
import os
import re

import numpy as np
import pytest

from tests.test_cli import run_cli, stage

pytestmark = pytest.mark.gpu

T = 100
GOOD_ROWS = "aMax leafAllocation\n7.9 0.2\n8.1 0.2\n"
ALL_ROWS = GOOD_ROWS + "6.4 0.9\n"
NPP = r" \(NPP allocation params must be less than one individually and add to less than one\)$"


def staged(parent, name, **params):
    """russell_4 with the first T climate records in parent/name; `params` replace lines of sipnet.param"""
    d = parent / name
    d.mkdir()
    stage("russell_4", d)
    lines = open(d / "sipnet.clim").read().splitlines(keepends=True)
    assert len(lines) > T
    open(d / "sipnet.clim", "w").write("".join(lines[:T]))
    if params:
        txt = open(d / "sipnet.param").read().splitlines()
        txt = [(f"{l.split()[0]} {params[l.split()[0]]}" if l.split() and l.split()[0] in params else l) for l in txt]
        open(d / "sipnet.param", "w").write("\n".join(txt) + "\n")
    open(d / "good.txt", "w").write(GOOD_ROWS)
    open(d / "all.txt", "w").write(ALL_ROWS)
    return d


def failed_status(r, who):
    """the one `[ERROR  ] <who>: status <n> (NPP allocation ...` line of a run's stdout -> n, which is also the exit code"""
    hits = [re.match(r"\[ERROR  \] " + re.escape(who) + r": status (\d+)" + NPP, l) for l in r.stdout.splitlines()]
    hits = [h for h in hits if h]
    assert len(hits) == 1, r.stdout
    assert len([l for l in r.stdout.splitlines() if "NPP allocation" in l]) == 1, r.stdout
    n = int(hits[0].group(1))
    assert r.returncode == n, (r.returncode, r.stdout, r.stderr)
    assert n == 3
    return n


@pytest.mark.parametrize("devices", ["0", "0,0"], ids=["one-shard", "two-shards"])
def test_cli_text_ensemble_reports_the_member_that_did_not_run(tmp_path, devices):
    """--ensemble-params: one line naming member 2 -- the global index, also from the shard of members [1,3) -- the
    exit code is its status, members 0 and 1 have the files of the run without the bad row, member 2 has none"""
    good, bad = staged(tmp_path, "good"), staged(tmp_path, "bad")
    r = run_cli(good, "-i", "sipnet.in", "--ensemble-params", "good.txt")
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_cli(bad, "-i", "sipnet.in", "--ensemble-params", "all.txt", "--devices", devices)
    failed_status(r, "member 2")
    for m in (0, 1):
        want = open(good / f"sipnet.{m}.out", "rb").read()
        assert len(want.splitlines()) >= T
        assert open(bad / f"sipnet.{m}.out", "rb").read() == want
    assert not os.path.exists(bad / "sipnet.2.out")


@pytest.mark.parametrize("mode", [("p.nc",), ("s.nc", "--ensemble-out-sums", "8"),
                                  ("c.nc", "--ensemble-out-columns", "nee,plantWoodC", "--ensemble-out-segment", "32")],
                         ids=["planes", "sums", "segmented-columns"])
def test_cli_block_modes_report_the_member_that_did_not_run(tmp_path, mode):
    """--ensemble-out on two shards (members [0,1) and [1,3)): planes, sums over groups of 8 steps (13 groups, the
    last of 4 steps), named columns in segments of 32 steps (four launches, the last of 4 steps) -- one line naming
    member 2, the block holds all three members, the two that ran exactly as without the bad row"""
    from sipnet_amd import ensemble_io as eio
    d = staged(tmp_path, "run")
    common = ("-i", "sipnet.in", "--devices", "0,0", "--ensemble-out")
    r = run_cli(d, "--ensemble-params", "good.txt", *common, "good_" + mode[0], *mode[1:])
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_cli(d, "--ensemble-params", "all.txt", *common, *mode)
    failed_status(r, "member 2")
    want, got = eio.read_ensemble_netcdf(d / ("good_" + mode[0])), eio.read_ensemble_netcdf(d / mode[0])
    assert got["member"].tolist() == [0, 1, 2]
    assert got["nee"].shape == ((13 if "--ensemble-out-sums" in mode else T), 3)
    assert np.abs(want["nee"]).max() > 0
    np.testing.assert_array_equal(got["nee"][:, :2], want["nee"])


def test_cli_ensemble_stats_refuses_members_that_did_not_run(tmp_path):
    d = staged(tmp_path, "run")
    r = run_cli(d, "-i", "sipnet.in", "--ensemble-params", "all.txt", "--ensemble-stats", "st.txt")
    failed_status(r, "member 2")
    assert "the statistics would include members that did not run" in r.stdout
    assert not os.path.exists(d / "st.txt")


def test_cli_sites_reports_the_run_that_did_not_run(tmp_path):
    """--sites: three directories of one forcing are one site of three members; the failing one is named by its
    directory, once -- with text, with a block, and with both (the block of the three planes beside text comes out of
    the record's columns: before the CLI shared that mapping with the ensemble path, this run ended in a copy error)"""
    r0, r1 = staged(tmp_path, "r0"), staged(tmp_path, "r1")
    r2 = staged(tmp_path, "r2", leafAllocation=0.9)
    open(tmp_path / "good.txt", "w").write("r0\nr1\n")
    open(tmp_path / "runs.txt", "w").write("r0\nr1\nr2\n")
    r = run_cli(tmp_path, "--sites", "good.txt", "-i", "sipnet.in")
    assert r.returncode == 0, r.stdout + r.stderr
    want = []
    for d in (r0, r1):
        want.append(open(d / "sipnet.out", "rb").read())
        os.remove(d / "sipnet.out")
    assert len(want[0].splitlines()) >= T and len(want[1].splitlines()) >= T
    who = os.path.realpath(r2)
    r = run_cli(tmp_path, "--sites", "runs.txt", "-i", "sipnet.in")
    assert "1 site(s) x up to 3 member(s)" in r.stdout, r.stdout
    n = failed_status(r, who)
    assert [open(d / "sipnet.out", "rb").read() for d in (r0, r1)] == want
    assert not os.path.exists(r2 / "sipnet.out")
    r = run_cli(tmp_path, "--sites", "runs.txt", "-i", "sipnet.in", "--ensemble-out", "b.nc")
    assert failed_status(r, who) == n
    r = run_cli(tmp_path, "--sites", "runs.txt", "-i", "sipnet.in", "--ensemble-out", "b.nc", "--ensemble-text")
    assert failed_status(r, who) == n


def test_cli_single_variable_outputs_agree_among_the_run_paths(tmp_path):
    """DO_SINGLE_OUTPUTS = 1: a single run, a one-member ensemble of the same parameters (--math strict) and --sites on
    that one directory write the same sipnet.NEE / NEE_cum / GPP / GPP_cum, one token per step"""
    dirs = {k: staged(tmp_path, k) for k in ("single", "ensemble", "sites")}
    for d in dirs.values():
        open(d / "sipnet.in", "a").write("\nDO_SINGLE_OUTPUTS = 1\n")
    amax = [l.split()[1] for l in open(dirs["ensemble"] / "sipnet.param") if l.split() and l.split()[0] == "aMax"][0]
    open(dirs["ensemble"] / "one.txt", "w").write(f"aMax\n{amax}\n")
    open(tmp_path / "runs.txt", "w").write("sites\n")
    for r in (run_cli(dirs["single"], "-i", "sipnet.in"),
              run_cli(dirs["ensemble"], "-i", "sipnet.in", "--ensemble-params", "one.txt", "--math", "strict"),
              run_cli(tmp_path, "--sites", "runs.txt", "-i", "sipnet.in")):
        assert r.returncode == 0, r.stdout + r.stderr
    files = {}
    for item in ("NEE", "NEE_cum", "GPP", "GPP_cum"):
        single = open(dirs["single"] / f"sipnet.{item}", "rb").read()
        assert len(single.split()) == T
        assert open(dirs["ensemble"] / f"sipnet.0.{item}", "rb").read() == single
        assert open(dirs["sites"] / f"sipnet.{item}", "rb").read() == single
        files[item] = single
    assert files["NEE"] != files["NEE_cum"] and float(files["NEE_cum"].split()[-1]) != 0.0
