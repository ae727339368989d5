"""Where a gathering run of the node is cut into segments (csrc/node_cuts.h: segmentCuts, no HIP in it): the header built
on its own with g++ under AddressSanitizer + UndefinedBehaviourSanitizer (tests/c/node_cuts_check.cpp) and swept, in ONE
process, over step0 0..40 x n_steps 1..200 x n_segments 1..min(n_steps, 9) for the planes themselves (form 0) and for sums
over groups of 1, 7 and 48 steps (at most one segment per group) -- against the formulas restated here and against what the
callers rely on: the cuts start at 0, end at n_steps and increase strictly; a plane cut lies on a 16-step tile of the site
plan or is the plain proportional one; a sums cut lies on a whole group, and the reduced rows increase strictly up to the
number of groups."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = 2            # SIPNET_GATHER_SUMS

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def restated(step0, n_steps, n_seg, form, k):
    """the cuts as sipnet_node_run_gathering[_reduced] has always made them"""
    groups = (n_steps + k - 1) // k if form == SUMS else n_steps
    cuts = [0] * (n_seg + 1)
    cuts[n_seg] = n_steps
    for j in range(1, n_seg):
        raw = n_steps * j // n_seg
        tile = ((step0 + raw) & ~15) - step0
        cuts[j] = tile if tile > cuts[j - 1] else raw
        if form == SUMS:
            cuts[j] = (groups * j // n_seg) * k
    red = [(c + k - 1) // k if form == SUMS else c for c in cuts]
    return cuts, red


def cases():
    for form, k in ((0, 0), (SUMS, 1), (SUMS, 7), (SUMS, 48)):
        for step0 in range(41):
            for n_steps in range(1, 201):
                most = min(n_steps, 9) if form == 0 else min((n_steps + k - 1) // k, 9)
                for n_seg in range(1, most + 1):
                    yield step0, n_steps, n_seg, form, k


def test_segment_cuts_equal_the_restated_formulas_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "node_cuts_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "c", "node_cuts_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    todo = list(cases())
    r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in todo), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo) > 200000
    for (step0, n_steps, n_seg, form, k), line in zip(todo, lines):
        left, right = line.split("|")
        cuts, red = [int(x) for x in left.split()], [int(x) for x in right.split()]
        where = (step0, n_steps, n_seg, form, k, cuts, red)
        assert (cuts, red) == restated(step0, n_steps, n_seg, form, k), where
        assert len(cuts) == n_seg + 1 and cuts[0] == 0 and cuts[-1] == n_steps, where
        assert all(a < b for a, b in zip(cuts, cuts[1:])), where
        if form == 0:
            assert red == cuts, where
            assert all((step0 + c) % 16 == 0 or c == n_steps * j // n_seg for j, c in enumerate(cuts[1:-1], 1)), where
        else:
            assert all(c % k == 0 for c in cuts[1:-1]), where
            assert all(a < b for a, b in zip(red, red[1:])) and red[-1] == (n_steps + k - 1) // k, where
