"""The Cholesky plan is a function of the graph and the planner's knobs alone.

PoseGraph.debug_plan_digest hashes every list and record of a plan, section by
section (graphslam_amd/csrc/pgo_plan_digest.h), so two plans are the same
exactly when their digests agree -- task order and flops figures included.
Here: the designed front-shape graphs, C1 and C2, planned for one rank and for
each of 4 ranks, give the same digests whether the planner runs on 1 thread or
on 8 (levels are scheduled concurrently and merged in level order), and twice
in one process (the second plan is built from scratch, no state carried over).
The pool's size is fixed per process, hence the subprocesses.  Host only.

No digest is stored: an intended change of the schedule needs no new fixture
(scripts/plan_digests.py writes the whole case set's for an A/B of two builds).
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import front_shapes as fs
from graphslam_amd import datasets
from graphslam_amd.pose_graph import PoseGraph
for name in [c.name for c in fs.CASES] + ["C1", "C2"]:
    pg = PoseGraph.from_dataset(datasets.make(name) if name in datasets.CONFIGS else fs.build(name))
    for rep in range(2):
        for size, rank in [(1, 0), (4, 0), (4, 1), (4, 2), (4, 3)]:
            d, _ = pg.debug_plan_digest(size, rank)
            print(rep, f"{name}/{size}r{rank}", *(f"{v:016x}" for v in d))
"""


@pytest.fixture(scope="module")
def digests(pgo_lib):
    """{threads: [first pass's lines, second pass's lines]}"""
    out = {}
    for threads in ("1", "8"):
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, PGO_PLAN_THREADS=threads),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln.split(" ", 1) for ln in r.stdout.splitlines()]
        out[threads] = [[rest for rep, rest in lines if rep == p] for p in ("0", "1")]
    return out


def test_digest_covers_the_cases(digests):
    import front_shapes as fs
    first = digests["1"][0]
    assert len(first) == 5 * (len(fs.CASES) + 2)
    assert all(len(ln.split()) == 8 for ln in first)           # the case and its 7 sections
    assert len({ln.split(" ", 1)[1] for ln in first}) > len(fs.CASES)   # (not one constant)


@pytest.mark.parametrize("threads", ["1", "8"])
def test_same_plan_twice_in_one_process(digests, threads):
    assert digests[threads][0] == digests[threads][1]


def test_same_plan_for_any_thread_count(digests):
    assert digests["1"][0] == digests["8"][0]
