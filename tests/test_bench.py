"""bench.py's command line: a plain run does only the timed steps, --full adds
the side lines, --dump-outputs writes what the last timed step computed.

The GPU test runs the benchmark itself (that is what it is about) on C1, the
smallest config, once for the module.  The dumped arrays are compared bitwise
with an optimize of the same graph in this process: the library's results do
not vary from run to run (tests/test_multi_gpu.py asserts the same of values
and trace columns 0-6; column 7 is wall-clock time and is not dumped).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE_LINES = ("cpu_baseline", "gauss_newton", "converged_regime", "marginals", "closest_keyframe", "live_resolve",
              "scan_registration", "c5")


class _FakeGraph:
    """poses() / trace() of a PoseGraph, host only."""

    def __init__(self, n):
        self.n = n

    def poses(self):
        return np.arange(3.0 * self.n).reshape(self.n, 3)

    def trace(self):
        return np.arange(40.0).reshape(5, 8)


def _fake_stats(bench):
    return {k: float(i) for i, k in enumerate(bench.DUMP_STATS)}


def test_dump_outputs_files(tmp_path):
    import bench
    out = tmp_path / "a" / "b"          # created on demand
    bench.dump_outputs(str(out), _FakeGraph(10), _fake_stats(bench))
    assert sorted(os.listdir(out)) == ["poses.npy", "stats.npy", "trace.npy"]
    poses, trace, stats = (np.load(out / f) for f in ("poses.npy", "trace.npy", "stats.npy"))
    assert poses.dtype == trace.dtype == stats.dtype == np.float64
    np.testing.assert_array_equal(poses, _FakeGraph(10).poses())
    np.testing.assert_array_equal(trace, _FakeGraph(10).trace()[:, :7])     # no wall-clock column
    np.testing.assert_array_equal(stats, np.arange(len(bench.DUMP_STATS), dtype=np.float64))


def test_dump_outputs_samples_a_large_graph(tmp_path, monkeypatch):
    """More poses than DUMP_MAX_ROWS: the same seeded sample of rows every
    time, in ascending order, within the size limit."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 64)
    full = _FakeGraph(1000).poses()
    got = []
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), _FakeGraph(1000), _fake_stats(bench))
        got.append(np.load(tmp_path / d / "poses.npy"))
    np.testing.assert_array_equal(got[0], got[1])
    assert got[0].shape == (64, 3)
    rows = (got[0][:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(got[0], full[rows])


def test_dump_limit_is_under_64_mb():
    import bench
    assert bench.DUMP_MAX_ROWS * 3 * 8 + 2 ** 20 <= 64 * 10 ** 6      # poses + (small) trace and stats


def test_help_lists_the_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory, pgo_lib):
    out = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "C1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]                  # the JSON line is stdout's only output
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_result_line(plain_run):
    d, _ = plain_run
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "GN iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    # value = linearisations of the timed steps / their wall time
    assert d["value"] == pytest.approx(d["per_step"]["linearizations"] / (1e-3 * d["ms_per_step"]), rel=1e-9)
    for k in SIDE_LINES:
        assert d[k] is None, k
    assert d["roofline"]["families"] == {} and d["roofline"]["profiled_factorizations"] == 0


@pytest.mark.gpu
def test_dump_is_what_the_timed_path_computes(plain_run):
    import bench
    from graphslam_amd import datasets
    from graphslam_amd.pose_graph import PoseGraph, default_params
    d, out = plain_run
    with PoseGraph.from_dataset(datasets.make("C1")) as pg:
        st = pg.optimize(default_params(lambda_lanes=d["config"]["lambda_lanes"]))
        poses, trace = pg.poses(), pg.trace()
    np.testing.assert_array_equal(np.load(out / "poses.npy"), poses)
    np.testing.assert_array_equal(np.load(out / "trace.npy"), trace[:, :7])
    np.testing.assert_array_equal(np.load(out / "stats.npy"), [float(st[k]) for k in bench.DUMP_STATS])
    assert st["final_error"] == d["per_step"]["final_error"]
