"""The linear initialisation on the GPU (pgo_initialize_linear) against the
numpy twin tests/init_twin.py, through the C-ABI.

Tolerances (fp64 throughout):
* assembled systems (k_init_orient / k_init_trans): 1e-10 x max|hdiag| on the
  blocks and 1e-10 x max(|rhs|, 1) on the right-hand side, test_linearize_parity's
  -- the same formulas, another summation order;
* solutions: norm-wise 1e-8 against the twin's sparse LU, test_cholesky_step_vs_
  oracle's -- both exact solves, rounding amplified by the system's condition;
* independence from the current values, repeatability, the Huber copy: bitwise.
"""
import os
import subprocess

import numpy as np
import pytest

import init_twin as it
from graphslam_amd import _lib, datasets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def angdiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def c1_nondiagonal():
    g = datasets.make("C1")
    g.edge_cov = it.random_covariances(g.num_edges)
    return g


BUILDERS = {
    "square": datasets.square_loop,
    "C1": lambda: datasets.make("C1"),
    "C1-nn": lambda: datasets.make("C1-nn"),
    "star": it.star,                      # a row longer than kThreads and than any G
    "C1-nondiagonal": c1_nondiagonal,     # the Schur-complement weight, Omega_t,theta and R_z
    "C2": lambda: datasets.make("C2"),
}
_graphs, _twin = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = BUILDERS[name]()
    return _graphs[name]


def twin_solution(name):
    """The twin's (x, y, theta) of a graph, computed once and shared."""
    if name not in _twin:
        _twin[name] = it.initialize(graph(name))
        _twin[name].setflags(write=False)
    return _twin[name]


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


# ------------------------------------------------------------ 1. the systems
@pytest.mark.parametrize("name", ["square", "C1", "C1-nn", "star", "C1-nondiagonal"])
def test_system_parity(pg_cls, name):
    g = graph(name)
    pg = pg_cls.from_dataset(g)
    for stage in (1, 2):
        # stage 2 is assembled at the handle's current orientations: the dataset's initial ones
        ref = it.orientation_system(g) if stage == 1 else it.position_system(g, g.initial[:, 2])
        hd, ho, rhs = pg.debug_init_system(stage)
        scale_h = np.abs(ref.hdiag).max()
        scale_b = max(np.abs(ref.rhs).max(), 1.0)
        dh, do, db = np.abs(hd - ref.hdiag).max(), np.abs(ho - ref.hoff).max(), np.abs(rhs - ref.rhs).max()
        print(f"{name} stage {stage}: hdiag {dh / scale_h:.2e} hoff {do / scale_h:.2e} rhs {db / scale_b:.2e}")
        assert dh <= 1e-10 * scale_h
        assert do <= 1e-10 * scale_h
        assert db <= 1e-10 * scale_b
        # the embedding: the other slots are an exact identity / exact zeros
        other = [0, 1] if stage == 1 else [2]
        for a in other:
            assert np.all(hd[:, a, a] == 1.0) and np.all(rhs[:, a] == 0.0)
        mine = [2] if stage == 1 else [0, 1]
        mask = np.ones((3, 3), bool)
        mask[np.ix_(mine, mine)] = False
        assert np.all(ho[:, mask] == 0.0)
        offd = mask & ~np.eye(3, dtype=bool)
        assert np.all(hd[:, offd] == 0.0)
    # the values were only read
    assert np.array_equal(pg.poses(), pg_cls.from_dataset(g).poses())
    pg.close()


# ---------------------------------------------------------- 2. the solutions
@pytest.mark.parametrize("name", ["square", "C1", "C1-nn", "star", "C1-nondiagonal", "C2"])
def test_solution_parity(pg_cls, name):
    g = graph(name)
    ref = twin_solution(name)
    pg = pg_cls.from_dataset(g)
    st = pg.initialize_linear()
    x = pg.poses()
    rel_th = np.linalg.norm(angdiff(x[:, 2], ref[:, 2])) / np.linalg.norm(ref[:, 2])
    rel_p = np.linalg.norm(x[:, :2] - ref[:, :2]) / np.linalg.norm(ref[:, :2])
    print(f"{name}: theta {rel_th:.2e} positions {rel_p:.2e} error {st['error_before']:.6g} -> "
          f"{st['error_after']:.6g} depth {st['tree_depth']} wraps {st['wraps']}")
    assert rel_th <= 1e-8, rel_th
    assert rel_p <= 1e-8, rel_p
    t = it.tree(g)
    assert (st["status"], st["components"], st["tree_depth"], st["wraps"]) == (0, t.components, t.depth, t.wraps)
    print(f"{name}: twin error after {it.error(g, ref):.10g}")
    pg.close()


# ------------------------------------- 3. independence from the current values
def test_result_does_not_depend_on_the_current_values(pg_cls):
    g = graph("C1")
    pg = pg_cls.from_dataset(g)
    pg.initialize_linear()
    a = pg.poses()
    pg.initialize_linear()                      # from its own result
    assert np.array_equal(pg.poses(), a)
    rng = np.random.default_rng(11)
    scattered = rng.uniform(-50, 50, size=(g.num_poses, 3))
    scattered[:, 2] = rng.uniform(-np.pi, np.pi, size=g.num_poses)
    pg.set_poses(scattered)
    pg.initialize_linear()
    assert np.array_equal(pg.poses(), a)
    other = pg_cls.from_dataset(g)              # two runs from the same values, two handles
    other.initialize_linear()
    assert np.array_equal(other.poses(), a)
    other.close()
    pg.close()


# ------------------------------------------------------------ 4. edge cases
COV = np.diag([0.0025, 0.0025, 7.6e-5])


def test_single_vertex_with_a_prior(pg_cls):
    pg = pg_cls()
    pg.add_vertex(7, 30.0, -4.0, 2.0)
    pg.add_prior(7, [1.5, -2.0, 0.7], np.diag([0.01, 0.02, 0.03]))
    st = pg.initialize_linear()
    assert (st["components"], st["tree_depth"], st["wraps"]) == (1, 0, 0)
    assert np.abs(pg.poses() - [[1.5, -2.0, 0.7]]).max() <= 1e-12
    assert st["error_after"] <= 1e-20


def test_two_vertices_one_edge(pg_cls):
    pg = pg_cls()
    pg.add_vertex(1, 9.0, 9.0, 1.0)
    pg.add_vertex(2, -9.0, 3.0, -2.0)
    pg.add_prior(1, [1.0, 2.0, np.pi / 2], np.diag([0.01] * 3))
    pg.add_edge(1, 2, [3.0, 1.0, 0.25], COV)
    pg.initialize_linear()
    # pose 2 = pose 1 o z: (1 - 1, 2 + 3, pi / 2 + 0.25)
    assert np.abs(pg.poses() - [[1.0, 2.0, np.pi / 2], [0.0, 5.0, np.pi / 2 + 0.25]]).max() <= 1e-10
    assert pg.error() <= 1e-18


def test_two_components(pg_cls):
    g = it.two_components()
    ref = it.initialize(g)
    pg = pg_cls.from_dataset(g)
    st = pg.initialize_linear()
    x = pg.poses()
    assert st["components"] == 2
    assert np.linalg.norm(angdiff(x[:, 2], ref[:, 2])) <= 1e-8 * np.linalg.norm(ref[:, 2])
    assert np.linalg.norm(x[:, :2] - ref[:, :2]) <= 1e-8 * np.linalg.norm(ref[:, :2])


def test_component_without_a_prior(pg_cls):
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException
    g = it.two_components(prior_b=False)
    pg = pg_cls.from_dataset(g)
    assert np.isfinite(pg.error())              # the graph is on the device, values uploaded
    before = pg.poses()
    with pytest.raises(IndeterminantLinearSystemException) as ei:
        pg.initialize_linear()
    assert ei.value.status == _lib.PGO_E_INDETERMINANT
    assert np.array_equal(pg.poses(), before)


def test_robust_losses_are_ignored(pg_cls):
    """Huber on every loop closure: bitwise the result of the Gaussian copy."""
    g = graph("C1")
    pg = pg_cls.from_dataset(g)
    pg.initialize_linear()
    h = datasets.make("C1")
    loss = np.zeros(h.num_edges, dtype=np.int32)
    loss[datasets.loop_closure_indices(h)] = _lib.PGO_LOSS_HUBER
    assert loss.sum() > 0
    h.edge_loss, h.edge_loss_k = loss, 1.0
    ph = pg_cls.from_dataset(h)
    st = ph.initialize_linear()
    assert np.array_equal(ph.poses(), pg.poses())
    assert st["error_after"] == ph.error()      # (the robust error, as pgo_error reports it)


def test_stats_error_after_is_pgo_error(pg_cls):
    g = graph("C1-nn")
    pg = pg_cls.from_dataset(g)
    e0 = pg.error()
    st = pg.initialize_linear()
    assert st["error_before"] == e0
    assert st["error_after"] == pg.error()
    assert st["error_after"] < 1e-2 * e0
    assert st["ms_total"] >= st["ms_orient"] + st["ms_trans"] > 0


# ------------------------------------------------- 5. what the call is for
def test_lm_converges_from_the_linear_initialisation(pg_cls):
    """C2: from the dead-reckoned values default LM needs more lambda tries; from
    the two linear solves it converges to the error it reaches from ground truth."""
    g = graph("C2")
    pg = pg_cls.from_dataset(g)
    dead = pg.optimize()
    pg.set_poses(g.ground_truth)
    truth = pg.optimize()
    assert _lib.STOP_REASONS[truth["stop_reason"]] == "converged"
    pg.set_poses(g.initial)
    init = pg.initialize_linear()
    st = pg.optimize()
    print(f"C2: init {init['error_before']:.6g} -> {init['error_after']:.6g}; LM {st['final_error']:.10g} in "
          f"{st['inner_iterations']} tries; from truth {truth['final_error']:.10g}; from dead reckoning "
          f"{dead['final_error']:.6g} in {dead['inner_iterations']} tries")
    assert _lib.STOP_REASONS[st["stop_reason"]] == "converged"     # PGO_STOP_CONVERGED
    assert abs(st["final_error"] - truth["final_error"]) <= 1e-5 * truth["final_error"]
    assert st["inner_iterations"] <= dead["inner_iterations"]
    assert st["initial_error"] == init["error_after"]


# -------------------------------------------------------------- 6. mirrors
def test_gtsam_lago_mirror(pg_cls):
    from graphslam_amd import gtsam as gt
    g = it.square_turn()
    pg = pg_cls.from_dataset(g)
    pg.initialize_linear()
    graph_, values = gt.NonlinearFactorGraph(), gt.Values()
    for k, p in zip(g.keys, g.initial):
        values.insert(int(k), gt.Pose2(*p))
    for k, p, c in zip(g.prior_keys, g.prior_pose, g.prior_cov):
        graph_.add(gt.PriorFactorPose2(int(k), gt.Pose2(*p), gt.noiseModel.Gaussian.Covariance(c.reshape(3, 3))))
    for a, b, z, c in zip(g.edge_k1, g.edge_k2, g.edge_z, g.edge_cov):
        graph_.add(gt.BetweenFactorPose2(int(a), int(b), gt.Pose2(*z), gt.noiseModel.Gaussian.Covariance(c.reshape(3, 3))))
    out = gt.lago.initialize(graph_, values)
    assert out.keys() == values.keys()
    assert np.array_equal(out.as_array(), pg.poses())


LAGO_CPP_STYLE = r'''
// lago::initialize ahead of the optimiser (INTEGRATION.md), written against
// include/pgo_gtsam.hpp: a 2 m square, odometry and one closure.
#include <cstdio>
#include "pgo_gtsam.hpp"
using namespace pgo_gtsam;
int main() {
  NonlinearFactorGraph graph;
  Values initial;
  Matrix3 Q = Matrix3::Zero();
  Q(0, 0) = 0.1 * 0.1; Q(1, 1) = 0.1 * 0.1; Q(2, 2) = 0.1 * 0.1;
  graph.add(PriorFactor<Pose2>(1, Pose2(0, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  initial.insert(1, Pose2(5, 5, 1));
  Matrix3 R = Matrix3::Zero();
  R(0, 0) = R(1, 1) = 0.0025; R(2, 2) = 7.6e-5;
  for (Key k = 2; k <= 8; k++) {
    initial.insert(k, Pose2(-3.0 * k, 2.0 * k, 0.5 * k));   // only the keys matter
    const bool turn = (k % 2) == 1;
    graph.add(BetweenFactor<Pose2>(k - 1, k, Pose2(1.0, 0, turn ? 1.5707963267948966 : 0.0),
                                   noiseModel::Gaussian::Covariance(R)));
  }
  graph.add(BetweenFactor<Pose2>(8, 1, Pose2(1.0, 0, 1.5707963267948966), noiseModel::Gaussian::Covariance(R)));
  try {
    const Values start = lago::initialize(graph, initial);
    for (Key k = 1; k <= 8; k++)
      std::printf("%llu %.12f %.12f %.12f\n", (unsigned long long)k, start.at<Pose2>(k).x(), start.at<Pose2>(k).y(),
                  start.at<Pose2>(k).theta());
    LevenbergMarquardtOptimizer optimizer(graph, start);
    optimizer.optimize();
    std::printf("error %.3e\n", optimizer.error());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
    return 3;
  }
  return 0;
}
'''


def test_cpp_lago_mirror(tmp_path, pg_cls):
    src = tmp_path / "lago_style.cpp"
    src.write_text(LAGO_CPP_STYLE)
    exe = tmp_path / "lago_style"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[:8]])
    # the measurements are exact: the square's corners, every side two steps
    th = np.pi / 2
    want = np.array([[0, 0, 0], [1, 0, 0], [2, 0, th], [2, 1, th], [2, 2, 2 * th], [1, 2, 2 * th], [0, 2, -th],
                     [0, 1, -th]])
    assert np.abs(got[:, :2] - want[:, :2]).max() <= 1e-9
    assert angdiff(got[:, 2], want[:, 2]).max() <= 1e-9
    assert lines[8].startswith("error ") and float(lines[8].split()[1]) <= 1e-12
