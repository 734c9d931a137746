"""Robust losses (Huber, Cauchy, Geman-McClure) on between factors, without a
GPU: the numpy twin tests/robust_twin.py checks itself, shows what the losses
buy on a graph with wrong loop closures, and the host side of the C-ABI and of
the GTSAM-named mirrors accepts and validates the new arguments."""
import os
import re
import subprocess

import numpy as np
import pytest

import robust_twin as rt
from graphslam_amd import _lib, datasets
from oracle import pgo_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = np.diag([0.0025, 0.0025, 7.6e-5])


# ------------------------------------------------------------ the twin
@pytest.mark.parametrize("loss,k", [(rt.HUBER, 1.345), (rt.CAUCHY, 1.0), (rt.GEMAN_MCCLURE, 2.0), (rt.NONE, 1.0)])
def test_twin_gradient_is_derivative_of_rho(loss, k):
    """w = rho' / r: the twin's weighted gradient g = J' (w Omega) e equals a
    central finite difference of sum rho in the tangent space (retract), 1e-6
    relative, on square_loop with two corrupted edges (residuals far into the
    tails, others inside the quadratic zone).  GTSAM's BetweenFactor Jacobian
    (no Hlocal, restated by the oracle) is the exact derivative of the residual
    only where the angular residual vanishes, so the edges are corrupted in
    translation and the evaluation point keeps the true headings: there the
    check isolates the weight."""
    g = datasets.square_loop()
    g.edge_z = g.edge_z.copy()
    g.edge_z[3] += [0.8, -0.5, 0.0]
    g.edge_z[11] += [-1.5, 0.7, 0.0]
    rp = rt.problem(g, loss, k)
    xyt = g.ground_truth.copy()
    xyt[:, :2] += 0.2 * (g.initial[:, :2] - g.ground_truth[:, :2])   # some residuals inside r < k
    x = pn.from_xyt(xyt)
    r2, _, _ = rt.r_squared(rp, x)
    if loss == rt.HUBER:
        assert (np.sqrt(r2) > k).any() and (np.sqrt(r2) < k).any()   # both branches
    _, lin = rt.linearize(rp, x)
    h = 1e-6
    fd = np.zeros(3 * g.num_poses)
    for a in range(fd.size):
        d = np.zeros(fd.size)
        d[a] = h
        fd[a] = (rt.error(rp, pn.retract(x, d.reshape(-1, 3))) - rt.error(rp, pn.retract(x, -d.reshape(-1, 3)))) / (2 * h)
    assert np.abs(fd - lin.g).max() <= 1e-6 * np.abs(lin.g).max()


def test_twin_weights_and_rho_formulas():
    r = np.array([0.0, 0.5, 1.0, 2.0, 10.0])
    assert np.array_equal(rt.weight(rt.NONE, 1.0, r * r), np.ones(5))
    assert np.allclose(rt.weight(rt.HUBER, 1.0, r * r), [1, 1, 1, 0.5, 0.1])
    assert np.allclose(rt.weight(rt.CAUCHY, 2.0, r * r), 1 / (1 + r * r / 4))
    assert np.allclose(rt.weight(rt.GEMAN_MCCLURE, 2.0, r * r), 16 / (4 + r * r) ** 2)
    assert np.allclose(rt.rho(rt.HUBER, 1.0, r * r), [0, 0.125, 0.5, 1.5, 9.5])
    assert np.allclose(rt.rho(rt.CAUCHY, 2.0, r * r), 2 * np.log1p(r * r / 4))
    assert np.allclose(rt.rho(rt.GEMAN_MCCLURE, 2.0, r * r), 2 * r * r / (4 + r * r))


@pytest.fixture(scope="module")
def outlier_runs():
    """The Gaussian and the Huber(1.345)-on-loop-closures twin runs on the graph
    with 10 % wrong loop closures, from the dead-reckoned start (shared)."""
    g, bad, lc = rt.outlier_graph()
    x0 = pn.from_xyt(g.initial)
    gauss, _ = rt.levenberg_marquardt(rt.problem(g, 0, 1.0), x0)
    rp = rt.problem(rt.with_loss_on(g, lc, rt.HUBER, 1.345))
    huber, margin = rt.levenberg_marquardt(rp, x0)
    return g, bad, rp, gauss, huber, margin


def _rmse(g, res):
    return float(np.sqrt(np.mean(np.sum((res.xyt()[:, :2] - g.ground_truth[:, :2]) ** 2, axis=1))))


def test_twin_shows_the_benefit(outlier_runs):
    """manhattan(1000, 16, 1500, seed=2001), 50 of 501 loop closures replaced by
    random poses: Huber(1.345) on the loop closures gives a position RMSE below
    a quarter of the Gaussian run's (measured 0.088 m against 2.148 m) and every
    corrupted edge ends with weight < 0.1 (measured maximum 0.016)."""
    g, bad, rp, gauss, huber, _ = outlier_runs
    assert len(bad) == 50
    print("rmse gauss", _rmse(g, gauss), "huber", _rmse(g, huber))
    assert _rmse(g, huber) < 0.25 * _rmse(g, gauss)
    w = rt.weights(rp, huber.poses)
    print("max weight of a corrupted edge", w[bad].max())
    assert w[bad].max() < 0.1
    assert np.array_equal(w[rp.loss == 0], np.ones((rp.loss == 0).sum()))


@pytest.mark.parametrize("loss,k", [(rt.HUBER, 1.345), (rt.CAUCHY, 1.0)])
def test_twin_trajectory_decision_margins(loss, k):
    """The LM-trajectory GPU test compares decisions (accepted, lambda, stop)
    with the twin's; that is sound only if no decision quantity sits at its
    threshold.  Over the twin's whole trajectory the closest one is 29 % away
    (Huber) / 9.4 % (Cauchy); at least 1 % is required of the input."""
    g, _, lc = rt.outlier_graph()
    rp = rt.problem(rt.with_loss_on(g, lc, loss, k))
    res, margin = rt.levenberg_marquardt(rp, pn.from_xyt(g.initial))
    print("iterations", res.iterations, "margin", margin)
    assert margin >= 0.01


def test_corrupt_loop_closures_is_seeded_and_leaves_the_rest():
    g0 = datasets.manhattan(1000, 16, 1500, seed=2001)
    g1 = datasets.manhattan(1000, 16, 1500, seed=2001)
    bad = datasets.corrupt_loop_closures(g1, 0.1, 2008)
    lc = datasets.loop_closure_indices(g1)
    assert len(lc) == 501 and len(bad) == 50 and np.isin(bad, lc).all()
    keep = np.setdiff1d(np.arange(g0.num_edges), bad)
    assert np.array_equal(g0.edge_z[keep], g1.edge_z[keep]) and not np.allclose(g0.edge_z[bad], g1.edge_z[bad])
    g2 = datasets.manhattan(1000, 16, 1500, seed=2001)
    assert np.array_equal(datasets.corrupt_loop_closures(g2, 0.1, 2008), bad) and np.array_equal(g2.edge_z, g1.edge_z)
    assert g0.edge_loss is None and g0.edge_loss_k is None


# ------------------------------------------------------------ host side / ABI
def test_symbols_and_constants(pgo_lib):
    syms = _lib.declared_symbols()
    new = {"pgo_add_edge_robust", "pgo_add_edges_robust", "pgo_get_edge_weights"}
    assert new <= set(syms)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert new <= set(re.findall(r"\bT (pgo_\w+)", out))
    for name in new:
        assert getattr(pgo_lib, name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "pgo.h")).read()
    defs = dict(re.findall(r"#define (PGO_LOSS_\w+) (\d+)", text))
    assert defs == {"PGO_LOSS_NONE": "0", "PGO_LOSS_HUBER": "1", "PGO_LOSS_CAUCHY": "2", "PGO_LOSS_GEMAN_MCCLURE": "3"}
    for name, val in defs.items():
        assert getattr(_lib, name) == int(val)
    assert (rt.NONE, rt.HUBER, rt.CAUCHY, rt.GEMAN_MCCLURE) == (0, 1, 2, 3)
    assert pgo_lib.pgo_abi_version() == 6


def test_loss_argument_checks(pgo_lib):
    from graphslam_amd.pose_graph import PgoError, PoseGraph
    pg = PoseGraph()
    pg.add_vertices(np.array([1, 2, 3], dtype=np.uint64), np.zeros((3, 3)))
    for loss, k in [(4, 1.0), (-1, 1.0), (_lib.PGO_LOSS_HUBER, 0.0), (_lib.PGO_LOSS_CAUCHY, -2.0),
                    (_lib.PGO_LOSS_GEMAN_MCCLURE, float("nan")), (_lib.PGO_LOSS_HUBER, float("inf")),
                    (_lib.PGO_LOSS_NONE, float("nan"))]:
        with pytest.raises(PgoError) as ei:
            pg.add_edge(1, 2, [1, 0, 0], DIAG, loss=loss, k=k)
        assert ei.value.status == _lib.PGO_E_ARG, (loss, k)
    assert pg.num_factors == 0
    with pytest.raises(PgoError) as ei:   # a bad entry anywhere in a per-edge array: nothing is added
        pg.add_edges([1, 2], [2, 3], np.zeros((2, 3)) + [1, 0, 0], DIAG.ravel(), loss=[1, 7], k=[1.0, 1.0])
    assert ei.value.status == _lib.PGO_E_ARG and pg.num_factors == 0
    with pytest.raises(ValueError):
        pg.add_edge(1, 2, [1, 0, 0], DIAG, loss="tukey", k=1.0)
    pg.add_edge(1, 2, [1, 0, 0], DIAG, loss=_lib.PGO_LOSS_NONE, k=0.0)      # k is unused with NONE
    pg.add_edge(2, 3, [1, 0, 0], DIAG, loss="huber", k=1.345)
    pg.add_edges([1, 2], [3, 1], np.zeros((2, 3)) + [1, 0, 0], DIAG.ravel(), loss="cauchy", k=1.0)
    pg.add_edges([1, 2], [3, 1], np.zeros((2, 3)) + [1, 0, 0], DIAG.ravel(), loss=[0, 3], k=[1.0, 2.0])
    pg.add_edges([3], [1], [[1, 0, 0]], DIAG.ravel())
    pg.add_prior(1, [0, 0, 0], np.diag([0.01] * 3))
    assert pg.num_factors == 8
    with pytest.raises(PgoError) as ei:
        pg.edge_weights(first=5, n=4)                                       # past the 7 between factors
    assert ei.value.status == _lib.PGO_E_ARG
    pg.close()
    plain = PoseGraph()                                                     # all Gaussian: every weight is 1
    plain.add_vertices(np.array([1, 2], dtype=np.uint64), np.zeros((2, 3)))
    plain.add_edge(1, 2, [1, 0, 0], DIAG)
    assert np.array_equal(plain.edge_weights(), [1.0])
    plain.close()


def test_from_dataset_honours_edge_loss(pgo_lib):
    from graphslam_amd.pose_graph import PgoError, PoseGraph
    g = datasets.square_loop()
    g.edge_loss = np.full(g.num_edges, 9, dtype=np.int32)
    g.edge_loss_k = 1.0
    with pytest.raises(PgoError):
        PoseGraph.from_dataset(g)
    g.edge_loss = _lib.PGO_LOSS_HUBER
    pg = PoseGraph.from_dataset(g)
    assert pg.num_factors == g.num_edges + 1
    pg.close()


def test_gtsam_mirror_robust_models(pgo_lib):
    from graphslam_amd import gtsam as gt
    Q = np.diag([0.01, 0.01, 0.001])
    rob = gt.noiseModel.Robust.Create(gt.noiseModel.mEstimator.Huber.Create(1.345), gt.noiseModel.Gaussian.Covariance(Q))
    assert rob.robust.loss == _lib.PGO_LOSS_HUBER and rob.robust.k == 1.345 and np.array_equal(rob.covariance, Q)
    assert gt.noiseModel.mEstimator.Cauchy.Create(1.0).loss == _lib.PGO_LOSS_CAUCHY
    assert gt.noiseModel.mEstimator.GemanMcClure.Create(2.0).loss == _lib.PGO_LOSS_GEMAN_MCCLURE
    with pytest.raises(ValueError):
        gt.noiseModel.mEstimator.Huber.Create(0.0)
    with pytest.raises(TypeError):
        gt.noiseModel.Robust.Create(1.345, gt.noiseModel.Gaussian.Covariance(Q))
    graph = gt.NonlinearFactorGraph()
    graph.add(gt.BetweenFactorPose2(1, 2, gt.Pose2(1, 0, 0), rob))
    with pytest.raises(TypeError, match="robust"):
        gt.PriorFactorPose2(1, gt.Pose2(0, 0, 0), rob)
    assert graph.nrFactors() == 1
    v = gt.Values()
    v.insert(1, gt.Pose2(0, 0, 0))
    v.insert(2, gt.Pose2(1, 0, 0))
    h = gt._build(graph, v)                       # the model reaches the handle (host side only)
    assert h.pg.num_factors == 1
    h.pg.close()


C_CONSUMER = r'''
#include <math.h>
#include <stdio.h>
#include "pgo.h"
int main(void) {
  pgo_graph *g = pgo_create(NULL);
  double cov[9] = {0.01,0,0, 0,0.01,0, 0,0,0.01}, z[6] = {1,0,0, 1,0,0};
  uint64_t k1[2] = {1, 2}, k2[2] = {2, 3};
  int loss[2] = {PGO_LOSS_CAUCHY, PGO_LOSS_GEMAN_MCCLURE}, bad[2] = {PGO_LOSS_HUBER, 4};
  double k[2] = {1.0, 2.0};
  if (pgo_add_vertex(g, 1, 0, 0, 0) || pgo_add_vertex(g, 2, 1, 0, 0) || pgo_add_vertex(g, 3, 2, 0, 0)) return 1;
  if (pgo_add_edge_robust(g, 1, 2, z, cov, PGO_LOSS_HUBER, 1.345)) return 2;
  if (pgo_add_edge_robust(g, 1, 2, z, cov, 17, 1.0) != PGO_E_ARG) return 3;
  if (pgo_add_edge_robust(g, 1, 2, z, cov, PGO_LOSS_HUBER, 0.0) != PGO_E_ARG) return 4;
  if (pgo_add_edge_robust(g, 1, 2, z, cov, PGO_LOSS_CAUCHY, NAN) != PGO_E_ARG) return 5;
  if (pgo_add_edges_robust(g, 2, k1, k2, z, cov, 0, loss, k, 1)) return 6;
  if (pgo_add_edges_robust(g, 2, k1, k2, z, cov, 0, loss, k, 0)) return 7;
  if (pgo_add_edges_robust(g, 2, k1, k2, z, cov, 0, bad, k, 1) != PGO_E_ARG) return 8;
  if (pgo_add_edges_robust(g, 2, k1, k2, z, cov, 0, loss, k, 2) != PGO_E_ARG) return 9;
  if (pgo_add_edge(g, 3, 1, z, cov)) return 10;
  if (pgo_num_factors(g) != 6) return 11;
  if (pgo_get_edge_weights(g, 4, 3, k) != PGO_E_ARG) return 12;
  pgo_destroy(g);
  printf("ok %d\n", pgo_abi_version());
  return 0;
}
'''

CPP_CONSUMER = r'''
#include <cstdio>
#include "pgo_gtsam.hpp"
using namespace pgo_gtsam;
int main() {
  NonlinearFactorGraph graph;
  Values initial;
  Matrix3 Q = Matrix3::Zero();
  Q(0, 0) = Q(1, 1) = 0.0025; Q(2, 2) = 7.6e-5;
  graph.add(PriorFactor<Pose2>(1, Pose2(0, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  initial.insert(1, Pose2(0, 0, 0));
  initial.insert(2, Pose2(1, 0, 0));
  auto huber = noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(1.345),
                                          noiseModel::Gaussian::Covariance(Q));
  graph.add(BetweenFactor<Pose2>(1, 2, Pose2(1, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  graph.add(BetweenFactor<Pose2>(2, 1, Pose2(-1, 0, 0), huber));
  graph.add(BetweenFactor<Pose2>(2, 1, Pose2(-1, 0, 0), noiseModel::Robust::Create(
      noiseModel::mEstimator::Cauchy::Create(1.0), noiseModel::Gaussian::Covariance(Q))));
  graph.add(BetweenFactor<Pose2>(2, 1, Pose2(-1, 0, 0), noiseModel::Robust::Create(
      noiseModel::mEstimator::GemanMcClure::Create(2.0), noiseModel::Gaussian::Covariance(Q))));
  const auto& b = graph.betweens();
  if (b[0].loss != PGO_LOSS_NONE || b[1].loss != PGO_LOSS_HUBER || b[1].k != 1.345 || b[2].loss != PGO_LOSS_CAUCHY ||
      b[3].loss != PGO_LOSS_GEMAN_MCCLURE || b[3].k != 2.0)
    return 2;
  std::printf("factors %zu\n", graph.nrFactors());
  try {
    LevenbergMarquardtOptimizer optimizer(graph, initial);
    Values out = optimizer.optimize();
    std::printf("x2 %.9f error %.3e\n", out.at<Pose2>(2).x(), optimizer.error());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
  }
  return 0;
}
'''


def _compile(tmp_path, name, text, cc):
    src = tmp_path / name
    src.write_text(text)
    exe = tmp_path / name.split(".")[0]
    subprocess.run(cc + ["-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe), _lib.LIB_PATH,
                         f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}", "-lm"], check=True)
    return exe


def test_plain_c_consumer_robust(tmp_path, pgo_lib):
    exe = _compile(tmp_path, "use_robust.c", C_CONSUMER, ["gcc", "-std=c99"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok 6"), (r.returncode, r.stdout, r.stderr)


def test_cpp_adapter_consumer_robust(tmp_path, pgo_lib):
    exe = _compile(tmp_path, "graph_robust.cpp", CPP_CONSUMER, ["g++", "-std=c++17"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith("factors 5")
    # no GPU here: the optimiser reports it instead of falling back to the CPU
    assert ("runtime_error" in r.stdout and "device" in r.stdout) or "x2 1.0000" in r.stdout
