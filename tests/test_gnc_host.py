"""Fixed weights and graduated non-convexity without a GPU: the argument checks
of pgo_set_edge_weights / pgo_optimize_gnc, the weight formulas and the outer
loop's control against the numpy twin (tests/gnc_twin.py), the twin against
itself, the stand-alone sanitizer self-test of the host module, the symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gnc_twin as gt
from graphslam_amd import _lib, datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = gt.CHI2_99_3
MUS = (1e-6, 1.0, 1.4, 1e6)


@pytest.fixture(scope="module")
def pgm(pgo_lib):
    from graphslam_amd import pose_graph
    return pose_graph


def _small(pgm, loss=None):
    g = datasets.square_loop()
    if loss is not None:
        g.edge_loss = np.zeros(g.num_edges, np.int32)
        g.edge_loss[-1] = loss
        g.edge_loss_k = np.ones(g.num_edges)
    return g, pgm.PoseGraph.from_dataset(g)


def _status(pgm, fn, *a, **kw):
    with pytest.raises(pgm.PgoError) as ei:
        fn(*a, **kw)
    return ei.value.status


# ------------------------------------------------------------ argument checks
def test_set_edge_weights_argument_checks(pgm):
    g, pg = _small(pgm)
    E = g.num_edges
    for bad in (-1e-300, 1.0 + 1e-15, math.nan, math.inf, -math.inf):
        assert _status(pgm, pg.set_edge_weights, [0.5, bad]) == _lib.PGO_E_ARG
    assert _status(pgm, pg.set_edge_weights, np.ones(E + 1)) == _lib.PGO_E_ARG       # range past the last factor
    assert _status(pgm, pg.set_edge_weights, [1.0], first=E) == _lib.PGO_E_ARG
    assert _status(pgm, pg.set_edge_weights, [1.0], first=E + 5) == _lib.PGO_E_ARG
    pg.set_edge_weights([], first=E)                                                  # empty range at the end: fine
    pg.set_edge_weights([0.0, 1.0, 0.25])                                             # the closed interval
    pg.set_edge_weights(np.ones(E))
    assert np.array_equal(pg.edge_weights(), np.ones(E))                              # (all 1: no device needed)
    # a factor under a loss takes no fixed weight, wherever it sits in the range
    g2, pg2 = _small(pgm, loss=_lib.PGO_LOSS_HUBER)
    assert _status(pgm, pg2.set_edge_weights, np.ones(g2.num_edges)) == _lib.PGO_E_ARG
    assert _status(pgm, pg2.set_edge_weights, [0.5], first=g2.num_edges - 1) == _lib.PGO_E_ARG
    assert pgo_rc_null(pgm)


def pgo_rc_null(pgm):
    L = _lib.lib()
    w = np.ones(1)
    return (L.pgo_set_edge_weights(None, 0, 1, _lib.dptr(w)) == _lib.PGO_E_ARG
            and L.pgo_optimize_gnc(None, None, None, 0, None, None) == _lib.PGO_E_ARG
            and L.pgo_get_gnc_trace(None, None, 0) == _lib.PGO_E_ARG)


def test_loss_four_stays_internal(pgm):
    """The fixed-weight kind is internal: the public entry rejects loss 4."""
    g, pg = _small(pgm)
    cov = np.diag([0.01] * 3)
    assert _status(pgm, pg.add_edge, 1, 3, [1, 0, 0], cov, loss=4, k=0.5) == _lib.PGO_E_ARG


@pytest.mark.parametrize("field,value", [("loss", 2), ("loss", -1), ("barc_sq", 0.0), ("barc_sq", -1.0),
                                         ("barc_sq", math.nan), ("mu_step", 1.0), ("mu_step", 0.5),
                                         ("mu_step", math.inf), ("max_iterations", -1),
                                         ("relative_cost_tol", -1e-9), ("relative_cost_tol", math.nan),
                                         ("weights_tol", -1e-9), ("weights_tol", math.inf)])
def test_gnc_bad_params(pgm, field, value):
    g, pg = _small(pgm)
    gp = pgm.default_gnc_params()
    setattr(gp, field, value)
    assert _status(pgm, pg.optimize_gnc, gnc=gp) == _lib.PGO_E_ARG
    assert pg.last_gnc_stats["status"] == _lib.PGO_E_ARG
    # the control's own entry rejects the same
    mu, stop = np.zeros(2), C.c_int(0)
    a = np.ones(2)
    assert _lib.lib().pgo_debug_gnc_control(C.byref(gp), 1.0, 2, _lib.dptr(a), _lib.dptr(a), _lib.dptr(a),
                                            _lib.dptr(mu), C.byref(stop)) == _lib.PGO_E_ARG


def test_gnc_argument_checks(pgm):
    g, pg = _small(pgm)
    E = g.num_edges
    assert _status(pgm, pg.optimize_gnc, candidates=[0, E]) == _lib.PGO_E_ARG          # index past the end
    assert _status(pgm, pg.optimize_gnc, candidates=[1, 2, 1]) == _lib.PGO_E_ARG       # duplicate
    # a candidate under a loss, and any factor under a loss
    g2, pg2 = _small(pgm, loss=_lib.PGO_LOSS_CAUCHY)
    assert _status(pgm, pg2.optimize_gnc, candidates=[g2.num_edges - 1]) == _lib.PGO_E_ARG
    assert _status(pgm, pg2.optimize_gnc, candidates=[0]) == _lib.PGO_E_ARG
    assert _status(pgm, pg2.optimize_gnc) == _lib.PGO_E_ARG
    # more than one rank: one rank only
    comm = _lib.PgoHostComm()
    comm.rank, comm.size = 0, 2
    comm.allgather = _lib.ALLGATHER_FN(lambda ctx, i, o, n: 0)
    comm.broadcast = _lib.BROADCAST_FN(lambda ctx, b, n, r: 0)
    pg.comm_init_host(comm)
    assert _status(pgm, pg.optimize_gnc) == _lib.PGO_E_ARG
    pg.comm_free()
    # the defaults
    gp = pgm.default_gnc_params()
    assert (gp.loss, gp.barc_sq, gp.mu_step, gp.max_iterations) == (0, C2, 1.4, 100)
    assert (gp.relative_cost_tol, gp.weights_tol, gp.keep_weights) == (1e-5, 1e-4, 1)
    assert pg.gnc_trace().shape == (0, 8)
    assert _lib.lib().pgo_debug_gnc_weight(2, 1.0, C2, 0, None, None) == _lib.PGO_E_ARG


# ------------------------------------------------------------------- weights
def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("loss", [gt.GM, gt.TLS])
def test_weight_matches_twin(pgm, loss, mu):
    lo, up = gt.tls_bounds(np.float64(mu), np.float64(C2))
    r2 = np.array([0.0, lo, up, np.nextafter(lo, 0), np.nextafter(lo, np.inf), np.nextafter(up, 0),
                   np.nextafter(up, np.inf), 1e300, 0.5 * (lo + up), C2, 1e-300, mu * C2])
    w = pgm.debug_gnc_weight(loss, mu, C2, r2)
    ref = gt.weight(loss, mu, C2, r2)
    assert np.all(np.isfinite(w)) and w.min() >= 0.0 and w.max() <= 1.0 + 4e-10 * (1 + mu)
    assert _ulps(w, ref).max() <= 2, (w, ref)
    if loss == gt.TLS:
        assert np.array_equal(w[r2 <= lo], np.ones((r2 <= lo).sum()))      # exactly 1 up to lo
        assert np.array_equal(w[r2 >= up], np.zeros((r2 >= up).sum()))     # exactly 0 from up on
        assert 0.0 < w[8] < 1.0
    else:
        assert w[0] == 1.0 and w[7] == 0.0 and abs(w[11] - 0.25) <= 1e-15


def test_weight_random_against_twin(pgm):
    rng = np.random.default_rng(5)
    r2 = np.exp(rng.uniform(-20, 20, 4000))
    for loss in (gt.GM, gt.TLS):
        for mu in MUS:
            assert _ulps(pgm.debug_gnc_weight(loss, mu, C2, r2), gt.weight(loss, mu, C2, r2)).max() <= 2


# ------------------------------------------------------------------- control
def _replay_both(pgm, p, rmax, cost, nb):
    gp = pgm.default_gnc_params(loss=p.loss, barc_sq=p.barc_sq, mu_step=p.mu_step, max_iterations=p.max_iterations,
                                relative_cost_tol=p.relative_cost_tol, weights_tol=p.weights_tol)
    mu, stop, n = pgm.debug_gnc_control(rmax, cost, nb, params=gp)
    mu_t, stop_t, n_t = gt.control_replay(p, rmax, cost, nb)
    assert n == n_t and stop == stop_t
    assert np.array_equal(mu, mu_t, equal_nan=True)          # the same arithmetic: equal as doubles
    return mu, stop, n


def test_control_matches_twin(pgm):
    rng = np.random.default_rng(11)
    R = 60
    for loss in (gt.GM, gt.TLS):
        for trial in range(40):
            p = gt.GncParams(loss=loss, mu_step=float(rng.choice([1.1, 1.4, 2.0, 7.3])),
                             max_iterations=int(rng.choice([0, 1, 5, 100])),
                             relative_cost_tol=float(rng.choice([0.0, 1e-5, 1e-2])))
            rmax = np.concatenate([[C2 * float(np.exp(rng.uniform(-2, 8)))], rng.uniform(0, 100, R - 1)])
            cost = 100.0 * np.cumprod(np.concatenate([[1.0], 1.0 - rng.choice([0.0, 1e-6, 0.05, 0.2], R - 1)]))
            nb = np.concatenate([[0.0], rng.integers(0, 3, R - 1) * (np.arange(R - 1) < rng.integers(1, R))])
            _replay_both(pgm, p, rmax, cost, nb.astype(np.float64))


def test_control_schedules_and_stops(pgm):
    ones, zeros = np.ones(40), np.zeros(40)
    # GM from mu0 = 100 down to exactly 1 in 15 solves
    mu, stop, n = _replay_both(pgm, gt.GncParams(), np.full(40, 50 * C2), 100.0 * 0.9 ** np.arange(40), zeros)
    assert stop == gt.STOP_MU and n == 16 and mu[-1] == 1.0
    assert mu[1] == 2.0 * (50 * C2) / C2 and abs(mu[1] - 100.0) < 1e-12 and mu[2] == mu[1] / 1.4
    # the cost rule; rows running out
    _, stop, n = _replay_both(pgm, gt.GncParams(), np.full(4, 50 * C2), np.array([10.0, 9.0, 8.0, 8.0]), zeros[:4])
    assert stop == gt.STOP_COST and n == 4
    _, stop, n = _replay_both(pgm, gt.GncParams(), np.full(2, 50 * C2), np.array([10.0, 9.0]), zeros[:2])
    assert stop == -1 and n == 2
    # TLS: mu grows by mu_step until no weight is non-binary
    nb = np.array([0, 5, 3, 1, 0, 0], dtype=np.float64)
    mu, stop, n = _replay_both(pgm, gt.GncParams(loss=gt.TLS), np.full(6, 3 * C2), 10.0 * 0.8 ** np.arange(6), nb)
    assert stop == gt.STOP_MU and n == 5 and mu[1] == C2 / (2 * 3 * C2 - C2) and mu[2] == mu[1] * 1.4
    # max_iterations, 0 included
    _, stop, n = _replay_both(pgm, gt.GncParams(max_iterations=3), np.full(9, 50 * C2), 10.0 * 0.8 ** np.arange(9),
                              zeros[:9])
    assert stop == gt.STOP_MAX_ITER and n == 4
    _, stop, n = _replay_both(pgm, gt.GncParams(max_iterations=0), ones[:3] * 50 * C2, ones[:3], zeros[:3])
    assert stop == gt.STOP_MAX_ITER and n == 1


@pytest.mark.parametrize("rmax", [0.0, 0.25 * C2, 0.5 * C2, math.nan, math.inf])
def test_control_degenerate_starts(pgm, rmax):
    """TLS with no residual beyond the threshold (mu not positive or not finite)
    stops ALL_INLIERS after row 0; GM starts at mu = 1 there and runs one solve."""
    r = np.array([rmax, 0.0, 0.0])
    cost, nb = np.array([5.0, 4.0, 3.0]), np.zeros(3)
    _, stop, n = _replay_both(pgm, gt.GncParams(loss=gt.TLS), r, cost, nb)
    assert stop == gt.STOP_ALL_INLIERS and n == 1
    if math.isfinite(rmax):
        mu, stop, n = _replay_both(pgm, gt.GncParams(), r, cost, nb)
        assert stop == gt.STOP_MU and n == 2 and mu[1] == 1.0


# ----------------------------------------------------------- the twin itself
def test_twin_rejects_the_corrupted_closures():
    """manhattan(120, 6, 180) with 20 % of its loop closures replaced, from dead
    reckoning: TLS ends binary with every replaced closure at weight 0 (and one
    true closure beyond the threshold with them), GM's weights separate the two
    classes, both beat the plain solve."""
    g, bad, lc = gt.corrupted(120, 6, 180, 2001, 0.2)
    assert len(bad) >= 5
    plain = pn_lm(g)
    good = np.setdiff1d(lc, bad)
    for loss in (gt.GM, gt.TLS):
        r = gt.optimize(g, lc, gt.GncParams(loss=loss))
        assert r.stop_reason in (gt.STOP_MU, gt.STOP_COST) and r.outer_iterations >= 2
        assert gt.rmse(r.xyt(), g) < 0.5 * gt.rmse(plain.xyt(), g)
        assert r.weights[bad].max() < 0.05
        assert set(bad) <= set(r.outliers)
        assert np.array_equal(r.weights[np.setdiff1d(np.arange(g.num_edges), lc)],
                              np.ones(g.num_edges - len(lc)))
        if loss == gt.TLS:
            assert np.array_equal(r.weights[bad], np.zeros(len(bad)))
            assert np.all((r.weights[good] == 0.0) | (r.weights[good] == 1.0)) and (r.weights[good] == 0).sum() <= 1
            assert np.isfinite(r.weight_distance)
        else:
            assert r.weights[bad].max() < r.weights[good].min()
        assert np.isnan(r.rows[0, 0]) and r.rows[0, 2] == len(lc) and len(r.rows) == r.outer_iterations + 1


def pn_lm(g):
    from oracle import pgo_numpy as pn
    return pn.levenberg_marquardt(pn.problem_from_graph(g), pn.from_xyt(g.initial))


def test_twin_degenerate_runs():
    g = datasets.square_loop()
    r = gt.optimize(g, None, gt.GncParams(loss=gt.TLS))
    assert r.stop_reason == gt.STOP_ALL_INLIERS and r.outer_iterations == 0 and np.all(r.weights == 1.0)
    r = gt.optimize(g, [])
    plain = pn_lm(g)
    assert r.stop_reason == gt.STOP_NO_CANDIDATES and np.array_equal(r.poses, plain.poses)


# --------------------------------------------------------- module and symbols
def test_gnc_host_module_under_asan_ubsan():
    """pgo_gnc.cpp / pgo_gnc.h driven by gnc_selftest.cpp under ASan + UBSan: a
    stand-alone host program, nothing preloaded."""
    b = subprocess.run(["make", "-s", "-C", "graphslam_amd/csrc", "asan-gnc"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "graphslam_amd", "csrc", "build", "gnc_selftest_asan")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "gnc selftest ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_symbols_declared_and_bound(pgo_lib):
    names = {"pgo_set_edge_weights", "pgo_gnc_default_params", "pgo_optimize_gnc", "pgo_get_gnc_trace",
             "pgo_debug_gnc_control", "pgo_debug_gnc_weight", "pgo_debug_gnc_sweep"}
    assert names <= set(_lib.declared_symbols())
    for n in names:
        assert getattr(pgo_lib, n).argtypes is not None
    assert pgo_lib.pgo_abi_version() == 6
    assert C.sizeof(_lib.PgoGncParams) == 56 and C.sizeof(_lib.PgoGncStats) == 96


# ------------------------------------------------------------------- mirrors
def test_gtsam_mirror_host_side(pgo_lib):
    from graphslam_amd import gtsam as gs
    p = gs.GncLMParams()
    p.setLossType(gs.GncLossType.TLS)
    p.setKnownInliers([2, 0])
    p.setMuStep(2.0)
    p.setMaxIterations(7)
    p.setRelativeCostTol(1e-4)
    p.setWeightsTol(1e-3)
    r = p.raw
    assert (r.loss, r.mu_step, r.max_iterations, r.relative_cost_tol, r.weights_tol) == (1, 2.0, 7, 1e-4, 1e-3)
    assert p.known_inliers == [0, 2] and r.barc_sq == C2 and gs.GncLossType.GM == 0
    graph = gs.NonlinearFactorGraph()
    noise = gs.noiseModel.Gaussian.Covariance(np.diag([0.01, 0.01, 0.01]))
    graph.add(gs.PriorFactorPose2(1, gs.Pose2(0, 0, 0), noise))
    graph.add(gs.BetweenFactorPose2(1, 2, gs.Pose2(1, 0, 0), noise))
    v = gs.Values()
    v.insert(1, gs.Pose2(0, 0, 0))
    v.insert(2, gs.Pose2(1, 0, 0))
    opt = gs.GncLMOptimizer(graph, v, p)
    assert np.array_equal(opt.getWeights(), np.ones(2))
    robust = gs.noiseModel.Robust.Create(gs.noiseModel.mEstimator.Huber.Create(1.0), noise)
    graph.add(gs.BetweenFactorPose2(2, 1, gs.Pose2(-1, 0, 0), robust))
    with pytest.raises(ValueError):
        gs.GncLMOptimizer(graph, v, p)


GNC_CPP = r'''
#include <cstdio>
#include "pgo_gtsam.hpp"
using namespace pgo_gtsam;
int main() {
  NonlinearFactorGraph graph;
  Values initial;
  Matrix3 Q = Matrix3::Zero();
  Q(0, 0) = Q(1, 1) = Q(2, 2) = 0.01;
  graph.add(PriorFactor<Pose2>(1, Pose2(0, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  for (Key k = 1; k <= 4; k++) initial.insert(k, Pose2(double(k - 1), 0, 0));
  for (Key k = 1; k < 4; k++)
    graph.add(BetweenFactor<Pose2>(k, k + 1, Pose2(1, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  graph.add(BetweenFactor<Pose2>(4, 1, Pose2(5, 5, 1), noiseModel::Gaussian::Covariance(Q)));   // a wrong closure
  GncLMParams params;
  params.setLossType(GncLossType::TLS);
  params.setKnownInliers({0, 1, 2});
  params.setMuStep(1.4);
  params.setMaxIterations(50);
  params.setRelativeCostTol(1e-5);
  params.setWeightsTol(1e-4);
  if (params.g.loss != PGO_GNC_TLS || params.knownInliers.size() != 3) return 2;
  try {
    GncLMOptimizer opt(graph, initial, params);
    Values out = opt.optimize();
    const std::vector<double>& w = opt.getWeights();
    std::printf("weights %zu %.3f %.3f stop %d x4 %.6f\n", w.size(), w[0], w[3], opt.stats().stop_reason,
                out.at<Pose2>(4).x());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
  }
  return 0;
}
'''


def test_cpp_adapter_gnc_compiles_and_runs_host_side(tmp_path, pgo_lib):
    src = tmp_path / "gnc_style.cpp"
    src.write_text(GNC_CPP)
    exe = tmp_path / "gnc_style"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # no GPU here: the optimiser reports it instead of falling back to the CPU; with
    # one, TLS drops the wrong closure and keeps the chain
    assert ("runtime_error" in r.stdout and "device" in r.stdout) or \
        r.stdout.startswith("weights 4 1.000 0.000 stop 0 x4 3.0000")
