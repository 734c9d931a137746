"""PoseGraph.marginal_covariances_all: every pose's covariance and every factor's
cross-covariance from one selected-inversion pass (pgo_marginal_covariances_all).

CPU (unmarked): the float64 restatement of the recurrence
(marginals_all_ref.selinv_emulation) against the longdouble inverse, within
the project's bound 8 max(y, n eps) of a yardstick that does not contain it;
the host side of the binding.

GPU: every designed front case (front_shapes.CASES) against the longdouble
inverse with the emulation added to the yardstick, the benchmark graphs
against the numpy twin at the tolerances of test_marginal_covariances, and
the bitwise properties: the pass only reads the factorisation's workspaces,
so whatever runs after it equals a run without it.

Tolerance of the designed cases: err = max|d - ref| / max|ref| per 3 x 3 pose
block and per 6 x 6 joint block of an edge, err <= 8 max(y, n 2.2e-16), y the
worst of front_shapes.marginals_reference's members (for the checked blocks)
and of the emulation.  Largest err / max(y, n eps) on an MI355X
(profiles/marginals_all_gpu.txt), all under the 8:
  small fronts (m <= 128, w <= 32: cliques, separator leaves)    2.27 (sep30_10x3)
  blocked fronts (cliques 11 .. 256, narrow-under-tall, wide)    2.67 (clique43)
  the multi-level case nested25_30x2_5x2                         6.32 (the per-pose path has 5.79
                                                                 there: the GPU's H is a third rounding of H)
The emulation alone, against a yardstick without it (the CPU test): 0.48, 0.39,
0.19, 0.23 on clique22, sep8_5x4, clique86, nested25_30x2_5x2.
"""
import subprocess

import numpy as np
import pytest

import front_shapes as fs
import marginals_all_ref as mr
from graphslam_amd import _lib, datasets

ALL = [c.name for c in fs.CASES]
EMULATED = ["clique22", "sep8_5x4", "clique86", "nested25_30x2_5x2"]


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


@pytest.fixture(scope="module")
def longdouble():
    eps = np.finfo(np.longdouble).eps
    if not eps < 2e-19:
        pytest.skip(f"np.longdouble is no extended precision here (eps {eps:.3g}): no reference")


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", EMULATED)
def test_emulation_vs_longdouble(pgo_lib, longdouble, name):
    """The recurrence in float64, 64-column blocks and explicit tile inverses
    under the plan's order: every pose block and every edge's joint block
    within the bound of a yardstick made of the other members alone."""
    r = mr.reference(name)
    assert len(r["idx"]) == r["g"].num_poses and len(r["edges"]) == r["g"].num_edges
    n = r["n"]
    worst = 0.0
    for err, y in list(zip(r["emu_pose"], r["y_pose"])) + list(zip(r["emu_edge"], r["y_edge"])):
        worst = max(worst, err / max(y, n * 2.2e-16))
        assert err <= fs.bound(y, n), (name, err, y)
    print(f"marginals_all emulation {name}: n {n} worst err/y {worst:.3f}")


def test_emulation_is_the_inverse():
    """On a small SPD matrix with three blocks of 4: Z H = I."""
    rng = np.random.default_rng(0)
    B = rng.standard_normal((11, 11))
    A = B @ B.T + 11 * np.eye(11)
    p = rng.permutation(11)
    Z = mr.selinv_emulation(fs.GpuScheme(A, p, nb=4))
    assert np.abs(Z @ A - np.eye(11)).max() < 1e-12 and np.array_equal(Z, Z.T)


def test_empty_graph_and_no_device(pgo_lib):
    from graphslam_amd.pose_graph import PgoError, PoseGraph
    with PoseGraph() as pg:
        cov = pg.marginal_covariances_all()
        assert cov.shape == (0, 3, 3)
        cov, cross = pg.marginal_covariances_all(edges=True)
        assert cov.shape == (0, 3, 3) and cross.shape == (0, 3, 3)
    g = datasets.square_loop()
    with PoseGraph.from_dataset(g) as pg:
        try:
            cov, cross = pg.marginal_covariances_all(edges=True)
        except PgoError as e:   # no GPU here: reported, no CPU fall-back
            assert e.status == _lib.PGO_E_NO_DEVICE
        else:
            assert cov.shape == (g.num_poses, 3, 3) and cross.shape == (g.num_edges, 3, 3)


def test_selinv_plan_host_only(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    with PoseGraph.from_dataset(datasets.make("C1")) as pg:
        sp = pg.debug_selinv_plan()
        plan = pg.debug_plan()
    assert sp["launches"] > 0 and sp["flops"] > 0 and sp["workspace_doubles"] > 0
    assert sp["levels"] == int(plan["levels"]) and len(sp["level_launches"]) == sp["levels"]
    assert (sp["level_launches"] > 0).all() and sp["level_launches"].sum() + 1 == sp["launches"]


def test_selinv_plan_counts_blocked_steps(pgo_lib):
    """clique86: one front of 258 columns -> five pivot blocks, each a diagonal
    launch, the four with rows below them a panel and a tile launch too."""
    from graphslam_amd.pose_graph import PoseGraph
    with PoseGraph.from_dataset(fs.build("clique86")) as pg:
        sp = pg.debug_selinv_plan()
    assert sp["levels"] == 1 and sp["launches"] == 1 + 5 + 2 * 4


# ------------------------------------------------------------------ GPU
def _check(tag, got, ref, y, n, worst):
    err = fs.rel_err(got, ref)
    yy = max(y, n * 2.2e-16)
    worst[0] = max(worst[0], err / yy)
    assert err <= fs.bound(y, n), (tag, err, y, err / yy)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_designed_fronts_vs_longdouble(pg_cls, longdouble, name):
    r = mr.reference(name)
    g, idx, n = r["g"], r["idx"], r["n"]
    cov, cross = pg_cls.from_dataset(g).marginal_covariances_all(edges=True)
    assert cov.shape == (g.num_poses, 3, 3) and cross.shape == (g.num_edges, 3, 3)
    assert np.isfinite(cov).all() and np.isfinite(cross).all()
    ref = r["ref"]
    y_pose, y_edge = np.maximum(r["y_pose"], r["emu_pose"]), np.maximum(r["y_edge"], r["emu_edge"])
    ei, ej = g.edge_index()
    wp, we = [0.0], [0.0]
    ep = max([_check(f"{name} pose {i}", cov[i], mr.pose_block(ref, q), float(y_pose[q]), n, wp)
              for q, i in enumerate(idx)], default=0.0)
    ee = max([_check(f"{name} edge {f}", mr.joint_from_parts(cov[ei[f]], cov[ej[f]], cross[f]),
                     mr.joint_block(ref, a, b), float(y_edge[k]), n, we)
              for k, (f, (a, b)) in enumerate(zip(r["edges"], r["eq"]))], default=0.0)
    cls = ",".join(sorted(set(fs.CASE_BY_NAME[name].classes)))
    print(f"marginals_all {name} [{cls}]: n {n} poses {len(idx)} err {ep:.3e} y {y_pose.max():.3e} err/y {wp[0]:.3f}"
          f" | edges {len(r['edges'])} err {ee:.3e} y {y_edge.max(initial=0.0):.3e} err/y {we[0]:.3f}")


def _twin_check(g, pg, prob=None, twin_cov=None):
    """All poses and all cross blocks of the handle against the twin at the
    handle's poses: symmetry 1e-12, 1e-8 relative (test_marginal_covariances);
    the cross blocks relative to the joint block's largest entry."""
    from oracle import pgo_numpy as pn
    import scipy.sparse.linalg as spla
    prob = prob if prob is not None else pn.problem_from_graph(g)
    x = pn.from_xyt(pg.poses())
    n = g.num_poses
    cov, cross = pg.marginal_covariances_all(edges=True)
    ref = (twin_cov or pn.marginal_covariances)(prob, x, list(range(n)))
    for q in range(n):
        assert np.abs(cov[q] - cov[q].T).max() <= 1e-12 * np.abs(cov[q]).max(), q
        assert np.abs(cov[q] - ref[q]).max() <= 1e-8 * np.abs(ref[q]).max(), (q, cov[q], ref[q])
    return cov, cross, x


def _cross_check(prob, x, cov, cross):
    from oracle import pgo_numpy as pn
    import scipy.sparse.linalg as spla
    lu = spla.splu(pn.linearize(prob, x).H.tocsc(), permc_spec="COLAMD")
    inv = lu.solve(np.eye(3 * prob.n))
    for f, (i, j) in enumerate(zip(prob.ei, prob.ej)):
        want = inv[3 * i:3 * i + 3, 3 * j:3 * j + 3]
        scale = max(np.abs(cov[i]).max(), np.abs(cov[j]).max(), np.abs(want).max())
        assert np.abs(cross[f] - want).max() <= 1e-8 * scale, (f, cross[f], want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "C1-nn"])
def test_all_poses_and_edges_at_the_optimum(pg_cls, name):
    from oracle import pgo_numpy as pn
    g = datasets.make(name)
    pg = pg_cls.from_dataset(g)
    pg.optimize()
    cov, cross, x = _twin_check(g, pg)
    _cross_check(pn.problem_from_graph(g), x, cov, cross)


@pytest.mark.gpu
def test_c2_matches_the_per_pose_path(pg_cls):
    """All 10 000 poses against pgo_marginal_covariances on the same handle:
    two results, each within 1e-8 of the truth."""
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    cov = pg.marginal_covariances_all()
    one = pg.marginal_covariances(np.asarray(g.keys))
    scale = np.abs(one).max(axis=(1, 2))
    assert (np.abs(cov - one).max(axis=(1, 2)) <= 2e-8 * scale).all()


@pytest.mark.gpu
def test_two_calls_bitwise_and_lanes(pg_cls):
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    pg.optimize(lambda_lanes=3, max_outer=2)
    # (the handle keeps (cos, sin) as the retraction left them; both handles get
    # the same (x, y, theta), so both hold cos / sin of the same angle)
    pg.set_poses(pg.poses())
    a = pg.marginal_covariances_all(edges=True)
    b = pg.marginal_covariances_all(edges=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert pg.marginal_covariances_all().tobytes() == a[0].tobytes()
    fresh = pg_cls.from_dataset(g)
    fresh.set_poses(pg.poses())
    c = fresh.marginal_covariances_all(edges=True)
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True])
def test_next_optimize_is_a_clean_one(pg_cls, poison):
    """The scheme of test_fronts_rezeroed_after_marginals and
    test_poisoned_workspace_bitwise with the new call between two optimizes."""
    g = datasets.make("C2")
    ref = pg_cls.from_dataset(g)
    ref.save_values()
    st0 = ref.optimize(lambda_lanes=3)
    p0 = ref.poses()
    for graphs in (1, 0):
        pg = pg_cls.from_dataset(g)
        pg.save_values()
        pg.optimize(use_graphs=graphs, lambda_lanes=3, max_outer=2)
        pg.marginal_covariances_all(edges=True)
        if poison:
            pg.debug_poison_fronts()
        pg.restore_values()
        st = pg.optimize(use_graphs=graphs, lambda_lanes=3)
        assert st["final_error"] == st0["final_error"], graphs
        assert np.array_equal(pg.poses(), p0), graphs


@pytest.mark.gpu
def test_per_pose_path_untouched_after_the_pass(pg_cls):
    g = datasets.make("C1-nn")
    keys = np.asarray(g.keys)[::7]
    want = pg_cls.from_dataset(g).marginal_covariances(keys)
    pg = pg_cls.from_dataset(g)
    pg.marginal_covariances_all(edges=True)
    assert pg.marginal_covariances(keys).tobytes() == want.tobytes()


@pytest.mark.gpu
def test_robust_loss_uses_weighted_hessian(pg_cls):
    """The graph of test_marginals_use_weighted_hessian: all poses against the
    twin's weighted H, that test's 1e-8."""
    import copy
    import robust_twin as rt
    g, _, lc = rt.outlier_graph()
    gl = rt.with_loss_on(copy.copy(g), lc, rt.HUBER, 1.345)
    rp = rt.problem(gl)
    pg = pg_cls.from_dataset(gl)
    pg.optimize()
    _twin_check(gl, pg, prob=rp, twin_cov=rt.marginal_covariances)


@pytest.mark.gpu
def test_live_append_rebuilds_the_lists(pg_cls):
    """A keyframe with its odometry and a loop closure appended to the plan
    (plan_update 4), then the call: the grown graph's covariances."""
    from oracle import pgo_numpy as pn
    from test_gpu_parity import _extend
    g = datasets.make("C1")
    pg = pg_cls.from_dataset(g)
    pg.optimize()
    before = pg.marginal_covariances_all()
    ext, init, (ei, ej, z) = _extend(g, pg.poses(), [], 1, np.random.default_rng(5))
    v = g.num_poses
    pg.add_vertex(v + 1, *init[v])
    cov = np.diag(datasets.SIGMA ** 2)
    for a, b, zz in zip(ei, ej, z):
        pg.add_edge(int(a) + 1, int(b) + 1, zz, cov)
    st = pg.optimize()
    assert st["plan_update"] == 4
    got, cross, x = _twin_check(ext, pg)
    assert got.shape == (v + 1, 3, 3) and cross.shape == (ext.num_edges, 3, 3) and before.shape == (v, 3, 3)
    _cross_check(pn.problem_from_graph(ext), x, got, cross)


@pytest.mark.gpu
def test_errors_and_python_adapter(pg_cls):
    from graphslam_amd import gtsam
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException, PgoError
    free = pg_cls()
    free.add_vertices(np.array([1, 2], dtype=np.uint64), np.array([[0, 0, 0], [1, 0, 0]], float))
    free.add_edge(1, 2, [1, 0, 0], np.diag([0.01, 0.01, 0.001]))
    with pytest.raises(IndeterminantLinearSystemException):
        free.marginal_covariances_all()
    free.add_prior(1, [0, 0, 0], np.diag([0.01] * 3))
    free.add_edge(2, 777, [1, 0, 0], np.diag([0.01, 0.01, 0.001]))
    with pytest.raises(PgoError) as ei:
        free.marginal_covariances_all()
    assert ei.value.status == _lib.PGO_E_NO_KEY
    # the mirror: all keys in the Values' order (inserted 5..1 here)
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    cov = np.diag([0.01, 0.01, 0.01])
    noise = gtsam.noiseModel.Gaussian.Covariance(np.diag([0.05 ** 2, 0.05 ** 2, 0.01]))
    graph.add(gtsam.PriorFactorPose2(1, gtsam.Pose2(0, 0, 0), gtsam.noiseModel.Gaussian.Covariance(cov)))
    for k in range(5, 0, -1):
        values.insert(k, gtsam.Pose2(k - 1.0, 0.0, 0.0))
    for k in range(1, 5):
        graph.add(gtsam.BetweenFactorPose2(k, k + 1, gtsam.Pose2(1, 0, 0), noise))
    m = gtsam.Marginals(graph, values)
    allc = m.marginalCovariances()
    assert allc.shape == (5, 3, 3)
    with gtsam._build(graph, values, 0) as pg:
        assert np.array_equal(allc, pg.marginal_covariances_all())
    for q, k in enumerate(range(5, 0, -1)):
        one = m.marginalCovariance(k)
        assert np.abs(allc[q] - one).max() <= 1e-9 * np.abs(one).max(), k
    assert np.array_equal(m.marginalCovariances([1, 5]), np.stack([m.marginalCovariance(1), m.marginalCovariance(5)]))


GRAPH_CPP_ALL = r'''
// graph.cpp:120-131 against include/pgo_gtsam.hpp: Marginals once, then the
// covariance of every keyframe -- as one call, and the last key's by itself.
#include <cstdio>
#include "pgo_gtsam.hpp"
using namespace pgo_gtsam;
int main() {
  NonlinearFactorGraph graph;
  Values initial;
  Matrix3 Q = Matrix3::Zero();
  Q(0, 0) = 0.1 * 0.1; Q(1, 1) = 0.1 * 0.1; Q(2, 2) = 0.1 * 0.1;
  graph.add(PriorFactor<Pose2>(1, Pose2(0, 0, 0), noiseModel::Gaussian::Covariance(Q)));
  initial.insert(1, Pose2(0, 0, 0));
  Matrix3 R = Matrix3::Zero();
  R(0, 0) = R(1, 1) = 0.0025; R(2, 2) = 7.6e-5;
  for (Key k = 2; k <= 8; k++) {
    const double th = 1.5707963267948966 * ((k - 2) / 2);
    initial.insert(k, Pose2(0.05 * k, -0.03 * k, th + 0.01));
    graph.add(BetweenFactor<Pose2>(k - 1, k, Pose2(1.0, 0, (k % 2) == 1 ? 1.5707963267948966 : 0.0),
                                   noiseModel::Gaussian::Covariance(R)));
  }
  graph.add(BetweenFactor<Pose2>(8, 1, Pose2(1.0, 0, 1.5707963267948966), noiseModel::Gaussian::Covariance(R)));
  try {
    LevenbergMarquardtOptimizer optimizer(graph, initial);
    Values poses_opti = optimizer.optimize();
    Marginals marginals(graph, poses_opti);
    const std::vector<Matrix3> all = marginals.marginalCovariances();
    const Matrix3 c = marginals.marginalCovariance(8);
    std::printf("n %zu\n", all.size());
    std::printf("all8 %.17g %.17g %.17g\n", all.back()(0, 0), all.back()(1, 1), all.back()(2, 2));
    std::printf("cov8 %.17g %.17g %.17g\n", c(0, 0), c(1, 1), c(2, 2));
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
    return 3;
  }
  return 0;
}
'''


@pytest.mark.gpu
def test_cpp_adapter_all_keys(tmp_path, pgo_lib):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "graph_all.cpp", tmp_path / "graph_all"
    src.write_text(GRAPH_CPP_ALL)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{root}/include", str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "n 8", r.stdout
    a = np.array([float(v) for v in lines[1].split()[1:]])
    c = np.array([float(v) for v in lines[2].split()[1:]])
    assert lines[1].startswith("all8") and (c > 0).all()
    assert (np.abs(a - c) <= 1e-9 * np.abs(c)).all(), (a, c)
