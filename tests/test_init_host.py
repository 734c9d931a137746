"""The linear initialisation without a GPU: the numpy twin (tests/init_twin.py)
checks itself -- its stage 2 against a brute-force minimisation of the graph
error over the positions -- and the library's host side (pgo_debug_init_tree:
components, roots, breadth-first tree, 2 pi integers) must reproduce the twin's
tree exactly.  The host module's own sanitizer self-test is built and run as a
stand-alone program."""
import os
import subprocess

import numpy as np
import pytest
import scipy.optimize

import init_twin as it
from graphslam_amd import _lib, datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPHS = {
    "square": datasets.square_loop,
    "square-turn": it.square_turn,
    "C1": lambda: datasets.make("C1"),
    "C1-nn": lambda: datasets.make("C1-nn"),
    "star": it.star,
    "two-components": it.two_components,
}


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


# ------------------------------------------------------------------ the twin
def test_twin_stage2_is_the_minimiser_over_positions():
    """Stage 2 against scipy's minimisation of pgo_numpy.error over the 2n
    positions, orientations held at stage 1's (the error is quadratic in them,
    so BFGS with an exact line search ends at the minimiser)."""
    g = it.square_turn()
    x = it.initialize(g)
    theta = x[:, 2]

    def f(p):
        return it.error(g, np.column_stack([p.reshape(-1, 2), theta]))

    p0 = g.initial[:, :2].ravel()
    res = scipy.optimize.minimize(f, p0, method="BFGS", options=dict(gtol=1e-9, maxiter=10000))
    assert f(x[:, :2].ravel()) <= res.fun * (1 + 1e-9) + 1e-12
    assert np.abs(res.x - x[:, :2].ravel()).max() <= 1e-5, np.abs(res.x - x[:, :2].ravel()).max()
    # and a numeric gradient of error() over the positions vanishes at it
    h = 1e-6
    grad = np.array([(f(x[:, :2].ravel() + h * e) - f(x[:, :2].ravel() - h * e)) / (2 * h)
                     for e in np.eye(2 * g.num_poses)])
    scale = np.abs(it.position_system(g, theta).rhs).max()
    assert np.abs(grad).max() <= 1e-6 * scale, (np.abs(grad).max(), scale)


def test_twin_stage1_is_the_minimiser_over_orientations():
    g = it.square_turn()
    t = it.tree(g)
    s = it.orientation_system(g, t)
    theta = it.solve(s)
    prob = it.tw.problem_from_graph(g)
    w, wq = it.theta_information(prob.eom), it.theta_information(prob.pom)

    def cost(th):
        return (w * (th[prob.ej] - th[prob.ei] - t.delta - it.TWO_PI * t.k_edge) ** 2).sum() + \
            (wq * (th[prob.pi] - t.ptheta - it.TWO_PI * t.k_prior) ** 2).sum()

    rng = np.random.default_rng(0)
    c0 = cost(theta)
    for _ in range(20):
        assert cost(theta + 1e-3 * rng.standard_normal(len(theta))) > c0
    assert np.any(t.k_edge != 0)          # the turns sum to 2 pi: some factor carries the wrap
    # after the two solves the graph's error is far below the error at the scattered initial values
    assert it.error(g, it.initialize(g)) < 1e-3 * it.error(g, g.initial)


def test_twin_reproduces_ground_truth_on_noise_free_graphs():
    g = datasets.square_loop()
    x = it.initialize(g)
    assert np.abs(x[:, :2] - g.ground_truth[:, :2]).max() <= 1e-9
    assert np.abs(it.tw_wrap(x[:, 2] - g.ground_truth[:, 2])).max() <= 1e-9
    assert it.error(g, x) <= 1e-15


# ------------------------------------------------------- the library's tree
@pytest.mark.parametrize("name", list(GRAPHS))
def test_tree_matches_twin_exactly(pg_cls, name):
    g = GRAPHS[name]()
    t = it.tree(g)
    pg = pg_cls.from_dataset(g)
    parent, k_edge, k_prior = pg.debug_init_tree()
    assert np.array_equal(parent, t.parent)
    assert np.array_equal(k_edge, t.k_edge)
    assert np.array_equal(k_prior, t.k_prior)
    if name == "square-turn":
        assert np.any(k_edge != 0)
    if name == "star":
        assert np.all(parent[1:] == 0) and parent[0] == -1
    if name == "two-components":
        assert (parent == -1).sum() == 2 and t.components == 2
    pg.close()


def test_tree_with_keys_that_are_not_indices(pg_cls):
    """Keys out of order and 64-bit: the tree is in insertion indices."""
    g = it.square_turn()
    n = g.num_poses
    keys = (np.arange(n, dtype=np.uint64)[::-1] * np.uint64(7) + np.uint64(2 ** 40))
    lut = {int(k): int(keys[p]) for p, k in enumerate(g.keys)}
    t = it.tree(g)
    g.edge_k1 = np.array([lut[int(k)] for k in g.edge_k1], dtype=np.uint64)
    g.edge_k2 = np.array([lut[int(k)] for k in g.edge_k2], dtype=np.uint64)
    g.prior_keys = np.array([lut[int(k)] for k in g.prior_keys], dtype=np.uint64)
    g.keys = keys
    pg = pg_cls.from_dataset(g)
    parent, k_edge, k_prior = pg.debug_init_tree()
    assert np.array_equal(parent, t.parent) and np.array_equal(k_edge, t.k_edge)
    assert np.array_equal(k_prior, t.k_prior)


def test_component_without_prior_is_indeterminant(pg_cls):
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException
    g = it.two_components(prior_b=False)
    with pytest.raises(it.Indeterminant):
        it.tree(g)
    pg = pg_cls.from_dataset(g)
    with pytest.raises(IndeterminantLinearSystemException) as ei:
        pg.debug_init_tree()
    assert ei.value.status == _lib.PGO_E_INDETERMINANT
    # the call itself reports it before it needs a device, with the values untouched
    before = pg.poses()
    with pytest.raises(IndeterminantLinearSystemException):
        pg.initialize_linear()
    assert pg.last_init_stats["status"] == _lib.PGO_E_INDETERMINANT
    assert np.array_equal(pg.poses(), before)


def test_empty_graph_and_missing_key(pg_cls):
    from graphslam_amd.pose_graph import PgoError, ValuesKeyDoesNotExist
    pg = pg_cls()
    assert pg.initialize_linear()["status"] == _lib.PGO_OK      # no vertex: nothing to do
    parent, k_edge, k_prior = pg.debug_init_tree()
    assert len(parent) == 0 and len(k_edge) == 0 and len(k_prior) == 0
    pg.add_vertex(1, 0, 0, 0)
    pg.add_prior(1, [0, 0, 0], np.diag([0.01] * 3))
    pg.add_edge(1, 99, [1, 0, 0], np.diag([0.01] * 3))           # key 99 never inserted
    with pytest.raises(ValuesKeyDoesNotExist):
        pg.debug_init_tree()
    with pytest.raises(PgoError) as ei:
        pg.initialize_linear()
    assert ei.value.status == _lib.PGO_E_NO_KEY


def test_abi_version_is_unchanged(pgo_lib):
    assert pgo_lib.pgo_abi_version() == 6
    assert {"pgo_initialize_linear", "pgo_debug_init_tree", "pgo_debug_init_system"} <= set(_lib.declared_symbols())


def test_init_host_module_under_asan_ubsan():
    """pgo_init.cpp driven by init_selftest.cpp under ASan + UBSan: a stand-alone
    host program, nothing preloaded."""
    b = subprocess.run(["make", "-s", "-C", "graphslam_amd/csrc", "asan-init"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "graphslam_amd", "csrc", "build", "init_selftest_asan")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "init selftest ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
