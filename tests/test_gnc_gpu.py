"""Fixed per-factor weights and graduated non-convexity on the GPU against the
numpy twin (tests/gnc_twin.py): the fixed-weight case of the robust kernels,
the return to the Gaussian kernel set, the weights sweep kernel, the GNC
trajectories, keep_weights with a live append, the degenerate stops and
determinism."""
import copy

import numpy as np
import pytest

import gnc_twin as gt
import robust_twin as rt
from graphslam_amd import _lib, datasets
from oracle import pgo_numpy as pn

pytestmark = pytest.mark.gpu

C2 = gt.CHI2_99_3
TIMING = ("ms_", "kernel_")

# GPU against the twin over a whole GNC run (test_trajectory_matches_twin), each
# 5 x the largest difference measured on the MI355X, rounded up to a power of
# ten; the measured values are in that test's docstring.
MU_RTOL = 1e-14
COST_RTOL = 1e-13
SUMW_RTOL = 1e-13
POSE_ATOL = 1e-12     # metres
ANGLE_ATOL = 1e-13    # radians
WEIGHT_ATOL = 1e-13


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


@pytest.fixture(scope="module")
def small():
    """manhattan(300, 8, 450, seed=2001) with 10 % of its loop closures replaced:
    (graph, replaced indices, loop-closure indices)."""
    return gt.corrupted(300, 8, 450, 2001, 0.1)


@pytest.fixture(scope="module")
def twin_runs(small):
    """The twin's GNC runs over all loop closures from dead reckoning, computed once."""
    g, _, lc = small
    return {loss: gt.optimize(g, lc, gt.GncParams(loss=loss)) for loss in (gt.GM, gt.TLS)}


def angdiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def _plain(g):
    h = copy.copy(g)
    for f in ("edge_loss", "edge_loss_k"):
        if hasattr(h, f):
            delattr(h, f)
    return h


def _check_linearize(pg, g, w):
    """Both sweeps and error() against the twin on the weight-scaled problem:
    1e-10 of max|H|, max|g|, and of the error (the bounds of test_robust_gpu)."""
    rp = gt.scaled(pn.problem_from_graph(g), w)
    x = pn.from_xyt(pg.poses())
    hd0, ho0, g0 = rt.blocks(rp, x)
    err0 = rt.error(rp, x)
    scale_h, scale_g = np.abs(hd0).max(), max(np.abs(g0).max(), 1.0)
    for chol in (False, True):
        hd, ho, grad, err = pg.debug_linearize(g.num_edges, cholesky=chol)
        print("cholesky" if chol else "two-slot", "dH", np.abs(hd - hd0).max() / scale_h, "dHoff",
              np.abs(ho - ho0).max() / scale_h, "dg", np.abs(grad - g0).max() / scale_g, "derr", abs(err - err0) / err0)
        assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
        assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
        assert np.abs(grad - g0).max() <= 1e-10 * scale_g
        assert abs(err - err0) <= 1e-10 * err0
    assert abs(pg.error() - err0) <= 1e-10 * err0
    assert np.array_equal(pg.edge_weights(), w)           # the set weights, bitwise


# ------------------------------------------------ 1. fixed weights, linearised
def test_fixed_weights_star(pg_cls):
    """robust_twin.star_graph() without its losses, random weights of which 50
    are exactly 0 and 50 exactly 1: the hub's side-0 row exceeds a block of
    k_linearize_own_robust, its side-1 list a sub-group of
    k_linearize_side1_robust."""
    g = _plain(rt.star_graph())
    rng = np.random.default_rng(41)
    w = rng.uniform(0.0, 1.0, g.num_edges)
    pick = rng.permutation(g.num_edges)
    w[pick[:50]] = 0.0
    w[pick[50:100]] = 1.0
    pg = pg_cls.from_dataset(g)
    pg.set_edge_weights(w)                      # before the first upload
    _check_linearize(pg, g, w)
    w2 = w[::-1].copy()
    pg.set_edge_weights(w2[100:350], first=100)  # a range, on the resident graph
    w[100:350] = w2[100:350]
    _check_linearize(pg, g, w)


def test_fixed_weights_grid_tail(pg_cls):
    """E = 257 factors: one full block and a tail of one thread."""
    g = datasets.manhattan(200, 8, 257, seed=5)
    assert g.num_edges == 257
    w = np.random.default_rng(42).uniform(0.0, 1.0, 257)
    w[256], w[0] = 0.0, 1.0
    pg = pg_cls.from_dataset(g)
    assert np.array_equal(pg.edge_weights(), np.ones(257))
    pg.debug_linearize(257)                     # resident and all Gaussian first
    pg.set_edge_weights(w)                      # the first weight below 1 on a resident graph
    _check_linearize(pg, g, w)


# ------------------------------------------------ 2. back to the Gaussian set
def test_return_to_gaussian_is_bitwise(pg_cls, small):
    g = small[0]
    a, b = pg_cls.from_dataset(g), pg_cls.from_dataset(g)
    a.debug_linearize(g.num_edges)
    b.debug_linearize(g.num_edges)
    w = np.random.default_rng(43).uniform(0.0, 1.0, g.num_edges)
    a.set_edge_weights(w)
    assert a.error() < b.error()
    a.set_edge_weights(np.ones(g.num_edges))
    assert a.error() == b.error()
    for chol in (False, True):
        for u, v in zip(a.debug_linearize(g.num_edges, cholesky=chol), b.debug_linearize(g.num_edges, cholesky=chol)):
            assert np.array_equal(u, v)
    sa, sb = a.optimize(), b.optimize()
    for key in sa:
        if not key.startswith(TIMING):
            assert sa[key] == sb[key], key
    assert np.array_equal(a.trace()[:, :7], b.trace()[:, :7], equal_nan=True)
    assert np.array_equal(a.poses(), b.poses())


# ------------------------------------------------------- 3. the sweep kernel
@pytest.mark.parametrize("mu", [1e-5, 1.0, 1e4])
@pytest.mark.parametrize("loss", [gt.GM, gt.TLS])
def test_sweep_kernel(pg_cls, small, loss, mu):
    """The sweep at the initial values over every second loop closure; the
    other closures hold fixed weights of their own, which the sweep must leave."""
    g, _, lc = small
    cand, rest = lc[::2], lc[1::2]
    r2 = rt.r_squared(gt.scaled(pn.problem_from_graph(g), np.ones(g.num_edges)), pn.from_xyt(g.initial))[0]
    ref = gt.weight(loss, mu, C2, r2[cand])
    # (the chosen mu keep every twin weight and r^2 clear of the counting thresholds)
    assert np.minimum(np.abs(ref - 1e-4), np.abs(ref - (1 - 1e-4))).min() >= 1e-8
    assert np.abs(r2[cand] - C2).min() >= 1e-8 * C2
    pg = pg_cls.from_dataset(g)
    own = np.random.default_rng(44).uniform(0.1, 0.9, len(rest))
    for e, v in zip(rest, own):
        pg.set_edge_weights([v], first=int(e))
    before = pg.edge_weights()
    w, s5 = pg.debug_gnc_sweep(loss, mu, C2, candidates=cand)          # read-only
    assert np.array_equal(pg.edge_weights(), before)
    mask = np.zeros(g.num_edges, bool)
    mask[cand] = True
    print("dw", np.abs(w[cand] - ref).max(), "rmax", s5[0], r2[cand].max())
    assert np.abs(w[cand] - ref).max() <= 1e-10
    assert np.array_equal(w[~mask], np.ones((~mask).sum()))            # non-candidates read exactly 1
    assert abs(s5[0] - r2[cand].max()) <= 1e-10 * r2[cand].max()
    assert abs(s5[1] - ref.sum()) <= 1e-10 * max(ref.sum(), 1.0)
    assert s5[2] == gt.nonbinary(ref, 1e-4).sum() and s5[3] == (r2[cand] > C2).sum() and s5[4] == len(cand)
    w2, t5 = pg.debug_gnc_sweep(loss, mu, C2, candidates=cand, write=True)
    assert np.array_equal(w2, w) and np.array_equal(t5, s5)            # sum of w included: bitwise repeatable
    after = pg.edge_weights()
    assert np.array_equal(after[cand], w[cand])                        # written ...
    assert np.array_equal(after[~mask], before[~mask])                 # ... and every other ek untouched
    assert np.array_equal(after[rest], own)


# ------------------------------------------------------------ 4. trajectories
def _run(pg, lc, loss, **kw):
    st = pg.optimize_gnc(candidates=lc, loss=loss, **kw)
    return st, pg.gnc_trace()


@pytest.mark.parametrize("loss", [gt.GM, gt.TLS])
def test_trajectory_matches_twin(pg_cls, small, twin_runs, loss):
    """All loop closures as candidates, from dead reckoning.  The twin's own
    margins first (inner >= 1 %, outer >= 1, TLS weight distance >= 1e-8: measured
    0.059 / 2.4e3 for GM, 0.18 / 1.8e2 / 3.9e-7 for TLS), then every decision
    exactly: the outer count, the inner tries and accepted steps of every row,
    the stop reason, the set with r^2 > c^2.  The continuous quantities are held
    to 5 x the differences measured on the MI355X, rounded up to a power of ten.
    Measured (GM / TLS): mu 7.6e-16 / 1.3e-15 relative, cost 2.7e-15 / 6.1e-15
    relative, sum of weights 2.5e-16 / 5.4e-15 relative, poses 2.0e-14 /
    2.8e-14 m and 5.3e-15 / 6.7e-15 rad, final weights 3.3e-15 / 0 -- over
    29 and 33 warm-started inner solves the GPU and the twin stay within a
    few hundred ulp of each other."""
    g, bad, lc = small
    r = twin_runs[loss]
    assert r.inner_margin >= 0.01 and r.outer_margin >= 1.0
    assert r.final_r2_margin >= 1e-8
    if loss == gt.TLS:
        assert r.weight_distance >= 1e-8
    pg = pg_cls.from_dataset(g)
    st, tr = _run(pg, lc, loss)
    ref = r.rows
    d_mu = np.nanmax(np.abs(tr[1:, 0] - ref[1:, 0]) / ref[1:, 0]) if len(ref) > 1 and len(tr) == len(ref) else np.nan
    print("rows", len(tr), len(ref), "stop", st["stop_reason"], r.stop_reason)
    if tr.shape == ref.shape:
        p, q = pg.poses(), r.xyt()
        wg = pg.edge_weights()
        print("MEASURED loss", loss, "mu", d_mu, "cost", np.abs(tr[:, 1] - ref[:, 1]).max() / 1.0,
              "cost_rel", (np.abs(tr[:, 1] - ref[:, 1]) / ref[:, 1]).max(),
              "sumw_rel", (np.abs(tr[:, 2] - ref[:, 2]) / ref[:, 2]).max(),
              "rmax_rel", (np.abs(tr[:, 4] - ref[:, 4]) / ref[:, 4]).max(),
              "pose", np.abs(p[:, :2] - q[:, :2]).max(), "angle", angdiff(p[:, 2], q[:, 2]).max(),
              "w", np.abs(wg - r.weights).max())
    # decisions, exactly
    assert tr.shape == ref.shape and st["outer_iterations"] == r.outer_iterations == len(ref) - 1
    assert np.array_equal(tr[:, 5], ref[:, 5]) and np.array_equal(tr[:, 6], ref[:, 6])     # inner tries, accepted
    assert np.array_equal(tr[:, 3], ref[:, 3])                                             # non-binary counts
    assert st["stop_reason"] == r.stop_reason
    assert st["inner_tries"] == r.inner_tries and st["candidates"] == len(lc)
    assert st["outliers"] == len(r.outliers)
    r2 = rt.r_squared(gt.scaled(pn.problem_from_graph(g), np.ones(g.num_edges)), pn.from_xyt(pg.poses()))[0]
    assert np.array_equal(lc[r2[lc] > C2], r.outliers)
    # continuous quantities
    assert np.isnan(tr[0, 0]) and d_mu <= MU_RTOL
    assert st["mu_initial"] == tr[1, 0] and st["mu_final"] == tr[-1, 0]
    assert (np.abs(tr[:, 1] - ref[:, 1]) / ref[:, 1]).max() <= COST_RTOL
    assert (np.abs(tr[:, 2] - ref[:, 2]) / ref[:, 2]).max() <= SUMW_RTOL
    assert abs(st["final_cost"] - r.final_cost) <= COST_RTOL * r.final_cost
    assert abs(st["initial_error"] - r.initial_error) <= 1e-10 * r.initial_error
    p, q = pg.poses(), r.xyt()
    assert np.abs(p[:, :2] - q[:, :2]).max() <= POSE_ATOL and angdiff(p[:, 2], q[:, 2]).max() <= ANGLE_ATOL
    w = pg.edge_weights()
    assert np.abs(w - r.weights).max() <= WEIGHT_ATOL
    if loss == gt.TLS:   # every corrupted closure out, every true one in
        good = np.setdiff1d(lc, bad)
        assert np.array_equal(w[bad], np.zeros(len(bad))) and np.array_equal(w[good], np.ones(len(good)))
        assert np.array_equal(r.weights, w)
    # pgo_get_trace still describes the last inner optimize
    assert len(pg.trace()) >= tr[-1, 5] >= 1


# ------------------------------------------------------------ 5. keep_weights
def test_keep_weights_and_live_append(pg_cls, small, twin_runs):
    g, bad, lc = small
    pg = pg_cls.from_dataset(g)
    st, tr = _run(pg, lc, gt.GM)                      # keep_weights = 1 is the default
    w = pg.edge_weights()
    rest = np.setdiff1d(np.arange(g.num_edges), lc)
    assert np.array_equal(w[rest], np.ones(len(rest)))
    assert abs(w[lc].sum() - tr[-1, 2]) <= 1e-12 * tr[-1, 2]          # the final sweep's weights
    assert np.abs(w - twin_runs[gt.GM].weights).max() <= WEIGHT_ATOL
    assert abs(pg.error() - st["final_cost"]) <= 1e-12 * st["final_cost"]
    # one keyframe with its odometry and a closure: appended in place
    x = pg.poses()
    n = g.num_poses
    step = np.array([1.0, 0.0, 0.0])
    truth = np.vstack([g.ground_truth, datasets.compose_xyt(g.ground_truth[n - 1], step)])
    xn = np.vstack([x, datasets.compose_xyt(x[n - 1], step)])
    j = n // 3
    z_odo = datasets.between_xyt(truth[n - 1], truth[n])
    z_lc = datasets.between_xyt(truth[n], truth[j]) + [0.04, -0.03, 0.005]
    cov = np.diag(datasets.SIGMA ** 2)
    pg.add_vertex(n + 1, *xn[n])
    pg.add_edge(n, n + 1, z_odo, cov)
    pg.add_edge(n + 1, j + 1, z_lc, cov)
    st2 = pg.optimize()
    assert st2["upload_kind"] == 2
    w2 = pg.edge_weights()
    assert np.array_equal(w2[:g.num_edges], w) and np.array_equal(w2[g.num_edges:], np.ones(2))
    grown = copy.copy(g)
    grown.keys = np.arange(1, n + 2, dtype=np.uint64)
    grown.ground_truth = truth
    grown.initial = xn
    grown.edge_k1 = np.concatenate([g.edge_k1, np.array([n, n + 1], dtype=np.uint64)])
    grown.edge_k2 = np.concatenate([g.edge_k2, np.array([n + 1, j + 1], dtype=np.uint64)])
    grown.edge_z = np.concatenate([g.edge_z, [z_odo, z_lc]])
    grown.edge_cov = np.concatenate([g.edge_cov, np.tile(cov.reshape(1, 9), (2, 1))])
    rp = gt.scaled(pn.problem_from_graph(grown), w2)
    res, margin = rt.levenberg_marquardt(rp, pn.from_xyt(xn))
    assert margin >= 0.01
    p, q = pg.poses(), res.xyt()
    print("MEASURED append cost_rel", abs(st2["final_error"] - res.error) / res.error, "pose",
          np.abs(p[:, :2] - q[:, :2]).max(), "angle", angdiff(p[:, 2], q[:, 2]).max())
    assert st2["iterations"] == res.iterations and st2["inner_iterations"] == res.inner_iterations
    assert abs(st2["final_error"] - res.error) <= COST_RTOL * res.error
    p, q = pg.poses(), res.xyt()
    assert np.abs(p[:, :2] - q[:, :2]).max() <= POSE_ATOL and angdiff(p[:, 2], q[:, 2]).max() <= ANGLE_ATOL
    idx = [0, 1, n // 3, n // 2, n]
    covs = pg.marginal_covariances(np.asarray(grown.keys)[idx])
    refc = rt.marginal_covariances(rp, pn.from_xyt(pg.poses()), idx)
    for k in range(len(idx)):
        assert np.abs(covs[k] - refc[k]).max() <= 1e-8 * np.abs(refc[k]).max(), idx[k]


def test_keep_weights_off_leaves_a_plain_graph(pg_cls, small):
    g, _, lc = small
    pg, fresh = pg_cls.from_dataset(g), pg_cls.from_dataset(g)
    pg.save_values()
    st, _ = _run(pg, lc, gt.TLS, keep_weights=0)
    assert st["outliers"] > 0 and np.array_equal(pg.edge_weights(), np.ones(g.num_edges))
    pg.restore_values()
    sa, sb = pg.optimize(), fresh.optimize()
    assert np.array_equal(pg.trace()[:, :7], fresh.trace()[:, :7], equal_nan=True)
    assert sa["final_error"] == sb["final_error"] and np.array_equal(pg.poses(), fresh.poses())


# -------------------------------------------------------------- 6. degenerate
def test_degenerate_stops(pg_cls):
    g = datasets.square_loop()
    pg, plain = pg_cls.from_dataset(g), pg_cls.from_dataset(g)
    sp = plain.optimize()
    st = pg.optimize_gnc(loss="tls")
    assert st["stop_reason"] == _lib.PGO_GNC_STOP_ALL_INLIERS and st["outer_iterations"] == 0
    assert st["status"] == _lib.PGO_OK and np.isnan(st["mu_initial"]) and st["outliers"] == 0
    assert np.array_equal(pg.edge_weights(), np.ones(g.num_edges))
    assert pg.gnc_trace().shape == (1, 8) and np.array_equal(pg.poses(), plain.poses())
    none = pg_cls.from_dataset(g)
    st = none.optimize_gnc(candidates=[])
    assert st["stop_reason"] == _lib.PGO_GNC_STOP_NO_CANDIDATES and st["candidates"] == 0
    assert st["final_cost"] == sp["final_error"] and st["initial_error"] == sp["initial_error"]
    assert np.array_equal(none.poses(), plain.poses())
    assert np.array_equal(none.trace()[:, :7], plain.trace()[:, :7], equal_nan=True)
    assert st["inner_tries"] == sp["inner_iterations"]


# ------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("loss", [gt.GM, gt.TLS])
def test_two_runs_agree_bitwise(pg_cls, small, loss):
    g, _, lc = small
    pg = pg_cls.from_dataset(g)
    pg.save_values()
    s1, t1 = _run(pg, lc, loss)
    p1, w1 = pg.poses(), pg.edge_weights()
    pg.restore_values()
    s2, t2 = _run(pg, lc, loss)
    assert np.array_equal(t1, t2, equal_nan=True)
    assert np.array_equal(pg.poses(), p1) and np.array_equal(pg.edge_weights(), w1)
    for key in ("stop_reason", "outer_iterations", "outliers", "inner_tries", "linearizations", "final_cost",
                "mu_final"):
        assert s1[key] == s2[key], key
