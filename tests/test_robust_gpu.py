"""Robust losses on the GPU against the numpy twin (tests/robust_twin.py): the
robust linearisation sweeps (two-slot and Cholesky-mode), error, weights, the
LM trajectory, PCG, marginals, live appends and determinism; and the Gaussian
path, which a handle without a robust factor must still take bit for bit."""
import numpy as np
import pytest

import robust_twin as rt
from graphslam_amd import _lib, datasets
from oracle import pgo_numpy as pn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


@pytest.fixture(scope="module")
def outliers():
    """manhattan(1000, 16, 1500, seed=2001) with 50 of its 501 loop closures
    replaced by random poses: (graph, replaced indices, loop-closure indices)."""
    return rt.outlier_graph()


def _with(g, idx, loss, k):
    import copy
    return rt.with_loss_on(copy.copy(g), idx, loss, k)


@pytest.fixture(scope="module")
def twin_runs(outliers):
    """The twin's LM trajectories from the dead-reckoned start, computed once."""
    g, _, lc = outliers
    out = {}
    for name, loss, k in (("huber", rt.HUBER, 1.345), ("cauchy", rt.CAUCHY, 1.0)):
        gl = _with(g, lc, loss, k)
        rp = rt.problem(gl)
        res, margin = rt.levenberg_marquardt(rp, pn.from_xyt(g.initial))
        out[name] = (gl, rp, res, margin)
    return out


def angdiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def _check_linearize(pg, g, rp):
    """Both sweeps against the twin (1e-10 of max|H|, max|g|; the error 1e-10
    relative), and against each other at the tolerances of
    test_linearize_cholesky_mode_parity."""
    x = pn.from_xyt(pg.poses())
    hd0, ho0, g0 = rt.blocks(rp, x)
    err0 = rt.error(rp, x)
    scale_h, scale_g = np.abs(hd0).max(), max(np.abs(g0).max(), 1.0)
    got = {}
    for chol in (False, True):
        hd, ho, grad, err = pg.debug_linearize(g.num_edges, cholesky=chol)
        print("cholesky" if chol else "two-slot", "dH", np.abs(hd - hd0).max() / scale_h, "dHoff",
              np.abs(ho - ho0).max() / scale_h, "dg", np.abs(grad - g0).max() / scale_g, "derr", abs(err - err0) / err0)
        assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
        assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
        assert np.abs(grad - g0).max() <= 1e-10 * scale_g
        assert abs(err - err0) <= 1e-10 * err0
        got[chol] = (hd, ho, grad)
    assert abs(pg.error() - err0) <= 1e-10 * err0
    assert np.abs(got[True][0] - got[False][0]).max() <= 1e-12 * scale_h
    assert np.abs(got[True][1] - got[False][1]).max() <= 1e-14 * scale_h
    assert np.abs(got[True][2] - got[False][2]).max() <= 1e-12 * scale_g


def test_linearize_parity_mixed_losses(pg_cls, outliers):
    """Per-edge losses drawn from all four kinds (mixed inside a wave), k in
    [0.5, 3], at the dead-reckoned values (many factors far into the tails)."""
    import copy
    g = copy.copy(outliers[0])
    rng = np.random.default_rng(17)
    g.edge_loss = rng.integers(0, 4, g.num_edges).astype(np.int32)
    g.edge_loss_k = rng.uniform(0.5, 3.0, g.num_edges)
    rp = rt.problem(g)
    r = np.sqrt(rt.r_squared(rp, pn.from_xyt(g.initial))[0])
    assert (r > 3 * rp.k).sum() > 100 and (r < rp.k).sum() > 100
    _check_linearize(pg_cls.from_dataset(g), g, rp)


def test_linearize_star_block_and_row_boundaries(pg_cls):
    """The hub is k1 of 300 edges (one row of k_linearize_own_robust with more
    side-0 factors than kThreads, taken in chunks) and k2 of 300 others (a
    side-1 list much longer than the sub-group of k_linearize_side1_robust)."""
    g = rt.star_graph()
    _check_linearize(pg_cls.from_dataset(g), g, rt.problem(g))


def test_edge_weights(pg_cls, outliers, twin_runs):
    g, bad, lc = outliers
    gl, rp, res, _ = twin_runs["huber"]
    pg = pg_cls.from_dataset(gl)
    w0 = pg.edge_weights()
    assert w0.shape == (g.num_edges,)
    assert np.abs(w0 - rt.weights(rp, pn.from_xyt(g.initial))).max() <= 1e-10
    assert np.array_equal(w0[rp.loss == 0], np.ones((rp.loss == 0).sum()))      # NONE: exactly 1
    assert np.array_equal(pg.edge_weights(first=1200, n=37), w0[1200:1237])
    pg.optimize()
    w1 = pg.edge_weights()
    assert np.abs(w1 - rt.weights(rp, pn.from_xyt(pg.poses()))).max() <= 1e-10
    assert np.array_equal(w1[rp.loss == 0], np.ones((rp.loss == 0).sum()))
    assert w1[bad].max() < 0.1          # the caller's use: the wrong loop closures stand out


def test_gaussian_path_untouched(pg_cls):
    """C1 through add_edges_robust with loss NONE is the plain handle bit for
    bit (it launches the Gaussian kernels); Huber with k = 1e300 (all w = 1)
    runs the robust kernels and agrees to 1e-12 relative."""
    g = datasets.make("C1")
    plain = pg_cls.from_dataset(g)
    g_none = _with(g, np.arange(g.num_edges), _lib.PGO_LOSS_NONE, 1.0)
    none = pg_cls.from_dataset(g_none)
    g_big = _with(g, np.arange(g.num_edges), _lib.PGO_LOSS_HUBER, 1e300)
    big = pg_cls.from_dataset(g_big)
    for chol in (False, True):
        a = plain.debug_linearize(g.num_edges, cholesky=chol)
        b = none.debug_linearize(g.num_edges, cholesky=chol)
        c = big.debug_linearize(g.num_edges, cholesky=chol)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
        sh, sg = np.abs(a[0]).max(), np.abs(a[2]).max()
        assert np.abs(c[0] - a[0]).max() <= 1e-12 * sh and np.abs(c[1] - a[1]).max() <= 1e-12 * sh
        assert np.abs(c[2] - a[2]).max() <= 1e-12 * sg and abs(c[3] - a[3]) <= 1e-12 * a[3]
    assert np.array_equal(big.edge_weights(), np.ones(g.num_edges))
    sa, sb = plain.optimize(), none.optimize()
    timing = ("ms_", "kernel_", "ms_total")
    for key in sa:
        if not key.startswith(timing):
            assert sa[key] == sb[key], key
    assert np.array_equal(plain.poses(), none.poses())
    assert np.array_equal(plain.trace()[:, :7], none.trace()[:, :7], equal_nan=True)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", ["huber", "cauchy"])
def test_lm_trajectory_matches_twin(pg_cls, twin_runs, name, lanes):
    """optimize() defaults (Cholesky) from the dead-reckoned start, Huber(1.345)
    and Cauchy(1.0) on the loop closures: accepted steps, lambda, solved and
    accepted flags identical to the twin's, candidate errors to rtol 1e-8, model
    decrease to rtol 1e-6, final error to rtol 1e-8, poses within 1e-6 m and
    1e-7 rad.  The comparison of decisions is sound because in the twin's own
    trajectory every decision quantity (fidelity vs min_model_fidelity, |cost
    change| vs relative_error_tol * error, checkConvergence's differences) is
    at least 1 % from its threshold: measured 29 % (Huber) and 9.4 % (Cauchy),
    asserted here and in tests/test_robust.py on the CPU."""
    gl, rp, res, margin = twin_runs[name]
    assert margin >= 0.01
    pg = pg_cls.from_dataset(gl)
    st = pg.optimize(lambda_lanes=lanes)
    tr, ot = pg.trace(), rt.trace_array(res.trace)
    assert tr.shape == (ot.shape[0], 8)
    for c in (0, 1, 2, 6):   # accepted steps, lambda, solved, accepted
        assert np.array_equal(tr[:, c], ot[:, c]), c
    fin = np.isfinite(ot[:, 4])
    assert np.array_equal(np.isfinite(tr[:, 4]), fin)
    assert np.allclose(tr[fin, 4], ot[fin, 4], rtol=1e-8, atol=0)
    ok = np.isfinite(ot[:, 3])
    assert np.allclose(tr[ok, 3], ot[ok, 3], rtol=1e-6, atol=1e-9 * np.abs(ot[ok, 3]).max())
    assert st["iterations"] == res.iterations and st["inner_iterations"] == res.inner_iterations
    assert abs(st["initial_error"] - res.initial_error) <= 1e-8 * res.initial_error
    assert abs(st["final_error"] - res.error) <= 1e-8 * res.error
    p, q = pg.poses(), res.xyt()
    assert np.abs(p[:, :2] - q[:, :2]).max() <= 1e-6 and angdiff(p[:, 2], q[:, 2]).max() <= 1e-7


def _assert_trace(pg, st, res):
    tr, ot = pg.trace(), rt.trace_array(res.trace)
    assert tr.shape == (ot.shape[0], 8)
    for c in (0, 1, 2, 6):   # accepted steps, lambda, solved, accepted
        assert np.array_equal(tr[:, c], ot[:, c]), c
    fin = np.isfinite(ot[:, 4])
    assert np.array_equal(np.isfinite(tr[:, 4]), fin)
    assert np.allclose(tr[fin, 4], ot[fin, 4], rtol=1e-8, atol=0)
    ok = np.isfinite(ot[:, 3])
    assert np.allclose(tr[ok, 3], ot[ok, 3], rtol=1e-6, atol=1e-9 * np.abs(ot[ok, 3]).max())
    assert st["iterations"] == res.iterations and st["inner_iterations"] == res.inner_iterations
    assert abs(st["final_error"] - res.error) <= 1e-8 * res.error


@pytest.mark.parametrize("lanes", [1, 3])
def test_lm_rejected_tries_with_lanes(pg_cls, outliers, lanes):
    """Huber on the first 250 loop closures only: the wrong closures among the
    others stay Gaussian, so LM rejects tries (the twin: 5 accepted steps, then
    15 rejected tries up to lambda's bound) and the batched lambda lanes run on
    a robust graph -- the same rows as one lane and as the twin.  Closest
    decision quantity in the twin's trajectory: 100 % from its threshold."""
    g, _, lc = outliers
    gl = _with(g, lc[:250], rt.HUBER, 1.345)
    res, margin = rt.levenberg_marquardt(rt.problem(gl), pn.from_xyt(g.initial))
    assert margin >= 0.01 and res.inner_iterations > res.iterations + 5
    pg = pg_cls.from_dataset(gl)
    st = pg.optimize(lambda_lanes=lanes)
    assert st["stop_reason"] == 1          # PGO_STOP_LAMBDA_BOUND
    _assert_trace(pg, st, res)


def test_pcg_solver_matches_twin(pg_cls, outliers):
    g, _, lc = outliers
    gl = _with(g, lc, rt.HUBER, 1.345)
    rp = rt.problem(gl)
    res, _ = rt.levenberg_marquardt(rp, pn.from_xyt(g.initial), pn.LMParams(max_outer=2))
    pg = pg_cls.from_dataset(gl)
    st = pg.optimize(linear_solver=_lib.PGO_SOLVER_PCG, max_outer=2)
    tr, ot = pg.trace(), rt.trace_array(res.trace)
    assert tr.shape[0] == ot.shape[0]
    assert np.array_equal(tr[:, 6], ot[:, 6])
    fin = np.isfinite(ot[:, 4])
    assert np.allclose(tr[fin, 4], ot[fin, 4], rtol=1e-6, atol=0)
    assert abs(st["final_error"] - res.error) <= 1e-6 * res.error


def test_marginals_use_weighted_hessian(pg_cls, twin_runs):
    gl, rp, _, _ = twin_runs["huber"]
    pg = pg_cls.from_dataset(gl)
    pg.optimize()
    n = gl.num_poses
    idx = [0, 1, n // 3, n // 2, n - 1]
    cov = pg.marginal_covariances(np.asarray(gl.keys)[idx])
    ref = rt.marginal_covariances(rp, pn.from_xyt(pg.poses()), idx)
    gauss = pn.marginal_covariances(rp.prob, pn.from_xyt(pg.poses()), idx)
    for q in range(len(idx)):
        assert np.abs(cov[q] - ref[q]).max() <= 1e-8 * np.abs(ref[q]).max(), idx[q]
    # (the unweighted H would miss the tolerance by orders of magnitude: the check tells them apart)
    assert np.abs(gauss[-1] - ref[-1]).max() > 1e3 * 1e-8 * np.abs(ref[-1]).max()


def _compare_with_fresh(pg_cls, pg, st, grown, x_start, **kw):
    """Against a fresh handle of the same factors from the same values: equal
    step counts and decisions, and the tolerances the Cholesky append tests
    (test_incremental_append_matches_oracle, test_registrations_plan_append_
    matches_oracle) allow between two solvers of the same system -- the
    resident handle factors with an incrementally refreshed plan, the fresh
    one with a new ordering: final error 1e-8 relative, poses 1e-6 m, 1e-7 rad."""
    import copy
    fg = copy.copy(grown)
    fg.initial = x_start
    fresh = pg_cls.from_dataset(fg)
    ref = fresh.optimize(**kw)
    assert st["iterations"] == ref["iterations"] and st["inner_iterations"] == ref["inner_iterations"]
    assert abs(st["initial_error"] - ref["initial_error"]) <= 1e-9 * ref["initial_error"]
    assert abs(st["final_error"] - ref["final_error"]) <= 1e-8 * ref["final_error"]
    ta, tb = pg.trace(), fresh.trace()
    assert ta.shape == tb.shape
    for c in (0, 1, 2, 6):
        assert np.array_equal(ta[:, c], tb[:, c]), c
    p, q = pg.poses(), fresh.poses()
    assert np.abs(p[:, :2] - q[:, :2]).max() <= 1e-6 and angdiff(p[:, 2], q[:, 2]).max() <= 1e-7


def test_live_append_of_robust_factors(pg_cls, outliers):
    """An all-Gaussian resident graph gets its last 5 loop closures with Huber
    through add_edge(..., loss=...): the kernels launched change (a full upload
    is accepted there); then a keyframe with a Gaussian odometry factor and a
    Huber loop closure is appended onto the now-robust graph in place
    (upload_kind 2).  Each re-solve equals a fresh handle of the same factors
    from the same values."""
    import copy
    g = outliers[0]
    E = g.num_edges
    head = copy.copy(g)
    for f in ("edge_k1", "edge_k2", "edge_z", "edge_cov"):
        setattr(head, f, getattr(g, f)[:E - 5])
    pg = pg_cls.from_dataset(head)
    pg.optimize()
    x1 = pg.poses()
    for e in range(E - 5, E):
        pg.add_edge(int(g.edge_k1[e]), int(g.edge_k2[e]), g.edge_z[e], g.edge_cov[e], loss="huber", k=1.345)
    st = pg.optimize()
    assert st["upload_kind"] in (1, 2)
    grown = _with(g, np.arange(E - 5, E), rt.HUBER, 1.345)
    _compare_with_fresh(pg_cls, pg, st, grown, x1)
    # a registration onto the graph that holds robust factors: appended in place
    x2 = pg.poses()
    n = g.num_poses
    step = np.array([1.0, 0.0, 0.0])
    gt = np.vstack([g.ground_truth, datasets.compose_xyt(g.ground_truth[n - 1], step)])
    xn = np.vstack([x2, datasets.compose_xyt(x2[n - 1], step)])
    j = n // 3
    z_odo, z_lc = datasets.between_xyt(gt[n - 1], gt[n]), datasets.between_xyt(gt[n], gt[j]) + [0.4, -0.3, 0.05]
    cov = np.diag(datasets.SIGMA ** 2)
    pg.add_vertex(n + 1, *xn[n])
    pg.add_edge(n, n + 1, z_odo, cov)
    pg.add_edge(n + 1, j + 1, z_lc, cov, loss=_lib.PGO_LOSS_HUBER, k=1.345)
    st2 = pg.optimize()
    assert st2["upload_kind"] == 2
    grown2 = copy.copy(grown)
    grown2.keys = np.arange(1, n + 2, dtype=np.uint64)
    grown2.ground_truth = gt
    grown2.edge_k1 = np.concatenate([g.edge_k1, np.array([n, n + 1], dtype=np.uint64)])
    grown2.edge_k2 = np.concatenate([g.edge_k2, np.array([n + 1, j + 1], dtype=np.uint64)])
    grown2.edge_z = np.concatenate([g.edge_z, [z_odo, z_lc]])
    grown2.edge_cov = np.concatenate([g.edge_cov, np.tile(cov.reshape(1, 9), (2, 1))])
    grown2.edge_loss = np.concatenate([grown.edge_loss, [0, rt.HUBER]]).astype(np.int32)
    grown2.edge_loss_k = np.concatenate([grown.edge_loss_k, [1.0, 1.345]])
    _compare_with_fresh(pg_cls, pg, st2, grown2, xn)
    w = pg.edge_weights()
    rp = rt.problem(grown2)
    assert np.abs(w - rt.weights(rp, pn.from_xyt(pg.poses()))).max() <= 1e-10


def test_save_restore_determinism_cauchy(pg_cls, twin_runs):
    gl = twin_runs["cauchy"][0]
    pg = pg_cls.from_dataset(gl)
    pg.save_values()
    st1 = pg.optimize()
    p1 = pg.poses()
    w1 = pg.edge_weights()
    pg.restore_values()
    assert pg.error() == st1["initial_error"]
    st2 = pg.optimize()
    assert st2["final_error"] == st1["final_error"]          # bitwise reproducible
    assert np.array_equal(pg.poses(), p1) and np.array_equal(pg.edge_weights(), w1)
