"""GPU parity: libpgo.so (HIP, gfx950) against the CPU oracle, through the C-ABI.

Tolerances (fp64 throughout):
* linearisation (H blocks, gradient, error): rtol 1e-10 -- same formulas,
  different summation order / FMA contraction;
* PCG step vs the oracle's direct sparse Cholesky: relative 1e-6 in the
  2-norm at pcg_relative_tol 1e-10 (the PCG stops on the preconditioned
  residual, so the step error is bounded by cond(H) x tol);
* optimiser result vs oracle/golden: same accepted-iteration count, final
  error rtol 1e-8, poses within 1e-6 m / 1e-7 rad (KAT graphs: ground truth
  to 1e-9).
"""
import os

import numpy as np
import pytest

from graphslam_amd import datasets

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def angdiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def assert_poses(a, b, tol_xy, tol_th):
    a, b = np.asarray(a), np.asarray(b)
    dxy = np.abs(a[:, :2] - b[:, :2]).max() if len(a) else 0.0
    dth = angdiff(a[:, 2], b[:, 2]).max() if len(a) else 0.0
    assert dxy <= tol_xy and dth <= tol_th, (dxy, dth)


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


def load(name):
    if name == "square":
        return datasets.square_loop()
    if name == "chain":
        return datasets.straight_chain()
    return datasets.make(name)


# ------------------------------------------------------------ linearisation
@pytest.mark.parametrize("name", ["square", "C1", "C1-nn", "C2"])
def test_linearize_parity(pg_cls, oracle_lib, name):
    g = load(name)
    pg = pg_cls.from_dataset(g)
    hd, ho, grad, err = pg.debug_linearize(g.num_edges)
    o = oracle_lib.Oracle(g)
    hd0, ho0, g0, err0 = o.linearize()
    scale_h = np.abs(hd0).max()
    assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
    assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
    assert np.abs(grad - g0).max() <= 1e-10 * max(np.abs(g0).max(), 1.0)
    assert abs(err - err0) <= 1e-10 * max(err0, 1e-30)
    assert abs(pg.error() - o.error()) <= 1e-10 * max(err0, 1e-30)


@pytest.mark.parametrize("name", ["square", "C1", "C1-nn", "C2"])
def test_linearize_cholesky_mode_parity(pg_cls, oracle_lib, name):
    """k_linearize_own + k_linearize_side1 (owner blocks in factor order, W
    hand-off, row sums through LDS) vs the oracle, same tolerance as the
    two-slot sweep; also vs that sweep on the same handle."""
    g = load(name)
    pg = pg_cls.from_dataset(g)
    hd, ho, grad, err = pg.debug_linearize(g.num_edges, cholesky=True)
    hd0, ho0, g0, err0 = oracle_lib.Oracle(g).linearize()
    scale_h = np.abs(hd0).max()
    assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
    assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
    assert np.abs(grad - g0).max() <= 1e-10 * max(np.abs(g0).max(), 1.0)
    assert abs(err - err0) <= 1e-10 * max(err0, 1e-30)
    hd1, ho1, g1, _ = pg.debug_linearize(g.num_edges)
    assert np.abs(hd - hd1).max() <= 1e-12 * scale_h
    assert np.abs(ho - ho1).max() <= 1e-14 * scale_h   # same per-factor arithmetic, no sums
    assert np.abs(grad - g1).max() <= 1e-12 * max(np.abs(g1).max(), 1.0)


def test_linearize_nondiagonal_covariance(pg_cls, oracle_lib):
    g = datasets.make("C1")
    rng = np.random.default_rng(5)
    L = np.tril(rng.normal(size=(g.num_edges, 3, 3)) * 0.02) + np.eye(3) * 0.05
    cov = L @ np.transpose(L, (0, 2, 1))
    g.edge_cov = cov.reshape(-1, 9)
    pg = pg_cls.from_dataset(g)
    hd, ho, grad, err = pg.debug_linearize(g.num_edges)
    hd0, ho0, g0, err0 = oracle_lib.Oracle(g).linearize()
    assert np.allclose(hd, hd0, rtol=1e-10, atol=1e-10 * np.abs(hd0).max())
    assert np.allclose(ho, ho0, rtol=1e-10, atol=1e-10 * np.abs(hd0).max())
    assert abs(err - err0) <= 1e-10 * err0


def test_spmv_parity(pg_cls, oracle_lib):
    from oracle import pgo_numpy as tw
    g = datasets.make("C1-nn")
    pg = pg_cls.from_dataset(g)
    x = np.random.default_rng(1).normal(size=(g.num_poses, 3))
    y = pg.debug_spmv(x, lam=0.37)
    lin = tw.linearize(tw.problem_from_graph(g), tw.from_xyt(g.initial))
    ref = (lin.H @ x.ravel() + 0.37 * x.ravel()).reshape(-1, 3)
    assert np.abs(y - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("name,lam", [("square", 1e-5), ("C1", 1e-5), ("C1-nn", 1e-3), ("C2", 1e-5), ("C2", 1e-9)])
def test_cholesky_step_vs_oracle(pg_cls, oracle_lib, name, lam):
    """GPU supernodal Cholesky vs the oracle's CPU Cholesky (different orderings):
    both exact, so they agree to rounding amplified by cond(H)."""
    g = load(name)
    pg = pg_cls.from_dataset(g)
    d, _ = pg.debug_solve(lam, linear_solver=1)
    rc, d0 = oracle_lib.Oracle(g).solve(lam)
    assert rc == 0
    rel = np.linalg.norm(d - d0) / np.linalg.norm(d0)
    assert rel <= 1e-8, rel   # C2 at lambda 1e-9: cond(H) ~ 1e8, observed 2.6e-9


@pytest.mark.parametrize("name,lam", [("C1", 1e-5), ("C1-nn", 1e-3), ("C2", 1e-5)])
def test_pcg_step_vs_direct_cholesky(pg_cls, oracle_lib, name, lam):
    g = load(name)
    pg = pg_cls.from_dataset(g)
    d, it = pg.debug_solve(lam, linear_solver=0, pcg_relative_tol=1e-12, pcg_max_iterations=200000)
    rc, d0 = oracle_lib.Oracle(g).solve(lam)
    assert rc == 0 and it > 0
    rel = np.linalg.norm(d - d0) / np.linalg.norm(d0)
    assert rel <= 1e-6, rel


def test_cholesky_detects_non_pd(pg_cls):
    """GN on a gauge-free graph reaches the factorisation only through debug_solve:
    the zero pivot must be reported, not silently produce a step."""
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException
    pg = pg_cls()
    pg.add_vertex(1, 0, 0, 0)
    pg.add_vertex(2, 1.1, 0, 0)
    pg.add_edge(1, 2, [1, 0, 0], np.diag([0.01, 0.01, 0.01]))
    with pytest.raises(IndeterminantLinearSystemException):
        pg.debug_solve(-1.0, linear_solver=1)


# ------------------------------------------------------------ full optimiser
@pytest.mark.parametrize("name", ["square", "chain"])
def test_kat_ground_truth(pg_cls, name):
    g = load(name)
    pg = pg_cls.from_dataset(g)
    st = pg.optimize()
    assert st["final_error"] < 1e-18
    assert_poses(pg.poses(), g.ground_truth, 1e-9, 1e-9)


@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["square", "C1", "C1-nn", "C2"])
def test_lm_parity_with_golden(pg_cls, name, solver):
    gold = np.load(os.path.join(GOLDEN, f"golden_{name}.npz"), allow_pickle=False)
    g = load(name)
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(linear_solver=solver)
    assert st["iterations"] == int(gold["iterations"])
    fe = float(gold["final_error"])
    assert abs(st["final_error"] - fe) <= 1e-8 * fe + 1e-18
    assert_poses(pg.poses(), gold["final"], 1e-6, 1e-7)


def test_lm_trace_matches_oracle_c1nn(pg_cls, oracle_lib):
    g = datasets.make("C1-nn")
    o = oracle_lib.Oracle(g).optimize()
    pg = pg_cls.from_dataset(g)
    st = pg.optimize()
    assert st["iterations"] == o.stats["iterations"]
    assert st["inner_iterations"] == o.stats["inner_iterations"]
    assert st["linearizations"] == o.stats["linearizations"]
    assert abs(st["initial_error"] - o.stats["initial_error"]) <= 1e-12 * o.stats["initial_error"]
    assert abs(st["final_error"] - o.stats["final_error"]) <= 1e-11 * o.stats["final_error"]


def test_trace_matches_oracle_c1nn(pg_cls, oracle_lib):
    """pgo_get_trace (per lambda try: accepted steps, lambda, solved, model
    decrease, candidate error, fidelity, accepted, ms) vs the oracle's trace
    on C1-nn: decisions and lambdas identical, values to 1e-8 relative; the
    speculative lambda lanes record the same rows as one lane."""
    g = datasets.make("C1-nn")
    o = oracle_lib.Oracle(g).optimize()
    for lanes in (1, 2):
        pg = pg_cls.from_dataset(g)
        st = pg.optimize(lambda_lanes=lanes)
        tr = pg.trace()
        ot = o.trace
        assert tr.shape == (ot.shape[0], 8)
        for c in (0, 1, 2, 6):   # iteration, lambda, solved, accepted
            assert np.array_equal(tr[:, c], ot[:, c]), c
        fin = np.isfinite(ot[:, 4])
        assert np.array_equal(np.isfinite(tr[:, 4]), fin)
        assert np.allclose(tr[fin, 4], ot[fin, 4], rtol=1e-8)
        ok = np.isfinite(ot[:, 3])
        assert np.allclose(tr[ok, 3], ot[ok, 3], rtol=1e-6, atol=1e-9 * np.abs(ot[ok, 3]).max())
        assert np.all(np.diff(tr[:, 7]) >= 0) and tr[-1, 7] <= st["ms_total"]
        assert tr[tr[:, 6] == 1].shape[0] == st["iterations"]


@pytest.mark.parametrize("kw", [{}, {"lambda_initial": 1e-9}], ids=["defaults", "rejections"])
def test_lm_replay_reproduces_optimize_c2(pg_cls, kw):
    """The host-only replay of the optimiser's control (pgo_debug_lm_replay,
    tests/test_lm_control.py) is what pgo_optimize really does: C2 optimised
    with 1 and 3 lambda lanes, each trace's outcomes fed back to the replay at
    1 and 3 lanes, gives the GPU's own rows (without the wall ms) bit for bit,
    its counters, and -- at the lanes it ran with -- its lambda rounds.
    (lambda_initial 1e-9: four tries of C2 are rejected, so the lanes matter.)"""
    from graphslam_amd.pose_graph import debug_lm_replay, trace_linearisations
    adapt = int(os.environ.get("PGO_LANES_ADAPT", "1"))
    g = datasets.make("C2")
    rejected = 0
    for run_lanes in (1, 3):
        pg = pg_cls.from_dataset(g)
        st = pg.optimize(lambda_lanes=run_lanes, **kw)
        tr = pg.trace()
        rejected += int((tr[:, 6] == 0).sum())
        for lanes in (1, 3):
            r = debug_lm_replay(trace_linearisations(tr), st["initial_error"], 1, lanes, adapt_mode=adapt, **kw)
            assert not r["exhausted"]
            assert r["trace"].tobytes() == np.ascontiguousarray(tr[:, :7]).tobytes(), (run_lanes, lanes)
            for k in ("iterations", "inner_iterations", "linearizations", "status", "stop_reason", "final_error"):
                assert r[k] == st[k], (k, run_lanes, lanes)
            if lanes == run_lanes:
                assert r["lambda_rounds"] == st["lambda_rounds"], (run_lanes, lanes)
    assert rejected > 0 or not kw


def test_stop_reason(pg_cls):
    """pgo_stats.stop_reason tells apart what GTSAM reports as convergence."""
    g = datasets.make("C1")
    pg = pg_cls.from_dataset(g)
    assert pg.optimize(max_outer=1)["stop_reason"] == 3             # PGO_STOP_MAX_OUTER
    pg = pg_cls.from_dataset(g)
    assert pg.optimize(max_iterations=1)["stop_reason"] == 2        # PGO_STOP_MAX_ITER
    pg = pg_cls.from_dataset(datasets.square_loop())
    st = pg.optimize()
    assert st["stop_reason"] in (0, 4) and st["final_error"] < 1e-18


def test_kernel_profile_accounts_every_launch(pg_cls):
    """profile_every: every launch of the profiled factorisations is timed and
    attributed to its kernel family; the Cholesky flops are all accounted."""
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(profile_every=1, max_outer=1, lambda_lanes=1)
    kp = pg.kernel_profile()
    assert kp and all(v["launches"] > 0 and v["ms"] > 0 for v in kp.values())
    nfac = st["kernel_syrk_count"]          # profiled factorisations = every solve here
    assert nfac == st["solves"] >= 1
    assert st["ms_factor_profiled"] > 0 and st["ms_solve_profiled"] > 0
    fl = sum(v["flops"] for k, v in kp.items() if not k.startswith("k_bwd"))
    # the launches' algorithmic flops cover the factorisation's (same formula
    # for the fronts, plus the inverses the GPU forms for its TRSM / solves)
    assert fl >= 0.99 * nfac * st["factor_flops"]


def test_gauss_newton_parity(pg_cls, oracle_lib):
    g = datasets.make("C1")
    o = oracle_lib.Oracle(g).optimize(algorithm=1)
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(algorithm=1)
    assert st["iterations"] == o.stats["iterations"]
    assert abs(st["final_error"] - o.stats["final_error"]) <= 1e-8 * o.stats["final_error"]
    assert_poses(pg.poses(), o.poses, 1e-6, 1e-7)


def test_warm_start_write_back(pg_cls):
    """graph.cpp:130 `initial = poses_opti`: a second optimize starts at the optimum."""
    g = datasets.make("C1")
    pg = pg_cls.from_dataset(g)
    st1 = pg.optimize()
    st2 = pg.optimize()
    assert abs(st2["initial_error"] - st1["final_error"]) <= 1e-9 * st1["final_error"]
    assert st2["final_error"] <= st2["initial_error"]


def test_save_restore_and_determinism(pg_cls):
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    pg.save_values()
    st1 = pg.optimize()
    p1 = pg.poses()
    pg.restore_values()
    assert abs(pg.error() - st1["initial_error"]) == 0.0
    st2 = pg.optimize()
    assert st2["final_error"] == st1["final_error"]          # bitwise reproducible
    assert np.array_equal(pg.poses(), p1)


def test_fronts_rezeroed_after_marginals(pg_cls):
    """The backward solve zeroes the fronts behind itself (the next factorisation
    skips its zeroing); a factorisation without a solve (the marginals) leaves
    them dirty, and the next optimize must zero them first: results bitwise
    equal to a run that never computed marginals, graph replay and eager."""
    g = datasets.make("C2")
    ref = pg_cls.from_dataset(g)
    ref.save_values()
    st0 = ref.optimize()
    p0 = ref.poses()
    for graphs in (1, 0):
        pg = pg_cls.from_dataset(g)
        pg.save_values()
        pg.optimize(use_graphs=graphs, max_outer=2)
        pg.marginal_covariances(np.asarray(g.keys)[:8])
        pg.restore_values()
        st = pg.optimize(use_graphs=graphs)
        assert st["final_error"] == st0["final_error"], graphs
        assert np.array_equal(pg.poses(), p0), graphs


@pytest.mark.parametrize("name", ["C2", "C1-nn"])
def test_poisoned_workspace_bitwise(pg_cls, name):
    """Round 4's r04b failure (a first optimize off in the 12th digit, then a
    non-positive pivot in the marginals) is the signature of an element read
    before the factorisation wrote it.  Every element a factorisation must
    write first -- the fronts' lower trapezoids, the frontal vectors, the
    diagonal inverses, every lambda lane -- is set to NaN between two
    optimizes: the second must equal a clean run bit for bit (a stale read
    would carry the NaN into the factor), replayed graphs and eager launches."""
    g = datasets.make(name)
    ref = pg_cls.from_dataset(g)
    ref.save_values()
    st0 = ref.optimize(lambda_lanes=3)
    p0 = ref.poses()
    for graphs in (1, 0):
        pg = pg_cls.from_dataset(g)
        pg.save_values()
        pg.optimize(use_graphs=graphs, lambda_lanes=3, max_outer=2)
        pg.debug_poison_fronts()
        pg.restore_values()
        st = pg.optimize(use_graphs=graphs, lambda_lanes=3)
        assert st["final_error"] == st0["final_error"], graphs
        assert np.array_equal(pg.poses(), p0), graphs


_KNOB_RUN = r"""
import hashlib, json, sys
sys.path.insert(0, {root!r})
from graphslam_amd import datasets
from graphslam_amd.pose_graph import PoseGraph, default_params
pg = PoseGraph.from_dataset(datasets.make({name!r}))
st = pg.optimize(default_params(lambda_lanes=3, profile_every=1))
prof = pg.kernel_profile()
print(json.dumps({{"final": st["final_error"].hex(), "poses": hashlib.sha256(pg.poses().tobytes()).hexdigest(),
                   "split_launches": prof.get("k_step_diag", {{}}).get("launches", 0),
                   "vec_launches": prof.get("k_vec_assemble", {{}}).get("launches", 0)}}))
"""


def test_step_split_bitwise_fresh_processes(pgo_lib):
    """The split step (k_step_diag beside k_panel_syrk_lds on a fifth stream,
    then k_first_trsm; PGO_STEP_SPLIT), the deferred far updates (PGO_FAR) and
    the frontal vectors in their own side-stream launch instead of the tile
    assembly's (PGO_VEC_FUSE=0) reorder launches across streams, never the
    arithmetic: forced on C2 (every step split), each in a fresh process, the
    trajectory must be bitwise the default's, and the forced runs must actually
    have taken their path."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _KNOB_RUN.format(root=root, name="C2")
    res = {}
    for tag, env in (("default", {}), ("split", {"PGO_STEP_SPLIT": "1"}), ("nosplit", {"PGO_STEP_SPLIT": "0"}),
                     ("split_far", {"PGO_STEP_SPLIT": "1", "PGO_FAR": "1"}), ("vec_sep", {"PGO_VEC_FUSE": "0"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["split"]["split_launches"] > 0 and res["split_far"]["split_launches"] > 0
    assert res["nosplit"]["split_launches"] == 0
    assert res["vec_sep"]["vec_launches"] > 0 and res["default"]["vec_launches"] == 0
    for tag in ("split", "nosplit", "split_far", "vec_sep"):
        assert (res[tag]["final"], res[tag]["poses"]) == (res["default"]["final"], res["default"]["poses"]), tag


# ------------------------------------------------------------ headline size
@pytest.mark.parametrize("solver", [1, 0])
def test_c3_full_size_against_golden(pg_cls, solver):
    """C3 (100k poses / 500k edges): the oracle's trajectory -- LM gives up at
    lambda >= 1e5 after 7 accepted steps from the dead-reckoned start -- and
    its final error, plus a 1000-pose sample of the final values.  Cholesky
    (exact solves, the oracle's per-try trace): final error rel 3e-8 (observed
    8.1e-9 on the box), poses 1e-6 m / 1e-7 rad (observed 1.6e-7 m, 1.7e-8
    rad), as for C1 / C2; PCG (inexact solves, relative residual
    1e-10, so the 7 accepted steps differ slightly): final error rel 1e-6,
    poses 1e-4 m / 1e-5 rad.  The observed differences are printed."""
    gold = np.load(os.path.join(GOLDEN, "golden_C3.npz"), allow_pickle=False)
    g = datasets.make("C3")
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(linear_solver=solver)
    if solver == 1:   # exact solves: the oracle's per-try trace
        assert st["inner_iterations"] == int(gold["inner_iterations"])
        assert st["linearizations"] == int(gold["linearizations"])
    assert abs(st["initial_error"] - float(gold["initial_error"])) <= 1e-10 * float(gold["initial_error"])
    assert st["iterations"] == int(gold["iterations"])
    fe = float(gold["final_error"])
    idx = gold["sample_index"]
    x = pg.poses()[idx]
    dxy = np.abs(x[:, :2] - gold["final_sample"][:, :2]).max()
    dth = np.abs(np.angle(np.exp(1j * (x[:, 2] - gold["final_sample"][:, 2])))).max()
    print(f"C3 solver {solver}: final error rel diff {abs(st['final_error'] - fe) / fe:.2e}, "
          f"max |dxy| {dxy:.2e} m, max |dtheta| {dth:.2e} rad")
    tol_e, tol_xy, tol_th = (3e-8, 1e-6, 1e-7) if solver == 1 else (1e-6, 1e-4, 1e-5)
    assert abs(st["final_error"] - fe) <= tol_e * fe
    assert_poses(x, gold["final_sample"], tol_xy, tol_th)


def test_c3_gauss_newton_against_golden(pg_cls):
    """GTSAM's Gauss-Newton (PGO_ALG_GN) on C3 from the dead-reckoned values
    against the C oracle's run (golden_C3-gn.npz): the step count, the error
    after every step, the final error and a 1000-pose sample of the final
    values.  Undamped steps from a start 3e5 x the optimum's error amplify the
    two factorisations' different rounding: errors rel 3e-7, poses 3e-5 m /
    5e-6 rad, about 5x the differences observed on the round-6 build (6.8e-8,
    6.0e-6 m, 9.0e-7 rad, profiles/r06t_diffs.log; round 5: 1e-6, 1e-4 m,
    1e-5 rad); the observed differences are printed."""
    gold = np.load(os.path.join(GOLDEN, "golden_C3-gn.npz"), allow_pickle=False)
    g = datasets.make("C3")
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(algorithm=1)
    assert st["iterations"] == int(gold["iterations"])
    assert st["linearizations"] == int(gold["linearizations"])
    errs = pg.trace()[:, 4]
    x = pg.poses()[gold["sample_index"]]
    dxy = np.abs(x[:, :2] - gold["final_sample"][:, :2]).max()
    dth = np.abs(np.angle(np.exp(1j * (x[:, 2] - gold["final_sample"][:, 2])))).max()
    print(f"C3 GN: per-step error rel diff {np.max(np.abs(errs / gold['errors'] - 1)):.2e}, "
          f"max |dxy| {dxy:.2e} m, max |dtheta| {dth:.2e} rad")
    assert np.allclose(errs, gold["errors"], rtol=3e-7, atol=0)
    fe = float(gold["final_error"])
    assert abs(st["final_error"] - fe) <= 3e-7 * fe
    assert_poses(x, gold["final_sample"], 3e-5, 5e-6)


def test_c3_first_two_linearisations_vs_numpy_twin(pg_cls):
    """The headline size pinned by a second, independent restatement: the
    numpy/SuperLU twin's first 2 linearisations of C3 (golden_C3-numpy2.npz)."""
    gold = np.load(os.path.join(GOLDEN, "golden_C3-numpy2.npz"), allow_pickle=False)
    g = datasets.make("C3")
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(max_outer=2)
    tr = pg.trace()
    gt = gold["trace"]
    assert tr.shape[0] == gt.shape[0]
    assert np.array_equal(tr[:, 1], gt[:, 1]) and np.array_equal(tr[:, 6], gt[:, 3])
    ok = np.isfinite(gt[:, 2])
    assert np.allclose(tr[ok, 4], gt[ok, 2], rtol=1e-6)
    fe = float(gold["final_error"])
    assert abs(st["final_error"] - fe) <= 1e-6 * fe
    assert_poses(pg.poses()[gold["sample_index"]], gold["final_sample"], 1e-5, 1e-6)


def test_c3_whole_trajectory_vs_numpy_twin(pg_cls):
    """The headline run end to end against the second, independent restatement
    (golden_C3-numpy.npz: numpy / SuperLU, all 24 lambda tries): the same tries
    and accept decisions, the candidate error of every solved try to 2e-6
    relative and the final error to 1e-6 (the two CPU restatements agree to
    8.8e-7 / 4.2e-7, tests/test_oracle.py), a 1000-pose sample to 1e-4 m /
    5e-6 rad (restatements: 2.9e-5 m, 6.5e-7 rad).  The observed differences
    are printed."""
    gold = np.load(os.path.join(GOLDEN, "golden_C3-numpy.npz"), allow_pickle=False)
    g = datasets.make("C3")
    pg = pg_cls.from_dataset(g)
    st = pg.optimize()
    tr, gt = pg.trace(), gold["trace"]
    assert tr.shape[0] == gt.shape[0] == int(gold["inner_iterations"])
    assert np.array_equal(tr[:, 1], gt[:, 1]) and np.array_equal(tr[:, 6], gt[:, 3])
    assert st["iterations"] == int(gold["iterations"])
    ok = np.isfinite(gt[:, 2])
    idx = gold["sample_index"]
    x = pg.poses()[idx]
    fe = float(gold["final_error"])
    print(f"C3 vs numpy twin: per-try error rel diff {np.max(np.abs(tr[ok, 4] / gt[ok, 2] - 1)):.2e}, "
          f"final {abs(st['final_error'] - fe) / fe:.2e}, max |dxy| {np.abs(x[:, :2] - gold['final_sample'][:, :2]).max():.2e} m")
    assert np.allclose(tr[ok, 4], gt[ok, 2], rtol=2e-6, atol=0)
    assert abs(st["final_error"] - fe) <= 1e-6 * fe
    assert_poses(x, gold["final_sample"], 1e-4, 5e-6)


# ------------------------------------------------------------ edge cases
def test_empty_graph(pg_cls):
    pg = pg_cls()
    st = pg.optimize()
    assert st["final_error"] == 0.0 and st["iterations"] == 0


def test_single_vertex_prior(pg_cls):
    pg = pg_cls()
    pg.add_vertex(1, 0.3, -0.2, 0.4)
    pg.add_prior(1, [1.0, 2.0, 0.5], np.diag([0.01, 0.01, 0.01]))
    pg.optimize()
    assert_poses(pg.poses(), [[1.0, 2.0, 0.5]], 1e-9, 1e-9)


def test_no_prior_gauge_freedom_lm(pg_cls, oracle_lib):
    """No prior: H is singular; LM's damping keeps the system solvable."""
    g = datasets.square_loop()
    g.prior_keys = g.prior_keys[:0]
    g.prior_pose = g.prior_pose[:0]
    g.prior_cov = g.prior_cov[:0]
    pg = pg_cls.from_dataset(g)
    st = pg.optimize()
    assert st["final_error"] < 1e-12


def test_gauss_newton_singular_raises(pg_cls):
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException
    pg = pg_cls()
    pg.add_vertex(1, 0, 0, 0)
    pg.add_vertex(2, 1.1, 0, 0)
    pg.add_edge(1, 2, [1, 0, 0], np.diag([0.01, 0.01, 0.01]))   # no prior: gauge freedom
    with pytest.raises(IndeterminantLinearSystemException):
        pg.optimize(algorithm=1)


def test_unknown_key_at_optimize(pg_cls):
    from graphslam_amd.pose_graph import ValuesKeyDoesNotExist
    pg = pg_cls()
    pg.add_vertex(1, 0, 0, 0)
    pg.add_edge(1, 5, [1, 0, 0], np.diag([0.01, 0.01, 0.01]))
    with pytest.raises(ValuesKeyDoesNotExist):
        pg.optimize()


def test_duplicate_and_parallel_edges(pg_cls, oracle_lib):
    """Two factors between the same pair (both orientations) are summed."""
    g = datasets.square_loop()
    i, j = g.edge_index()
    extra_z = datasets.between_xyt(g.ground_truth[j[:3]], g.ground_truth[i[:3]]) + 0.01
    g.edge_k1 = np.concatenate([g.edge_k1, g.edge_k2[:3], g.edge_k1[:2]])
    g.edge_k2 = np.concatenate([g.edge_k2, g.edge_k1[:3], g.edge_k2[:2]])
    g.edge_z = np.concatenate([g.edge_z, extra_z, g.edge_z[:2] - 0.02])
    g.edge_cov = np.concatenate([g.edge_cov, g.edge_cov[:5]])
    pg = pg_cls.from_dataset(g)
    st = pg.optimize()
    o = oracle_lib.Oracle(g).optimize()
    assert abs(st["final_error"] - o.stats["final_error"]) <= 1e-9 * o.stats["final_error"]
    assert_poses(pg.poses(), o.poses, 1e-7, 1e-8)


def test_arbitrary_keys_and_insertion_order(pg_cls, oracle_lib):
    g = datasets.make("C1")
    perm = np.random.default_rng(2).permutation(g.num_poses)
    keys = (np.arange(g.num_poses, dtype=np.uint64) * 7919 + 2 ** 33)
    pg = pg_cls()
    pg.add_vertices(keys[perm], g.initial[perm])
    pg.add_prior(int(keys[0]), g.prior_pose[0], g.prior_cov[0])
    i, j = g.edge_index()
    pg.add_edges(keys[i], keys[j], g.edge_z, g.edge_cov)
    pg.optimize()
    gold = np.load(os.path.join(GOLDEN, "golden_C1.npz"), allow_pickle=False)
    assert_poses(pg.poses(keys), gold["final"], 1e-6, 1e-7)


def test_gtsam_mirror_end_to_end(pgo_lib):
    """The graph.cpp call sequence, verbatim in the mirror's names."""
    from graphslam_amd import gtsam as gt
    g = datasets.square_loop()
    graph = gt.NonlinearFactorGraph()
    initial = gt.Values()
    for k, p in zip(g.keys, g.initial):
        initial.insert(int(k), gt.Pose2(*p))
    graph.add(gt.PriorFactorPose2(1, gt.Pose2(0, 0, 0), gt.noiseModel.Gaussian.Covariance(np.diag([0.01] * 3))))
    for k1, k2, z, c in zip(g.edge_k1, g.edge_k2, g.edge_z, g.edge_cov):
        graph.add(gt.BetweenFactorPose2(int(k1), int(k2), gt.Pose2(*z),
                                        gt.noiseModel.Gaussian.Covariance(c.reshape(3, 3))))
    opt = gt.LevenbergMarquardtOptimizer(graph, initial)
    poses_opti = opt.optimize()
    for k, p in zip(g.keys, g.ground_truth):
        q = poses_opti.atPose2(int(k))
        assert abs(q.x() - p[0]) < 1e-9 and abs(q.y() - p[1]) < 1e-9
    assert graph.error(poses_opti) < 1e-18
    e1 = opt.error()
    opt.optimize()                       # GTSAM state: continues from the optimum
    assert opt.stats["initial_error"] == e1 and opt.error() <= e1


# ------------------------------------------------------------ marginals
@pytest.mark.parametrize("name,at", [("square", "initial"), ("C1", "initial"), ("C1", "optimum"),
                                     ("C1-nn", "optimum"), ("C2", "initial")])
def test_marginal_covariances(pg_cls, name, at):
    """pgo_marginal_covariances vs the oracle's columns of H^-1 (sparse LU) at the
    same values: both exact, agreement to rounding amplified by cond(H)."""
    from oracle import pgo_numpy as pn
    g = load(name)
    pg = pg_cls.from_dataset(g)
    if at == "optimum":
        pg.optimize()
    n = g.num_poses
    idx = sorted(set([0, 1, n // 3, n // 2, n - 2, n - 1]))
    keys = np.asarray(g.keys)[idx]
    cov = pg.marginal_covariances(keys)
    prob = pn.problem_from_graph(g)
    ref = pn.marginal_covariances(prob, pn.from_xyt(pg.poses()), idx)
    for q in range(len(idx)):
        assert np.abs(cov[q] - cov[q].T).max() <= 1e-12 * np.abs(cov[q]).max()
        assert np.abs(cov[q] - ref[q]).max() <= 1e-8 * np.abs(ref[q]).max(), (idx[q], cov[q], ref[q])


def test_marginals_batch_and_errors(pg_cls):
    """A batch larger than one launch (256 keys), repeated keys, an unknown key,
    and a graph without a prior (singular H, GTSAM's Cholesky throws)."""
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException, PgoError
    g = load("C1")
    pg = pg_cls.from_dataset(g)
    keys = np.asarray(g.keys)[np.arange(0, g.num_poses, 3)]
    keys = np.concatenate([keys, keys[:5]])
    cov = pg.marginal_covariances(keys)
    assert cov.shape == (len(keys), 3, 3)
    assert np.array_equal(cov[-5:], cov[:5])            # deterministic
    with pytest.raises(PgoError):
        pg.marginal_covariances([10 ** 12])
    free = pg_cls()
    free.add_vertices(np.array([1, 2], dtype=np.uint64), np.array([[0, 0, 0], [1, 0, 0]], float))
    free.add_edge(1, 2, [1, 0, 0], np.diag([0.01, 0.01, 0.001]))
    with pytest.raises(IndeterminantLinearSystemException):
        free.marginal_covariances([1])


def test_gtsam_mirror_marginals(pgo_lib):
    from graphslam_amd import gtsam
    graph, values = gtsam.NonlinearFactorGraph(), gtsam.Values()
    cov = np.diag([0.01, 0.01, 0.01])
    graph.add(gtsam.PriorFactorPose2(1, gtsam.Pose2(0, 0, 0), gtsam.noiseModel.Gaussian.Covariance(cov)))
    for k in range(1, 6):
        values.insert(k, gtsam.Pose2(k - 1.0, 0.0, 0.0))
    for k in range(1, 5):
        graph.add(gtsam.BetweenFactorPose2(k, k + 1, gtsam.Pose2(1, 0, 0),
                                           gtsam.noiseModel.Gaussian.Covariance(np.diag([0.05 ** 2, 0.05 ** 2, 0.01]))))
    m = gtsam.Marginals(graph, values)
    c1, c5 = m.marginalCovariance(1), m.marginalCovariance(5)
    assert np.allclose(c1, cov, rtol=1e-12, atol=1e-15)   # a chain leaves the prior pose at the prior
    assert c5[0, 0] > c1[0, 0] and c5[1, 1] > c1[1, 1] and c5[2, 2] > c1[2, 2]   # uncertainty grows


def test_cpp_adapter_on_gpu(tmp_path, pgo_lib):
    """graph.cpp's call sequence through include/pgo_gtsam.hpp, optimize + Marginals, on the GPU."""
    import subprocess
    from test_abi import build_graph_cpp_style
    exe = build_graph_cpp_style(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "factors 9" and len(lines) == 11, r.stdout
    assert lines[1] == "second 1 1", r.stdout      # optimize() twice: continues from the optimum
    xyt = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[2:10]])
    assert np.all(np.isfinite(xyt))
    cov = [float(v) for v in lines[10].split()[1:]]
    assert lines[10].startswith("cov8") and all(v > 0 for v in cov)


# ------------------------------------------------------------ C5 (1M poses / 5M edges)
def test_c5_full_size_against_fixture(pg_cls):
    """BASELINE configs[4] at full size on one MI355X (2.4 TFLOP per
    factorisation, ~34 GB of fronts): the first linearisation (gradient and H
    diagonal blocks at every 1000th pose, error), the Cholesky step at
    lambda = 1e-5 (sampled, and its 2-norm) and the first LM linearisation's
    lambda tries, against the C oracle's (tests/golden/golden_C5.npz)."""
    gold = np.load(os.path.join(GOLDEN, "golden_C5.npz"), allow_pickle=False)
    g = datasets.make("C5")
    import sys
    sys.path.insert(0, GOLDEN)
    from make_golden import input_digest
    assert input_digest(g) == str(gold["digest"])
    idx = gold["sample_index"]
    pg = pg_cls.from_dataset(g)
    hd, _, grad, err = pg.debug_linearize(g.num_edges, cholesky=True)
    e0 = float(gold["initial_error"])
    assert abs(err - e0) <= 1e-10 * e0
    assert np.abs(grad[idx] - gold["grad_sample"]).max() <= 1e-10 * np.abs(gold["grad_sample"]).max()
    assert np.abs(hd[idx] - gold["hdiag_sample"]).max() <= 1e-10 * np.abs(gold["hdiag_sample"]).max()
    # the same linearisation against the numpy twin (a second, independent source)
    tw = np.load(os.path.join(GOLDEN, "golden_C5-numpy.npz"), allow_pickle=False)
    assert str(tw["digest"]) == str(gold["digest"])
    e1 = float(tw["initial_error"])
    assert abs(err - e1) <= 1e-10 * e1
    assert np.abs(grad[idx] - tw["grad_sample"]).max() <= 1e-10 * np.abs(tw["grad_sample"]).max()
    hd9 = hd[idx].reshape(-1, 9)
    assert np.abs(hd9 - tw["hdiag_sample"]).max() <= 1e-10 * np.abs(tw["hdiag_sample"]).max()
    del hd, grad
    d, _ = pg.debug_solve(float(gold["delta_lambda"]))
    dn = float(gold["delta_norm"])
    assert abs(np.linalg.norm(d) - dn) <= 1e-8 * dn
    assert np.abs(d[idx] - gold["delta_sample"]).max() <= 1e-8 * np.abs(d).max()
    st = pg.optimize(max_outer=1)
    tr, gt = pg.trace(), gold["trace"]
    assert tr.shape[0] == gt.shape[0]
    assert np.array_equal(tr[:, 1], gt[:, 1]) and np.array_equal(tr[:, 6], gt[:, 3])
    ok = np.isfinite(gt[:, 2])
    assert np.allclose(tr[ok, 4], gt[ok, 2], rtol=1e-8)
    ea = float(gold["error_after"])
    assert abs(st["final_error"] - ea) <= 1e-8 * ea
    assert_poses(pg.poses()[idx], gold["poses_after_sample"], 1e-6, 1e-7)


def _c5_trajectory_against_fixture(pg_cls, n_lin, rtol=3e-8, tol_xy=1e-6, tol_th=1e-7):
    gold = np.load(os.path.join(GOLDEN, f"golden_C5-lm{n_lin}.npz"), allow_pickle=False)
    g = datasets.make("C5")
    import sys
    sys.path.insert(0, GOLDEN)
    from make_golden import input_digest
    assert input_digest(g) == str(gold["digest"])
    pg = pg_cls.from_dataset(g)
    st = pg.optimize(max_outer=n_lin, lambda_lanes=3)
    tr, gt = pg.trace(), gold["trace"]
    assert st["linearizations"] == int(gold["linearizations"]) == n_lin
    assert st["iterations"] == int(gold["iterations"])
    assert tr.shape[0] == gt.shape[0] == int(gold["inner_iterations"])
    assert np.array_equal(tr[:, 1], gt[:, 1]) and np.array_equal(tr[:, 6], gt[:, 3])
    ok = np.isfinite(gt[:, 2])
    assert np.array_equal(np.isfinite(tr[:, 4]), ok)
    fe = float(gold["final_error"])
    x = pg.poses()[gold["sample_index"]]
    print(f"C5 lm{n_lin}: per-try error rel diff {np.max(np.abs(tr[ok, 4] / gt[ok, 2] - 1)):.2e}, "
          f"final {abs(st['final_error'] - fe) / fe:.2e}, "
          f"max |dxy| {np.abs(x[:, :2] - gold['final_sample'][:, :2]).max():.2e} m, "
          f"max |dtheta| {angdiff(x[:, 2], gold['final_sample'][:, 2]).max():.2e} rad")
    assert np.allclose(tr[ok, 4], gt[ok, 2], rtol=rtol, atol=0)
    assert abs(st["final_error"] - fe) <= rtol * fe
    assert_poses(x, gold["final_sample"], tol_xy, tol_th)


def test_c5_five_linearisations_against_fixture(pg_cls):
    """C5 past its first linearisation (round 6): the C oracle's first 5 LM
    linearisations of the 1M-pose graph (golden_C5-lm5.npz, 18 lambda tries:
    10, 1, 2, 2, 3) -- the same tries, lambdas and accept decisions, every
    solved try's candidate error, the error after the 5th linearisation and a
    1000-pose sample of the values, at the C3 Cholesky tolerances (errors rel
    3e-8, poses 1e-6 m / 1e-7 rad).  Run with the bench's 3 lambda lanes
    (bitwise the sequential search, test_lanes_match_sequential).  The observed
    differences are printed."""
    _c5_trajectory_against_fixture(pg_cls, 5)


def test_c5_twenty_five_linearisations_against_fixture(pg_cls):
    """The same over the C oracle's first 25 linearisations of C5
    (golden_C5-lm25.npz: a quarter of the bench's timed c5 line, whose 100
    linearisations and 208 tries no CPU fixture covers whole), same tolerances."""
    _c5_trajectory_against_fixture(pg_cls, 25)


def test_c5_whole_timed_trajectory_against_fixture(pg_cls):
    """The same over the bench's whole c5 line: the C oracle's 100
    linearisations of C5 (golden_C5-lm100.npz, 208 tries, stopped at GTSAM's
    maxIterations): every try's lambda and accept decision identical; the
    errors and values drift apart over the 100 damped steps (the bench's own
    run ends 3.0e-8 relative from the oracle's chi^2 of 3.6e12, far from the
    optimum), so this one is held to rel 1e-6 and 1e-3 m / 1e-4 rad."""
    _c5_trajectory_against_fixture(pg_cls, 100, rtol=1e-6, tol_xy=1e-3, tol_th=1e-4)


# ------------------------------------------------------------ incremental re-solve
def _extend(g, x_now, new_pairs, n_new, rng):
    """g plus `new_pairs` loop closures (exact ground-truth measurements) and
    `n_new` appended poses continuing the walk (odometry + one closure each to an
    old pose); returns (extended graph, its initial values = x_now + dead-reckoned
    new poses, the appended vertices / edges)."""
    from graphslam_amd.datasets import PoseGraph as DG, between_xyt, compose_xyt, _diag_cov, SIGMA
    n = g.num_poses
    gt = np.array(g.ground_truth)
    init = np.array(x_now)
    ei, ej = [], []
    for i, j in new_pairs:
        ei.append(i)
        ej.append(j)
    for k in range(n_new):
        v = n + k
        step = np.array([1.0, 0.0, (np.pi / 2) * (k % 3 == 2)])
        gt = np.vstack([gt, compose_xyt(gt[v - 1], step)])
        init = np.vstack([init, compose_xyt(init[v - 1], step)])
        ei.append(v - 1)
        ej.append(v)
        ei.append(v)
        ej.append(int(rng.integers(0, n - 20)))
    ei, ej = np.array(ei), np.array(ej)
    z = between_xyt(gt[ei], gt[ej])
    keys = np.arange(1, n + n_new + 1, dtype=np.uint64)
    ext = DG(name="ext", keys=keys, initial=init, ground_truth=gt,
             edge_k1=np.concatenate([g.edge_k1, (ei + 1).astype(np.uint64)]),
             edge_k2=np.concatenate([g.edge_k2, (ej + 1).astype(np.uint64)]),
             edge_z=np.concatenate([g.edge_z, z]), edge_cov=np.concatenate([g.edge_cov, _diag_cov(SIGMA, len(ei))]),
             prior_keys=g.prior_keys, prior_pose=g.prior_pose, prior_cov=g.prior_cov)
    return ext, init, (ei, ej, z)


@pytest.mark.parametrize("n_new", [0, 6])
def test_incremental_append_matches_oracle(pg_cls, oracle_lib, n_new):
    """graph.cpp:180-200 / :130: after an optimize, loop closures (parallel to
    existing ones -- inside the plan's fill -- and new ones) and appended poses
    are added to the same handle; the next optimize keeps the resident values
    bit for bit, refreshes the solver plan incrementally (no full analysis) and
    matches the oracle's optimize of the extended graph from the same values."""
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    pg.optimize()
    x_now = pg.poses()
    rng = np.random.default_rng(11)
    i_lc, j_lc = g.edge_index()
    par = [(int(i_lc[q]), int(j_lc[q])) for q in rng.choice(np.arange(g.num_poses - 1, g.num_edges), 8)]
    newp = [(int(a), int(a) - 30 - int(rng.integers(0, 50))) for a in rng.integers(200, g.num_poses, 4)]
    ext, init, (ei, ej, z) = _extend(g, x_now, par + newp, n_new, rng)
    for v in range(g.num_poses, g.num_poses + n_new):
        pg.add_vertex(v + 1, *init[v])
    cov = np.diag(datasets.SIGMA ** 2)
    for a, b, zz in zip(ei, ej, z):
        pg.add_edge(int(a) + 1, int(b) + 1, zz, cov)
    st = pg.optimize()
    assert st["plan_update"] in (1, 2, 4)                 # no new nested dissection
    assert abs(st["initial_error"] - oracle_lib.Oracle(ext).error(init)) <= 1e-9 * st["initial_error"]
    ref = oracle_lib.Oracle(ext).optimize(init=init)
    assert st["iterations"] == ref.stats["iterations"]
    assert abs(st["final_error"] - ref.stats["final_error"]) <= 1e-8 * ref.stats["final_error"]
    assert_poses(pg.poses(), ref.poses, 1e-6, 1e-7)


def _registrations(pg_cls, g, k, seed=7, lanes=1):
    """The live node's per-registration re-solve on one handle: k times a new
    keyframe (dead-reckoned), its odometry factor and one loop closure to an
    earlier keyframe, then optimize; returns the stats and the final values."""
    from graphslam_amd.datasets import between_xyt, compose_xyt
    pg = pg_cls.from_dataset(g)
    pg.optimize(lambda_lanes=lanes)
    rng = np.random.default_rng(seed)
    n = g.num_poses
    gt = np.array(g.ground_truth)
    x = pg.poses()
    cov = np.diag(datasets.SIGMA ** 2)
    sts = []
    for r in range(k):
        v = n + r
        step = np.array([1.0, 0.0, 0.0])
        gt = np.vstack([gt, compose_xyt(gt[v - 1], step)])
        x = np.vstack([x, compose_xyt(x[v - 1], step)])
        j = int(rng.integers(0, v - 20))
        pg.add_vertex(v + 1, *x[v])
        pg.add_edge(v, v + 1, between_xyt(gt[v - 1], gt[v]), cov)
        pg.add_edge(v + 1, j + 1, between_xyt(gt[v], gt[j]), cov)
        sts.append(pg.optimize(lambda_lanes=lanes))
    return sts, pg.poses()


@pytest.mark.parametrize("lanes", [1, 3])
def test_append_in_place_matches_full_upload(pg_cls, monkeypatch, lanes):
    """A registration's keyframe, odometry and loop closure are appended to the
    device graph in place (pgo_stats.upload_kind 2: only the new factors, the
    per-row arrays and the slots uploaded) -- bitwise the same optimisations as
    the full re-upload of the grown graph (PGO_NO_APPEND=1, upload_kind 1)."""
    g = datasets.make("C2")
    monkeypatch.delenv("PGO_NO_APPEND", raising=False)
    a, xa = _registrations(pg_cls, g, 3, lanes=lanes)
    monkeypatch.setenv("PGO_NO_APPEND", "1")
    b, xb = _registrations(pg_cls, g, 3, lanes=lanes)
    assert [s["upload_kind"] for s in a] == [2, 2, 2] and [s["upload_kind"] for s in b] == [1, 1, 1]
    for sa, sb in zip(a, b):
        assert sa["plan_update"] == sb["plan_update"] and sa["iterations"] == sb["iterations"]
        assert sa["inner_iterations"] == sb["inner_iterations"] and sa["final_error"] == sb["final_error"]
    np.testing.assert_array_equal(xa, xb)


def test_pcg_after_cholesky_and_append_matches_fresh_handle(pg_cls):
    """A Cholesky optimize binds the plan's owner bits to the device slots; an
    in-place append then rewrites only the rows from the first changed one with
    the pre-plan codes.  A PCG optimize on that handle must count every factor
    exactly once in its model decrease (k_model_decrease, `se & 2`), i.e. run
    the same optimisation as a fresh handle of the grown graph from the same
    values (the mixed codes double-counted factors spanning the
    first changed row)."""
    from graphslam_amd.datasets import PoseGraph as DG, between_xyt, compose_xyt, _diag_cov
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    pg.optimize(max_outer=2)
    n = g.num_poses
    gt = np.array(g.ground_truth)
    x = pg.poses()
    step = np.array([1.0, 0.0, 0.0])
    gt = np.vstack([gt, compose_xyt(gt[n - 1], step)])
    x = np.vstack([x, compose_xyt(x[n - 1], step)])
    cov = np.diag(datasets.SIGMA ** 2)
    j = n // 3   # the closure's target row: many old factors span it
    new = [(n - 1, n), (n, j)]
    pg.add_vertex(n + 1, *x[n])
    for a, b in new:
        pg.add_edge(a + 1, b + 1, between_xyt(gt[a], gt[b]), cov)
    kw = dict(linear_solver=0, max_outer=3, pcg_relative_tol=1e-10)   # PGO_SOLVER_PCG
    st = pg.optimize(**kw)
    assert st["upload_kind"] == 2
    ei = np.array([a for a, _ in new])
    ej = np.array([b for _, b in new])
    fresh = pg_cls.from_dataset(DG(
        name="grown", keys=np.arange(1, n + 2, dtype=np.uint64), initial=x, ground_truth=gt,
        edge_k1=np.concatenate([g.edge_k1, (ei + 1).astype(np.uint64)]),
        edge_k2=np.concatenate([g.edge_k2, (ej + 1).astype(np.uint64)]),
        edge_z=np.concatenate([g.edge_z, between_xyt(gt[ei], gt[ej])]),
        edge_cov=np.concatenate([g.edge_cov, _diag_cov(datasets.SIGMA, len(ei))]),
        prior_keys=g.prior_keys, prior_pose=g.prior_pose, prior_cov=g.prior_cov), device=0)
    ref = fresh.optimize(**kw)
    assert st["iterations"] == ref["iterations"] and st["inner_iterations"] == ref["inner_iterations"]
    assert abs(st["final_error"] - ref["final_error"]) <= 1e-12 * ref["final_error"]
    np.testing.assert_allclose(pg.poses(), fresh.poses(), rtol=0, atol=1e-9)


@pytest.mark.parametrize("lanes", [1, 3])
def test_registrations_plan_append_matches_oracle(pg_cls, oracle_lib, lanes):
    """The live registrations (one keyframe, its odometry and one loop closure
    each) go into the solver's plan incrementally (plan_update 4: the new pose
    eliminated last, rows added along its fill paths, no re-analysis), with the
    lanes and workspaces kept -- each re-solve matches the oracle's optimize of
    the grown graph from the same values."""
    g = datasets.make("C2")
    pg = pg_cls.from_dataset(g)
    pg.optimize(lambda_lanes=lanes)
    rng = np.random.default_rng(5)
    cov = np.diag(datasets.SIGMA ** 2)
    for r in range(3):
        ext, init, (ei, ej, z) = _extend(g, pg.poses(), [], 1, rng)
        v = g.num_poses
        pg.add_vertex(v + 1, *init[v])
        for a, b, zz in zip(ei, ej, z):
            pg.add_edge(int(a) + 1, int(b) + 1, zz, cov)
        st = pg.optimize(lambda_lanes=lanes)
        assert st["plan_update"] == 4 and st["upload_kind"] == 2
        ref = oracle_lib.Oracle(ext).optimize(init=init)
        assert st["iterations"] == ref.stats["iterations"]
        assert abs(st["final_error"] - ref.stats["final_error"]) <= 1e-8 * ref.stats["final_error"]
        assert_poses(pg.poses(), ref.poses, 1e-6, 1e-7)
        g = ext


def test_incremental_loop_closure_inside_fill_keeps_plan(pg_cls):
    """A loop closure parallel to an existing factor changes no fill: the plan's
    fronts are kept (plan_update 1), only its H assembly is rebuilt; the values
    already resident are kept bit for bit."""
    g = datasets.make("C1-nn")
    pg = pg_cls.from_dataset(g)
    pg.optimize()
    pg.save_values()
    before = pg.poses()
    i, j = g.edge_index()
    cov = np.diag(datasets.SIGMA ** 2)
    pg.add_edge(int(i[-1]) + 1, int(j[-1]) + 1, g.edge_z[-1], cov)
    assert np.array_equal(pg.poses(), before)
    st = pg.optimize(max_outer=1)
    assert st["plan_update"] == 1 and st["ms_plan"] > 0
