"""The PCG solver and the row kernels at every sub-group width, against longdouble twins.

tests/row_shapes.py builds graphs whose mean row length fixes the sub-group
width G of k_linearize / k_pcg_spmv / k_spmv / k_model_decrease (and G1 of
k_linearize_side1), with rows of exactly 0, 1, G - 1, G, G + 1, 2 G, 2 G + 1
and 3 G + 5 slots, a 600-slot hub, and two graphs past the grid cap.  The
unmarked tests prove on the host that every case reaches its (G, G1) and row
lengths, that the twin is sound and that the comparison has resolving power;
the gpu tests run the kernels.

PCG iterates: debug_solve(pcg_max_iterations=k, pcg_relative_tol=0) returns
the k-th iterate, which is far from the fixed point: a wrong block inverse, a
wrong beta or a wrong partial-sum slice still converges (every SPD
preconditioner does), but its k-th iterate is another vector.  The reference is
the recurrence in np.longdouble (row_shapes.pcg_iterates); the error measure
is max|x - x_ref| / max|x_ref|; the yardstick y is the largest such error among
float64 CPU runs of the same recurrence (block inverses by cofactors, by
LAPACK, a permuted summation order, and the longdouble recurrence on the C
oracle's float64 H and g); the GPU must satisfy err <= 8 max(y, n 2.2e-16).
test_comparison_has_resolving_power asserts that x_k is more than 1e3 bounds
from the converged solution, from x_{k-1}, from plain CG's x_k and (k >= 3:
the first two iterates do not depend on it) from x_k with beta formed over
the initial r.z.

One exception, found on the CPU and asserted there: block-Jacobi PCG on a pure
star (hub4) has a preconditioned matrix I + (rank 6) with at most 7 distinct
eigenvalues, so it terminates at its 7th step: the longdouble x_8 is the
converged solution to 6e-11 (lambda 1e-5) and 2e-14 (lambda 100), and at
lambda 1e-5 the 5th step stalls (x_5 is 2.0e-6 from x_4, under the 8.4e-6 of
1e3 bounds there; 0.49 from the solution and 0.09 from the wrong-beta
iterate).  Those three (lambda, k) of hub4, listed in TERMINATED, are run and
held to the same bound, but cannot tell x_k from the fixed point (k = 8) or
from x_{k-1} (k = 5); the other seven of hub4 can.

Largest err / max(y, n eps) of the PCG iterates per case on an MI355X, all
under the 8 (profiles/row_shapes_gpu.log; lambda and k of the largest):
  w4 (G 4) 0.56 (1e-5, k 3);  w8 (G 8) 1.73 (1e-5, k 1);  w16 (G 16) 0.06 (100, k 2);
  w32 (G 32) 0.91 (1e-5, k 8);  hub4 (G 4) 1.21 (1e-5, k 3);  hub32 (G 32) 0.76 (1e-5, k 1);
  stride32 and chain263k: under 0.001 (err 1e-14; n eps is 5.5e-12 and 1.7e-10 there)
SpMV errors are at most 2.2e-15 of max|ref| (bound 1e-10), the linearisation
sweeps within 8.6e-15 (1e-10), the model decrease within 3.4e-16 of its scale
(1e-10), the retract within 0.11 of its limit.
"""
import numpy as np
import pytest

import robust_twin as rt
import row_shapes as rs
from oracle import pgo_numpy as pn

LAMBDAS = rs.LAMBDAS
KS = rs.KS
ITER_CASES = ("w4", "w8", "w16", "w32", "hub4", "hub32")
ALL = [c.name for c in rs.CASES]
# hub4: (lambda, k) at which the longdouble recurrence has terminated (module docstring)
TERMINATED = {("hub4", 1e-5): (5, 8), ("hub4", 100.0): (8,)}
SPMV_LAMBDA = 0.37


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


@pytest.fixture(scope="module")
def longdouble():
    eps = np.finfo(np.longdouble).eps
    if not eps < 2e-19:
        pytest.skip(f"np.longdouble is no extended precision here (eps {eps:.3g}): no reference")


def angdiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def iterate_ks(name):
    """The iterates checked on a case: fewer on the large ones, whose longdouble twin takes seconds."""
    return {"stride32": (3,), "chain263k": (1, 2)}.get(name, KS)


# ------------------------------------------------------------------ CPU: the graphs
@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_lanes(pg_cls, name):
    """The handle reports the (G, G1) the case exists for: which instantiation
    of every row kernel the case runs."""
    case = rs.CASE_BY_NAME[name]
    g = rs.build(name)
    with pg_cls.from_dataset(g) as pg:
        assert pg.debug_row_lanes() == (case.G, case.G1)
    mean = g.num_edges / g.num_poses
    assert (rs.lanes_for(2 * mean), rs.lanes_for(mean)) == (case.G, case.G1)   # the rule as row_shapes restates it


def test_every_width_has_a_case():
    assert {c.G for c in rs.CASES} == {4, 8, 16, 32} and {c.G1 for c in rs.CASES} == {4, 8, 16}
    assert rs.CASE_BY_NAME["hub4"].G == 4 and rs.CASE_BY_NAME["hub32"].G == 32


@pytest.mark.parametrize("name", ["w4", "w8", "w16", "w32", "hub32"])
def test_designed_row_lengths(name):
    """Rows of exactly 0, 1, G - 1, G, G + 1, 2 G, 2 G + 1 and 3 G + 5 slots,
    counted from edge_index(); every one but the prior-only row mixes side-0
    and side-1 slots; a duplicated and a reversed pair exist."""
    g = rs.build(name)
    G = rs.CASE_BY_NAME[name].G
    L = rs.row_lengths(g)
    ei, ej = g.edge_index()
    for want in rs.designed_lengths(G):
        v = g.meta["rows"][f"len{want}"]
        assert L[v] == want, (name, want, L[v])
        if want > 1:
            assert (ei == v).any() and (ej == v).any()
    pairs = list(zip(ei.tolist(), ej.tolist()))
    assert len(set(pairs)) == len(pairs) - 1                       # one duplicated (i, j)
    assert any((j, i) in set(pairs) for i, j in pairs)             # one reversed (j, i)
    assert len(g.prior_keys) == 2 and L[g.prior_index()[1]] == 0   # the prior-only vertex


@pytest.mark.parametrize("name", ["hub4", "hub32"])
def test_hub_rows(name):
    """The hub is k1 of 300 factors (more side-0 factors than a block of
    k_linearize_own has threads: the chunk path) and k2 of 300 others.  hub32's
    first factor has an odd index in (ei, ej) order, hub4's an even one: both
    heads of the chunk's 16-byte stores."""
    g = rs.build(name)
    hub = g.meta["rows"]["hub"]
    ei, ej = g.edge_index()
    assert (ei == hub).sum() == 300 and (ej == hub).sum() == 300 and (ei == hub).sum() > rs.K_THREADS
    assert (ei < hub).sum() % 2 == (1 if name == "hub32" else 0)


def test_strided_cases_pass_the_grid_cap():
    g = rs.build("stride32")
    assert g.num_poses * rs.CASE_BY_NAME["stride32"].G > rs.GRID_CAP     # grid_rows capped: the row loops stride
    assert g.num_poses <= rs.GRID_CAP
    c = rs.build("chain263k")
    assert c.num_poses > rs.GRID_CAP and c.num_edges + len(c.prior_keys) > rs.GRID_CAP
    for gg in (g, c):
        r = gg.meta["rows"]
        assert r["last_pass0"] + 1 == r["first_pass1"] and r["last"] == gg.num_poses - 1


@pytest.mark.parametrize("name", ALL)
def test_graph_properties(name):
    """Full covariances, no zero residual, angular residuals away from the
    branch cut, start angles within 1e-12 of +-pi."""
    g = rs.build(name)
    cov = g.edge_cov.reshape(-1, 3, 3)
    assert (np.abs(cov[:, 0, 1]) > 1e-9).all() and (np.abs(cov[:, 1, 2]) > 1e-9).all()
    rp = rs.problem(name)
    ee, ep, *_ = pn.residuals(rp.prob, pn.from_xyt(g.initial))
    assert np.abs(ee).min() > 0 and np.abs(ep[0]).min() > 0
    assert np.abs(ee[:, 2]).max() < 3 and np.abs(ep[:, 2]).max() < 3
    near = g.meta["near_pi"]
    assert len(near) >= 4
    d = np.pi - np.abs(g.initial[near, 2])
    assert (d > 0).all() and (d < 1e-12).all() and {1.0, -1.0} <= set(np.sign(g.initial[near, 2]))


def test_cached_paths_are_the_twins():
    """The large cases' shortcuts (information without the per-factor loop,
    blocks from the cached linearisation) are robust_twin's results bit for bit."""
    g = rs.build("w8")
    assert np.array_equal(rs._information(g.edge_cov), pn.information(g.edge_cov))
    for a, b in zip(rs._blocks("w8", False), rt.blocks(rt.problem(g), pn.from_xyt(g.initial))):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ CPU: the twin
@pytest.mark.parametrize("lam", LAMBDAS)
def test_twin_converges_to_the_cholesky_solve(longdouble, lam):
    """The longdouble recurrence run for 3 n iterations on w4 meets the
    longdouble Cholesky solve within the yardstick of that iterate (the float64
    runs of the same 3 n iterations against the longdouble one): the
    recurrence's fixed point is the system's solution."""
    n = 3 * rs.build("w4").num_poses
    ref, y, members, _ = rs.iterate_reference("w4", lam, 3 * n)
    sol = rs.converged_solution("w4", lam)
    err = rs.rel_err(ref[3 * n], sol)
    print(f"row_shapes twin w4 lambda {lam:g}: {3 * n} iterations, err {err:.3e}, y {y[3 * n]:.3e}")
    assert err <= y[3 * n]


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", ITER_CASES)
def test_yardstick_members_are_sound(longdouble, name, lam):
    """Every float64 run of the recurrence stays within the textbook
    n eps cond(H + lambda I) of the longdouble one, at every k."""
    _, y, members, n = rs.iterate_reference(name, lam)
    H, _ = rs.dense_system(rs.build(name))
    lim = n * 2.2e-16 * np.linalg.cond(H + lam * np.eye(n))
    for k in KS:
        for tag, e in members[k].items():
            assert 0 < e <= lim, (name, lam, k, tag, e, lim)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", ITER_CASES + ("stride32", "chain263k"))
def test_comparison_has_resolving_power(longdouble, name, lam):
    ks = iterate_ks(name)
    _, y, _, n = rs.iterate_reference(name, lam, max(ks))
    margins = rs.power_margins(name, lam, ks)
    for k in ks:
        need = 1e3 * rs.bound(y[k], n)
        m = margins[k]
        print(f"row_shapes power {name} lambda {lam:g} k {k}: 1e3 bound {need:.2e} " +
              " ".join(f"{t} {v:.2e}" for t, v in m.items()))
        if k in TERMINATED.get((name, lam), ()):
            # the star's PCG has terminated or stalled (module docstring); the rest still holds
            assert min(m["converged"], m["previous"]) <= need < m["plain_cg"], (name, lam, k, m)
            assert m["beta_initial"] > need
            continue
        for tag in ("converged", "previous", "plain_cg"):
            assert m[tag] > need, (name, lam, k, tag, m[tag], need)
        if k >= 3:
            assert m["beta_initial"] > need, (name, lam, k, m["beta_initial"], need)
        else:
            assert m["beta_initial"] == 0.0    # beta_0 = r.z_1 / r.z_0 either way: x_1 and x_2 cannot tell


# ------------------------------------------------------------------ GPU
def check(tag, got, ref, y, n):
    err = rs.rel_err(got, ref)
    yy = max(y, n * 2.2e-16)
    print(f"row_shapes {tag}: n {n} err {err:.3e} y {y:.3e} err/y {err / yy:.3f}")
    assert err <= rs.bound(y, n), (tag, err, y, err / yy)


def _iterate(pg_cls, name, lam, k):
    ref, y, _, n = rs.iterate_reference(name, lam, max(iterate_ks(name)))
    with pg_cls.from_dataset(rs.build(name)) as pg:     # a fresh handle per run
        d, it = pg.debug_solve(lam, linear_solver=0, pcg_max_iterations=k, pcg_relative_tol=0.0)
    assert it == k
    check(f"pcg_iterate {name} G {rs.CASE_BY_NAME[name].G} lambda {lam:g} k {k}", d.ravel(), ref[k], y[k], n)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", ["w4", "w8", "w16", "w32"])
def test_pcg_iterates(pg_cls, longdouble, name, lam, k):
    _iterate(pg_cls, name, lam, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("lam", LAMBDAS)
def test_pcg_iterates_hub4(pg_cls, longdouble, lam, k):
    _iterate(pg_cls, "hub4", lam, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("lam", LAMBDAS)
def test_pcg_iterates_hub32(pg_cls, longdouble, lam, k):
    _iterate(pg_cls, "hub32", lam, k)


@pytest.mark.gpu
@pytest.mark.parametrize("lam", LAMBDAS)
def test_pcg_iterates_stride32(pg_cls, longdouble, lam):
    """k = 3 with grid_rows at its cap: every sub-group of k_pcg_spmv<32> takes a second row."""
    _iterate(pg_cls, "stride32", lam, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("lam", LAMBDAS)
def test_pcg_iterates_chain263k(pg_cls, longdouble, lam, k):
    """k = 1, 2 with the vector kernels' grid at its cap (nb = kMaxBlocks
    partials per dot product, every thread of k_pcg_init / update / dir a
    second pose).  The twin here is blockwise; its host side takes a few
    seconds, so no later iterate is checked."""
    _iterate(pg_cls, "chain263k", lam, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w8", "w32"])
def test_check_interval_is_invisible(pg_cls, name):
    """The launches enqueued after convergence and before the next read-back
    are no-ops: the step and the iteration count do not depend on the interval."""
    out = []
    for chk in (1, 7, 32):
        with pg_cls.from_dataset(rs.build(name)) as pg:
            out.append(pg.debug_solve(1e-5, linear_solver=0, pcg_relative_tol=1e-10, pcg_max_iterations=200000,
                                      pcg_check_interval=chk))
    print(f"row_shapes check_interval {name}: iterations {[it for _, it in out]}")
    assert out[0][1] > 0
    for d, it in out[1:]:
        assert it == out[0][1]
        assert d.tobytes() == out[0][0].tobytes()


@pytest.mark.gpu
def test_pcg_flags(pg_cls):
    """r.z = 0 at the start (zero gradient) is "converged" with no iteration
    and a zero step, not 0 / 0; a block determinant <= 0 is a breakdown.  The
    lone pose sits on its prior at theta = 0: at another angle the contracted
    -s c + c s of the residual's rotation leaves a gradient of 1e-17, not 0."""
    from graphslam_amd.pose_graph import IndeterminantLinearSystemException
    with pg_cls() as pg:
        pg.add_vertex(1, 0.7, -0.4, 0.0)
        pg.add_prior(1, [0.7, -0.4, 0.0], np.diag([0.01, 0.01, 0.01]))
        d, it = pg.debug_solve(1e-5, linear_solver=0)
    assert it == 0 and d.shape == (1, 3) and np.array_equal(d, np.zeros((1, 3))) and not np.signbit(d).any()
    with pg_cls.from_dataset(rs.build("w4")) as pg:
        with pytest.raises(IndeterminantLinearSystemException):
            pg.debug_solve(-1e12, linear_solver=0)


def _spmv(pg_cls, name):
    g = rs.build(name)
    x = np.random.default_rng(1).normal(size=(g.num_poses, 3))
    ref = rs.spmv_reference(name, x, SPMV_LAMBDA)
    with pg_cls.from_dataset(g) as pg:
        y = pg.debug_spmv(x, lam=SPMV_LAMBDA)
    scale = float(np.abs(ref).max())
    diff = np.abs(np.asarray(y, rs.LD) - ref).max(axis=1)
    print(f"row_shapes spmv {name} G {rs.CASE_BY_NAME[name].G}: max err {float(diff.max()) / scale:.3e} of max|ref|")
    L = rs.row_lengths(g)
    for tag, v in g.meta["rows"].items():
        print(f"row_shapes spmv {name} row {tag} (vertex {v}, {L[v]} slots): err {float(diff[v]) / scale:.3e}")
    assert diff.max() <= 1e-10 * scale
    rows = np.array(list(g.meta["rows"].values()))
    assert diff[rows].max() <= 1e-10 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w4", "w8", "w16", "w32"])
def test_spmv_rows(pg_cls, longdouble, name):
    _spmv(pg_cls, name)


@pytest.mark.gpu
def test_spmv_rows_hub4(pg_cls, longdouble):
    _spmv(pg_cls, "hub4")


@pytest.mark.gpu
def test_spmv_rows_hub32(pg_cls, longdouble):
    _spmv(pg_cls, "hub32")


@pytest.mark.gpu
def test_spmv_rows_stride32(pg_cls, longdouble):
    _spmv(pg_cls, "stride32")


@pytest.mark.gpu
def test_spmv_rows_chain263k(pg_cls, longdouble):
    _spmv(pg_cls, "chain263k")


def _linearize(pg_cls, oracle_lib, name):
    """Both sweeps against the C oracle at the tolerances of
    test_linearize_parity and test_linearize_cholesky_mode_parity."""
    g = rs.build(name)
    o = oracle_lib.Oracle(g)
    hd0, ho0, g0, err0 = o.linearize()
    scale_h, scale_g = np.abs(hd0).max(), max(np.abs(g0).max(), 1.0)
    rows = np.array(list(g.meta["rows"].values()))
    got = {}
    with pg_cls.from_dataset(g) as pg:
        for chol in (False, True):
            hd, ho, grad, err = pg.debug_linearize(g.num_edges, cholesky=chol)
            print(f"row_shapes linearize {name} {'cholesky' if chol else 'two-slot'}: dH {np.abs(hd - hd0).max() / scale_h:.3e}"
                  f" dHoff {np.abs(ho - ho0).max() / scale_h:.3e} dg {np.abs(grad - g0).max() / scale_g:.3e}"
                  f" derr {abs(err - err0) / err0:.3e} designed rows dH {np.abs(hd[rows] - hd0[rows]).max() / scale_h:.3e}"
                  f" dg {np.abs(grad[rows] - g0[rows]).max() / scale_g:.3e}")
            assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
            assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
            assert np.abs(grad - g0).max() <= 1e-10 * scale_g
            assert abs(err - err0) <= 1e-10 * max(err0, 1e-30)
            got[chol] = (hd, ho, grad)
        assert abs(pg.error() - o.error()) <= 1e-10 * max(err0, 1e-30)
    assert np.abs(got[True][0] - got[False][0]).max() <= 1e-12 * scale_h
    assert np.abs(got[True][1] - got[False][1]).max() <= 1e-14 * scale_h   # same per-factor arithmetic, no sums
    assert np.abs(got[True][2] - got[False][2]).max() <= 1e-12 * scale_g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w4", "w8", "w16", "w32"])
def test_linearize_rows(pg_cls, oracle_lib, name):
    _linearize(pg_cls, oracle_lib, name)


@pytest.mark.gpu
def test_linearize_rows_hub4(pg_cls, oracle_lib):
    """One row of the Gaussian k_linearize_own with 300 side-0 factors: two
    chunks, the first from an even factor index."""
    _linearize(pg_cls, oracle_lib, "hub4")


@pytest.mark.gpu
def test_linearize_rows_hub32(pg_cls, oracle_lib):
    """The same under G = 32 / G1 = 16, the chunks from an odd factor index."""
    _linearize(pg_cls, oracle_lib, "hub32")


@pytest.mark.gpu
def test_linearize_rows_w32_robust(pg_cls):
    """w32 with losses drawn from all four kinds against robust_twin:
    k_linearize_robust<32> and k_linearize_side1_robust<16>."""
    g = rs.with_random_losses(rs.build("w32"))
    rp = rt.problem(g)
    x = pn.from_xyt(g.initial)
    hd0, ho0, g0 = rt.blocks(rp, x)
    err0 = rt.error(rp, x)
    assert len(set(rp.loss.tolist())) == 4
    scale_h, scale_g = np.abs(hd0).max(), max(np.abs(g0).max(), 1.0)
    got = {}
    with pg_cls.from_dataset(g) as pg:
        assert pg.debug_row_lanes() == (32, 16)
        for chol in (False, True):
            hd, ho, grad, err = pg.debug_linearize(g.num_edges, cholesky=chol)
            print(f"row_shapes linearize w32 robust {'cholesky' if chol else 'two-slot'}: dH {np.abs(hd - hd0).max() / scale_h:.3e}"
                  f" dHoff {np.abs(ho - ho0).max() / scale_h:.3e} dg {np.abs(grad - g0).max() / scale_g:.3e}"
                  f" derr {abs(err - err0) / err0:.3e}")
            assert np.abs(hd - hd0).max() <= 1e-10 * scale_h
            assert np.abs(ho - ho0).max() <= 1e-10 * scale_h
            assert np.abs(grad - g0).max() <= 1e-10 * scale_g
            assert abs(err - err0) <= 1e-10 * err0
            got[chol] = (hd, ho, grad)
        assert abs(pg.error() - err0) <= 1e-10 * err0
    assert np.abs(got[True][0] - got[False][0]).max() <= 1e-12 * scale_h
    assert np.abs(got[True][1] - got[False][1]).max() <= 1e-14 * scale_h
    assert np.abs(got[True][2] - got[False][2]).max() <= 1e-12 * scale_g


_LM_RUNS = {}


def lm_run(pg_cls, name, solver):
    """One LM linearisation on a case: (trace, poses after it, the first try's
    lambda, that try's step from a fresh handle's debug_solve), computed once."""
    if (name, solver) not in _LM_RUNS:
        g = rs.build(name)
        with pg_cls.from_dataset(g) as pg:
            pg.optimize(max_outer=1, lambda_lanes=1, linear_solver=solver)
            trace, poses = pg.trace(), pg.poses()
        lam = float(trace[0, 1])
        with pg_cls.from_dataset(g) as pg:
            delta, _ = pg.debug_solve(lam, linear_solver=solver)
        _LM_RUNS[name, solver] = (trace, poses, lam, delta)
    return _LM_RUNS[name, solver]


LM_CASES = ("w8", "w32", "hub4")


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", LM_CASES)
def test_model_decrease_both_layouts(pg_cls, longdouble, name, solver):
    """k_model_decrease on the slot-planar blocks (PCG) and on the owner blocks
    in factor order (Cholesky mode), against the twin's linear_error(0) -
    linear_error(delta) in longdouble at the step the GPU took."""
    trace, _, lam, delta = lm_run(pg_cls, name, solver)
    assert trace[0, 6] == 1 and trace[0, 2] == 1, trace[0]
    g = rs.build(name)
    ref, scale = rs.model_decrease_reference(rs.problem(name), pn.from_xyt(g.initial), delta)
    err = abs(float(rs.LD(trace[0, 3]) - ref))
    print(f"row_shapes model_decrease {name} solver {solver} lambda {lam:g}: decrease {trace[0, 3]:.6e} "
          f"err {err:.3e} scale {scale:.3e} err/scale {err / scale:.3e}")
    assert err <= 1e-10 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", LM_CASES)
def test_retract(pg_cls, longdouble, name, solver):
    """k_retract: the values after the accepted try against a longdouble
    retract of the initial values by that try's step; the yardstick is the
    numpy twin's float64 retract."""
    trace, poses, lam, delta = lm_run(pg_cls, name, solver)
    assert trace[0, 6] == 1
    g = rs.build(name)
    ref = rs.retract_reference(g.initial, delta)
    twin = pn.to_xyt(pn.retract(pn.from_xyt(g.initial), delta))
    y = rs.retract_errors(twin, ref).max(axis=0).astype(np.float64)
    scale = np.abs(g.initial) + np.abs(delta)
    scale[:, 2] = np.pi
    lim = 8.0 * np.maximum(y[None, :], 2.2e-16 * scale)
    err = rs.retract_errors(poses, ref).astype(np.float64)
    near = g.meta["near_pi"]
    print(f"row_shapes retract {name} solver {solver}: worst err/limit {float((err / lim).max()):.3f} "
          f"(poses near +-pi: {float((err[near] / lim[near]).max()):.3f}) y {y}")
    assert (np.abs(delta) > 0).all() and len(near) >= 4
    assert (err <= lim).all(), float((err / lim).max())
    assert angdiff(poses[:, 2], np.asarray(ref[:, 2], np.float64)).max() <= 1e-14


@pytest.mark.gpu
def test_error_strided(pg_cls):
    """k_error over more factors than its capped grid has threads."""
    g = rs.build("chain263k")
    ref = rs.error_reference("chain263k")
    with pg_cls.from_dataset(g) as pg:
        err = pg.error()
    print(f"row_shapes error chain263k: {err:.12e} ref {ref:.12e} rel {abs(err - ref) / ref:.3e}")
    assert abs(err - ref) <= 1e-10 * ref
