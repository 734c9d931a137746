"""Designed row-shape graphs: one pose graph per sub-group width of the row kernels.

The row kernels of pgo_kernels.hip (k_linearize, k_pcg_spmv, k_spmv,
k_model_decrease; k_linearize_side1 with G1) give every vertex row a sub-group
of G lanes, G = lanes_for(2 E / n) in {4, 8, 16, 32} (pgo_structure.cpp).  A
band graph fixes the mean row length, hence G; pendant vertices joined to a
chosen number of band poses give rows of exactly 1, G - 1, G, G + 1, 2 G,
2 G + 1 and 3 G + 5 slots, a vertex with nothing but a prior a row of 0, and a
hub a row of 600.  CASES names the (G, G1) every case exists to reach;
tests/test_row_shapes.py asserts them through PoseGraph.debug_row_lanes().

Every graph: a prior on pose 0 (and the one on the prior-only vertex), a random
non-diagonal covariance per factor, noisy measurements and a noisy start (no
residual is zero), a few poses whose start angle is within 1e-12 of +-pi.

The twin of the PCG solver is ``pcg_iterates``: the recurrences of k_pcg_init /
k_pcg_spmv / k_pcg_update / k_pcg_dir restated literally.  Its k-th iterate in
np.longdouble is the reference of debug_solve(pcg_max_iterations=k,
pcg_relative_tol=0); the yardstick of the tolerance is the worst float64 CPU
run of the same recurrence (``iterate_reference``).  This module does no GPU
work.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import robust_twin as rt
from front_shapes import LD, bound, dense_system, dense_system_c_oracle, ld_cholesky, ld_solve, rel_err  # noqa: F401
from graphslam_amd import datasets
from oracle import pgo_numpy as pn

# ------------------------------------------------------------------ the rule
K_THREADS = 256        # pgo_device.h kThreads
K_MAX_BLOCKS = 1024    # pgo_device.h kMaxBlocks
GRID_CAP = K_THREADS * K_MAX_BLOCKS   # 262144: rows x G (row kernels) or rows (vector kernels) past it stride
LAMBDAS = (1e-5, 100.0)
KS = (1, 2, 3, 5, 8)
LD_PI = LD(np.pi) + LD(1.2246467991473532e-16)


def lanes_for(mean):
    """pgo_structure.cpp lanes_for, restated."""
    G = 4
    while G < 32 and G < mean:
        G *= 2
    return G


def designed_lengths(G):
    return (0, 1, G - 1, G, G + 1, 2 * G, 2 * G + 1, 3 * G + 5)


# --------------------------------------------------------------- the builders
def band_pairs(n, h):
    """Pose a joined to a + 1 ... a + h; the direction alternates with a + k
    odd or even, so every row mixes side-0 and side-1 slots."""
    a, k = np.meshgrid(np.arange(n), np.arange(1, h + 1), indexing="ij")
    a, b = a.ravel(), (a + k).ravel()
    keep = b < n
    a, b = a[keep], b[keep]
    even = (b % 2) == 0
    return np.where(even, a, b), np.where(even, b, a)


def _information(cov):
    """pn.information for full covariances, vectorised (the lower triangle of
    the inverse mirrored); test_row_shapes checks it against pn.information."""
    inv = np.linalg.inv(cov.reshape(-1, 3, 3))
    low = np.tril(inv)
    return low + np.transpose(np.tril(inv, -1), (0, 2, 1))


def _graph(name, n, i, j, seed, prior=(0,), near_pi=(), rows=None, walk=False):
    """datasets.PoseGraph over the pairs (i, j) (i is k1); one prior per pose of
    `prior`; the poses of `near_pi` start within 1e-12 of +-pi."""
    rng = np.random.default_rng(seed)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    E = len(i)
    gt = np.empty((n, 3))
    if walk:
        gt[:, :2] = np.cumsum(rng.uniform(-1.0, 1.0, size=(n, 2)), axis=0)
    else:
        gt[:, :2] = rng.uniform(-10.0, 10.0, size=(n, 2))
    gt[:, 2] = rng.uniform(-2.9, 2.9, size=n)
    init = gt + rng.normal(size=(n, 3)) * [0.1, 0.1, 0.03]
    near_pi = np.asarray(near_pi, np.int64)
    sign = np.where(np.arange(len(near_pi)) % 2 == 0, 1.0, -1.0)
    gt[near_pi, 2] = sign * np.pi
    init[near_pi, 2] = sign * (np.pi - 5e-13)
    z = datasets.compose_xyt(datasets.between_xyt(gt[i], gt[j]), rng.normal(size=(E, 3)) * [0.05, 0.05, 0.02])
    # Cholesky factors with a diagonal in [0.03, 0.08]: no covariance among 263000 is nearly singular
    Lc = np.tril(rng.normal(size=(E, 3, 3)) * 0.02, -1) + rng.uniform(0.03, 0.08, size=(E, 3, 1)) * np.eye(3)
    cov = (Lc @ np.transpose(Lc, (0, 2, 1))).reshape(-1, 9)
    prior = np.asarray(prior, np.int64)
    g = datasets.PoseGraph(
        name=name, keys=np.arange(1, n + 1, dtype=np.uint64), initial=init, ground_truth=gt,
        edge_k1=(i + 1).astype(np.uint64), edge_k2=(j + 1).astype(np.uint64), edge_z=z, edge_cov=cov,
        prior_keys=(prior + 1).astype(np.uint64), prior_pose=gt[prior].copy(),
        prior_cov=np.tile(np.diag([0.01, 0.01, 0.01]).reshape(1, 9), (len(prior), 1)))
    g.meta["rows"] = dict(rows or {})
    g.meta["near_pi"] = near_pi
    return g


def width_graph(name, nb, h, G, seed, hub=False):
    """band(nb, h) + one pendant vertex per designed row length of G + one
    prior-only vertex + a duplicated pair and a reversed pair (+ a hub that is
    k1 of 300 and k2 of 300 other band poses)."""
    rng = np.random.default_rng(seed + 1000)
    i, j = band_pairs(nb, h)
    ei, ej = [i], [j]
    rows = {}
    v = nb
    for L in designed_lengths(G)[1:]:
        t = np.sort(rng.choice(nb, L, replace=False))
        out = (np.arange(L) % 2) == 0          # alternate: the pendant is k1 of every other factor
        ei.append(np.where(out, v, t))
        ej.append(np.where(out, t, v))
        rows[f"len{L}"] = v
        v += 1
    rows["len0"] = v                           # the prior-only vertex
    lone = v
    v += 1
    ei.append(np.array([i[0], j[1]]))          # (i, j) once more; (j, i) of another factor
    ej.append(np.array([j[0], i[1]]))
    if hub:
        ei.append(np.concatenate([np.full(300, v), np.sort(rng.permutation(nb)[:300])]))
        ej.append(np.concatenate([np.sort(rng.permutation(nb)[:300]), np.full(300, v)]))
        rows["hub"] = v
        v += 1
    near_pi = [3, 10, rows["len1"], rows[f"len{G}"], nb - 2]
    return _graph(name, v, np.concatenate(ei), np.concatenate(ej), seed, prior=(0, lone), near_pi=near_pi, rows=rows)


def hub4_graph(seed=3):
    """The shape of robust_twin.star_graph() without losses: pose 0 (with the
    prior) is k1 of 300 factors and k2 of 300 others, 600 leaves."""
    n = 601
    i = np.concatenate([np.zeros(300, np.int64), np.arange(301, 601)])
    j = np.concatenate([np.arange(1, 301), np.zeros(300, np.int64)])
    return _graph("hub4", n, i, j, seed, near_pi=[5, 299, 300, 301, 600], rows={"hub": 0, "len1": 1, "len1b": 600})


def stride32_graph():
    n = 8400
    i, j = band_pairs(n, 9)
    last = GRID_CAP // 32 - 1                  # the last row of the first pass over the grid
    return _graph("stride32", n, i, j, 32, near_pi=[7, last, last + 1, n - 1],
                  rows={"first": 0, "last_pass0": last, "first_pass1": last + 1, "last": n - 1})


def chain263k_graph():
    n = 263000
    a = np.arange(n - 1)
    return _graph("chain263k", n, a, a + 1, 263, near_pi=[9, GRID_CAP - 1, GRID_CAP, n - 1], walk=True,
                  rows={"first": 0, "last_pass0": GRID_CAP - 1, "first_pass1": GRID_CAP, "last": n - 1})


@dataclass(frozen=True)
class Case:
    name: str
    G: int
    G1: int
    dense: bool       # small enough for the dense longdouble twin
    why: str


CASES = (
    Case("w4", 4, 4, True, "band(40, 1): k_*<4> at every row-length edge of 4"),
    Case("w8", 8, 4, True, "band(60, 3)"),
    Case("w16", 16, 8, True, "band(60, 6)"),
    Case("w32", 32, 16, True, "band(120, 12): the widest sub-group, never run in PCG mode before"),
    Case("hub4", 4, 4, True, "a 600-slot row under G = 4; 300 side-0 factors: k_linearize_own's chunk path"),
    Case("hub32", 32, 16, True, "band(320, 12) + the designed rows + a 600-slot hub under G = 32"),
    Case("stride32", 32, 16, False, "band(8400, 9): n G > 262144, the row loops stride"),
    Case("chain263k", 4, 4, False, "n > 262144: the vector kernels and k_error stride, nb = kMaxBlocks"),
)
CASE_BY_NAME = {c.name: c for c in CASES}
SMALL = tuple(c.name for c in CASES if c.dense)

_BUILD = {
    "w4": lambda: width_graph("w4", 40, 1, 4, 4),
    "w8": lambda: width_graph("w8", 60, 3, 8, 8),
    "w16": lambda: width_graph("w16", 60, 6, 16, 16),
    "w32": lambda: width_graph("w32", 120, 12, 32, 32),
    "hub4": hub4_graph,
    "hub32": lambda: width_graph("hub32", 320, 12, 32, 33, hub=True),
    "stride32": stride32_graph,
    "chain263k": chain263k_graph,
}


@functools.lru_cache(maxsize=None)
def build(name):
    return _BUILD[name]()


def row_lengths(g):
    ei, ej = g.edge_index()
    return np.bincount(ei, minlength=g.num_poses) + np.bincount(ej, minlength=g.num_poses)


def with_random_losses(g, seed=17):
    """A copy of g with losses drawn from all four kinds, k in [0.5, 3]."""
    import copy
    rng = np.random.default_rng(seed)
    h = copy.copy(g)
    h.edge_loss = rng.integers(0, 4, g.num_edges).astype(np.int32)
    h.edge_loss_k = rng.uniform(0.5, 3.0, g.num_edges)
    return h


# -------------------------------------------------------------- the twin's system
@functools.lru_cache(maxsize=None)
def problem(name):
    """robust_twin.RobustProblem of a case (Gaussian).  The large cases skip
    pn.information's per-factor loop (every covariance here is full)."""
    g = build(name)
    if CASE_BY_NAME[name].dense:
        return rt.problem(g)
    ei, ej = g.edge_index()
    prob = pn.Problem(n=g.num_poses, ei=np.asarray(ei), ej=np.asarray(ej), ez=pn.from_xyt(g.edge_z),
                      eom=_information(g.edge_cov), pi=g.prior_index(), pz=pn.from_xyt(g.prior_pose),
                      pom=pn.information(g.prior_cov))
    E = len(prob.ei)
    return rt.RobustProblem(prob, np.zeros(E, np.int64), np.ones(E))


class BlockSystem:
    """H in blocks (diagonal [n, 3, 3]; H_{ei, ej} per factor [E, 3, 3]) in a
    number format; the product is formed blockwise with np.add.at, the factors
    taken in `order`."""

    def __init__(self, hd, B, ei, ej, dtype=LD, order=None):
        o = np.arange(len(ei)) if order is None else order
        self.hd, self.B = np.asarray(hd, dtype), np.asarray(B, dtype)[o]
        self.ei, self.ej = np.asarray(ei)[o], np.asarray(ej)[o]
        self.dtype, self.n = dtype, 3 * len(hd)

    def diag(self):
        return self.hd

    def matvec(self, p, lam):
        y = np.einsum("nij,nj->ni", self.hd, p) + self.dtype(lam) * p
        np.add.at(y, self.ei, np.einsum("eij,ej->ei", self.B, p[self.ej]))
        np.add.at(y, self.ej, np.einsum("eji,ej->ei", self.B, p[self.ei]))
        return y


class DenseSystem:
    """H dense in a number format; `perm`: the columns summed in that order."""

    def __init__(self, H, dtype=LD, perm=None):
        self.H = np.asarray(H, dtype)
        self.perm, self.dtype, self.n = perm, dtype, H.shape[0]
        self.Hp = self.H[:, perm] if perm is not None else self.H

    def diag(self):
        m = self.n // 3
        return self.H.reshape(m, 3, m, 3)[np.arange(m), :, np.arange(m), :]

    def matvec(self, p, lam):
        v = p.ravel()
        y = self.Hp @ (v[self.perm] if self.perm is not None else v)
        return (y + self.dtype(lam) * v).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def edge_index(name):
    return build(name).edge_index()


@functools.lru_cache(maxsize=None)
def linearized(name):
    """(weighted problem, pn.Linear) of a case at its initial values."""
    return rt.linearize(problem(name), pn.from_xyt(build(name).initial))


@functools.lru_cache(maxsize=None)
def _blocks(name, oracle):
    g = build(name)
    if oracle:
        from oracle.oracle import Oracle
        hd, B, grad, _ = Oracle(g).linearize()
    else:   # robust_twin.blocks on the cached linearisation
        wp, lin = linearized(name)
        B = np.einsum("eki,ekl->eil", lin.J1, wp.eom)
        hd = np.zeros((wp.n, 3, 3))
        np.add.at(hd, wp.ei, np.einsum("eil,elj->eij", B, lin.J1))
        np.add.at(hd, wp.ej, wp.eom)
        np.add.at(hd, wp.pi, wp.pom)
        grad = lin.g.reshape(-1, 3).copy()
    for a in (hd, B, grad):
        a.setflags(write=False)
    return hd, B, grad


def block_system(name, dtype=LD, order=None, oracle=False):
    """(BlockSystem, gradient [n, 3]) of a case at its initial values: the numpy
    twin's blocks, or the C oracle's (a second float64 rounding of the same H)."""
    ei, ej = edge_index(name)
    hd, B, grad = _blocks(name, bool(oracle))
    return BlockSystem(hd, B, ei, ej, dtype, order), grad


# ------------------------------------------------------------------ the PCG twin
def block_inverses(D, lam, how="cofactor"):
    """Inverses of the blocks D_i + lam I: by cofactors in D's own number
    format, as k_pcg_init forms them, or by LAPACK (float64)."""
    A = D + D.dtype.type(lam) * np.eye(3, dtype=D.dtype)
    if how == "lapack":
        return np.linalg.inv(A)
    a00, a01, a02, a11, a12, a22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    inv = 1 / (a00 * c00 + a01 * c01 + a02 * c02)
    M = np.empty_like(A)
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2] = c00 * inv, c11 * inv, c22 * inv
    M[:, 0, 1] = M[:, 1, 0] = c01 * inv
    M[:, 0, 2] = M[:, 2, 0] = c02 * inv
    M[:, 1, 2] = M[:, 2, 1] = c12 * inv
    return M


def pcg_iterates(H, g, lam, kmax, dtype=LD, inverse="cofactor", perm=None, precondition=True,
                 beta_from_initial=False):
    """x_1 ... x_kmax of block-Jacobi PCG on (H + lam I) x = -g as the kernels
    run it: M_i = (H_ii + lam I)^-1; x = 0, r = -g, z = M r, p = z; then
    q = (H + lam I) p, alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M r,
    beta = r.z_new / r.z_old, p = z + beta p.  H: a dense matrix, a
    DenseSystem or a BlockSystem.  `perm` permutes the summation order of the
    dense product and of the dot products.  precondition=False (plain CG) and
    beta_from_initial=True (beta over the first r.z) are the wrong recurrences
    the comparison must tell from the right one."""
    op = H if hasattr(H, "matvec") else DenseSystem(H, dtype, perm)
    grad = np.asarray(g, dtype).reshape(-1, 3)
    M = block_inverses(np.asarray(op.diag(), dtype), lam, inverse) if precondition else None

    def apply(r):
        return np.einsum("nij,nj->ni", M, r) if precondition else r.copy()

    def dot(a, b):
        t = (a * b).ravel()
        return (t[perm] if perm is not None else t).sum()

    x = np.zeros_like(grad)
    r = -grad
    z = apply(r)
    p = z.copy()
    rz = rz0 = dot(r, z)
    out = []
    for _ in range(kmax):
        q = op.matvec(p, lam)
        alpha = rz / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        z = apply(r)
        rzn = dot(r, z)
        beta = rzn / (rz0 if beta_from_initial else rz)
        p = z + beta * p
        rz = rzn
        out.append(x.ravel().copy())
    return out


def _systems(name):
    """The float64 (H, g) of a case from the numpy twin and from the C oracle:
    dense matrices for the small cases, BlockSystem makers for the large."""
    if CASE_BY_NAME[name].dense:
        H, grad = dense_system(build(name))
        H2, grad2 = dense_system_c_oracle(build(name))
        return (lambda dt, perm=None: DenseSystem(H, dt, perm)), grad, (lambda dt: DenseSystem(H2, dt)), grad2
    E = build(name).num_edges
    grad = block_system(name)[1]
    grad2 = block_system(name, oracle=True)[1]

    def twin(dt, perm=None):
        return block_system(name, dt, None if perm is None else np.random.default_rng(5).permutation(E))[0]
    return twin, grad, (lambda dt: block_system(name, dt, oracle=True)[0]), grad2


def yardstick_runs(name, lam, kmax):
    """The float64 CPU runs of the recurrence (and the longdouble run on the C
    oracle's float64 H and g): {member: [x_1 ... x_kmax]}."""
    twin, grad, orc, grad2 = _systems(name)
    perm = np.random.default_rng(len(grad.ravel())).permutation(len(grad.ravel()))
    f8 = np.float64
    return {
        "cofactor": pcg_iterates(twin(f8), grad, lam, kmax, f8),
        "lapack": pcg_iterates(twin(f8), grad, lam, kmax, f8, inverse="lapack"),
        "permuted": pcg_iterates(twin(f8, perm), grad, lam, kmax, f8, perm=perm),
        "oracle_H": pcg_iterates(orc(LD), grad2, lam, kmax, LD),
    }


@functools.lru_cache(maxsize=None)
def iterate_reference(name, lam, kmax=max(KS)):
    """({k: longdouble x_k}, {k: yardstick y_k}, {k: {member: error}}, n) of a case."""
    twin, grad, _, _ = _systems(name)
    ref = pcg_iterates(twin(LD), grad, lam, kmax, LD)
    runs = yardstick_runs(name, lam, kmax)
    members = {k: {m: rel_err(x[k - 1], ref[k - 1]) for m, x in runs.items()} for k in range(1, kmax + 1)}
    for x in ref:
        x.setflags(write=False)
    return ({k: ref[k - 1] for k in members}, {k: max(members[k].values()) for k in members}, members,
            len(grad.ravel()))


@functools.lru_cache(maxsize=None)
def converged_solution(name, lam):
    """(H + lam I)^-1 (-g): a longdouble Cholesky solve (small cases), a float64
    sparse LU (large cases; only distances of order 1 are measured against it)."""
    g = build(name)
    if CASE_BY_NAME[name].dense:
        H, grad = dense_system(g)
        return ld_solve(ld_cholesky(H + lam * np.eye(H.shape[0])), -grad)
    _, lin = linearized(name)
    return pn.solve(lin.H, -lin.g, lam)


def power_margins(name, lam, ks):
    """{k: distances (rel_err against x_k) of the things the comparison must
    tell from x_k: the converged solution, x_{k-1}, plain CG's k-th iterate, the
    k-th iterate with beta over the initial r.z}."""
    twin, grad, _, _ = _systems(name)
    kmax = max(ks)
    ref = iterate_reference(name, lam, kmax)[0]
    cg = pcg_iterates(twin(LD), grad, lam, kmax, LD, precondition=False)
    b0 = pcg_iterates(twin(LD), grad, lam, kmax, LD, beta_from_initial=True)
    sol = converged_solution(name, lam)
    out = {}
    for k in ks:
        prev = ref[k - 1] if k > 1 else np.zeros_like(ref[1])
        out[k] = {"converged": rel_err(sol, ref[k]), "previous": rel_err(prev, ref[k]),
                  "plain_cg": rel_err(cg[k - 1], ref[k]), "beta_initial": rel_err(b0[k - 1], ref[k])}
    return out


# ------------------------------------------------------- spmv, model decrease, retract
def spmv_reference(name, x, lam):
    """(H + lam I) x, the twin's blocks multiplied in longdouble: [n, 3]."""
    op, _ = block_system(name, LD)
    return op.matvec(np.asarray(x, LD).reshape(-1, 3), lam)


def model_decrease_reference(rp, x0, delta):
    """(linear_error(0) - linear_error(delta) of the twin in longdouble, the
    scale |g.delta| + |delta'H delta| / 2 of the two sums k_model_decrease forms)."""
    wp, lin = rt.linearize(rp, x0)
    d = np.asarray(delta, LD).reshape(-1, 3)
    om, pom = np.asarray(wp.eom, LD), np.asarray(wp.pom, LD)

    def lin_err(dd):
        re = np.asarray(lin.ee, LD) + np.einsum("eij,ej->ei", np.asarray(lin.J1, LD), dd[wp.ei]) + dd[wp.ej]
        rp_ = np.asarray(lin.ep, LD) + dd[wp.pi]
        return (np.einsum("ei,eij,ej->", re, om, re) + np.einsum("ei,eij,ej->", rp_, pom, rp_)) / 2

    dec = lin_err(np.zeros_like(d)) - lin_err(d)
    d8 = np.asarray(delta, np.float64).ravel()
    return dec, abs(float(lin.g @ d8)) + 0.5 * abs(float(d8 @ (lin.H @ d8)))


def wrap_ld(a):
    return a - 2 * LD_PI * np.round(a / (2 * LD_PI))


def retract_reference(xyt, delta):
    """Pose2 retract (x * Pose2(delta)) on (x, y, theta) in longdouble; the angle is not wrapped."""
    x, d = np.asarray(xyt, LD), np.asarray(delta, LD).reshape(-1, 3)
    c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
    return np.stack([x[:, 0] + c * d[:, 0] - s * d[:, 1], x[:, 1] + s * d[:, 0] + c * d[:, 1], x[:, 2] + d[:, 2]],
                    axis=1)


def retract_errors(got, ref):
    """|got - ref| per coordinate in longdouble, the angle through its wrapped difference."""
    e = np.asarray(got, LD) - ref
    e[:, 2] = wrap_ld(e[:, 2])
    return np.abs(e)


def error_reference(name):
    """The graph error at the initial values: the twin's residuals (float64), summed in longdouble."""
    rp = problem(name)
    ee, ep, *_ = pn.residuals(rp.prob, pn.from_xyt(build(name).initial))
    t = np.einsum("ei,eij,ej->e", ee, rp.prob.eom, ee).astype(LD).sum()
    return float((t + np.einsum("ei,eij,ej->e", ep, rp.prob.pom, ep).astype(LD).sum()) / 2)
