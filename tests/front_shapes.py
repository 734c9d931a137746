"""Designed dense-front graphs: one pose graph per Cholesky front-kernel class.

The multifrontal Cholesky picks its kernel per front from the front's pivot
width w and height m (pgo_schedule.cpp, LevelCtx::small_classes;
pgo_chol.h front_packed).  Nested dissection leaves little control over (w, m)
on the benchmark graphs; on these graphs it leaves none to chance:

* ``clique(k)``: k fully connected poses -> one front, w = m = 3k;
* ``separator_leaves(a, b, G)``: a clique of a poses (the separator) and G
  cliques of b poses, each fully connected to the separator -> G leaf fronts
  (3b, 3b + 3a) under a top front (3a, 3a);
* ``nested(a, b, G, c, H, t)``: the leaves of separator_leaves(a, b, G) are
  themselves separators: H cliques of c poses hang off the last t poses of each
  of them, so their update matrices are extend-added into a blocked parent at
  a row offset that is no multiple of 64.

Every case of CASES names the (w, m) fronts it exists to reach and their
class; tests/test_front_shapes.py asserts on the CPU that the plan has them.

The reference of a solve is a Cholesky factorisation carried out in
np.longdouble (x87 extended precision, eps 1.1e-19); the yardstick of a
tolerance is the worst of several float64 CPU solves of the same system
against that reference (see ``yardstick_solvers``), and of the longdouble
solve of the system as the C oracle's float64 linearisation rounds it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from graphslam_amd import datasets

# ------------------------------------------------------------------ the rule
# One statement of the rule in pgo_schedule.cpp / pgo_chol.h (default knobs):
# a front is packed and takes the blocked path when m > 128 or w > 32; else one
# wavefront factorises it, compiled for a panel of 8, 16 or 32 columns and for
# one (m <= 64) or two (m <= 128) rows per lane.
K_SMALL_FRONT = 128
K_WAVE_W = 32
K_NB = 64           # panel width of the blocked path
K_KB = 256          # Schur updates deferred per block of this many columns
K_LOOKAHEAD_M = 512

WAVE_CLASSES = tuple(f"wave{W}_{rows}" for rows in ("m64", "m128") for W in (8, 16, 32))


def front_class(w: int, m: int) -> str:
    if m > K_SMALL_FRONT or w > K_WAVE_W:
        return "blocked"
    W = 8 if w <= 8 else 16 if w <= 16 else 32
    return f"wave{W}_{'m64' if m <= 64 else 'm128'}"


# --------------------------------------------------------------- the builders
def _ground_truth(n, seed):
    rng = np.random.default_rng(seed)
    gt = np.empty((n, 3))
    gt[:, :2] = rng.uniform(0.0, 10.0, size=(n, 2))
    gt[:, 2] = rng.uniform(-3.0, 3.0, size=n)
    return gt


def _all_pairs(idx):
    idx = list(idx)
    return [(idx[i], idx[j]) for i in range(len(idx)) for j in range(i + 1, len(idx))]


def _cross(a, b):
    return [(i, j) for i in a for j in b]


def clique(k, seed=1):
    g = datasets.noise_free(_ground_truth(k, seed), _all_pairs(range(k)), name=f"clique{k}")
    g.meta["groups"] = []
    if k == 1:   # noise_free starts the prior's pose at its optimum: a lone pose would have no gradient at all
        g.initial[0] += (0.05, -0.03, 0.02)
    return g


def separator_leaves(a, b, G, seed=2):
    sep = range(a)
    pairs = _all_pairs(sep)
    groups = []
    for q in range(G):
        leaf = range(a + q * b, a + (q + 1) * b)
        pairs += _all_pairs(leaf) + _cross(sep, leaf)
        groups.append(leaf[0])
    g = datasets.noise_free(_ground_truth(a + G * b, seed), pairs, name=f"sep{a}_{b}x{G}")
    g.meta["groups"] = groups
    return g


def nested(a, b, G, c, H, t, seed=3):
    """separator_leaves(a, b, G) whose leaves carry H cliques of c poses each,
    fully connected to the last t poses of their leaf."""
    sep = range(a)
    pairs = _all_pairs(sep)
    groups = []
    n = a
    mids = []
    for q in range(G):
        mid = range(n, n + b)
        n += b
        pairs += _all_pairs(mid) + _cross(sep, mid)
        groups.append(mid[0])
        mids.append(mid)
    for mid in mids:
        for h in range(H):
            leaf = range(n, n + c)
            n += c
            pairs += _all_pairs(leaf) + _cross(mid[b - t:], leaf)
            groups.append(leaf[0])
    g = datasets.noise_free(_ground_truth(n, seed), pairs, name=f"nested{a}_{b}x{G}_{c}x{H}")
    g.meta["groups"] = groups
    g.meta["mids"] = [(m[0], m[-1] + 1, t) for m in mids]
    return g


_BUILDERS = {"clique": clique, "separator_leaves": separator_leaves, "nested": nested}


@dataclass(frozen=True)
class Case:
    name: str
    builder: str
    args: tuple
    fronts: tuple     # ((w, m), ...): fronts the plan must have
    why: str

    @property
    def classes(self):
        return tuple(front_class(w, m) for w, m in self.fronts)

    @property
    def blocked(self):
        return "blocked" in self.classes


def _clique_case(k, why):
    return Case(f"clique{k}", "clique", (k,), ((3 * k, 3 * k),), why)


def _sep_case(a, b, G, why, fronts=None):
    return Case(f"sep{a}_{b}x{G}", "separator_leaves", (a, b, G),
                fronts if fronts is not None else ((3 * b, 3 * b + 3 * a),), why)


CASES = (
    # wave cliques: no update matrix, w = m
    _clique_case(1, "one pose: the smallest front (W = 8, 3 of 8 panel columns)"),
    _clique_case(2, "W = 8 panel, 6 columns"),
    _clique_case(5, "W = 16 panel, 15 columns"),
    _clique_case(10, "W = 32 panel, 30 columns: the widest one-wavefront front"),
    # blocked cliques
    _clique_case(11, "smallest packed front: one panel of 33 columns"),
    _clique_case(21, "one panel, one column short of whole"),
    _clique_case(22, "second panel of 2 columns"),
    _clique_case(43, "third panel of 1 column; the first m past 128"),
    _clique_case(64, "three whole panels"),
    _clique_case(85, "last panel of 63 columns, one short of a whole 256-column block"),
    _clique_case(86, "first panel past a 256-column block end, 2 columns wide"),
    _clique_case(171, "m >= 512: look-ahead skip and prep active; last panel of 1 column"),
    _clique_case(192, "nine whole panels: prep on whole 64-column pivot blocks"),
    _clique_case(256, "three whole 256-column blocks; the largest case"),
    # wave fronts with an update matrix: m <= 64 | m <= 128  x  w <= 8 | <= 16 | <= 32
    _sep_case(8, 2, 8, "w <= 8, m <= 64"),
    _sep_case(8, 5, 4, "w <= 16, m <= 64"),
    _sep_case(8, 10, 4, "w <= 32, m <= 64"),
    _sep_case(20, 2, 8, "w <= 8, 64 < m <= 128: m = 66, two rows in the first lanes only"),
    _sep_case(30, 5, 3, "w <= 16, 64 < m <= 128"),
    _sep_case(30, 10, 3, "w <= 32, 64 < m <= 128"),
    _sep_case(16, 5, 4, "m = 63: one row per lane, the last lane idle"),
    _sep_case(17, 5, 4, "m = 66: the first m of the two-rows-per-lane class"),
    _sep_case(32, 10, 3, "m = 126: the last pose-sized m of the one-wavefront path"),
    # blocked fronts with small w under tall m, and w > 32 with m <= 128
    _sep_case(33, 10, 3, "m = 129: the first packed m under a narrow panel"),
    _sep_case(40, 10, 3, "w = 30 under m = 150"),
    _sep_case(60, 10, 3, "w = 30 under m = 210"),
    _sep_case(41, 2, 12, "w <= 8 under m > 128: a 6-column panel, 123 rows of Schur tiles"),
    _sep_case(20, 22, 3, "w > 32 with m <= 128: packed storage of a tiny front",
              fronts=((51, 126), (66, 126))),
    # multi-level
    Case("nested25_30x2_5x2", "nested", (25, 30, 2, 5, 2, 15), ((90, 165), (15, 60)),
         "child update matrices extend-added into a blocked parent at row 45"),
)
CASE_BY_NAME = {c.name: c for c in CASES}
BLOCKED_CASES = tuple(c for c in CASES if c.blocked)
# (c) lambda lanes: one case per family
LANES_CASES = ("clique10", "sep20_2x8", "clique22", "clique86", "sep41_2x12", "nested25_30x2_5x2")


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASE_BY_NAME[name]
    return _BUILDERS[c.builder](*c.args)


def with_last_prior(g):
    """A copy of g with one more prior, on the last pose (marginals: a clique
    held by a single prior is needlessly ill-conditioned for an inverse)."""
    import copy
    h = copy.deepcopy(g)
    last = g.num_poses - 1
    h.prior_keys = np.append(g.prior_keys, np.uint64(last + 1))
    h.prior_pose = np.vstack([g.prior_pose, g.ground_truth[last:last + 1]])
    h.prior_cov = np.vstack([g.prior_cov, g.prior_cov[:1]])
    return h


def marginal_keys(g):
    n = g.num_poses
    idx = sorted({0, n // 2, n - 1, *g.meta.get("groups", [])})
    return np.asarray(idx, dtype=np.int64)


# -------------------------------------------------------------- the reference
LD = np.longdouble


def dense_system(g):
    """(H, gradient) at g's initial values from the numpy twin, dense float64."""
    from oracle import pgo_numpy as tw
    lin = tw.linearize(tw.problem_from_graph(g), tw.from_xyt(g.initial))
    return np.asarray(lin.H.todense()), np.asarray(lin.g)


def dense_system_c_oracle(g):
    """The same system from the C oracle: a second float64 evaluation of the
    same formulas, rounded differently (the GPU's linearisation is a third)."""
    from oracle.oracle import Oracle
    hd, ho, grad, _ = Oracle(g).linearize()
    n = g.num_poses
    H = np.zeros((n, 3, n, 3))
    H[np.arange(n), :, np.arange(n), :] = hd
    ei, ej = g.edge_index()
    np.add.at(H, (ei, slice(None), ej, slice(None)), ho)
    np.add.at(H, (ej, slice(None), ei, slice(None)), np.transpose(ho, (0, 2, 1)))
    return H.reshape(3 * n, 3 * n), grad.ravel()


def ld_cholesky(A):
    """Lower Cholesky factor of A, every operation in np.longdouble (left-looking column loop)."""
    n = A.shape[0]
    L = np.tril(A.astype(LD))
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} not positive")
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return L


def ld_solve(L, B):
    """(L L^T)^-1 B in np.longdouble: forward then backward substitution, column loops."""
    X = np.array(B, dtype=LD).reshape(L.shape[0], -1)
    n = L.shape[0]
    for j in range(n):
        X[j] /= L[j, j]
        X[j + 1:] -= np.outer(L[j + 1:, j], X[j])
    for j in range(n - 1, -1, -1):
        X[j] /= L[j, j]
        X[:j] -= np.outer(L[j, :j], X[j])
    return X.reshape(np.shape(B))


def unit_columns(n, idx):
    E = np.zeros((n, 3 * len(idx)))
    for q, i in enumerate(idx):
        E[3 * i:3 * i + 3, 3 * q:3 * q + 3] = np.eye(3)
    return E


def diag_blocks(X, idx):
    """[len(idx), 3, 3]: rows of pose idx[q] in its own three columns of X = A^-1 E."""
    return np.stack([X[3 * i:3 * i + 3, 3 * q:3 * q + 3] for q, i in enumerate(idx)])


# -------------------------------------------------------------- the yardstick
def _chol_solver(A):
    import scipy.linalg as sl
    L = np.linalg.cholesky(A)
    return lambda B: sl.solve_triangular(L, sl.solve_triangular(L, B, lower=True), lower=True, trans="T")


def _permuted(A, p):
    s = _chol_solver(A[np.ix_(p, p)])
    ip = np.argsort(p)
    return lambda B: s(B[p])[ip]


def _blocked_inverse_solver(A, nb=K_NB):
    """float64 emulation of the GPU's scheme: right-looking blocked Cholesky
    with nb-column panels; every diagonal block factorised, its factor inverted
    explicitly, the panel below multiplied by that inverse, the trailing matrix
    updated; the forward and backward solves multiply by the same inverses."""
    import scipy.linalg as sl
    n = A.shape[0]
    L = np.tril(A).copy()
    inv = []
    for k in range(0, n, nb):
        e = min(k + nb, n)
        Lkk = np.linalg.cholesky(L[k:e, k:e] + np.tril(L[k:e, k:e], -1).T)
        Ikk = sl.solve_triangular(Lkk, np.eye(e - k), lower=True)
        inv.append(Ikk)
        L[k:e, k:e] = Lkk
        if e < n:
            L[e:, k:e] = L[e:, k:e] @ Ikk.T
            L[e:, e:] -= np.tril(L[e:, k:e] @ L[e:, k:e].T)

    def solve(B):
        X = np.array(B, dtype=np.float64)
        for q, k in enumerate(range(0, n, nb)):
            e = min(k + nb, n)
            X[k:e] = inv[q] @ X[k:e]
            X[e:] -= L[e:, k:e] @ X[k:e]
        for q, k in reversed(list(enumerate(range(0, n, nb)))):
            e = min(k + nb, n)
            X[k:e] -= L[e:, k:e].T @ X[e:]
            X[k:e] = inv[q].T @ X[k:e]
        return X
    return solve


def _tile_factor_invert(T, sizes=(16, 8)):
    """(L, X = L^-1) of an SPD tile by the GPU's recursion (diag_factor_invert,
    diag16_*): right-looking over sub-blocks of sizes[0] columns, the diagonal
    sub-block factorised and inverted by the same scheme one size down (plain
    substitution at the bottom), and
      L_IJ = A_IJ X_JJ^T,  X_JK = X_JJ W_JK (K < J),
      A_IK -= L_IJ L_KJ^T (K > J),  W_IK -= L_IJ X_JK (K <= J)."""
    import scipy.linalg as sl
    n = T.shape[0]
    if not sizes or n <= sizes[-1]:
        L = np.linalg.cholesky(T)
        return L, sl.solve_triangular(L, np.eye(n), lower=True)
    b = sizes[0]
    A = np.tril(T) + np.tril(T, -1).T
    L = np.zeros((n, n))
    W = np.zeros((n, n))
    for j in range(0, n, b):
        e = min(j + b, n)
        L[j:e, j:e], X = _tile_factor_invert(A[j:e, j:e], sizes[1:])
        W[j:e, :j] = X @ W[j:e, :j]
        W[j:e, j:e] = X
        if e < n:
            L[e:, j:e] = A[e:, j:e] @ X.T
            A[e:, e:] -= L[e:, j:e] @ L[e:, j:e].T
            W[e:, :e] -= L[e:, j:e] @ W[j:e, :e]
    return L, W


class GpuScheme:
    """float64 emulation of the factorisation as the GPU carries it out, under
    the GPU's own elimination order p (row index per new position): 64-column
    panels, every diagonal tile factorised and inverted by the recursion over
    16- and 8-column sub-blocks, the panel below multiplied by that inverse;
    forward and backward solves multiply by the same inverses; a marginal
    covariance is the Gram matrix of the forward solve alone (k_marginals)."""

    def __init__(self, A, p, nb=K_NB):
        self.p, self.ip, self.nb = p, np.argsort(p), nb
        n = A.shape[0]
        L = np.tril(A[np.ix_(p, p)])
        self.inv = []
        for k in range(0, n, nb):
            e = min(k + nb, n)
            L[k:e, k:e], X = _tile_factor_invert(L[k:e, k:e])
            self.inv.append(X)
            if e < n:
                L[e:, k:e] = L[e:, k:e] @ X.T
                L[e:, e:] -= np.tril(L[e:, k:e] @ L[e:, k:e].T)
        self.L, self.n = L, n

    def forward(self, B):
        Y = np.array(B, dtype=np.float64)[self.p]
        for q, k in enumerate(range(0, self.n, self.nb)):
            e = min(k + self.nb, self.n)
            Y[k:e] = self.inv[q] @ Y[k:e]
            Y[e:] -= self.L[e:, k:e] @ Y[k:e]
        return Y

    def solve(self, B):
        X = self.forward(B)
        for q, k in reversed(list(enumerate(range(0, self.n, self.nb)))):
            e = min(k + self.nb, self.n)
            X[k:e] -= self.L[e:, k:e].T @ X[e:]
            X[k:e] = self.inv[q].T @ X[k:e]
        return X[self.ip]

    def gram(self, E):
        Y = self.forward(E)
        return Y.T @ Y


def scalar_order(pose_order):
    """Row permutation of the 3 n scalar unknowns from an elimination order of the n poses."""
    pose_order = np.asarray(pose_order, dtype=np.int64)
    return (3 * pose_order[:, None] + np.arange(3)[None, :]).ravel()


def yardstick_solvers(A, pose_order=None):
    """float64 CPU solvers of A X = B that differ from each other in the way the
    GPU differs from a textbook solver: LAPACK's LU, its Cholesky, Cholesky
    under the reversed and two random orderings, the blocked scheme with
    explicit diagonal-block inverses, and (given the plan's elimination order)
    the GPU's scheme under that order."""
    n = A.shape[0]
    rng = np.random.default_rng(n)
    out = {"lu": lambda B: np.linalg.solve(A, B), "chol": _chol_solver(A),
           "chol_rev": _permuted(A, np.arange(n)[::-1].copy()),
           "chol_perm1": _permuted(A, rng.permutation(n)), "chol_perm2": _permuted(A, rng.permutation(n)),
           "blocked_inverse": _blocked_inverse_solver(A)}
    if pose_order is not None:
        out["gpu_scheme"] = GpuScheme(A, scalar_order(pose_order)).solve
    return out


def plan_order(g):
    """The Cholesky plan's elimination order of g's poses (host only)."""
    from graphslam_amd.pose_graph import PoseGraph
    with PoseGraph.from_dataset(g) as pg:
        return pg.debug_ordering().astype(np.int64)


def rel_err(d, ref):
    """max|d - ref| / max|ref| (ref in longdouble; the difference is taken there)."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(d, dtype=LD).reshape(ref.shape) - ref).max() / np.abs(ref).max())


def bound(y, n):
    """The GPU's tolerance: 8 x the yardstick (MFMA summation order and the
    16 x 16 sub-block inverses, which the emulation does not copy), the
    yardstick floored at n eps against a lucky one."""
    return 8.0 * max(y, n * 2.2e-16)


@functools.lru_cache(maxsize=None)
def solve_reference(name, lam):
    """(longdouble solution of (H + lam I) d = -g, yardstick y, n) of a case."""
    H, grad = dense_system(build(name))
    n = H.shape[0]
    A = H + lam * np.eye(n)
    ref = ld_solve(ld_cholesky(A), -grad)
    y = max(rel_err(s(-grad), ref) for s in yardstick_solvers(A, plan_order(build(name))).values())
    # the GPU factorises its own float64 evaluation of H and g: the exact
    # solution of another such evaluation is as far from ref as rounding H puts it
    H2, grad2 = dense_system_c_oracle(build(name))
    y = max(y, rel_err(ld_solve(ld_cholesky(H2 + lam * np.eye(n)), -grad2), ref))
    ref.setflags(write=False)
    return ref, y, n


@functools.lru_cache(maxsize=None)
def marginals_reference(name):
    """(graph with the extra prior, pose indices, longdouble 3x3 blocks of H^-1,
    yardstick per block, n) of a case."""
    g = with_last_prior(build(name))
    idx = marginal_keys(g)
    H, _ = dense_system(g)
    n = H.shape[0]
    E = unit_columns(n, idx)
    ref = diag_blocks(ld_solve(ld_cholesky(H), E), idx)
    y = np.zeros(len(idx))
    order = plan_order(g)
    for s in yardstick_solvers(H, order).values():
        got = diag_blocks(s(E), idx)
        y = np.maximum(y, [rel_err(got[q], ref[q]) for q in range(len(idx))])
    G = GpuScheme(H, scalar_order(order)).gram(E)     # the marginals kernel's own form: Y^T Y
    y = np.maximum(y, [rel_err(G[3 * q:3 * q + 3, 3 * q:3 * q + 3], ref[q]) for q in range(len(idx))])
    H2, _ = dense_system_c_oracle(g)                  # rounding of H itself, as in solve_reference
    got = diag_blocks(ld_solve(ld_cholesky(H2), E), idx)
    y = np.maximum(y, [rel_err(got[q], ref[q]) for q in range(len(idx))])
    ref.setflags(write=False)
    return g, idx, ref, y, n
