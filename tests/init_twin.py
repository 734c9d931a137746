"""Numpy / scipy twin of the two-stage linear initialisation
(pgo_initialize_linear, include/pgo.h): the breadth-first spanning tree and the
2 pi integers, the two linear systems in the device's embedded 3x3-block
layout, and their solutions by scipy's sparse LU.  Test infrastructure only.

The tree is written to be reproduced bitwise: delta through libm's sin / cos /
atan2 (math, not numpy's vectorised ones), one add or subtract per tree edge.
"""
from __future__ import annotations

import math
from collections import deque
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import pgo_numpy as tw

TWO_PI = 2.0 * math.pi


class Indeterminant(RuntimeError):
    pass


def wrap1(t):
    return math.atan2(math.sin(t), math.cos(t))


@dataclass
class Tree:
    parent: np.ndarray      # int [n], -1 for a root
    theta: np.ndarray       # f64 [n] tree orientations, not wrapped
    delta: np.ndarray       # f64 [E] wrapped measured angles
    k_edge: np.ndarray      # int64 [E]
    k_prior: np.ndarray     # int64 [P]
    ptheta: np.ndarray      # f64 [P] wrapped prior angles
    depth: int
    components: int

    @property
    def wraps(self):
        return int(np.abs(self.k_edge).sum())


def tree(g) -> Tree:
    ei, ej = (np.asarray(a, dtype=np.int64) for a in g.edge_index())
    pi = np.asarray(g.prior_index(), dtype=np.int64)
    n, ne = g.num_poses, len(ei)
    delta = np.array([wrap1(float(t)) for t in g.edge_z[:, 2]], dtype=np.float64).reshape(ne)
    ptheta = np.array([wrap1(float(t)) for t in g.prior_pose[:, 2]], dtype=np.float64).reshape(len(pi))
    eil, ejl, dl = ei.tolist(), ej.tolist(), delta.tolist()   # (plain lists: the loops below are Python's)
    adj = [[] for _ in range(n)]                       # factors of a vertex, insertion order, either end
    for e in range(ne):
        adj[eil[e]].append(e)
        adj[ejl[e]].append(e)
    comp = np.full(n, -1, dtype=np.int64)
    nc = 0
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = nc
        q = deque([s])
        while q:
            u = q.popleft()
            for e in adj[u]:
                v = ejl[e] if eil[e] == u else eil[e]
                if comp[v] < 0:
                    comp[v] = nc
                    q.append(v)
        nc += 1
    first_prior = {}
    for k, v in enumerate(pi):
        first_prior.setdefault(int(v), k)
    root = [-1] * nc
    for v in range(n):
        if v in first_prior and root[comp[v]] < 0:
            root[comp[v]] = v
    if any(r < 0 for r in root):
        raise Indeterminant("a connected component has no prior")
    parent = np.full(n, -1, dtype=np.int64)
    theta = np.zeros(n)
    depth = np.full(n, -1, dtype=np.int64)
    for r in root:
        theta[r] = ptheta[first_prior[r]]
        depth[r] = 0
        q = deque([r])
        while q:
            u = q.popleft()
            for e in adj[u]:
                from_i = eil[e] == u
                v = ejl[e] if from_i else eil[e]
                if depth[v] >= 0:
                    continue
                depth[v] = depth[u] + 1
                parent[v] = u
                theta[v] = theta[u] + dl[e] if from_i else theta[u] - dl[e]
                q.append(v)
    k_edge = np.rint((theta[ej] - theta[ei] - delta) / TWO_PI).astype(np.int64)
    k_prior = np.rint((theta[pi] - ptheta) / TWO_PI).astype(np.int64)
    return Tree(parent, theta, delta, k_edge, k_prior, ptheta, int(depth.max()) if n else 0, nc)


def problem(g):
    """pgo_numpy's Problem of g, built once per graph object (change a graph's
    factors before its first use here)."""
    p = getattr(g, "_twin_problem", None)
    if p is None:
        p = tw.problem_from_graph(g)
        g._twin_problem = p
    return p


def theta_information(om):
    """o22 - (o02, o12) Omega_tt^-1 (o02, o12)': the angle's information with the
    translation marginalised out (om: [K,3,3])."""
    b = om[:, :2, 2]
    return om[:, 2, 2] - np.einsum("ki,kij,kj->k", b, np.linalg.inv(om[:, :2, :2]), b)


@dataclass
class System:
    hdiag: np.ndarray       # [n,3,3]
    hoff: np.ndarray        # [E,3,3] block (k1, k2) of every between factor
    rhs: np.ndarray         # [n,3]
    A: sp.csc_matrix        # the scalar (stage 1: n x n) or 2x2-block (stage 2: 2n x 2n) system
    b: np.ndarray


def orientation_system(g, t: Tree | None = None) -> System:
    prob = problem(g)
    t = t or tree(g)
    n, ne = prob.n, len(prob.ei)
    w, wq = theta_information(prob.eom), theta_information(prob.pom)
    tgt = t.delta + TWO_PI * t.k_edge
    ptgt = t.ptheta + TWO_PI * t.k_prior
    diag = np.zeros(n)
    np.add.at(diag, prob.ei, w)
    np.add.at(diag, prob.ej, w)
    np.add.at(diag, prob.pi, wq)
    b = np.zeros(n)
    np.add.at(b, prob.ej, w * tgt)
    np.add.at(b, prob.ei, -w * tgt)
    np.add.at(b, prob.pi, wq * ptgt)
    A = sp.coo_matrix((np.concatenate([diag, -w, -w]),
                       (np.concatenate([np.arange(n), prob.ei, prob.ej]),
                        np.concatenate([np.arange(n), prob.ej, prob.ei]))), shape=(n, n)).tocsc()
    hd = np.zeros((n, 3, 3))
    hd[:, 0, 0] = hd[:, 1, 1] = 1.0
    hd[:, 2, 2] = diag
    ho = np.zeros((ne, 3, 3))
    ho[:, 2, 2] = -w
    rhs = np.zeros((n, 3))
    rhs[:, 2] = b
    return System(hd, ho, rhs, A, b)


def _rot(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)      # [K,2,2]


def position_system(g, theta) -> System:
    """The graph's Gaussian error over the positions, orientations held at theta."""
    prob = problem(g)
    theta = np.asarray(theta, dtype=np.float64)
    n, ne = prob.n, len(prob.ei)
    delta = np.arctan2(prob.ez[:, 3], prob.ez[:, 2])
    Rz = _rot(delta)
    A = np.einsum("kji,klj->kil", Rz, _rot(theta[prob.ei]))                  # R_z' R_i'
    c = np.einsum("kji,kj->ki", Rz, prob.ez[:, :2])                           # R_z' t_z
    eth = tw_wrap(theta[prob.ej] - theta[prob.ei] - delta)
    ott, oth = prob.eom[:, :2, :2], prob.eom[:, :2, 2]
    M = np.einsum("kji,kjl,klm->kim", A, ott, A)
    r = np.einsum("kji,kj->ki", A, np.einsum("kij,kj->ki", ott, c) - oth * eth[:, None])
    Rv = _rot(theta[prob.pi])
    ptheta = np.arctan2(prob.pz[:, 3], prob.pz[:, 2])
    Mq = np.einsum("kij,kjl,kml->kim", Rv, prob.pom[:, :2, :2], Rv)
    ethq = tw_wrap(theta[prob.pi] - ptheta)
    bq = np.einsum("kij,kj->ki", Mq, prob.pz[:, :2]) - np.einsum("kij,kj->ki", Rv, prob.pom[:, :2, 2] * ethq[:, None])
    D = np.zeros((n, 2, 2))
    np.add.at(D, prob.ei, M)
    np.add.at(D, prob.ej, M)
    np.add.at(D, prob.pi, Mq)
    b = np.zeros((n, 2))
    np.add.at(b, prob.ej, r)
    np.add.at(b, prob.ei, -r)
    np.add.at(b, prob.pi, bq)
    rows, cols, vals = [], [], []

    def add_block(rr, cc, blk):
        rows.append((2 * rr[:, None, None] + np.arange(2)[None, :, None]).repeat(2, axis=2).ravel())
        cols.append((2 * cc[:, None, None] + np.arange(2)[None, None, :]).repeat(2, axis=1).ravel())
        vals.append(blk.ravel())

    add_block(np.arange(n), np.arange(n), D)
    add_block(prob.ei, prob.ej, -M)
    add_block(prob.ej, prob.ei, -np.transpose(M, (0, 2, 1)))
    Asp = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                        shape=(2 * n, 2 * n)).tocsc()
    hd = np.zeros((n, 3, 3))
    hd[:, :2, :2] = D
    hd[:, 2, 2] = 1.0
    ho = np.zeros((ne, 3, 3))
    ho[:, :2, :2] = -M
    rhs = np.zeros((n, 3))
    rhs[:, :2] = b
    return System(hd, ho, rhs, Asp, b.ravel())


def tw_wrap(t):
    return np.arctan2(np.sin(t), np.cos(t))


def solve(system: System):
    x = spla.splu(system.A, permc_spec="COLAMD").solve(system.b)
    if not np.all(np.isfinite(x)):
        raise Indeterminant("singular system")
    return x


def initialize(g):
    """(x, y, theta) of every pose after the two solves; theta is stage 1's
    solution as it comes, not wrapped."""
    theta = solve(orientation_system(g))
    xy = solve(position_system(g, theta)).reshape(-1, 2)
    return np.column_stack([xy, theta])


def error(g, xyt):
    """pgo_numpy.error (no loss) at (x, y, theta) values."""
    return tw.error(problem(g), tw.from_xyt(xyt))


# ------------------------------------------------------------ designed graphs
def from_truth(name, gt, pairs, prior_vertices, seed, nondiagonal=False):
    """Noisy measurements between ground-truth poses over `pairs` (i, j), priors
    at the true pose of `prior_vertices`; initial values far from the truth."""
    from graphslam_amd import datasets as ds
    rng = np.random.default_rng(seed)
    gt = np.asarray(gt, dtype=np.float64)
    n = len(gt)
    i = np.array([p[0] for p in pairs], dtype=np.int64).reshape(-1)
    j = np.array([p[1] for p in pairs], dtype=np.int64).reshape(-1)
    z = ds.compose_xyt(ds.between_xyt(gt[i], gt[j]), rng.standard_normal((len(i), 3)) * ds.SIGMA).reshape(-1, 3)
    cov = ds._diag_cov(ds.SIGMA, len(i))
    if nondiagonal:
        cov = random_covariances(len(i), seed + 1)
    pv = np.asarray(prior_vertices, dtype=np.int64)
    init = gt + rng.standard_normal((n, 3)) * np.array([2.0, 2.0, 1.0])
    return ds.PoseGraph(name=name, keys=np.arange(1, n + 1, dtype=np.uint64), initial=init, ground_truth=gt,
                        edge_k1=(i + 1).astype(np.uint64), edge_k2=(j + 1).astype(np.uint64), edge_z=z, edge_cov=cov,
                        prior_keys=(pv + 1).astype(np.uint64), prior_pose=gt[pv].copy(),
                        prior_cov=ds._diag_cov(ds.PRIOR_SIGMA, len(pv)), meta={})


def random_covariances(count, seed=5):
    """The non-diagonal covariances of test_linearize_nondiagonal_covariance."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.normal(size=(count, 3, 3)) * 0.02) + np.eye(3) * 0.05
    return (L @ np.transpose(L, (0, 2, 1))).reshape(-1, 9)


def square_turn(side_poses=3, seed=21):
    """A noisy closed square walked once: the measured turns sum to 2 pi, so the
    factor where the two arms of the breadth-first tree meet has k != 0.  The
    prior sits on a vertex in the middle of the insertion order."""
    from graphslam_amd import datasets as ds
    gt = ds.square_loop(side_poses).ground_truth
    n = len(gt)
    return from_truth("square-turn", gt, [(k, k + 1) for k in range(n - 1)] + [(n - 1, 0)], [n // 3], seed)


def star(spokes=300, seed=22):
    """One hub with `spokes` spokes, every second one with the hub as k2: the
    hub's row is longer than a workgroup."""
    a = np.linspace(0.0, 2 * np.pi, spokes, endpoint=False)
    gt = np.vstack([[0.5, -0.25, 0.3], np.column_stack([3 * np.cos(a), 3 * np.sin(a), 2.5 * a - 3.0])])
    pairs = [(0, k) if k & 1 else (k, 0) for k in range(1, spokes + 1)]
    return from_truth("star", gt, pairs, [0], seed)


def two_components(seed=23, prior_b=True):
    """Two loops that share no factor, a prior in each (the second one's not on
    its first vertex); prior_b False leaves the second without one."""
    na, nb = 7, 9

    def ring(m, r, x0):
        a = np.linspace(0.0, 2 * np.pi, m, endpoint=False)
        return np.column_stack([x0 + r * np.cos(a), r * np.sin(a), a + np.pi / 2])

    gt = np.vstack([ring(na, 2.0, 0.0), ring(nb, 3.0, 10.0)])
    pairs = [(k, (k + 1) % na) for k in range(na)] + [(na + (k + 1) % nb, na + k) for k in range(nb)]
    return from_truth("two-components", gt, pairs, [0, na + 4] if prior_b else [0], seed)
