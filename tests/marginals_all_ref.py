"""Reference, yardstick and float64 emulation for PoseGraph.marginal_covariances_all.

The selected inverse Z = H^-1 on the pattern of L follows from the factor in
one pass from the last 64-column block to the first (Takahashi's recurrence):
with X the inverted diagonal tile of block b, R the rows below the block and
L_Rb the stored panel,

    G = L_Rb X,    Z_Rb = -Z_RR G,    Z_bb = X^T X - G^T Z_Rb.

``selinv_emulation`` restates it in float64 numpy on top of
front_shapes.GpuScheme (the GPU's 64-column panels and explicit tile inverses
under the plan's elimination order; one dense front, so every entry of H^-1
is "selected").  ``reference`` gives, per designed case, the longdouble
blocks and the yardstick of front_shapes.marginals_reference -- the same
members, for the checked index set, 6 x 6 joint blocks of the edges included
-- with the emulation's own error beside it.
"""
from __future__ import annotations

import functools

import numpy as np

import front_shapes as fs

MAX_FULL_POSES = 110    # cases up to this size: every pose and every edge is referenced
SUBSET_STRIDE = 16      # larger cases: marginal_keys and every 16th pose, the edges among them


def selinv_emulation(S: fs.GpuScheme):
    """H^-1 (original row order) from a GpuScheme by the blocked recurrence."""
    n, nb, L = S.n, S.nb, S.L
    Z = np.zeros((n, n))
    for q, k in reversed(list(enumerate(range(0, n, nb)))):
        e = min(k + nb, n)
        X = S.inv[q]
        T = X.T @ X
        if e < n:
            G = L[e:, k:e] @ X
            Zrb = -(Z[e:, e:] @ G)
            Z[e:, k:e] = Zrb
            Z[k:e, e:] = Zrb.T
            T = T - G.T @ Zrb
        Z[k:e, k:e] = np.tril(T) + np.tril(T, -1).T    # (the lower triangle is what is kept)
    return Z[np.ix_(S.ip, S.ip)]


def checked_set(g):
    """(pose indices, edge indices) the reference covers for graph g."""
    n = g.num_poses
    if n <= MAX_FULL_POSES:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = np.asarray(sorted({*map(int, fs.marginal_keys(g)), *range(0, n, SUBSET_STRIDE)}), dtype=np.int64)
    inside = np.zeros(n, dtype=bool)
    inside[idx] = True
    ei, ej = g.edge_index()
    edges = np.flatnonzero(inside[ei] & inside[ej])
    return idx, edges


def pose_block(M, q):
    return M[3 * q:3 * q + 3, 3 * q:3 * q + 3]


def joint_block(M, qi, qj):
    r = np.r_[3 * qi:3 * qi + 3, 3 * qj:3 * qj + 3]
    return M[np.ix_(r, r)]


def joint_from_parts(ci, cj, x):
    """The 6 x 6 joint marginal from cov[k1], cov[k2] and the cross block (k1 rows, k2 columns)."""
    return np.block([[ci, x], [x.T, cj]])


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict of a case: the graph with the extra prior ``g``, checked poses
    ``idx`` and edges ``edges`` (with ``eq``: their endpoints' positions in
    idx), the longdouble H^-1 restricted to idx ``ref`` [3k, 3k], the
    yardsticks ``y_pose`` / ``y_edge`` (the members of
    front_shapes.marginals_reference), the emulation's errors ``emu_pose`` /
    ``emu_edge`` by the same measure, and the scalar size ``n``."""
    g = fs.with_last_prior(fs.build(name))
    idx, edges = checked_set(g)
    pos = {int(i): q for q, i in enumerate(idx)}
    ei, ej = g.edge_index()
    eq = [(pos[int(ei[f])], pos[int(ej[f])]) for f in edges]
    H, _ = fs.dense_system(g)
    n = H.shape[0]
    E = fs.unit_columns(n, idx)
    sel = fs.scalar_order(idx)
    ref = fs.ld_solve(fs.ld_cholesky(H), E)[sel]
    order = fs.plan_order(g)
    members = [s(E)[sel] for s in fs.yardstick_solvers(H, order).values()]
    S = fs.GpuScheme(H, fs.scalar_order(order))
    members.append(S.gram(E))                              # the k_marginals form: Y^T Y
    H2, _ = fs.dense_system_c_oracle(g)                    # rounding of H itself
    members.append(fs.ld_solve(fs.ld_cholesky(H2), E)[sel])
    emu = selinv_emulation(S)[np.ix_(sel, sel)]

    def errs(M):
        p = np.array([fs.rel_err(pose_block(M, q), pose_block(ref, q)) for q in range(len(idx))])
        e = np.array([fs.rel_err(joint_block(M, a, b), joint_block(ref, a, b)) for a, b in eq])
        return p, e

    y_pose, y_edge = np.zeros(len(idx)), np.zeros(len(eq))
    for M in members:
        p, e = errs(M)
        y_pose, y_edge = np.maximum(y_pose, p), np.maximum(y_edge, e)
    emu_pose, emu_edge = errs(emu)
    ref.setflags(write=False)
    return dict(g=g, idx=idx, edges=edges, eq=eq, ref=ref, y_pose=y_pose, y_edge=y_edge, emu_pose=emu_pose,
                emu_edge=emu_edge, n=n)
