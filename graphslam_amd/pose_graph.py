"""Native handle over libpgo.so: a device-resident pose graph.

``PoseGraph`` is the bulk, zero-copy-ish entry point (numpy arrays in, numpy
arrays out) used by the GTSAM-named mirror in ``graphslam_amd.gtsam`` and by
bench.py.  Every call goes through the C-ABI of include/pgo.h.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class PgoError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"[{status}] {message}")
        self.status = status


class ValuesKeyAlreadyExists(PgoError, KeyError):
    """gtsam::ValuesKeyAlreadyExists (Values::insert on an existing key)."""


class ValuesKeyDoesNotExist(PgoError, KeyError):
    """gtsam::ValuesKeyDoesNotExist (Values::at / a factor on a missing key)."""


class IndeterminantLinearSystemException(PgoError):
    """gtsam::IndeterminantLinearSystemException (singular Gauss-Newton system)."""


class BadCovariance(PgoError, ValueError):
    """Covariance is not symmetric positive definite (GTSAM's LLT would fail)."""


class NotEnoughKeyframes(PgoError):
    """closest_keyframe service returning false (graph.cpp:170-171)."""


_EXC = {
    L.PGO_E_DUP_KEY: ValuesKeyAlreadyExists,
    L.PGO_E_NO_KEY: ValuesKeyDoesNotExist,
    L.PGO_E_INDETERMINANT: IndeterminantLinearSystemException,
    L.PGO_E_BAD_COV: BadCovariance,
    L.PGO_E_NOT_ENOUGH: NotEnoughKeyframes,
}

KEYFRAMES_TO_SKIP_IN_LOOP_CLOSING = 10   # graph.cpp:15


def _loss_code(loss):
    if isinstance(loss, str):
        if loss.lower() not in L.LOSSES:
            raise ValueError(f"unknown robust loss {loss!r}; have {sorted(L.LOSSES)}")
        return L.LOSSES[loss.lower()]
    return int(loss)


def default_params(**kw) -> L.PgoParams:
    p = L.PgoParams()
    L.lib().pgo_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"pgo_params has no field {k!r}")
        setattr(p, k, v)
    return p


def gnc_loss_code(loss):
    if isinstance(loss, str):
        if loss.lower() not in L.GNC_LOSSES:
            raise ValueError(f"unknown GNC loss {loss!r}; have {sorted(L.GNC_LOSSES)}")
        return L.GNC_LOSSES[loss.lower()]
    return int(loss)


def default_gnc_params(**kw) -> L.PgoGncParams:
    p = L.PgoGncParams()
    L.lib().pgo_gnc_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"pgo_gnc_params has no field {k!r}")
        setattr(p, k, gnc_loss_code(v) if k == "loss" else v)
    return p


def debug_gnc_weight(loss, mu, barc_sq, r2):
    """Host-only (pgo_debug_gnc_weight): the GNC weight of every r2."""
    r2 = np.ascontiguousarray(np.atleast_1d(r2), dtype=np.float64)
    w = np.zeros_like(r2)
    rc = L.lib().pgo_debug_gnc_weight(gnc_loss_code(loss), float(mu), float(barc_sq), len(r2), L.dptr(r2), L.dptr(w))
    if rc != L.PGO_OK:
        raise ValueError(f"pgo_debug_gnc_weight: {rc}")
    return w


def debug_gnc_control(rmax_sq, cost, nonbinary, initial_error=0.0, params=None, **kw):
    """Host-only (pgo_debug_gnc_control): the GNC control on recorded rows
    (row 0 the plain solve).  Returns (mu per walked row, stop reason or -1
    when the rows ran out, rows walked)."""
    p = params if params is not None else default_gnc_params(**kw)
    rmax_sq, cost, nonbinary = (np.ascontiguousarray(a, dtype=np.float64) for a in (rmax_sq, cost, nonbinary))
    rows = len(cost)
    mu, stop = np.full(max(rows, 1), np.nan), C.c_int(0)
    n = L.lib().pgo_debug_gnc_control(C.byref(p), float(initial_error), rows, L.dptr(rmax_sq), L.dptr(cost),
                                      L.dptr(nonbinary), L.dptr(mu), C.byref(stop))
    if n < 0:
        raise ValueError(f"pgo_debug_gnc_control: {n}")
    return mu[:n].copy(), stop.value, n


def trace_linearisations(trace, gn=False):
    """A trace's tries (solved, candidate error, model decrease) split where
    the optimiser linearised again: after every accepted try (a linearisation
    without one is the last); Gauss-Newton: every step."""
    trace = np.asarray(trace)
    tries = trace[:, [2, 4, 3]]
    if gn or not len(tries):
        return [tries[i:i + 1] for i in range(len(tries))]
    cuts = list(np.nonzero(trace[:, 6] == 1)[0] + 1)
    if not cuts or cuts[-1] != len(trace):
        cuts.append(len(trace))
    return [tries[a:b] for a, b in zip([0] + cuts[:-1], cuts)]


def debug_lm_replay(lins, initial_error, ranks=1, lanes=1, lin_err=None, adapt_mode=1, params=None, **kw):
    """Host-only (pgo_debug_lm_replay): the optimiser's control driven as
    pgo_optimize drives it over ranks x lanes tries per round, on recorded
    tries instead of a device.  ``lins``: per linearisation an (n, 3) array of
    (solved, error at the candidate, model decrease) -- a trace's columns 2,
    4, 3.  Returns the seven-column trace, the counters and the (rank, lane)
    of every accepted try."""
    p = params if params is not None else default_params(**kw)
    lins = [np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in lins]
    ptr = np.cumsum([0] + [len(t) for t in lins]).astype(np.int32)
    tries = np.ascontiguousarray(np.concatenate(lins) if lins else np.zeros((0, 3)))
    le = None if lin_err is None else np.ascontiguousarray(lin_err, dtype=np.float64)
    cap = 8 * (len(tries) + len(lins) + 1)
    trace, out = np.zeros((cap, 7)), np.zeros(11 + 2 * cap)
    n = L.lib().pgo_debug_lm_replay(C.byref(p), float(initial_error), int(ranks), int(lanes), int(adapt_mode),
                                    len(lins), ptr.ctypes.data_as(C.POINTER(C.c_int)), L.dptr(tries), L.dptr(le),
                                    L.dptr(trace), cap, L.dptr(out), len(out))
    if n < 0 or n > cap:
        raise ValueError(f"pgo_debug_lm_replay: {n}")
    names = ("iterations", "inner_iterations", "linearizations", "status", "stop_reason")
    res = {k: int(out[i]) for i, k in enumerate(names)}
    res.update(lam=out[5], factor=out[6], final_error=out[7], lambda_rounds=int(out[8]), exhausted=bool(out[9]),
               trace=trace[:n].copy(), winners=out[11:11 + 2 * int(out[10])].astype(int).reshape(-1, 2))
    return res


class PoseGraph:
    """One pgo_graph handle (one HIP stream, graph + values resident in HBM)."""

    def __init__(self, device: int = 0, ordering: int = L.PGO_ORDERING_ND):
        self._L = L.lib()
        opts = L.PgoOpts()
        opts.device = device
        opts.ordering = ordering
        self._h = self._L.pgo_create(C.byref(opts))
        if not self._h:
            raise MemoryError("pgo_create failed")
        self.last_stats = None
        self._priors = 0

    # ------------------------------------------------------------------ utils
    def _check(self, rc):
        if rc < 0:
            msg = self._L.pgo_last_error(self._h).decode()
            raise _EXC.get(rc, PgoError)(rc, msg)
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._L.pgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------ construction
    def add_vertex(self, key, x, y, theta):
        self._check(self._L.pgo_add_vertex(self._h, int(key), float(x), float(y), float(theta)))

    def add_vertices(self, keys, xyt):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        xyt = np.ascontiguousarray(xyt, dtype=np.float64).reshape(-1, 3)
        self._check(self._L.pgo_add_vertices(self._h, len(keys), L.u64ptr(keys), L.dptr(xyt)))

    def add_prior(self, key, pose, cov):
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3)
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(9)
        self._check(self._L.pgo_add_prior(self._h, int(key), L.dptr(pose), L.dptr(cov)))
        self._priors += 1

    def add_edge(self, k1, k2, z, cov, loss=None, k=None):
        """One between factor; ``loss`` (PGO_LOSS_* or its name in _lib.LOSSES)
        with parameter ``k`` makes it robust (pgo_add_edge_robust)."""
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(3)
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(9)
        if loss is None:
            self._check(self._L.pgo_add_edge(self._h, int(k1), int(k2), L.dptr(z), L.dptr(cov)))
            return
        self._check(self._L.pgo_add_edge_robust(self._h, int(k1), int(k2), L.dptr(z), L.dptr(cov),
                                                _loss_code(loss), 1.0 if k is None else float(k)))

    def add_edges(self, k1, k2, z, cov, loss=None, k=None):
        """Bulk between factors; ``loss`` / ``k``: None (Gaussian), scalars
        (shared by all), or one per edge (pgo_add_edges_robust)."""
        k1 = np.ascontiguousarray(k1, dtype=np.uint64)
        k2 = np.ascontiguousarray(k2, dtype=np.uint64)
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 3)
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        stride = 0 if cov.size == 9 else 9
        if stride and cov.reshape(-1, 9).shape[0] != len(k1):
            raise ValueError("cov must be one [9] or [E,9]")
        if loss is None:
            self._check(self._L.pgo_add_edges(self._h, len(k1), L.u64ptr(k1), L.u64ptr(k2), L.dptr(z),
                                              L.dptr(cov), stride))
            return
        per_edge = np.ndim(loss) > 0 or np.ndim(k) > 0
        m = len(k1) if per_edge else 1
        if np.ndim(loss) > 0:
            codes = np.array([_loss_code(v) for v in loss], dtype=np.int32)
        else:
            codes = np.full(m, _loss_code(loss), dtype=np.int32)
        ks = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if k is None else k, dtype=np.float64), (m,)))
        if len(codes) != m:
            raise ValueError("loss must be a scalar or one per edge")
        self._check(self._L.pgo_add_edges_robust(self._h, len(k1), L.u64ptr(k1), L.u64ptr(k2), L.dptr(z),
                                                 L.dptr(cov), stride, codes.ctypes.data_as(C.POINTER(C.c_int)),
                                                 L.dptr(ks), 1 if per_edge else 0))

    def edge_weights(self, first=0, n=None):
        """w(r) of the between factors [first, first + n) in insertion order at
        the current values (1.0 for Gaussian factors): low weights mark the loop
        closures the robust loss has rejected."""
        if n is None:
            n = self.num_factors - self._priors - int(first)
        out = np.zeros(int(n))
        self._check(self._L.pgo_get_edge_weights(self._h, int(first), int(n), L.dptr(out)))
        return out

    def set_edge_weights(self, w, first=0):
        """Fixed weights in [0, 1] on the between factors [first, first + len(w))
        in insertion order (pgo_set_edge_weights; they must be PGO_LOSS_NONE):
        the factor's error becomes w r^2 / 2 whatever the values, 1 makes it a
        plain Gaussian factor again, 0 takes it out of every later solve."""
        w = np.ascontiguousarray(np.atleast_1d(w), dtype=np.float64)
        self._check(self._L.pgo_set_edge_weights(self._h, int(first), len(w), L.dptr(w)))

    def _between(self):
        return self.num_factors - self._priors

    @staticmethod
    def _size_t_array(idx):
        a = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        if len(a) and a.min() < 0:
            raise ValueError("candidate indices must be non-negative")
        a = a.astype(np.uintp)
        return a, a.ctypes.data_as(C.POINTER(C.c_size_t))

    def optimize_gnc(self, candidates=None, params: L.PgoParams | None = None, gnc: L.PgoGncParams | None = None,
                     **kw):
        """Graduated non-convexity (pgo_optimize_gnc) over the between factors
        ``candidates`` (insertion indices; None: all of them).  ``params`` /
        keywords naming pgo_params fields configure the inner optimizes,
        ``gnc`` / keywords naming pgo_gnc_params fields (loss also by name,
        "gm" / "tls") the outer loop; a name both structs have
        (``max_iterations``) goes to the outer loop.  Returns the pgo_gnc_stats
        as a dict; ``edge_weights()`` then holds the final weights unless
        ``keep_weights=0``."""
        gp = gnc if gnc is not None else default_gnc_params()
        inner_kw = {}
        for k, v in kw.items():
            if hasattr(gp, k):
                setattr(gp, k, gnc_loss_code(v) if k == "loss" else v)
            else:
                inner_kw[k] = v
        p = params if params is not None else default_params(**inner_kw)
        if params is not None and inner_kw:
            raise AttributeError(f"unknown fields {sorted(inner_kw)}")
        if candidates is None:
            n, ip, keep = self._between(), None, None
        else:
            keep, ip = self._size_t_array(candidates)
            n = len(keep)
            if n == 0:   # (an empty list is "none", NULL would be "all")
                keep = np.zeros(1, np.uintp)
                ip = keep.ctypes.data_as(C.POINTER(C.c_size_t))
        st = L.PgoGncStats()
        rc = self._L.pgo_optimize_gnc(self._h, C.byref(p), C.byref(gp), n, ip, C.byref(st))
        self.last_gnc_stats = st.as_dict()
        self._check(rc)
        return self.last_gnc_stats

    def gnc_trace(self):
        """Per inner solve of the last optimize_gnc (pgo_get_gnc_trace), row 0
        the plain solve: (mu, cost, sum of the candidates' weights, non-binary
        weights, largest candidate r^2 of the sweep, inner tries, inner
        accepted steps, inner stop reason)."""
        n = self._check(self._L.pgo_get_gnc_trace(self._h, None, 0))
        out = np.zeros((n, 8))
        if n:
            self._check(self._L.pgo_get_gnc_trace(self._h, L.dptr(out), n))
        return out

    def debug_gnc_sweep(self, loss, mu, barc_sq, candidates=None, write=False):
        """The GNC weights sweep once at the current values
        (pgo_debug_gnc_sweep): (one weight per between factor, non-candidates
        1; [max r^2, sum w, non-binary at 1e-4, r^2 > barc_sq, candidates])."""
        ne = self._between()
        w, s5 = np.ones(ne), np.zeros(5)
        if candidates is None:
            n, ip, keep = ne, None, None
        else:
            keep, ip = self._size_t_array(candidates)
            n = len(keep)
            if n == 0:
                keep = np.zeros(1, np.uintp)
                ip = keep.ctypes.data_as(C.POINTER(C.c_size_t))
        self._check(self._L.pgo_debug_gnc_sweep(self._h, gnc_loss_code(loss), float(mu), float(barc_sq), n, ip,
                                                1 if write else 0, L.dptr(w), L.dptr(s5)))
        return w, s5

    @classmethod
    def from_dataset(cls, g, device=0, ordering=L.PGO_ORDERING_ND):
        """Load a graphslam_amd.datasets.PoseGraph (vertices, priors, edges)."""
        pg = cls(device, ordering)
        pg.add_vertices(g.keys, g.initial)
        for k, p, c in zip(g.prior_keys, g.prior_pose, g.prior_cov):
            pg.add_prior(int(k), p, c)
        pg.add_edges(g.edge_k1, g.edge_k2, g.edge_z, g.edge_cov, loss=getattr(g, "edge_loss", None),
                     k=getattr(g, "edge_loss_k", None))
        return pg

    # -------------------------------------------------------------- optimise
    def optimize(self, params: L.PgoParams | None = None, **kw):
        p = params if params is not None else default_params(**kw)
        st = L.PgoStats()
        rc = self._L.pgo_optimize(self._h, C.byref(p), C.byref(st))
        self.last_stats = st.as_dict()
        self._check(rc)
        return self.last_stats

    def initialize_linear(self):
        """Two-stage linear initialisation (pgo_initialize_linear): the
        orientations as one linear least-squares problem, the 2 pi ambiguities
        fixed along a breadth-first spanning tree from each component's first
        vertex with a prior, then the positions as a second one with the
        orientations held.  Replaces the handle's values (which are not an
        input) and returns the pgo_init_stats as a dict; a following
        ``optimize()`` starts from the result.

        Not GTSAM's ``lago::initialize`` to the letter: a BFS tree instead of
        the odometric path or a minimum spanning tree, no orientation
        correction in stage 2, priors used as given instead of an added
        anchor.  Robust losses are ignored, and a wrong loop closure enters
        both solves at full weight."""
        st = L.PgoInitStats()
        rc = self._L.pgo_initialize_linear(self._h, C.byref(st))
        self.last_init_stats = st.as_dict()
        self._check(rc)
        return self.last_init_stats

    def debug_init_tree(self):
        """Host-only: initialize_linear's spanning tree -- (parent per vertex,
        -1 for a root; k per between factor; k per prior), insertion order."""
        n, np_ = self.num_vertices, self._priors
        ne = self.num_factors - np_
        parent = np.zeros(n, np.int32)
        ke, kp = np.zeros(ne, np.int64), np.zeros(np_, np.int64)
        llp = C.POINTER(C.c_longlong)
        self._check(self._L.pgo_debug_init_tree(self._h, parent.ctypes.data_as(C.POINTER(C.c_int)),
                                                ke.ctypes.data_as(llp), kp.ctypes.data_as(llp), n, ne, np_))
        return parent, ke, kp

    def debug_init_system(self, stage):
        """The assembled linear system of initialize_linear's stage 1
        (orientations) or 2 (positions, at the current orientations) in
        debug_linearize's layout: (hdiag [n,3,3], hoff [E,3,3], rhs [n,3])."""
        n = self.num_vertices
        hd = np.zeros((n, 3, 3))
        ho = np.zeros((self.num_factors - self._priors, 3, 3))
        rhs = np.zeros((n, 3))
        self._check(self._L.pgo_debug_init_system(self._h, int(stage), L.dptr(hd), L.dptr(ho), L.dptr(rhs)))
        return hd, ho, rhs

    def trace(self):
        """Per-iteration record of the last optimize (pgo_get_trace): rows of
        (accepted steps, lambda, solved, model decrease, candidate error,
        fidelity, accepted, wall ms)."""
        n = self._check(self._L.pgo_get_trace(self._h, None, 0))
        out = np.zeros((n, 8))
        if n:
            self._check(self._L.pgo_get_trace(self._h, L.dptr(out), n))
        return out

    def kernel_profile(self):
        """Profiled factorisations of the last optimize (profile_every > 0):
        {family: {launches, ms, flops, bytes}} for the families that ran."""
        nf = self._check(self._L.pgo_get_kernel_profile(self._h, None, 0))
        out = np.zeros((nf, 5))
        self._check(self._L.pgo_get_kernel_profile(self._h, L.dptr(out), nf))
        res = {}
        for f in range(nf):
            if out[f, 0] > 0:
                res[self._L.pgo_kernel_family_name(f).decode()] = dict(
                    launches=int(out[f, 0]), ms=float(out[f, 1]), flops=float(out[f, 2]), bytes=float(out[f, 3]))
        return res

    def debug_partition(self, size):
        """Host-only: the PGO_MULTI_PARTITION subtree partition over `size`
        ranks: (owner per supernode, -1 = replicated top; per-rank subtree
        flops; top flops)."""
        owner, out = self._partition(size)
        return owner, out[:size].copy(), float(out[size])

    def _partition(self, size):
        ns = self._check(self._L.pgo_debug_partition(self._h, int(size), None, None, 0))
        cap = max(ns, 2 * size + 4)
        owner = np.zeros(cap, np.int32)
        out = np.zeros(cap)
        self._check(self._L.pgo_debug_partition(self._h, int(size), owner.ctypes.data_as(C.POINTER(C.c_int)),
                                                L.dptr(out), cap))
        return owner[:ns], out

    def debug_partition_bound(self, size):
        """Host-only: the partitioned factorisation's per-rank flops with the
        distributed top (top fronts' columns dealt to the ranks), the work every
        rank repeats, and the plan-derived flop bound on the speed-up
        (factorisation flops / the busiest rank's)."""
        _, out = self._partition(size)
        total = self.debug_plan()["factor_flops"]
        rank = out[size + 1:2 * size + 1].copy()
        return {"ranks": int(size), "rank_flops": rank, "replicated_flops": float(out[2 * size + 1]),
                "replicated_top_flops": float(out[size]), "total_flops": float(total),
                "bound": float(total / rank.max()),
                "bound_replicated_top": float(total / (out[size] + out[:size].max())),
                "exchange_points": int(out[2 * size + 2]), "exchange_bytes": float(8.0 * out[2 * size + 3])}

    def debug_ordering(self):
        """Host-only: the Cholesky solver's pose ordering (new -> insertion index)."""
        n = self.num_vertices
        perm = np.zeros(n, np.int32)
        self._check(self._L.pgo_debug_ordering(self._h, perm.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return perm

    # ---------------------------------------------------------------- values
    @property
    def num_vertices(self):
        return int(self._L.pgo_num_vertices(self._h))

    @property
    def num_factors(self):
        return int(self._L.pgo_num_factors(self._h))

    def pose(self, key):
        out = np.zeros(3)
        self._check(self._L.pgo_get_pose(self._h, int(key), L.dptr(out)))
        return out

    def poses(self, keys=None):
        if keys is None:
            n = self.num_vertices
            out = np.zeros((n, 3))
            self._check(self._L.pgo_get_poses(self._h, n, None, L.dptr(out)))
            return out
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros((len(keys), 3))
        self._check(self._L.pgo_get_poses(self._h, len(keys), L.u64ptr(keys), L.dptr(out)))
        return out

    def marginal_covariances(self, keys):
        """3x3 covariances (x, y, theta) of the poses at the current values:
        gtsam::Marginals(graph, values).marginalCovariance(key) (graph.cpp:120,126-127)."""
        keys = np.ascontiguousarray(np.atleast_1d(keys), dtype=np.uint64)
        out = np.zeros((len(keys), 3, 3))
        self._check(self._L.pgo_marginal_covariances(self._h, len(keys), L.u64ptr(keys), L.dptr(out)))
        return out

    def marginal_covariances_all(self, edges=False):
        """Every pose's 3x3 covariance in one selected-inversion pass, (n, 3, 3) in
        insertion order: gtsam::Marginals once, then marginalCovariance(key) over
        all keyframes (graph.cpp:120,126-127).  With edges=True also (E, 3, 3):
        per between factor the block of H^-1 with k1's rows and k2's columns, so
        [[cov[k1], X], [X.T, cov[k2]]] is the factor's joint marginal."""
        n = self.num_vertices
        cov = np.zeros((n, 3, 3))
        if not edges:
            self._check(self._L.pgo_marginal_covariances_all(self._h, L.dptr(cov) if n else None, None))
            return cov
        cross = np.zeros((self.num_factors - self._priors, 3, 3))   # (the between factors)
        self._check(self._L.pgo_marginal_covariances_all(self._h, L.dptr(cov) if n else None, L.dptr(cross)))
        return cov, cross

    def set_poses(self, xyt, keys=None):
        xyt = np.ascontiguousarray(xyt, dtype=np.float64).reshape(-1, 3)
        kp = None
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
            kp = L.u64ptr(keys)
        self._check(self._L.pgo_set_poses(self._h, xyt.shape[0], kp, L.dptr(xyt)))

    def save_values(self):
        self._check(self._L.pgo_save_values(self._h))

    def restore_values(self):
        self._check(self._L.pgo_restore_values(self._h))

    def error(self):
        e = C.c_double(0)
        self._check(self._L.pgo_error(self._h, C.byref(e)))
        return e.value

    # ------------------------------------------------------------ diagnostics
    # ------------------------------------------------- loop-closure search
    def closest_keyframe(self, x, y, skip=KEYFRAMES_TO_SKIP_IN_LOOP_CLOSING):
        """closest_keyframe service (graph.cpp:146-178): (key, distance) of the
        vertex nearest to (x, y) among all but the last `skip` inserted."""
        key, dist = C.c_uint64(), C.c_double()
        self._check(self._L.pgo_closest_keyframe(self._h, float(x), float(y), int(skip), C.byref(key),
                                                 C.byref(dist)))
        return key.value, dist.value

    def closest_keyframes(self, query_keys, skip=KEYFRAMES_TO_SKIP_IN_LOOP_CLOSING):
        """Batched service: for each query key, the answer when it was the last
        keyframe (candidates inserted before it, minus skip - 1).  Keys with no
        candidate get PGO_NO_KEY and +inf."""
        q = np.ascontiguousarray(query_keys, dtype=np.uint64)
        keys = np.zeros(len(q), np.uint64)
        dist = np.zeros(len(q))
        self._check(self._L.pgo_closest_keyframes(self._h, len(q), L.u64ptr(q), int(skip), L.u64ptr(keys),
                                                  L.dptr(dist)))
        return keys, dist

    def debug_search_ms(self):
        a, b = C.c_double(), C.c_double()
        self._check(self._L.pgo_debug_search_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ------------------------------------------------- multi-GPU (pgo_comm_*)
    def comm_init_rccl(self, unique_id: bytes, rank: int, size: int):
        """ncclCommInitRank on this handle's device (collective over all ranks)."""
        buf = C.create_string_buffer(bytes(unique_id), len(unique_id))
        self._check(self._L.pgo_comm_init_rccl(self._h, buf, len(unique_id), rank, size))

    def comm_init_host(self, comm: L.PgoHostComm):
        """The caller's own host transport (callbacks must outlive the handle's use)."""
        self._comm_keepalive = comm
        self._check(self._L.pgo_comm_init_host(self._h, C.byref(comm)))

    def comm_init_rccl_part(self, unique_id: bytes, rank: int, size: int):
        """The hybrid mode's partition-group communicator over RCCL (collective over the group)."""
        buf = C.create_string_buffer(bytes(unique_id), len(unique_id))
        self._check(self._L.pgo_comm_init_rccl_part(self._h, buf, len(unique_id), rank, size))

    def comm_init_host_part(self, comm: L.PgoHostComm):
        """The hybrid mode's partition-group communicator over the caller's host transport."""
        self._pcomm_keepalive = comm
        self._check(self._L.pgo_comm_init_host_part(self._h, C.byref(comm)))

    def comm_part_rank(self):
        r, n = C.c_int(), C.c_int()
        self._check(self._L.pgo_comm_part_rank(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_free(self):
        self._check(self._L.pgo_comm_free(self._h))

    def comm_rank(self):
        r, n = C.c_int(), C.c_int()
        self._check(self._L.pgo_comm_rank(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_selftest(self):
        self._check(self._L.pgo_comm_selftest(self._h))

    def debug_linearize(self, num_edges, cholesky=False):
        """H diagonal / off-diagonal blocks, gradient and error at the current
        values; cholesky=True takes the Cholesky-mode sweep (owner blocks in
        factor order) instead of the two-slot block-CSR sweep."""
        n = self.num_vertices
        hd = np.zeros((n, 3, 3))
        ho = np.zeros((num_edges, 3, 3))
        g = np.zeros((n, 3))
        e = C.c_double(0)
        fn = self._L.pgo_debug_linearize_cholesky if cholesky else self._L.pgo_debug_linearize
        self._check(fn(self._h, L.dptr(hd), L.dptr(ho), L.dptr(g), C.byref(e)))
        return hd, ho, g, e.value

    def debug_poison_fronts(self):
        """NaN into the Cholesky workspace's written-before-read elements (tests)."""
        self._check(self._L.pgo_debug_poison_fronts(self._h))

    def debug_factor_time(self, lanes=1, reps=10):
        """Device ms of one replay of the captured factorisation graph with
        `lanes` lambda lanes (diagnostics; PGO_ABLATE applies)."""
        ms = C.c_double(0)
        self._check(self._L.pgo_debug_factor_time(self._h, int(lanes), int(reps), C.byref(ms)))
        return ms.value

    def debug_spmv(self, x, lam=0.0):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
        y = np.zeros_like(x)
        self._check(self._L.pgo_debug_spmv(self._h, float(lam), L.dptr(x), L.dptr(y)))
        return y

    def debug_plan(self, cap=4096):
        """Host-only symbolic analysis summary of the supernodal Cholesky plan."""
        out = np.zeros(cap)
        self._check(self._L.pgo_debug_plan(self._h, L.dptr(out), cap))
        keys = ["supernodes", "levels", "nnz_l", "factor_flops", "syrk_flops", "front_doubles",
                "launches_factor", "launches_solve", "max_front", "trsm_tasks", "syrk_tiles", "small_fronts",
                "fused_tiles", "fused_with_children", "fused_multipass", "fused_edge"]
        summary = {k: out[i] for i, k in enumerate(keys)}
        nl = int(out[1])
        lv = out[16:16 + 6 * nl].reshape(-1, 6)
        summary["levels_table"] = lv
        return summary

    def debug_plan_digest(self, part_size=1, part_rank=0):
        """Host-only: the digest of the Cholesky plan for rank `part_rank` of
        `part_size`: (one 64-bit hash per section of the plan -- two plans are
        the same exactly when all agree --, the counters of the scheduler's
        branches the plan took)."""
        out = np.zeros(64, np.uint64)
        ns = self._check(self._L.pgo_debug_plan_digest(self._h, int(part_size), int(part_rank), L.u64ptr(out), 64))
        return [int(v) for v in out[:ns]], [int(v) for v in out[ns:ns + 20]]

    def debug_selinv_plan(self, cap=4096):
        """Host-only summary of marginal_covariances_all's pass: launches,
        algorithmic flops, doubles of extra device workspace, levels, and the
        launches of each level (leaves first)."""
        out = np.zeros(cap)
        self._check(self._L.pgo_debug_selinv_plan(self._h, L.dptr(out), cap))
        nl = int(out[3])
        return {"launches": int(out[0]), "flops": float(out[1]), "workspace_doubles": float(out[2]), "levels": nl,
                "level_launches": out[4:4 + nl].astype(np.int64)}

    def debug_fronts(self):
        """Host-only: (w, m, level) of every supernode of the Cholesky plan."""
        ns = self._L.pgo_debug_fronts(self._h, None, None, None, 0)
        if ns < 0:
            self._check(ns)
        w = np.zeros(ns, np.int32)
        m = np.zeros(ns, np.int32)
        lv = np.zeros(ns, np.int32)
        ip = C.POINTER(C.c_int)
        self._check(min(0, self._L.pgo_debug_fronts(self._h, w.ctypes.data_as(ip), m.ctypes.data_as(ip),
                                                     lv.ctypes.data_as(ip), ns)))
        return w, m, lv

    def debug_row_lanes(self):
        """Host-only: (G, G1), the sub-group widths of the row kernels
        (k_linearize / k_pcg_spmv / k_spmv / k_model_decrease; k_linearize_side1)."""
        G, G1 = C.c_int(0), C.c_int(0)
        self._check(self._L.pgo_debug_row_lanes(self._h, C.byref(G), C.byref(G1)))
        return G.value, G1.value

    def debug_parents(self):
        """Host-only: the parent supernode of every supernode (-1: a root)."""
        ns = self._L.pgo_debug_fronts(self._h, None, None, None, 0)
        if ns < 0:
            self._check(ns)
        par = np.zeros(ns, np.int32)
        self._check(min(0, self._L.pgo_debug_parents(self._h, par.ctypes.data_as(C.POINTER(C.c_int)), ns)))
        return par

    def debug_solve(self, lam, params=None, **kw):
        p = params if params is not None else default_params(**kw)
        d = np.zeros((self.num_vertices, 3))
        it = C.c_int(0)
        self._check(self._L.pgo_debug_solve(self._h, float(lam), C.byref(p), L.dptr(d), C.byref(it)))
        return d, it.value
