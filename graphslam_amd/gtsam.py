"""GTSAM-named mirror of the surface /root/reference/src/graph/src/graph.cpp uses.

So a caller of the reference's path can switch with the same names, argument
meaning and error behaviour:

    graph.cpp:45   noiseModel::Gaussian::Covariance(Q)   -> noiseModel.Gaussian.Covariance(Q)
    graph.cpp:57   graph.add(PriorFactor<Pose2>(k, p, n))  -> graph.add(PriorFactorPose2(k, p, n))
    graph.cpp:58   initial.insert(k, Pose2(x, y, th))     -> initial.insert(k, Pose2(x, y, th))
    graph.cpp:87   graph.add(BetweenFactor<Pose2>(...))   -> graph.add(BetweenFactorPose2(...))
    graph.cpp:119  LevenbergMarquardtOptimizer(graph, initial).optimize()
                                                          -> same
    graph.cpp:123  poses_opti.at<Pose2>(k).x()            -> poses_opti.atPose2(k).x()
    graph.cpp:60   graph.nrFactors()                      -> graph.nrFactors()

The optimisation itself runs in libpgo.so on the GPU (no CPU fallback).
"""
from __future__ import annotations

import math

import numpy as np

from .pose_graph import (BadCovariance, IndeterminantLinearSystemException, PgoError, PoseGraph,  # noqa: F401
                         ValuesKeyAlreadyExists, ValuesKeyDoesNotExist, default_params)


class Pose2:
    """gtsam::Pose2 (x, y, theta); theta reported in (-pi, pi] like Rot2::theta()."""

    __slots__ = ("_x", "_y", "_t")

    def __init__(self, x=0.0, y=0.0, theta=0.0):
        self._x, self._y, self._t = float(x), float(y), float(theta)

    def x(self):
        return self._x

    def y(self):
        return self._y

    def theta(self):
        return math.atan2(math.sin(self._t), math.cos(self._t))

    def vector(self):
        return np.array([self._x, self._y, self.theta()])

    def __repr__(self):
        return f"Pose2({self._x!r}, {self._y!r}, {self.theta()!r})"


class _Gaussian:
    def __init__(self, cov):
        self.covariance = np.array(cov, dtype=np.float64).reshape(3, 3)

    @staticmethod
    def Covariance(Q):
        return _Gaussian(Q)

    @staticmethod
    def Information(I):
        return _Gaussian(np.linalg.inv(np.asarray(I, dtype=np.float64)))


class _Diagonal:
    @staticmethod
    def Sigmas(s):
        s = np.asarray(s, dtype=np.float64)
        return _Gaussian(np.diag(s * s))

    @staticmethod
    def Variances(v):
        return _Gaussian(np.diag(np.asarray(v, dtype=np.float64)))


class _MEstimatorBase:
    """gtsam::noiseModel::mEstimator::Base: a loss kind (PGO_LOSS_*) and its k."""

    loss = 0

    def __init__(self, k):
        k = float(k)
        if not (math.isfinite(k) and k > 0.0):
            raise ValueError("mEstimator parameter k must be finite and positive")
        self.k = k

    @classmethod
    def Create(cls, k):
        return cls(k)


class _Huber(_MEstimatorBase):
    loss = 1


class _Cauchy(_MEstimatorBase):
    loss = 2


class _GemanMcClure(_MEstimatorBase):
    loss = 3


class _mEstimator:
    Huber = _Huber
    Cauchy = _Cauchy
    GemanMcClure = _GemanMcClure


class _Robust:
    """gtsam::noiseModel::Robust: an mEstimator over a Gaussian model."""

    def __init__(self, estimator, gaussian):
        if not isinstance(estimator, _MEstimatorBase):
            raise TypeError("Robust.Create needs an mEstimator (Huber / Cauchy / GemanMcClure)")
        if not isinstance(gaussian, _Gaussian):
            raise TypeError("Robust.Create needs a Gaussian noise model")
        self.robust, self.noise = estimator, gaussian
        self.covariance = gaussian.covariance

    @staticmethod
    def Create(estimator, gaussian):
        return _Robust(estimator, gaussian)


class noiseModel:  # noqa: N801 -- mirrors gtsam::noiseModel
    Gaussian = _Gaussian
    Diagonal = _Diagonal
    mEstimator = _mEstimator
    Robust = _Robust


class PriorFactorPose2:
    def __init__(self, key, prior: Pose2, noise: _Gaussian):
        if isinstance(noise, _Robust):
            raise TypeError("PriorFactorPose2 takes a Gaussian noise model: robust losses are supported on "
                            "BetweenFactorPose2 only")
        self.key, self.prior, self.noise = int(key), prior, noise

    def keys(self):
        return [self.key]


class BetweenFactorPose2:
    def __init__(self, key1, key2, measured: Pose2, noise: _Gaussian):
        self.key1, self.key2, self.measured, self.noise = int(key1), int(key2), measured, noise

    def keys(self):
        return [self.key1, self.key2]


class NonlinearFactorGraph:
    def __init__(self):
        self.factors = []

    def add(self, factor):
        if not isinstance(factor, (PriorFactorPose2, BetweenFactorPose2)):
            raise TypeError("only PriorFactorPose2 / BetweenFactorPose2 are on this path")
        self.factors.append(factor)

    push_back = add

    def size(self):
        return len(self.factors)

    def nrFactors(self):
        return len(self.factors)

    def error(self, values: "Values") -> float:
        """0.5 * sum e' Omega e (rho(r) for a factor with a robust model), computed on the device."""
        with _build(self, values) as pg:
            return pg.error()


class Values:
    def __init__(self):
        self._keys = []
        self._xyt = {}

    def insert(self, key, pose: Pose2):
        key = int(key)
        if key in self._xyt:
            raise ValuesKeyAlreadyExists(-2, f"key {key} already inserted")
        self._keys.append(key)
        self._xyt[key] = (pose.x(), pose.y(), pose._t)

    def update(self, key, pose: Pose2):
        key = int(key)
        if key not in self._xyt:
            raise ValuesKeyDoesNotExist(-3, f"key {key} has no value")
        self._xyt[key] = (pose.x(), pose.y(), pose._t)

    def exists(self, key):
        return int(key) in self._xyt

    def atPose2(self, key) -> Pose2:
        key = int(key)
        if key not in self._xyt:
            raise ValuesKeyDoesNotExist(-3, f"key {key} has no value")
        return Pose2(*self._xyt[key])

    at = atPose2

    def size(self):
        return len(self._keys)

    def keys(self):
        return list(self._keys)

    def as_array(self):
        return np.array([self._xyt[k] for k in self._keys], dtype=np.float64).reshape(-1, 3)


class _Handle:
    def __init__(self, pg):
        self.pg = pg

    def __enter__(self):
        return self.pg

    def __exit__(self, *a):
        self.pg.close()


def _build(graph: NonlinearFactorGraph, values: Values, device=0):
    pg = PoseGraph(device)
    keys = values.keys()
    if keys:
        pg.add_vertices(np.array(keys, dtype=np.uint64), values.as_array())
    for f in graph.factors:
        if isinstance(f, PriorFactorPose2):
            pg.add_prior(f.key, [f.prior.x(), f.prior.y(), f.prior._t], f.noise.covariance)
        else:
            est = f.noise.robust if isinstance(f.noise, _Robust) else None
            pg.add_edge(f.key1, f.key2, [f.measured.x(), f.measured.y(), f.measured._t], f.noise.covariance,
                        loss=est.loss if est else None, k=est.k if est else None)
    return _Handle(pg)


class Marginals:
    """``gtsam::Marginals(graph, values)`` (graph.cpp:120, commented in the reference):
    ``marginalCovariance(key)`` -> 3x3 numpy array (x, y, theta)."""

    def __init__(self, graph: NonlinearFactorGraph, values: Values, device=0):
        self.graph, self.values, self.device = graph, values, device

    def marginalCovariance(self, key):
        return self.marginalCovariances([key])[0]

    def marginalCovariances(self, keys=None):
        """The given keys' covariances; with ``keys=None`` every key's, in the
        Values' order, from one selected-inversion pass (the loop over all
        keyframes of graph.cpp:121-131 as one call)."""
        with _build(self.graph, self.values, self.device) as pg:
            if keys is None:
                return pg.marginal_covariances_all()
            return pg.marginal_covariances(keys)


class lago:  # noqa: N801 -- mirrors gtsam::lago
    """``gtsam::lago::initialize(graph, values)``: linear initial values for LM."""

    @staticmethod
    def initialize(graph: NonlinearFactorGraph, values: "Values", device=0) -> "Values":
        """Two linear solves on the device (``PoseGraph.initialize_linear``):
        orientations, then positions with the orientations held.  ``values``
        only names the keys, as in GTSAM's two-argument form; its poses are
        not used.  Returns new Values in the same key order.

        Deviations from GTSAM's ``lago``: the spanning tree is breadth-first
        from each component's first vertex with a prior (GTSAM: the odometric
        path, or a minimum spanning tree); stage 2 applies no orientation
        correction; the graph's priors are used as given (GTSAM adds an
        anchor), so every connected component needs one
        (IndeterminantLinearSystemException otherwise).  Robust noise models
        are treated as their Gaussian part.  Parity with GTSAM is unpinned."""
        with _build(graph, values, device) as pg:
            pg.initialize_linear()
            xyt = pg.poses()
        out = Values()
        for k, p in zip(values.keys(), xyt):
            out.insert(k, Pose2(*p))
        return out


class LevenbergMarquardtParams:
    """gtsam::LevenbergMarquardtParams with GTSAM 4.0 defaults (+ PCG knobs)."""

    def __init__(self):
        self._p = default_params()

    def setMaxIterations(self, v):
        self._p.max_iterations = int(v)

    def setRelativeErrorTol(self, v):
        self._p.relative_error_tol = float(v)

    def setAbsoluteErrorTol(self, v):
        self._p.absolute_error_tol = float(v)

    def setErrorTol(self, v):
        self._p.error_tol = float(v)

    def setlambdaInitial(self, v):
        self._p.lambda_initial = float(v)

    def setlambdaFactor(self, v):
        self._p.lambda_factor = float(v)

    def setlambdaUpperBound(self, v):
        self._p.lambda_upper_bound = float(v)

    def setlambdaLowerBound(self, v):
        self._p.lambda_lower_bound = float(v)

    def setUseFixedLambdaFactor(self, v):
        self._p.use_fixed_lambda_factor = int(bool(v))

    def setPcgRelativeTol(self, v):
        self._p.pcg_relative_tol = float(v)

    @property
    def raw(self):
        return self._p


class GaussNewtonParams(LevenbergMarquardtParams):
    def __init__(self):
        super().__init__()
        self._p.algorithm = 1


class LevenbergMarquardtOptimizer:
    """``LevenbergMarquardtOptimizer(graph, initial[, params]).optimize()`` (graph.cpp:119)."""

    _params_cls = LevenbergMarquardtParams

    def __init__(self, graph: NonlinearFactorGraph, initial: Values, params=None, device=0):
        self.graph, self.initial = graph, initial
        self.params = params if params is not None else self._params_cls()
        self.device = device
        self.stats = None
        self._handle = None

    def optimize(self) -> Values:
        """GTSAM keeps the optimizer's state: the graph is loaded on the first
        call, a later call continues from the values the previous one reached."""
        if self._handle is None:
            self._handle = _build(self.graph, self.initial, self.device)
        pg = self._handle.pg
        self.stats = pg.optimize(self.params.raw)
        xyt = pg.poses()
        out = Values()
        for k, p in zip(self.initial.keys(), xyt):
            out.insert(k, Pose2(*p))
        return out

    def iterations(self):
        return self.stats["iterations"] if self.stats else 0

    def error(self):
        return self.stats["final_error"] if self.stats else None


class GaussNewtonOptimizer(LevenbergMarquardtOptimizer):
    _params_cls = GaussNewtonParams


class GncLossType:
    """gtsam::GncLossType."""
    GM = 0
    TLS = 1


class GncLMParams:
    """``gtsam::GncLMParams``: the outer loop's knobs over LM inner solves
    (pgo_gnc_params; defaults as pgo_gnc_default_params).  Known inliers are
    indices into the factor graph, as in GTSAM; the candidates of
    pgo_optimize_gnc are the between factors that are not among them."""

    def __init__(self, lm_params: LevenbergMarquardtParams | None = None):
        from .pose_graph import default_gnc_params
        self.lm = lm_params if lm_params is not None else LevenbergMarquardtParams()
        self._g = default_gnc_params()
        self.known_inliers = []

    def setLossType(self, v):
        self._g.loss = int(v)

    def setKnownInliers(self, idx):
        self.known_inliers = sorted(int(i) for i in idx)

    def setMuStep(self, v):
        self._g.mu_step = float(v)

    def setMaxIterations(self, v):
        self._g.max_iterations = int(v)

    def setRelativeCostTol(self, v):
        self._g.relative_cost_tol = float(v)

    def setWeightsTol(self, v):
        self._g.weights_tol = float(v)

    def setInlierCostThreshold(self, barc_sq):
        """One threshold on r^2 = e' Omega e for every candidate (GTSAM: per
        factor, on the factor error)."""
        self._g.barc_sq = float(barc_sq)

    @property
    def raw(self):
        return self._g


class GncLMOptimizer:
    """``GncOptimizer<GncLMParams>(graph, initial, params).optimize()`` /
    ``.getWeights()`` on pgo_optimize_gnc.  Not GncOptimizer to the letter:
    every inner solve starts from the previous result (GTSAM 4.1 restarts from
    the initial values) and the inlier threshold is one number on r^2; priors
    are never candidates.  Parity with GTSAM is unpinned."""

    def __init__(self, graph: NonlinearFactorGraph, initial: Values, params: GncLMParams | None = None, device=0):
        self.graph, self.initial = graph, initial
        self.params = params if params is not None else GncLMParams()
        self.device = device
        self.stats = None
        self._weights = np.ones(graph.nrFactors())
        for f in graph.factors:
            if isinstance(f, BetweenFactorPose2) and isinstance(f.noise, _Robust):
                raise ValueError("GncLMOptimizer: the graph's factors must have Gaussian noise models")

    def optimize(self) -> Values:
        between = [i for i, f in enumerate(self.graph.factors) if isinstance(f, BetweenFactorPose2)]
        known = set(self.params.known_inliers)
        cand = [e for e, i in enumerate(between) if i not in known]
        with _build(self.graph, self.initial, self.device) as pg:
            self.stats = pg.optimize_gnc(candidates=cand, params=self.params.lm.raw, gnc=self.params.raw)
            xyt = pg.poses()
            w = pg.edge_weights() if between else np.zeros(0)
        self._weights = np.ones(self.graph.nrFactors())
        self._weights[between] = w
        out = Values()
        for k, p in zip(self.initial.keys(), xyt):
            out.insert(k, Pose2(*p))
        return out

    def getWeights(self):
        """One weight per factor of the graph (priors and known inliers: 1)."""
        return self._weights.copy()
