"""numpy twin of the robust-loss path (test infrastructure only).

Restates, on top of ``oracle.pgo_numpy`` (residuals, linearize, linear_error,
solve, retract, check_convergence), what libpgo.so computes for between factors
with an m-estimator (include/pgo.h PGO_LOSS_*, GTSAM >= 4.1
``noiseModel::Robust``): with ``r = sqrt(e' Omega e)``

    loss            rho(r)                              w(r) = rho'(r) / r
    NONE (0)        r^2 / 2                             1
    HUBER (1)       r^2 / 2 (r <= k), k (r - k / 2)     1 (r <= k), k / r
    CAUCHY (2)      (k^2 / 2) log1p(r^2 / k^2)          1 / (1 + r^2 / k^2)
    GEMAN_MCCLURE   (k^2 / 2) r^2 / (k^2 + r^2)         k^4 / (k^2 + r^2)^2

error = sum rho(r) + the priors' 0.5 e' Omega e; the linearisation is the
Gaussian one with every factor's Omega scaled by w(r) at the linearisation
point (``Robust::WhitenSystem``), applied here by scaling ``Problem.eom``; LM's
model decrease and its guard ``lin_change > eps * old linear error`` use that
weighted system, the cost change uses the robust error.  Like the rest of the
project's twins it is parity-unpinned against GTSAM itself.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from oracle import pgo_numpy as pn

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3


def weight(loss, k, r2):
    loss, k, r2 = np.broadcast_arrays(np.asarray(loss), np.asarray(k, dtype=np.float64), np.asarray(r2, np.float64))
    r = np.sqrt(r2)
    w = np.ones_like(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        hub = np.where(r <= k, 1.0, k / r)
    w = np.where(loss == HUBER, hub, w)
    w = np.where(loss == CAUCHY, 1.0 / (1.0 + r2 / (k * k)), w)
    w = np.where(loss == GEMAN_MCCLURE, (1.0 / (1.0 + r2 / (k * k))) ** 2, w)
    return w


def rho(loss, k, r2):
    loss, k, r2 = np.broadcast_arrays(np.asarray(loss), np.asarray(k, dtype=np.float64), np.asarray(r2, np.float64))
    r = np.sqrt(r2)
    out = 0.5 * r2
    out = np.where(loss == HUBER, np.where(r <= k, 0.5 * r2, k * (r - 0.5 * k)), out)
    out = np.where(loss == CAUCHY, 0.5 * k * k * np.log1p(r2 / (k * k)), out)
    out = np.where(loss == GEMAN_MCCLURE, 0.5 * r2 / (1.0 + r2 / (k * k)), out)
    return out


@dataclasses.dataclass
class RobustProblem:
    prob: pn.Problem
    loss: np.ndarray     # int [E]
    k: np.ndarray        # f64 [E]


def problem(g, loss=None, k=None):
    """RobustProblem of a datasets.PoseGraph; loss / k default to its edge_loss /
    edge_loss_k fields (None: all Gaussian), scalars broadcast."""
    prob = pn.problem_from_graph(g)
    E = len(prob.ei)
    loss = getattr(g, "edge_loss", None) if loss is None else loss
    k = getattr(g, "edge_loss_k", None) if k is None else k
    loss = np.broadcast_to(np.asarray(0 if loss is None else loss, dtype=np.int64), (E,)).copy()
    k = np.broadcast_to(np.asarray(1.0 if k is None else k, dtype=np.float64), (E,)).copy()
    return RobustProblem(prob, loss, k)


def r_squared(rp, poses):
    ee, ep, *_ = pn.residuals(rp.prob, poses)
    return np.einsum("ei,eij,ej->e", ee, rp.prob.eom, ee), ee, ep


def weights(rp, poses):
    r2, _, _ = r_squared(rp, poses)
    return weight(rp.loss, rp.k, r2)


def error(rp, poses):
    r2, _, ep = r_squared(rp, poses)
    return float(rho(rp.loss, rp.k, r2).sum() + 0.5 * np.einsum("ei,eij,ej->", ep, rp.prob.pom, ep))


def weighted_problem(rp, poses):
    """The Gaussian problem whose linearisation at `poses` is the robust one."""
    w = weights(rp, poses)
    return dataclasses.replace(rp.prob, eom=rp.prob.eom * w[:, None, None])


def linearize(rp, poses):
    wp = weighted_problem(rp, poses)
    return wp, pn.linearize(wp, poses)


def blocks(rp, poses):
    """(H diagonal blocks [N,3,3], off-diagonal blocks H_{k1,k2} = w J1' Omega
    [E,3,3], gradient [N,3]) in the layout of PoseGraph.debug_linearize."""
    wp, lin = linearize(rp, poses)
    B = np.einsum("eki,ekl->eil", lin.J1, wp.eom)
    D1 = np.einsum("eil,elj->eij", B, lin.J1)
    hd = np.zeros((wp.n, 3, 3))
    np.add.at(hd, wp.ei, D1)
    np.add.at(hd, wp.ej, wp.eom)
    np.add.at(hd, wp.pi, wp.pom)
    return hd, B, lin.g.reshape(-1, 3)


def marginal_covariances(rp, poses, idx):
    return pn.marginal_covariances(weighted_problem(rp, poses), poses, idx)


def levenberg_marquardt(rp, poses0, params=None):
    """pgo_numpy.levenberg_marquardt with the robust error and the weighted
    linearisation.  Besides the Result it returns the smallest relative distance
    of a decision quantity from its threshold over the whole trajectory
    (fidelity vs min_model_fidelity, |cost change| vs relative_error_tol * error,
    checkConvergence's relative and absolute decrease vs their tolerances)."""
    p = params or pn.LMParams()
    poses = np.array(poses0, dtype=np.float64, copy=True)
    err = error(rp, poses)
    lam, factor = p.lambda_initial, p.lambda_factor
    iters = inner = 0
    trace = []
    margin = math.inf

    def away(q, thr):
        nonlocal margin
        if thr != 0 and math.isfinite(q):
            margin = min(margin, abs(q - thr) / abs(thr))

    err0 = err
    if err <= p.error_tol or iters >= p.max_iterations:
        return pn.Result(poses, err, err0, 0, 0, trace), margin
    new_err = err
    outer = 0
    while True:
        cur_err = new_err
        wp, lin = linearize(rp, poses)
        outer += 1
        while True:
            fidelity = 0.0
            success = stop = False
            new_e = math.inf
            lin_change = math.nan
            try:
                delta = pn.solve(lin.H, -lin.g, lam)
                solved = True
            except pn.Indeterminant:
                solved = False
            if solved:
                old_lin = pn.linear_error(wp, lin, np.zeros_like(delta))   # sum 0.5 w r^2 (+ priors)
                lin_change = old_lin - pn.linear_error(wp, lin, delta)
                if lin_change >= 0:
                    cand = pn.retract(poses, delta.reshape(-1, 3))
                    new_e = error(rp, cand)
                    cost_change = err - new_e
                    if lin_change > np.finfo(float).eps * old_lin:
                        fidelity = cost_change / lin_change
                        success = fidelity > p.min_model_fidelity
                        away(fidelity, p.min_model_fidelity)
                    if abs(cost_change) < p.relative_error_tol * err:
                        stop = True
                    away(abs(cost_change), p.relative_error_tol * err)
            trace.append(dict(iteration=iters, lam=lam, solved=solved, lin_change=lin_change, new_error=new_e,
                              fidelity=fidelity, accepted=success))
            if success:
                if p.use_fixed_lambda_factor:
                    lam /= p.lambda_factor
                else:
                    lam *= max(1.0 / 3.0, 1.0 - (2.0 * fidelity - 1.0) ** 3)
                    factor *= 2.0
                lam = max(p.lambda_lower_bound, lam)
                poses, err = cand, new_e
                iters += 1
                inner += 1
                break
            if not stop:
                lam *= factor
                inner += 1
                if not p.use_fixed_lambda_factor:
                    factor *= 2.0
                if lam >= p.lambda_upper_bound:
                    break
                continue
            break
        new_err = err
        if p.max_outer > 0 and outer >= p.max_outer:
            break
        if cur_err > 0:
            away((cur_err - new_err) / cur_err, p.relative_error_tol)
        away(cur_err - new_err, p.absolute_error_tol)
        if not (iters < p.max_iterations and not pn.check_convergence(p, cur_err, new_err)
                and math.isfinite(cur_err)):
            break
    return pn.Result(poses, err, err0, iters, inner, trace), margin


def trace_array(trace):
    """The twin's trace in pgo_get_trace's first seven columns."""
    return np.array([[t["iteration"], t["lam"], float(t["solved"]), t["lin_change"], t["new_error"], t["fidelity"],
                      float(t["accepted"])] for t in trace], dtype=np.float64).reshape(-1, 7)


# ---------------------------------------------------------------- shared inputs
def outlier_graph(seed=2001):
    """The issue's graph: manhattan(1000, 16, 1500) with 10 % of its 501 loop
    closures replaced by random poses; returns (graph, replaced indices, loop
    closure indices)."""
    from graphslam_amd import datasets
    g = datasets.manhattan(1000, 16, 1500, seed=seed)
    bad = datasets.corrupt_loop_closures(g, 0.1, seed + 7)
    return g, bad, datasets.loop_closure_indices(g)


def with_loss_on(g, idx, loss, k):
    """g with `loss`(k) on the factors idx (edge_loss / edge_loss_k set)."""
    el = np.zeros(g.num_edges, dtype=np.int32)
    ek = np.ones(g.num_edges)
    el[idx] = loss
    ek[idx] = k
    g.edge_loss, g.edge_loss_k = el, ek
    return g


def star_graph(seed=3):
    """601 poses; the hub (pose 0, with the prior) is k1 of 300 edges (one row
    with more side-0 factors than a block has threads) and k2 of 300 others (a
    side-1 list much longer than a sub-group); random losses, a random
    non-diagonal covariance per edge."""
    from graphslam_amd import datasets
    rng = np.random.default_rng(seed)
    n = 601
    gt = np.zeros((n, 3))
    gt[1:, 0] = rng.uniform(-10, 10, n - 1)
    gt[1:, 1] = rng.uniform(-10, 10, n - 1)
    gt[1:, 2] = rng.uniform(-np.pi, np.pi, n - 1)
    i = np.concatenate([np.zeros(300, np.int64), np.arange(301, 601)])
    j = np.concatenate([np.arange(1, 301), np.zeros(300, np.int64)])
    z = datasets.compose_xyt(datasets.between_xyt(gt[i], gt[j]), rng.normal(size=(600, 3)) * [0.3, 0.3, 0.1])
    init = gt + rng.normal(size=(n, 3)) * [0.2, 0.2, 0.05]
    init[0] = 0.0
    Lc = np.tril(rng.normal(size=(600, 3, 3)) * 0.02) + np.eye(3) * 0.05
    cov = (Lc @ np.transpose(Lc, (0, 2, 1))).reshape(-1, 9)
    g = datasets.PoseGraph(
        name="star", keys=np.arange(1, n + 1, dtype=np.uint64), initial=init, ground_truth=gt,
        edge_k1=(i + 1).astype(np.uint64), edge_k2=(j + 1).astype(np.uint64), edge_z=z, edge_cov=cov,
        prior_keys=np.array([1], dtype=np.uint64), prior_pose=np.zeros((1, 3)),
        prior_cov=np.diag([0.01, 0.01, 0.01]).reshape(1, 9).astype(np.float64))
    g.edge_loss = rng.integers(0, 4, 600).astype(np.int32)
    g.edge_loss_k = rng.uniform(0.5, 3.0, 600)
    return g
