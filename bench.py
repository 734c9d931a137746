"""Benchmark: GN iterations/s + ms-to-chi^2 convergence on the 100k-pose Manhattan graph.

A step = one complete pgo_optimize() (GTSAM-default Levenberg-Marquardt) of the
C3 graph (100k poses / 500k between factors, BASELINE.json configs[2]) from its
dead-reckoned initial values; the values are restored on the device (no PCIe)
before every step, the graph stays resident in HBM.  pgo_optimize returns only
after its HIP stream has drained (it reads the final error back), so the host
clock brackets all device work.

value = linearisations ("GN iterations": linearise + solve(s) + retract + chi^2)
of the job (replicas: summed over ranks) / max-over-ranks wall time of the K
timed steps.

Multi-GPU (--gpus N, one process per GPU via torch.distributed.run), DESIGN.md
§5: --multi auto (default) picks, by the plan-derived cost model of
graphslam_amd/multi_model.py, between the speculative lambda search (every rank
holds the graph, the ranks solve consecutive lambda tries of GTSAM's sequence at
once and exchange the outcomes and the accepted values over RCCL / xGMI) and the
partitioned factorisation (subtrees per rank, the top fronts' columns dealt to
the ranks).  Either is one job, bitwise the one-GPU trajectory -> value = that
job's linearisations / wall time, "strong" scaling.  --multi replicas runs N
independent copies instead ("weak").

A plain run does only what that figure needs: it loads the graph, warms up,
times the K steps, writes the last step's results (--dump-outputs DIR) and
prints the result line.  --full adds everything else the benchmark measures:
the per-launch kernel tables of one extra profiled step, marginals, the
closest-keyframe search, scan registration, the Gauss-Newton, converged-regime
and live re-solve lines, the 1M-pose C5 graph and the CPU baseline; the options
that size or skip those lines take effect only with it.

    python bench.py [--gpus N --steps K --warmup W --config C3 --dump-outputs DIR --full --no-cpu-baseline]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_MFMA_PEAK_TFS = 78.6  # MI355X datasheet: FP64 matrix (and vector) 78.6 TFLOP/s dense
# kernel families bound by HBM bytes even where they report flops (factor_roofline)
HBM_FAMILIES = ("k_bwd_part",)
# measured on the box (scripts/ubench_syrk.hip): a bare v_mfma_f64_16x16x4_f64 loop,
# 8 independent chains per wave, 8-32 waves per CU, sustains 45-49 TFLOP/s
FP64_MFMA_LOOP_TFS = 49.0


def spmv_bytes(n, slots):
    """Algorithmic bytes of one k_pcg_spmv launch (DESIGN.md 'Roofline'):
    per slot V 72 B + column 4 B; per row row_ptr 4 B + D 48 B + p 24 B + q 24 B."""
    return 76 * slots + 100 * n


def linearize_bytes(n, ne):
    """Algorithmic bytes of one linearisation: per factor ids 8 +
    z 24 + Omega 48 read, the owner block H_ij 72 written (152 B); per pose the
    pose 24 read, H_ii upper 48 + b_i 24 written (96 B).  The Cholesky-mode
    sweep is two launches (k_linearize_own + k_linearize_side1), timed together
    from the first one's start to the second one's end."""
    return ne * 152 + n * 96


def _host_info():
    import platform
    model = platform.processor()
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    quota = None
    try:   # cgroup v2 CPU quota of this job ("max" = none)
        quota = open("/sys/fs/cgroup/cpu.max").read().strip()
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)), "usable_cpus": usable_cpus(),
            "cpu_model": model,
            "cgroup_cpu_max": quota, "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}


def usable_cpus():
    """CPUs this process can actually run on: its affinity mask, capped by the
    cgroup CPU quota (cpu.max "quota period": the GPU box grants each job a
    share of a many-core host -- affinity alone shows every core of the host,
    and OpenMP threads beyond the quota only oversubscribe it)."""
    aff = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return max(1, min(aff, int(float(q) / float(per) + 0.5)))
    except (OSError, ValueError):
        pass
    return aff


def cpu_baseline(g, nd_order, per_step, reps=5, curve_reps=3, amd_reps=3):
    """The C restatement (oracle/pgo_oracle.c: same LM, supernodal multifrontal
    Cholesky, OpenMP: fronts of a level across the threads, a big front's
    panel solve, Schur update, assembly and copies across the threads) on the
    host cores of this box, like-for-like with the GPU step (SURVEY 8d /
    BASELINE.md):

    * same fill: the CPU factorises on the GPU plan's nested-dissection
      ordering (handed over from pgo_debug_ordering); the oracle's own AMD is
      timed too (amd_all_cores);
    * same try mix: one LM unit (initial error + 1 linearisation + 1 lambda
      try -- factor, solve, model decrease, retract, error; C3's first
      linearisation accepts lambda_initial) is timed, median of `reps` after
      one warm-up, and the GPU trajectory's counts (per_step: L linearisations,
      T tries, both identical to the oracle's, tests/test_gpu_parity.py) are
      priced with it: t = t_err0 + L t_lin + T t_try;
    * all the host cores this job can use (usable_cpus: the affinity mask
      capped by the cgroup CPU quota; the headline value, `cores`); the
      thread-scaling curve at 1, 4, 8, 16, 32, 64 up to that count (median of
      `curve_reps`); 1 core as one_core.  Results do not depend on the thread
      count (bitwise).
    """
    import statistics
    from oracle.oracle import Oracle, set_threads
    allc_threads = usable_cpus()
    L, T = per_step["linearizations"], per_step["lm_tries"]

    def unit(o, n):
        o.optimize(max_outer=1)                           # warm-up
        runs = []
        for k in range(n):
            runs.append(o.optimize(max_outer=1).stats)
            log(f"  cpu unit {k + 1}/{n}: {runs[-1]['t_total']:.2f} s")
        t_lin = statistics.median(r["t_linearize"] for r in runs)
        t_err0 = statistics.median(r["t_error"] for r in runs) / 2.0   # initial + candidate error
        t_try = statistics.median(r["t_total"] - r["t_linearize"] for r in runs) - t_err0
        t_traj = t_err0 + L * t_lin + T * t_try
        return {"value": L / t_traj, "ms_per_try": 1e3 * t_try, "ms_per_linearization": 1e3 * t_lin,
                "ms_trajectory": 1e3 * t_traj, "factor_flops": runs[0]["factor_flops"], "nnz_l": runs[0]["nnz_l"],
                "ms_factor": 1e3 * statistics.median(r["t_factor"] for r in runs),
                "ms_solve": 1e3 * statistics.median(r["t_solve"] for r in runs), "reps": n}

    o_nd = Oracle(g, order=nd_order)
    set_threads(allc_threads)
    log(f"cpu baseline: {allc_threads} threads")
    allc = unit(o_nd, reps)
    curve = {str(allc_threads): allc}
    for t in sorted({1, 4, 8, 16, 32, 64} - {allc_threads}):
        if t > allc_threads:
            continue
        set_threads(t)
        log(f"cpu baseline: {t} threads")
        curve[str(t)] = unit(o_nd, curve_reps if t > 1 else reps)
    one = curve["1"] if "1" in curve else allc
    o_nd.close()
    set_threads(allc_threads)
    log("cpu baseline: AMD ordering")
    o_amd = Oracle(g)
    amd = unit(o_amd, amd_reps)
    o_amd.close()
    best_t = max(curve, key=lambda k: curve[k]["value"])
    return {
        "value": allc["value"],
        "unit": "GN iterations/s",
        "cores": allc_threads,
        "kind": "port",
        "sample": (f"{g.name}: median of {reps} LM units (initial error + 1 linearisation + 1 lambda try: "
                   f"{allc['factor_flops'] / 1e9:.1f} GFLOP supernodal Cholesky on the GPU plan's nested-dissection "
                   f"ordering, nnz(L) {allc['nnz_l'] / 1e6:.0f}M) after 1 warm-up, oracle/pgo_oracle.c, "
                   f"{allc_threads} OpenMP threads (every CPU this job may use: affinity capped by the cgroup quota); "
                   f"priced on the GPU trajectory's "
                   f"{L} linearisations / {T} tries"),
        "all_cores": allc,
        "one_core": one,
        "thread_curve": {k: {"value": v["value"], "ms_per_try": v["ms_per_try"], "ms_factor": v["ms_factor"]}
                         for k, v in sorted(curve.items(), key=lambda kv: int(kv[0]))},
        "best_threads": int(best_t),
        "best_value": curve[best_t]["value"],
        "amd_all_cores": amd,
        "host": _host_info(),
    }


def _lane_traffic(pmc, kernel, fam):
    """PMC HBM bytes per launch of `kernel` (profiles/pmc_traffic.json, measured
    on one-lambda-lane launches) scaled to this run's launches by their
    algorithmic flops per launch (the lane mix); None when not profiled."""
    v = pmc.get(f"{kernel}_bytes_per_launch")
    f1 = pmc.get(f"{kernel}_flops_per_launch")
    if v is None:
        return None
    if f1 and fam.get("flops_per_launch"):
        return v * fam["flops_per_launch"] / f1
    return v


def factor_roofline(kprof, totals, factor_flops):
    """Roofline of the dominant kernel family of the factor + solve (largest
    summed device time over the profiled factorisations, every launch timed
    with dispatch events on its own stream): achieved = algorithmic flops (MFMA
    families) or HBM bytes (extend-add, zeroing, assembly) per launch / average
    launch time.  Also the factorisation aggregate: algorithmic flops / device
    time of the factorisation graphs the timed steps replayed (every
    unprofiled factorisation, lambda lanes included), and the same for the
    profiled (eager, every launch timed) factorisations."""
    fams = {}
    for k, v in kprof.items():
        if v["launches"] == 0:
            continue
        # the backward solve's partial products stream L once (2 flops per 8 B):
        # priced on HBM bytes like the other families without MFMA work
        mfma = v["flops"] > 0 and k not in HBM_FAMILIES
        per = (v["flops"] if mfma else v["bytes"]) / v["launches"]
        avg = v["ms"] / v["launches"]
        ach = per / (avg * 1e-3) / (1e12 if mfma else 1e9) if avg > 0 else None
        fams[k] = {"launches": v["launches"], "ms": v["ms"], "avg_launch_ms": avg,
                   "bound": "mfma" if mfma else "hbm", "unit": "TFLOP/s" if mfma else "GB/s",
                   ("flops_per_launch" if mfma else "bytes_per_launch"): per, "achieved": ach,
                   "frac": ach / (FP64_MFMA_PEAK_TFS if mfma else HBM_PEAK_GBS) if ach else None}
    total_ms = sum(f["ms"] for f in fams.values())
    for f in fams.values():
        f["share"] = f["ms"] / total_ms if total_ms else None
    top = max(fams, key=lambda k: fams[k]["ms"]) if fams else None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    pmc = json.load(open(pmc_path)).get("C3", {}) if os.path.exists(pmc_path) else {}
    agg = prof_agg = None
    if totals["gfac_ms"] > 0:
        tfs = totals["gfac_flops"] / (totals["gfac_ms"] * 1e-3) / 1e12
        agg = {"flops_per_factorization": factor_flops, "factorizations": totals["gfac_flops"] / factor_flops,
               "ms": totals["gfac_ms"], "achieved": tfs, "unit": "TFLOP/s", "frac": tfs / FP64_MFMA_PEAK_TFS,
               "timing": "factorisation graph replays of the timed steps (HIP events on the library stream)"}
    if totals["fac_n"]:
        fac_ms = totals["fac_ms"] / totals["fac_n"]
        tfs = factor_flops / (fac_ms * 1e-3) / 1e12
        prof_agg = {"flops": factor_flops, "ms": fac_ms, "achieved": tfs, "frac": tfs / FP64_MFMA_PEAK_TFS,
                    "solve_ms": totals["sol_ms"] / totals["fac_n"], "profiled_factorizations": totals["fac_n"],
                    "timing": "eager launches, every launch bracketed by dispatch events"}
    out = {"kernel": top, "profiled_factorizations": totals["fac_n"], "factorization": agg,
           "factorization_profiled": prof_agg, "families": fams, "measured_loop_peak_tfs": FP64_MFMA_LOOP_TFS}
    if top:
        t = fams[top]
        out.update(bound=t["bound"], achieved=t["achieved"], unit=t["unit"], frac=t["frac"],
                   peak=FP64_MFMA_PEAK_TFS if t["bound"] == "mfma" else HBM_PEAK_GBS,
                   avg_launch_ms=t["avg_launch_ms"], traffic=_lane_traffic(pmc, top, t))
    return out


def live_resolve_bench(pg, g, k=5, params=None):
    """The live node's per-registration re-solve (graph.cpp:180-200, :130):
    starting at the optimum, k registrations, each appending one keyframe
    (dead-reckoned initial value), its odometry factor and one loop closure
    to an earlier keyframe (exact measurements), then optimize() on the same
    handle -- the resident values, graph and solver plan are refreshed in place
    (pgo_stats.plan_update).  Reports wall ms per registration (append +
    optimize) and the plan work; `params` are the headline run's (lambda lanes,
    graphs)."""
    import numpy as np
    from graphslam_amd.datasets import between_xyt, compose_xyt
    from graphslam_amd import _lib
    rng = np.random.default_rng(7)
    n = g.num_poses
    gt = np.array(g.ground_truth)
    x = pg.poses()
    cov = np.diag([0.05 ** 2, 0.05 ** 2, 0.00873 ** 2])
    rows = []
    for r in range(k):
        v = n + r
        step = np.array([1.0, 0.0, 0.0])
        gt = np.vstack([gt, compose_xyt(gt[v - 1], step)])
        x = np.vstack([x, compose_xyt(x[v - 1], step)])
        j = int(rng.integers(0, v - 20))
        t0 = time.perf_counter()
        pg.add_vertex(v + 1, *x[v])
        pg.add_edge(v, v + 1, between_xyt(gt[v - 1], gt[v]), cov)
        pg.add_edge(v + 1, j + 1, between_xyt(gt[v], gt[j]), cov)
        st = pg.optimize(params)
        rows.append({"ms": 1e3 * (time.perf_counter() - t0), "plan_update": st["plan_update"],
                     "upload_kind": st["upload_kind"],
                     "ms_plan": st["ms_plan"], "ms_upload": st["ms_upload"], "ms_optimize": st["ms_total"],
                     "ms_linearize": st["ms_linearize"], "ms_solve": st["ms_solve"], "ms_update": st["ms_update"],
                     "linearizations": st["linearizations"],
                     "lm_tries": st["inner_iterations"], "initial_error": st["initial_error"],
                     "final_error": st["final_error"],
                     "stop_reason": _lib.STOP_REASONS.get(st["stop_reason"], str(st["stop_reason"]))})
    return {"registrations": k, "ms_median": float(np.median([r["ms"] for r in rows])), "per_registration": rows,
            "note": "append 1 keyframe + odometry + 1 loop closure, then optimize on the same handle"}


def gauss_newton_bench(pg, default_params, reps=3, **common):
    """GTSAM's Gauss-Newton (PGO_ALG_GN) on the same graph from the same
    dead-reckoned values: the GN-iterations/s of the metric's name taken
    literally (one linearise + factor + solve + retract + chi^2 per iteration,
    no lambda tries), the error trajectory and how it stopped (GTSAM's
    relative-decrease test).  Median of `reps` after one warm-up; the oracle's
    run is pinned in tests/golden/golden_C3-gn.npz."""
    import numpy as np
    from graphslam_amd import _lib
    p = default_params(algorithm=1, **common)
    runs = []
    for k in range(reps + 1):
        pg.restore_values()
        t0 = time.perf_counter()
        st = pg.optimize(p)
        dt = time.perf_counter() - t0
        if k:
            runs.append((dt, st))
    dt = float(np.median([r[0] for r in runs]))
    st = runs[-1][1]
    return {"iterations": st["iterations"], "linearizations": st["linearizations"], "ms_to_stop": 1e3 * dt,
            "gn_iterations_per_s": st["linearizations"] / dt, "initial_error": st["initial_error"],
            "final_error": st["final_error"], "errors": [float(v) for v in pg.trace()[:, 4]],
            "stop_reason": _lib.STOP_REASONS.get(st["stop_reason"], str(st["stop_reason"])), "reps": reps}


def converged_regime_bench(pg, g, default_params, reps=3, **common):
    """ms-to-chi^2 convergence where GTSAM's convergence test is what stops LM:
    GTSAM-default LM from the ground-truth poses (the values a warm-started
    live solve holds, graph.cpp:130) to the optimum of the noisy measurements.
    Values uploaded before each timed optimize (not timed); median of `reps`
    after one warm-up."""
    import numpy as np
    from graphslam_amd import _lib
    gt = np.asarray(g.ground_truth)
    p = default_params(**common)
    runs = []
    for k in range(reps + 1):
        pg.set_poses(gt)
        pg.error()                                    # upload the values outside the timed region
        t0 = time.perf_counter()
        st = pg.optimize(p)
        dt = time.perf_counter() - t0
        if k:
            runs.append((dt, st))
    dt = float(np.median([r[0] for r in runs]))
    st = runs[-1][1]
    return {"start": "ground truth", "ms_to_convergence": 1e3 * dt, "iterations": st["iterations"],
            "lm_tries": st["inner_iterations"], "linearizations": st["linearizations"],
            "gn_iterations_per_s": st["linearizations"] / dt, "initial_error": st["initial_error"],
            "final_error": st["final_error"],
            "stop_reason": _lib.STOP_REASONS.get(st["stop_reason"], str(st["stop_reason"])), "reps": reps}


def closest_keyframe_bench(pg, g, skip=10, reps=20):
    """closest_keyframe service (graph.cpp:146-178) at the optimum: one query
    over all keyframes (HBM scan: 16 B of (x, y) per candidate; the values are
    double4, so the scan touches 32 B) and the batched form with every keyframe
    as keyframes.back() (N queries, ~N^2/2 distance evaluations, fp64 VALU)."""
    import numpy as np
    n = g.num_poses
    last = pg.poses(np.asarray(g.keys[-1:], dtype=np.uint64))[0]
    pg.closest_keyframe(last[0], last[1], skip)            # warm
    scan = []
    t0 = time.perf_counter()
    for _ in range(reps):
        pg.closest_keyframe(last[0], last[1], skip)
        scan.append(pg.debug_search_ms()[0])
    wall_ms = 1e3 * (time.perf_counter() - t0) / reps
    keys = np.asarray(g.keys, dtype=np.uint64)
    pg.closest_keyframes(keys[:1024], skip)                # warm
    t0 = time.perf_counter()
    pg.closest_keyframes(keys, skip)
    bwall = 1e3 * (time.perf_counter() - t0)
    bms = pg.debug_search_ms()[1]
    pairs = sum(max(i + 1 - skip, 0) for i in range(n))
    scan_ms = float(np.mean(scan))
    return {
        "single_query": {"candidates": n - skip, "kernel_ms": scan_ms, "call_ms": wall_ms,
                         "achieved_gbs": 16.0 * (n - skip) / (scan_ms * 1e-3) / 1e9,
                         "bytes_per_candidate": 16},
        "batched": {"queries": n, "pairs": pairs, "kernel_ms": bms, "call_ms": bwall,
                    "gpairs_per_s": pairs / (bms * 1e-3) / 1e9},
    }


def scan_registration_bench(batch=1024, reps=3, cpu_sample=64):
    """The scanner's gicp() (scanner.cpp:35-74) on synthetic
    360-beam laser scans of a room: `batch` registrations (current scan ->
    keyframe scan) in one pgo_gicp_align_batch launch pair.  Reports
    registrations/s (device time and call time), the nearest-neighbour distance
    evaluations the batch performed (covariance kNN + correspondence rounds +
    fitness: the kernel's algorithmic work) per second, and the C restatement
    on one core over a sample of the same pairs."""
    import numpy as np
    from graphslam_amd.datasets import scan_pairs
    from graphslam_amd.scanner import ScanRegistrar
    pairs = scan_pairs(batch, seed=11)
    S, T = [p[0] for p in pairs], [p[1] for p in pairs]
    reg = ScanRegistrar(0)
    reg.align_batch(S[:64], T[:64])                          # warm
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = reg.align_batch(S, T, arrays=True)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(reg.device_ms())
    ns = np.array([len(s) for s in S], float)
    nt = np.array([len(t) for t in T], float)
    it = out["iterations"].astype(float)
    evals = float(np.sum(ns * ns + nt * nt + (it + 1) * ns * nt))
    dms = float(np.median(dev))
    res = {"batch": batch, "points_per_cloud": float(np.mean(np.concatenate([ns, nt]))),
           "mean_iterations": float(it.mean()), "mean_optimiser_steps": float(out["inner_iterations"].mean()),
           "keyframes": int(out["keyframe"].sum()),
           "device_ms": dms, "call_ms": float(np.median(wall)),
           "registrations_per_s": batch / (dms * 1e-3), "registrations_per_s_call": batch / (np.median(wall) * 1e-3),
           "nn_evals": evals, "gnn_evals_per_s": evals / (dms * 1e-3) / 1e9,
           # fp32 VALU bound: a distance evaluation is 3 sub + 1 mul + 2 fma = 8 flops
           # (the fp64 Gauss-Newton steps are not counted), against the 157.3 TFLOP/s
           # fp32 vector peak (MI355X_MICROARCH.md)
           "roofline": {"bound": "valu", "achieved": 8.0 * evals / (dms * 1e-3) / 1e12, "peak": 157.3,
                        "unit": "TFLOP/s", "frac": 8.0 * evals / (dms * 1e-3) / 1e12 / 157.3, "traffic": None}}
    try:
        from oracle import oracle as orc
        k = min(cpu_sample, batch)
        t0 = time.perf_counter()
        for b in range(k):
            orc.gicp_align(S[b], T[b])
        cpu_s = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": k / cpu_s, "unit": "registrations/s", "cores": 1, "kind": "port",
                               "sample": f"first {k} pairs, oracle/gicp_oracle.c (brute-force neighbours, gcc -O3)"}
        res["gpu_over_cpu"] = res["registrations_per_s"] / res["cpu_baseline"]["value"]
    except Exception as e:   # the oracle is optional on the GPU box
        res["cpu_baseline"] = {"error": str(e)}
    reg.close()
    return res


def tries_per_linearization(pg):
    """LM tries of each linearisation of the last optimize, from its trace
    (column 0: accepted steps before the try -- constant within a
    linearisation); the speculative multi-GPU model prices rounds with it."""
    import numpy as np
    tr = pg.trace()
    if len(tr) == 0:
        return []
    _, idx, cnt = np.unique(tr[:, 0], return_index=True, return_counts=True)
    return [int(c) for _, c in sorted(zip(idx, cnt))]


def c5_line(default_params, lanes=3, **common):
    """BASELINE.json configs[4] (1M poses / 5M between factors, the city-scale
    graph quoted on 8 GPUs) on this one GPU: one GTSAM-default LM optimize from
    the dead-reckoned values after one warm-up optimize (the warm-up includes
    the symbolic analysis, reported apart), 3 lambda lanes.  Reports GN
    iterations/s, the tries / rounds / factorisations, and the factorisation
    aggregate over the timed optimize's graph replays."""
    from graphslam_amd import _lib, datasets
    from graphslam_amd.pose_graph import PoseGraph
    t0 = time.perf_counter()
    g5 = datasets.make("C5")
    t_gen = time.perf_counter() - t0
    pg5 = PoseGraph.from_dataset(g5)
    pg5.save_values()
    p = default_params(lambda_lanes=lanes, **common)
    t0 = time.perf_counter()
    st0 = pg5.optimize(p)
    t_first = time.perf_counter() - t0
    pg5.restore_values()
    t0 = time.perf_counter()
    st = pg5.optimize(p)
    dt = time.perf_counter() - t0
    fl, fms = st["factor_graph_flops"], st["ms_factor_graph"]
    tfs = fl / (fms * 1e-3) / 1e12 if fms > 0 else None
    out = {"workload": f"C5: {g5.num_poses} poses / {g5.num_edges} between factors + 1 prior (seed "
                       f"{g5.meta.get('seed')}), GTSAM-default LM from dead-reckoned values, one GPU",
           "value": st["linearizations"] / dt, "unit": "GN iterations/s", "ms_per_optimize": 1e3 * dt,
           "lambda_lanes": lanes, "linearizations": st["linearizations"], "lm_tries": st["inner_iterations"],
           "accepted": st["iterations"], "lambda_rounds": st["lambda_rounds"], "factorizations": st["solves"],
           "final_error": st["final_error"], "initial_error": st["initial_error"],
           "stop_reason": _lib.STOP_REASONS.get(st["stop_reason"], str(st["stop_reason"])),
           "factor_flops": st["factor_flops"],
           "factorization": {"ms": fms, "flops": fl, "achieved": tfs, "unit": "TFLOP/s",
                             "frac": tfs / FP64_MFMA_PEAK_TFS if tfs else None,
                             "timing": "factorisation graph replays of the timed optimize"},
           "tries_per_linearization": tries_per_linearization(pg5),
           "handoff_retries": st0["handoff_retries"] + st["handoff_retries"],
           "ms_first_optimize_incl_analysis": 1e3 * t_first, "ms_plan_first": st0["ms_plan"],
           "s_generate": t_gen}
    pg5.close()
    return out


DUMP_STATS = ("initial_error", "final_error", "iterations", "linearizations", "inner_iterations", "stop_reason")
DUMP_MAX_ROWS = 2_000_000   # poses.npy stays under 48 MB; a larger graph is sampled


def dump_outputs(path, pg, st):
    """What the last timed step handed its caller, as float64 .npy files:
    poses.npy ([N, 3] optimised x, y, theta in insertion order; of a graph of
    more than DUMP_MAX_ROWS poses a fixed, seeded sample of rows), trace.npy
    (the per-try record of pgo_get_trace without its wall-clock column) and
    stats.npy (DUMP_STATS of pgo_stats, in that order)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    poses = pg.poses()
    if len(poses) > DUMP_MAX_ROWS:
        poses = poses[np.sort(np.random.default_rng(0).choice(len(poses), DUMP_MAX_ROWS, replace=False))]
    np.save(os.path.join(path, "poses.npy"), poses)
    np.save(os.path.join(path, "trace.npy"), np.ascontiguousarray(pg.trace()[:, :7]))
    np.save(os.path.join(path, "stats.npy"), np.array([st[k] for k in DUMP_STATS], dtype=np.float64))


def log(msg):
    """Progress on stderr (the JSON line is stdout's only output)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _partition_bounds(live):
    """{config: {P: {flop bounds, exchange points / bytes per rank, the model's
    speed-up per mode at its central constants and its min-max range over the
    swept ones, the auto choice}}}: profiles/r06_partition_bounds.json
    (host-computed for C3 and C5, scripts/partition_bounds.py), plus this
    run's own rank count when it was computed live.  All unmeasured on 8 GPUs."""
    path = os.path.join(ROOT, "profiles", "r06_partition_bounds.json")   # (round 6: fixed-top candidates)
    keep = ("bound", "bound_replicated_top", "exchange_points", "exchange_bytes", "est_speedup_distributed_top",
            "est_speedup_replicated_top", "est_speedup_spec", "est_speedup_hybrid", "range_min", "range_max", "auto")
    out = {}
    if os.path.exists(path):
        for c, per in json.load(open(path)).items():
            out[c] = {P: {k: v[k] for k in keep if k in v} for P, v in per.items()}
    if live:
        out["this_run"] = {P: {k: v[k] for k in keep if k in v} for P, v in live.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--profile-every", type=int, default=8,
                    help="in one extra untimed step, every k-th factorisation runs eagerly with per-launch events (0: none)")
    ap.add_argument("--cpu-reps", type=int, default=5, help="timed CPU LM units per thread count (median)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--solver", choices=["cholesky", "pcg"], default="cholesky")
    ap.add_argument("--no-graphs", action="store_true",
                    help="eager launches instead of the captured factor+solve hipGraph (rocprofv3 runs)")
    ap.add_argument("--marginals", type=int, default=64,
                    help="after the timed steps: time marginal covariances of this many poses (0: skip)")
    ap.add_argument("--lanes", type=int, default=None,
                    help="consecutive lambda tries per batched factorisation (pgo_params.lambda_lanes; "
                         "default 3 on one GPU -- the rounds are sized to the tries expected -- and 2 per "
                         "rank in the speculative multi-GPU search, whose rounds run every lane)")
    ap.add_argument("--multi", choices=["auto", "spec", "partition", "hybrid", "replicas"], default="auto",
                    help="N>1: speculative lambda search over RCCL (one job), partitioned factorisation "
                         "(one job: subtrees per rank, Schur complements all-gathered, the top fronts' columns "
                         "dealt to the ranks), hybrid (--groups G partition groups running the speculative "
                         "search), independent replicas, or auto: the built mode whose worst case over the "
                         "cost model's sensitivity range (graphslam_amd/multi_model.py) is best")
    ap.add_argument("--groups", type=int, default=0,
                    help="--multi hybrid: partition groups (N / groups ranks each); 0 = the model's choice")
    ap.add_argument("--same-device", action="store_true",
                    help="rehearsal on a one-GPU box: every rank on device 0, host (gloo) transport")
    ap.add_argument("--ordering", choices=["nd", "amd"], default="nd",
                    help="fill-reducing ordering of the Cholesky solver (pgo_opts.ordering)")
    ap.add_argument("--search", type=int, default=1,
                    help="after the timed steps: time the closest_keyframe search at the optimum (0: skip)")
    ap.add_argument("--gicp", type=int, default=1024,
                    help="scan registrations in the GICP batch line (0: skip)")
    ap.add_argument("--live", type=int, default=5,
                    help="after the timed steps: time this many per-registration re-solves (0: skip)")
    ap.add_argument("--gn", type=int, default=1, help="after the timed steps: the Gauss-Newton line (0: skip)")
    ap.add_argument("--converged", type=int, default=1,
                    help="after the timed steps: LM from the ground truth to convergence (0: skip)")
    ap.add_argument("--c5", type=int, default=1,
                    help="one GPU, C3 run: after the other lines, the 1M-pose C5 graph (BASELINE configs[4]): "
                         "one warm-up + one timed optimize (0: skip)")
    ap.add_argument("--max-outer", type=int, default=0,
                    help="profiling runs only: stop each optimize after this many linearisations")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also everything else the benchmark measures: the profiled step "
                         "(--profile-every), --marginals, --search, --gicp, --gn, --converged, --live, --c5 and the "
                         "CPU baseline; without it those options have no effect")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's results to DIR/poses.npy, trace.npy and "
                         "stats.npy (float64; the same arguments give the same inputs from run to run)")
    args = ap.parse_args()
    if not args.full:   # a plain run: set-up, warm-up, the timed steps, the result line
        args.profile_every = args.marginals = args.search = args.gicp = 0
        args.gn = args.converged = args.live = args.c5 = 0
        args.no_cpu_baseline = True

    from graphslam_amd import datasets
    from graphslam_amd.pose_graph import PoseGraph, default_params
    from graphslam_amd.replicas import init_from_env, timed_steps

    r = init_from_env()
    world, rank = r.world, r.rank
    g = datasets.make(args.config)
    from graphslam_amd import _lib
    ordering = _lib.PGO_ORDERING_AMD if args.ordering == "amd" else _lib.PGO_ORDERING_ND
    pg = PoseGraph.from_dataset(g, device=0 if args.same_device else r.local_rank, ordering=ordering)
    # plan-derived bounds of the partitioned factorisation (host only, before
    # anything is timed): the auto mode's choice, the line's config
    bounds = {}
    mode_why = None
    if world > 1 and (args.multi == "auto" or (args.multi == "hybrid" and args.groups <= 0)):
        from graphslam_amd import multi_model
        obj = [None]
        if rank == 0:
            pd = multi_model.PlanData(pg, args.config)
            b = dict(pd.bound(world))
            b["rank_flops"] = [float(v) for v in b["rank_flops"]]
            b.update(multi_model.estimate(pg, world, args.config, pd=pd))
            obj = [(multi_model.choose(b), b)]
        r.dist.broadcast_object_list(obj, src=0)
        (mode, groups, dist_top), b = obj[0]
        if args.multi == "auto":
            args.multi, args.groups = mode, groups
            if args.multi in ("partition", "hybrid") and not dist_top:
                os.environ["PGO_DIST_TOP"] = "0"   # the replicated top (read when the plan is built)
        elif args.groups <= 0:   # hybrid, groups from the model
            hy = b["range_min"]
            args.groups = max((int(k[6:]) for k in hy if k.startswith("hybrid") and "_" not in k),
                              key=lambda G: hy[f"hybrid{G}"],
                              default=world)
            if not b.get("hybrid_distributed_top", {}).get(str(args.groups), True):
                os.environ["PGO_DIST_TOP"] = "0"   # the top the model priced this layout with
        bounds[str(world)] = {k: v for k, v in b.items() if k != "sensitivity"}
        lo, hi = b["range_min"], b["range_max"]
        mode_why = (f"{'auto' if mode == args.multi else 'chosen'}: {args.multi}"
                    f"{' x' + str(args.groups) + ' groups' if args.multi == 'hybrid' else ''}; model speed-up "
                    "ranges (min-max over B, t_bcast): " +
                    ", ".join(f"{k} {lo[k]:.2f}-{hi[k]:.2f}x" for k in lo) +
                    f" ({b['model']}; level times: {b['level_times']}; unmeasured on 8 GPUs)")
    elif args.multi == "auto":
        args.multi = "spec"
    if args.multi == "hybrid" and (args.groups < 2 or world % args.groups or args.groups >= world):
        args.multi = "spec" if args.groups >= world else "partition"   # a degenerate hybrid
    if args.lanes is None:
        # speculative search: one lane per rank -- a round's time is its
        # slowest rank's replay, and a one-lane replay costs half a three-lane
        # one, while P ranks already cover P tries (C3 trajectory: 1-4 tries per
        # linearisation but one of 10: 8 ranks x 1 lane = 9 one-lane rounds
        # against 8 two-lane ones)
        args.lanes = 1 if world > 1 and args.multi in ("spec", "hybrid") else 3
    spec = world > 1 and args.multi in ("spec", "partition", "hybrid")   # one job over all ranks
    part = world > 1 and args.multi == "partition"
    hybrid = world > 1 and args.multi == "hybrid"
    hc = None
    transport = "host" if args.same_device else "rccl"
    if spec:
        from graphslam_amd import multi_gpu
        if hybrid and args.same_device:
            hc = multi_gpu.attach_hybrid(pg, r.dist, rank, world, args.groups, transport="host")
        elif hybrid:
            # both RCCL communicators; should any rank fail to bring one up,
            # every rank falls back to host-transport groups, as below
            import torch
            ok = 1
            try:
                hc = multi_gpu.attach_hybrid(pg, r.dist, rank, world, args.groups, transport="rccl")
            except Exception as e:  # noqa: BLE001
                ok = 0
                print(f"rank {rank}: RCCL communicators failed ({e}); falling back to the host transport",
                      file=sys.stderr)
            flag = torch.tensor([ok], dtype=torch.int32)
            r.dist.all_reduce(flag, op=r.dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                pg.comm_free()
                hc = multi_gpu.attach_hybrid(pg, r.dist, rank, world, args.groups, transport="host")
                transport = "host-fallback"
        elif args.same_device:
            hc = multi_gpu.attach_host(pg, r.dist, rank, world)
        else:
            # RCCL over xGMI; should any rank fail to bring its communicator up,
            # every rank falls back to the host transport (gloo) -- same results,
            # slower exchange -- and the line says so
            import torch
            ok = 1
            try:
                multi_gpu.attach_rccl(pg, r.dist, rank, world)
            except Exception as e:  # noqa: BLE001
                ok = 0
                print(f"rank {rank}: RCCL communicator failed ({e}); falling back to the host transport",
                      file=sys.stderr)
            flag = torch.tensor([ok], dtype=torch.int32)
            r.dist.all_reduce(flag, op=r.dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                if ok:
                    pg.comm_free()
                hc = multi_gpu.attach_host(pg, r.dist, rank, world)
                transport = "host-fallback"
    pg.save_values()                     # upload graph + values once; snapshot the initial values
    # the timed steps run the production configuration (no per-launch
    # profiling); with --full one more, untimed step with every profile_every-th
    # factorisation run eagerly with per-launch events feeds the kernel tables
    common = dict(max_outer=args.max_outer, linear_solver=1 if args.solver == "cholesky" else 0,
                  use_graphs=0 if args.no_graphs else 1, lambda_lanes=args.lanes,
                  multi_gpu=2 if hybrid else 1 if part else 0)
    params = default_params(profile_every=0, **common)
    prof_params = default_params(profile_every=args.profile_every, **common)

    kprof = {}

    def step(p=params):
        pg.restore_values()
        st = pg.optimize(p)              # returns after the handle's stream has drained
        for k, v in pg.kernel_profile().items():   # profiled factorisations of this step (host copy)
            a = kprof.setdefault(k, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            for f in a:
                a[f] += v[f]
        return st["linearizations"], st

    log(f"timed steps: {args.warmup} warm-up + {args.steps}")
    elapsed, lin_total, results = timed_steps(r, step, args.steps, args.warmup)
    log(f"timed steps done: {1e3 * elapsed / args.steps:.1f} ms per step")
    if spec:   # one job: every rank walked the same linearisations
        lin_total /= world
    if args.dump_outputs and rank == 0:   # before anything below optimises again
        dump_outputs(args.dump_outputs, pg, results[-1][1])
    # the timed steps' trajectory, read before the profiled step (which may stop
    # early under --max-outer) and the side lines re-optimize
    tries_lin = tries_per_linearization(pg)
    prof_stats = [step(prof_params)[1]] if args.profile_every > 0 else []
    marg = None
    if args.marginals > 0 and rank == 0:
        import numpy as np
        keys = np.asarray(g.keys)[np.linspace(0, g.num_poses - 1, args.marginals).astype(np.int64)]
        pg.marginal_covariances(keys[:1])            # plan + first factorisation warm
        t0 = time.perf_counter()
        pg.marginal_covariances(keys)
        dt = time.perf_counter() - t0
        marg = {"keys": int(len(keys)), "ms": 1e3 * dt,
                "note": "gtsam::Marginals::marginalCovariance per pose at the optimum: one undamped "
                        "factorisation + per-pose path solves (Y'Y, Y = L^-1 E)"}
    search = None
    if args.search and rank == 0:
        search = closest_keyframe_bench(pg, g)
    scan = None
    if args.gicp and rank == 0:
        scan = scan_registration_bench(args.gicp)
    if args.full:
        log("marginals / search / scan registration done")
    one = dict(linear_solver=common["linear_solver"], use_graphs=common["use_graphs"])
    gn = gauss_newton_bench(pg, default_params, **one) if args.gn and rank == 0 and not spec else None
    conv = (converged_regime_bench(pg, g, default_params, lambda_lanes=args.lanes, **one)
            if args.converged and rank == 0 and not spec else None)
    if args.full:
        log("Gauss-Newton and converged-regime lines done")
    # the GPU plan's ordering of g, taken before live_resolve appends to the handle
    nd_order = pg.debug_ordering() if rank == 0 and not args.no_cpu_baseline and world == 1 else None
    live = None
    if args.live and rank == 0 and not spec:
        log("live re-solve line")
        live = live_resolve_bench(pg, g, args.live, params)
    c5 = None
    if args.c5 and rank == 0 and world == 1 and args.config == "C3" and args.solver == "cholesky":
        log("C5 line")
        c5 = c5_line(default_params, lanes=args.lanes, **one)
        log(f"C5 line done: {c5['value']:.2f} GN it/s")
    stats = [s for _, s in results]
    last = stats[-1]
    ps = prof_stats
    totals = dict(spmv_ms=sum(s["kernel_spmv_ms"] for s in ps), spmv_n=sum(s["kernel_spmv_count"] for s in ps),
                  lin_ms=sum(s["kernel_linearize_ms"] for s in ps),
                  lin_n=sum(s["kernel_linearize_count"] for s in ps),
                  fac_n=sum(s["kernel_syrk_count"] for s in ps),
                  fac_ms=sum(s["ms_factor_profiled"] for s in ps),
                  sol_ms=sum(s["ms_solve_profiled"] for s in ps),
                  gfac_ms=sum(s["ms_factor_graph"] for s in stats),
                  gfac_flops=sum(s["factor_graph_flops"] for s in stats))

    if rank == 0:
        n, ne = g.num_poses, g.num_edges
        slots = 2 * ne
        spmv_avg_ms = totals["spmv_ms"] / max(totals["spmv_n"], 1)
        achieved = spmv_bytes(n, slots) / (spmv_avg_ms * 1e-3) / 1e9 if totals["spmv_n"] else None
        lin_avg_ms = totals["lin_ms"] / max(totals["lin_n"], 1)
        pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        pmc = json.load(open(pmc_path)).get(args.config, {}) if os.path.exists(pmc_path) else {}
        if args.solver == "pcg":
            roofline = {
                "kernel": "k_pcg_spmv", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS if achieved else None,
                "traffic": pmc.get("k_pcg_spmv_bytes_per_launch"),
                "bytes_per_launch": spmv_bytes(n, slots), "avg_launch_ms": spmv_avg_ms,
                "timed_launches": totals["spmv_n"],
            }
        else:
            roofline = factor_roofline(kprof, totals, last["factor_flops"])
        out = {
            "metric": "GN iterations/sec + ms-to-chi2 convergence, 100k-pose Manhattan graph",
            "value": lin_total / elapsed,
            "unit": "GN iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "full": args.full,
            "ms_per_step": 1e3 * elapsed / args.steps,
            # the timed optimize ends at GTSAM's stop -- on C3 lambda's upper bound, not
            # convergence (per_step.stop_reason); ms-to-chi2 convergence proper is the
            # converged_regime line (GTSAM's convergence test ends LM there)
            "ms_to_stop": 1e3 * elapsed / args.steps,
            "ms_to_convergence": conv["ms_to_convergence"] if conv else None,
            "higher_is_better": True,
            "scaling": "strong" if spec else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"{args.config}: {n} poses / {ne} between factors + 1 prior, Manhattan walk "
                            f"(seed {g.meta.get('seed')}), GTSAM-default LM from dead-reckoned values",
                "poses": n, "edges": ne,
                "parallelism": ((f"hybrid{args.groups}x{world // args.groups}" if hybrid else
                                 f"partition{world}" if part else f"spec-lambda{world}") +
                                "-" + transport) if spec else
                               (f"replicas{world}" if world > 1 else "single-gpu"),
                "lambda_lanes": args.lanes,
                "multi_mode": mode_why or (args.multi if world > 1 else None),
                # plan-derived flop bound of the partitioned factorisation (distributed top) and
                # the cost model's estimate, per rank count -- scripts/partition_bounds.py;
                # unmeasured on an 8-GPU node
                "partition_bounds": _partition_bounds(bounds),
                "solver": (f"GPU supernodal multifrontal Cholesky ({'nested-dissection' if args.ordering == 'nd' else 'AMD'} ordering, fp64 MFMA Schur updates)"
                           if args.solver == "cholesky" else
                           "block-Jacobi PCG, rel tol %.0e" % params.pcg_relative_tol),
            },
            "per_step": {
                "linearizations": last["linearizations"], "lm_tries": last["inner_iterations"],
                "accepted": last["iterations"], "pcg_iterations": last["pcg_iterations"],
                "initial_error": last["initial_error"], "final_error": last["final_error"],
                "ms_linearize": last["ms_linearize"], "ms_solve": last["ms_solve"], "ms_update": last["ms_update"],
                "lambda_rounds": last["lambda_rounds"], "solves_rank0": last["solves"], "ms_comm": last["ms_comm"],
                "stop_reason": _lib.STOP_REASONS.get(last["stop_reason"], str(last["stop_reason"])),
                # expected 0.5 chi^2 at the optimum: half the residual dimension minus the pose dof
                "expected_error_at_optimum": 0.5 * (3 * (ne + len(g.prior_keys)) - 3 * n),
                "tries_per_linearization": tries_lin,
                # factorisations re-run after an in-launch hand-off timed out, summed over
                # every timed and profiled step (0 = no hidden retry)
                "handoff_retries": sum(s["handoff_retries"] for s in stats + prof_stats),
                "transport": _lib.TRANSPORTS.get(last["transport"], str(last["transport"])),
                "part_transport": _lib.TRANSPORTS.get(last["part_transport"], str(last["part_transport"])),
            },
            "roofline": roofline,
            "linearize_kernel": {
                "kernel": "k_linearize_own+k_linearize_side1",
                "avg_launch_ms": lin_avg_ms,
                "bytes_per_launch": linearize_bytes(n, ne),
                "achieved_gbs": linearize_bytes(n, ne) / (lin_avg_ms * 1e-3) / 1e9 if totals["lin_n"] else None,
                "peak_gbs": 8000.0,
                "frac": linearize_bytes(n, ne) / (lin_avg_ms * 1e-3) / 8e12 if totals["lin_n"] else None,
                "traffic": (pmc["k_linearize_own_bytes_per_launch"] + pmc["k_linearize_side1_bytes_per_launch"]
                            if "k_linearize_own_bytes_per_launch" in pmc and "k_linearize_side1_bytes_per_launch" in pmc
                            else None),
            },
            "cpu_baseline": None,
            "gauss_newton": gn,
            "converged_regime": conv,
            "marginals": marg,
            "closest_keyframe": search,
            "live_resolve": live,
            "scan_registration": scan,
            "c5": c5,
        }
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(g, nd_order, out["per_step"], reps=args.cpu_reps)
            out["cpu_baseline"]["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            out["cpu_baseline"]["gpu_over_cpu_best_threads"] = out["value"] / out["cpu_baseline"]["best_value"]
            out["cpu_baseline"]["gpu_over_cpu_one_core"] = out["value"] / out["cpu_baseline"]["one_core"]["value"]
        print(json.dumps(out))
    if spec:
        pg.comm_free()
    pg.close()
    del hc
    r.close()


if __name__ == "__main__":
    main()
