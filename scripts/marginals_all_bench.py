#!/usr/bin/env python
"""Time PoseGraph.marginal_covariances_all on the C3 graph (100k poses / 500k
between factors) at the values a default optimize() ends at, and write
profiles/marginals_all.json:

  (a) wall time of marginal_covariances_all() and of
      marginal_covariances_all(edges=True): median of --reps calls after one
      warm call of each (host clock around calls that end in a device
      synchronise; linearisation, factorisation, the pass, the read-out and the
      copy to the host are all inside);
  (b) debug_factor_time(lanes=1) at the same values: one factorisation;
  (c) pgo_marginal_covariances on --keys evenly spaced keys, scaled by n / keys:
      the per-pose path's cost of the same job;
  (d) flops, workspace and launches of the pass from debug_selinv_plan, and the
      whole call's rate (a) as a fraction of the fp64 MFMA peak (an end-to-end
      figure, not a kernel's share of peak).

    python scripts/marginals_all_bench.py [--config C3 --reps 5 --keys 4096 --out profiles/marginals_all.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from graphslam_amd import datasets  # noqa: E402
from graphslam_amd.pose_graph import PoseGraph  # noqa: E402

FP64_MFMA_PEAK_TFS = 78.6   # MI355X datasheet, as bench.py


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals_all.json"))
    args = ap.parse_args()
    g = datasets.make(args.config)
    n = g.num_poses
    pg = PoseGraph.from_dataset(g)
    st = pg.optimize()
    plan = pg.debug_selinv_plan()
    pg.marginal_covariances_all()                      # warm: plan lists, workspaces, code objects
    pg.marginal_covariances_all(edges=True)            # ... and the edge table
    t_all = timed(pg.marginal_covariances_all, args.reps)
    t_edges = timed(lambda: pg.marginal_covariances_all(edges=True), args.reps)
    factor_ms = pg.debug_factor_time(lanes=1)
    keys = np.asarray(g.keys)[np.linspace(0, n - 1, min(args.keys, n)).astype(np.int64)]
    pg.marginal_covariances(keys[:1])                  # warm
    t_keys = timed(lambda: pg.marginal_covariances(keys), 3)
    a, ae = statistics.median(t_all), statistics.median(t_edges)
    c = statistics.median(t_keys) * n / len(keys)
    res = {
        "config": args.config, "poses": n, "between_factors": g.num_edges,
        "optimize": {"iterations": st["iterations"], "final_error": st["final_error"]},
        "a_all_ms": a, "a_all_ms_runs": t_all,
        "a_all_edges_ms": ae, "a_all_edges_ms_runs": t_edges,
        "b_factor_ms": factor_ms,
        "c_per_pose_keys": len(keys), "c_per_pose_ms_runs": t_keys, "c_per_pose_scaled_ms": c,
        "a_over_b": a / factor_ms, "a_over_c": a / c, "a_edges_over_c": ae / c,
        "d_plan": {"launches": plan["launches"], "flops": plan["flops"],
                   "workspace_doubles": plan["workspace_doubles"], "levels": plan["levels"]},
        "d_call_tflops": plan["flops"] / (a * 1e-3) / 1e12,
        "d_call_fraction_of_fp64_peak": plan["flops"] / (a * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFS,
        "note": "wall times of whole calls (host clock, each call ends in a device synchronise); the rate is "
                "the pass's algorithmic flops over the whole call, the factorisation and the copies included",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not a < c:
        print("marginals_all_bench: the pass is not faster than the per-pose path at this size", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
