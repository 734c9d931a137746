#!/usr/bin/env python
"""Time graduated non-convexity (PoseGraph.optimize_gnc) on the C3 graph (100k
poses / 500k between factors) with --share of its loop closures replaced by
random poses, GM and TLS, all loop closures as candidates, from dead reckoning,
and write a text report (profiles/gnc_gpu.txt).

Per loss: one warm-up call (plan, workspaces, captured graphs, code objects),
the values put back, then the measured call: pgo_gnc_stats (ms_total, ms_inner,
ms_weights, outer iterations, tries), how the final weights split the replaced
closures from the true ones, and the position RMSE.  Beside them the Gaussian
and the robust linearisation's device time per linearisation (HIP events,
profile_every=1) and the sweep's host wall per call (kernel, reduction and the
five-double read-back; ms_weights over the sweeps made), which bounds its device
time from above.

    python scripts/gnc_bench.py [--config C3 --share 0.1 --out profiles/gnc_gpu.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from graphslam_amd import datasets  # noqa: E402
from graphslam_amd.pose_graph import PoseGraph  # noqa: E402


def rmse(xyt, g):
    d = xyt[:, :2] - g.ground_truth[:, :2]
    return float(np.sqrt((d ** 2).sum(axis=1).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=2008)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnc_gpu.txt"))
    args = ap.parse_args()
    g = datasets.make(args.config)
    bad = datasets.corrupt_loop_closures(g, args.share, args.seed)
    lc = datasets.loop_closure_indices(g)
    good = np.setdiff1d(lc, bad)
    lines = [f"{args.config}: {g.num_poses} poses, {g.num_edges} between factors, {len(lc)} loop closures, "
             f"{len(bad)} replaced by random poses (seed {args.seed}); candidates: all loop closures; "
             "from dead reckoning; one call after a warm-up call from the same values"]
    pg = PoseGraph.from_dataset(g)
    pg.save_values()
    st = pg.optimize(profile_every=1)
    lines.append(f"plain LM: rmse {rmse(pg.poses(), g):.3f} m, {st['inner_iterations']} tries, "
                 f"{st['ms_total']:.1f} ms, Gaussian linearise {st['kernel_linearize_ms'] / st['kernel_linearize_count']:.4f} "
                 f"ms device per linearisation ({st['kernel_linearize_count']} timed)")
    # (TLS a second time with the cost rule off, to tell an early stop on that rule from a run
    # that ends with every candidate rejected)
    for loss, kw, tag in (("gm", {}, "GNC-GM"), ("tls", {}, "GNC-TLS"),
                          ("tls", {"relative_cost_tol": 0.0}, "GNC-TLS, relative_cost_tol 0")):
        pg.restore_values()
        pg.optimize_gnc(candidates=lc, loss=loss, keep_weights=0, **kw)        # warm-up
        pg.restore_values()
        s = pg.optimize_gnc(candidates=lc, loss=loss, **kw)
        w = pg.edge_weights()
        tr = pg.gnc_trace()
        sweeps = s["outer_iterations"] + 2
        lines.append(
            f"{tag}: ms_total {s['ms_total']:.1f}, ms_inner {s['ms_inner']:.1f}, ms_weights "
            f"{s['ms_weights']:.2f} ({sweeps} sweeps, {s['ms_weights'] / sweeps:.3f} ms host wall each), outer "
            f"iterations {s['outer_iterations']}, tries {s['inner_tries']}, linearisations {s['linearizations']}, "
            f"stop {s['stop_reason']}, mu {s['mu_initial']:.4g} -> {s['mu_final']:.4g}, cost {s['final_cost']:.6g}, "
            f"r^2 > c^2: {s['outliers']}, rmse {rmse(pg.poses(), g):.3f} m; weights: replaced max "
            f"{w[bad].max():.3g}, true min {w[good].min():.3g}, true below 0.5: {(w[good] < 0.5).sum()}; "
            f"rows {len(tr)}")
        # the robust sweep with the weights kept: device time per linearisation
        r = pg.optimize(profile_every=1, max_outer=3)
        lines.append(f"  robust linearise with the kept weights: "
                     f"{r['kernel_linearize_ms'] / max(r['kernel_linearize_count'], 1):.4f} ms device per linearisation")
        pg.set_edge_weights(np.ones(g.num_edges))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
