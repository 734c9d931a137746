#!/usr/bin/env python3
"""Plan digests of the planner's whole case set, one line per case (host only).

Two routes, every knob set in a fresh process (some knobs are read once per
process, and so is the planner's pool size):

* `host_selftest --digest` (graphslam_amd/csrc/host_selftest.cpp): its
  built-in graphs, ND and AMD, 1 / 2 / 4 / 8 ranks (every rank), a plan after
  chol_append -- under each set of the planner's knobs below;
* PoseGraph.debug_plan_digest: the designed front-shape graphs
  (tests/front_shapes.py CASES), C1, C2, C3 and C5, 1 / 2 / 4 / 8 ranks, under
  the default knobs and two more.

A line is `<knobs>:<case> <section digests> | <branch counters>`; the columns
are named by the header line.  Two builds schedule alike exactly when their
files are equal:

    python scripts/plan_digests.py --selftest BIN [--lib LIBPGO] --out FILE

--summary writes one line per knob set and route instead (what profiles/ keeps
of an A/B): the cases, a SHA-256 over their lines, and per branch counter the
cases that reached it / its sum.  Equal summaries: equal files.
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SELFTEST_KNOBS = [
    {}, {"PGO_BIGTILE_MIN": "1"}, {"PGO_LOOKAHEAD_M": "129"}, {"PGO_FAR": "1"},
    {"PGO_FAR": "1", "PGO_LOOKAHEAD_M": "129"}, {"PGO_FAR": "1", "PGO_BIGTILE_MIN": "1"}, {"PGO_NO_LOOKAHEAD": "1"},
    {"PGO_FUSE_UPDATE": "0"}, {"PGO_DIST_TOP": "0"}, {"PGO_ASM_XCD": "2"}, {"PGO_PLAN_THREADS": "1"},
]
PYTHON_KNOBS = [{}, {"PGO_LOOKAHEAD_M": "129"}, {"PGO_BIGTILE_MIN": "1"}]
KNOB_NAMES = sorted({k for ks in SELFTEST_KNOBS + PYTHON_KNOBS for k in ks})


def label(knobs):
    return ",".join(f"{k[4:]}={v}" for k, v in sorted(knobs.items())) or "default"


def summary(lines):
    """Header, then per (knob set, route) in order of appearance: cases, hash of their lines, counters."""
    groups = {}
    names = lines[0].split(" | ")[1] if lines[0].startswith("#") else "branch counters"   # (no header: no self-test run)
    for ln in lines[lines[0].startswith("#"):]:
        knobs, case = ln.split(" ", 1)[0].split(":", 1)
        route = "selftest" if case.count("/") == 2 or case.startswith("append") else "python"
        groups.setdefault(f"{knobs}:{route}", []).append(ln.split(":", 1)[1])   # (hashed without the knobs' label)
    out = ["# knobs:route cases sha256 | " + names]
    for key, g in groups.items():
        br = [[int(v) for v in ln.split(" | ")[1].split()] for ln in g]
        cols = " ".join(f"{sum(v > 0 for v in c)}/{sum(c)}" for c in zip(*br))
        out.append(f"{key} {len(g)} {hashlib.sha256(chr(10).join(g).encode()).hexdigest()[:16]} | {cols}")
    return out


def python_cases(names, sizes, skip):
    """The child: digests of the named graphs under this process's knobs."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import front_shapes as fs
    from graphslam_amd import datasets
    from graphslam_amd.pose_graph import PoseGraph
    for name in names or [c.name for c in fs.CASES] + ["C1", "C2", "C3", "C5"]:
        if name in skip:
            continue
        pg = PoseGraph.from_dataset(datasets.make(name) if name in datasets.CONFIGS else fs.build(name))
        for size in sizes:
            for rank in range(size):
                d, br = pg.debug_plan_digest(size, rank)
                print(f"{name}/{size}r{rank}", *(f"{v:016x}" for v in d), "|", *br, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--selftest", help="host_selftest binary (omit: the Python route only)")
    ap.add_argument("--lib", help="libpgo.so of the Python route (default: the tree's)")
    ap.add_argument("--out", help="file to write (default: stdout)")
    ap.add_argument("--summary", action="store_true", help="one line per knob set and route")
    ap.add_argument("--from", dest="src", help="summarise this file of case lines instead of running anything")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cases", nargs="*", help="Python route: these graphs only")
    ap.add_argument("--skip", nargs="*", default=[], help=argparse.SUPPRESS)
    ap.add_argument("--sizes", nargs="*", type=int, default=[1, 2, 4, 8])
    a = ap.parse_args()
    if a.child:
        return python_cases(a.cases, a.sizes, a.skip)
    base = {k: v for k, v in os.environ.items() if k not in KNOB_NAMES}
    if a.lib:
        base["PGO_LIB_PATH"] = os.path.abspath(a.lib)
    lines = open(a.src).read().splitlines() if a.src else []

    def run(cmd, knobs):
        r = subprocess.run(cmd, env=dict(base, **knobs), capture_output=True, text=True, check=True)
        for ln in r.stdout.splitlines():
            if ln.startswith("#"):
                if not lines:
                    lines.append(ln)
            else:
                lines.append(f"{label(knobs)}:{ln}")

    if a.selftest and not a.src:
        for knobs in SELFTEST_KNOBS:
            run([a.selftest, "--digest"], knobs)
    child = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", *map(str, a.sizes)]
    if a.cases:
        child += ["--cases", *a.cases]
    for knobs in [] if a.src else PYTHON_KNOBS:   # (C5, a million poses: under the default knobs only)
        run(child + (["--skip", "C5"] if knobs else []), knobs)
    text = "\n".join(summary(lines) if a.summary else lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
