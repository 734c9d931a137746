"""Update-matrix tiles formed by their first Schur update (PGO_FUSE_UPDATE).

A 64x64 tile of a blocked front's update matrix whose column block starts at
or past w rounded up to 64 holds no H entry, only what the front's children
extend-add into it.  Where its first Schur update is a 64-tile task, that task
gathers the children's rectangles itself and the tile has no assembly task
(pgo_chol.h syrk_gather, pgo_schedule.cpp fuse_level, pgo_chol.hip
syrk_lds_body).  Every element is the same sum in the same order, so the knob
changes no bit of any result.

The cases of tests/front_shapes.py reach fused tiles without a child
rectangle only (sep60_10x3: w = 30 under m = 210; in the nested case the
leaves land in pivot columns).  ``three_level`` adds graphs whose leaves are
fully connected to the last t poses of their mid clique and to a slice of the
top separator, so their update rows land in the mid front's update-matrix
columns.  Nested dissection and supernode relaxation decide the fronts; the
sizes below were tuned on the host plan and the CPU tests assert what the
plan has:

  tl25_30x2_3x18   fronts (45, 165) and (63, 138): fused tiles with child
                   rectangles, one with more than 16 of them (two gather
                   passes), tiles clipped by the front's edge (m = 165, 138)
  tl20_88x2_3x3    front (264, 324): w > 256, so its update matrix gets the
                   first 256-column block's update fused (k0 = 0, at the block
                   end) and the last panel's as a plain read-modify-write

The expected count of fused tiles is stated from the fronts alone: a blocked
front of (w, m) has T (T + 1) / 2 of them, T = ceil(m / 64) - ceil(w / 64)
(no case here is large enough for a 128-tile step, and none is distributed).
A clique has no update matrix, so its count is 0 with the knob on or off;
the count is positive on every case with a blocked front whose update matrix
reaches past w rounded up to 64.

The tolerance of the longdouble test is the one of tests/test_front_shapes.py
(8 x the yardstick of float64 CPU solves against a np.longdouble Cholesky),
from the same functions, applied to the new graphs.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import front_shapes as fs
from graphslam_amd import datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (1e-5, 100.0)
BLOCKED = [c.name for c in fs.BLOCKED_CASES]


def three_level(a, b, G, c, H, t, s0, s1, seed=4):
    """A separator clique of a poses, G mid cliques of b poses fully connected
    to it, and per mid H leaf cliques of c poses, each fully connected to the
    mid's last t poses and to the separator's poses [s0, s1)."""
    sep = range(a)
    pairs = fs._all_pairs(sep)
    n = a
    mids = []
    for _ in range(G):
        mid = range(n, n + b)
        n += b
        pairs += fs._all_pairs(mid) + fs._cross(sep, mid)
        mids.append(mid)
    for mid in mids:
        for _ in range(H):
            leaf = range(n, n + c)
            n += c
            pairs += fs._all_pairs(leaf) + fs._cross(mid[b - t:], leaf) + fs._cross(range(s0, s1), leaf)
    g = datasets.noise_free(fs._ground_truth(n, seed), pairs, name=f"tl{a}_{b}x{G}_{c}x{H}")
    g.meta["groups"] = []
    return g


NEW = {"tl25_30x2_3x18": (25, 30, 2, 3, 18, 15, 14, 20),
       "tl20_88x2_3x3": (20, 88, 2, 3, 3, 4, 17, 20)}
NEW_FRONTS = {"tl25_30x2_3x18": ((45, 165), (63, 138)), "tl20_88x2_3x3": ((264, 324),)}
PLAN_CASES = BLOCKED + list(NEW) + ["C2"]


@functools.lru_cache(maxsize=None)
def build(name):
    if name in NEW:
        return three_level(*NEW[name])
    return datasets.make(name) if name == "C2" else fs.build(name)


@pytest.fixture(scope="module")
def pg_cls(pgo_lib):
    from graphslam_amd.pose_graph import PoseGraph
    return PoseGraph


def expected_fused(fronts):
    n = 0
    for w, m in fronts:
        if fs.front_class(w, m) == "blocked":
            T = (m + 63) // 64 - (w + 63) // 64
            n += T * (T + 1) // 2 if T > 0 else 0
    return n


def _plan(pg_cls, name):
    pg = pg_cls.from_dataset(build(name))
    w, m, lv = pg.debug_fronts()
    return pg.debug_plan(), [(int(a), int(b)) for a, b in zip(w, m)], lv


# ------------------------------------------------------------------ CPU: the plan
@pytest.mark.parametrize("name", PLAN_CASES)
def test_knob_sets_fused_tiles(pg_cls, monkeypatch, name):
    """fused_tiles is what the fronts say by default and 0 under
    PGO_FUSE_UPDATE=0 (read at every plan); the fronts and the Schur tiles are
    the same either way."""
    monkeypatch.delenv("PGO_FUSE_UPDATE", raising=False)
    on, fronts, lv = _plan(pg_cls, name)
    want = expected_fused(fronts)
    print(f"fused_update {name}: {int(on['fused_tiles'])} fused tiles, {int(on['fused_with_children'])} with children, "
          f"{int(on['fused_multipass'])} multi-pass, {int(on['fused_edge'])} at the edge; expected {want}")
    assert on["fused_tiles"] == want
    if any(fs.front_class(w, m) == "blocked" and m > (w + 63) // 64 * 64 for w, m in fronts):
        assert on["fused_tiles"] > 0
    if name == "C2" or name in NEW:
        assert on["fused_tiles"] > 0 and on["fused_with_children"] > 0
    monkeypatch.setenv("PGO_FUSE_UPDATE", "0")
    off, fronts_off, lv_off = _plan(pg_cls, name)
    assert off["fused_tiles"] == 0 and off["fused_with_children"] == 0
    assert off["fused_multipass"] == 0 and off["fused_edge"] == 0
    assert fronts_off == fronts and np.array_equal(lv, lv_off)
    for k in ("supernodes", "levels", "syrk_tiles", "trsm_tasks", "launches_factor", "syrk_flops"):
        assert on[k] == off[k], k
    assert np.array_equal(on["levels_table"], off["levels_table"])


def test_new_cases_reach_the_designed_tiles(pg_cls, monkeypatch):
    """(a) a fused tile with a child rectangle, (b) one with more than 16 (two
    gather passes), (c) one clipped by the front's edge, (d) a front of more
    than 256 pivot columns whose update matrix is fused at its first update."""
    monkeypatch.delenv("PGO_FUSE_UPDATE", raising=False)
    p, fronts, _ = _plan(pg_cls, "tl25_30x2_3x18")
    for wm in NEW_FRONTS["tl25_30x2_3x18"]:
        assert wm in fronts, (wm, fronts)
    assert p["fused_with_children"] >= 1                                   # (a)
    assert p["fused_multipass"] >= 1                                       # (b)
    assert p["fused_edge"] >= 1 and any(m % 64 for w, m in fronts if fs.front_class(w, m) == "blocked")   # (c)
    p, fronts, _ = _plan(pg_cls, "tl20_88x2_3x3")
    assert (264, 324) in fronts, fronts
    wide = [(w, m) for w, m in fronts if w > fs.K_KB and m > (w + 63) // 64 * 64]
    assert wide == [(264, 324)]
    # (d) the only front with an update matrix past its pivot blocks is the wide
    # one: the fused tile (with its children's rectangles) is its tile (5, 5),
    # first updated at the end of the first 256-column block, again by the last panel
    assert expected_fused(fronts) == expected_fused(wide) == 1
    assert p["fused_tiles"] == 1 and p["fused_with_children"] == 1 and p["fused_edge"] == 1


# ------------------------------------------------------------------ GPU
# One fresh process per knob setting (the pattern of _knob_run in
# tests/test_front_shapes.py): every blocked front-shape case and the new
# cases; on the new cases also one against three lambda lanes and a poisoned
# workspace between two optimizes, graph replay and eager.
_RUN = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_fused_update as tf
from graphslam_amd.pose_graph import PoseGraph, default_params
out = {{}}
for name in {names!r}:
    g = tf.build(name)
    pg = PoseGraph.from_dataset(g)
    st = pg.optimize(default_params(max_outer=2))
    assert st["handoff_retries"] == 0, name
    out[name + "/final"] = np.array([st["final_error"]])
    out[name + "/poses"] = pg.poses()
    for lam in {lambdas!r}:
        out[name + "/solve%g" % lam] = PoseGraph.from_dataset(g).debug_solve(lam, linear_solver=1)[0]
for name in {new!r}:
    g = tf.build(name)
    for lanes in (3, 1):
        pg = PoseGraph.from_dataset(g)
        st = pg.optimize(lambda_lanes=lanes, max_outer=2)
        assert st["handoff_retries"] == 0, name
        out[name + "/lanes%d/trace" % lanes] = pg.trace()[:, :7]
        out[name + "/lanes%d/poses" % lanes] = pg.poses()
    ref = PoseGraph.from_dataset(g)
    st0 = ref.optimize(lambda_lanes=3)
    out[name + "/clean/final"] = np.array([st0["final_error"]])
    out[name + "/clean/poses"] = ref.poses()
    for graphs in (1, 0):
        pg = PoseGraph.from_dataset(g)
        pg.save_values()
        pg.optimize(use_graphs=graphs, lambda_lanes=3, max_outer=2)
        pg.debug_poison_fronts()
        pg.restore_values()
        st = pg.optimize(use_graphs=graphs, lambda_lanes=3)
        assert st["handoff_retries"] == 0, name
        out[name + "/poison%d/final" % graphs] = np.array([st["final_error"]])
        out[name + "/poison%d/poses" % graphs] = pg.poses()
np.savez({path!r}, **out)
"""


def _run(tmp_path_factory, tag, env):
    path = str(tmp_path_factory.mktemp("fused_update") / f"{tag}.npz")
    code = _RUN.format(root=ROOT, tests=os.path.join(ROOT, "tests"), names=BLOCKED + list(NEW), new=list(NEW),
                       lambdas=LAMBDAS, path=path)
    full = {k: v for k, v in os.environ.items() if k != "PGO_FUSE_UPDATE"}
    r = subprocess.run([sys.executable, "-c", code], env=dict(full, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def run_fused(pgo_lib, tmp_path_factory):
    return _run(tmp_path_factory, "fused", {})


@pytest.fixture(scope="module")
def run_plain(pgo_lib, tmp_path_factory):
    return _run(tmp_path_factory, "plain", {"PGO_FUSE_UPDATE": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("name", BLOCKED + list(NEW))
def test_knob_bitwise(run_fused, run_plain, name):
    """Default and PGO_FUSE_UPDATE=0: byte-identical final error, poses and
    debug_solve at both lambdas (each process asserts handoff_retries == 0)."""
    for k in ("/final", "/poses", "/solve%g" % LAMBDAS[0], "/solve%g" % LAMBDAS[1]):
        assert np.isfinite(run_fused[name + k]).all(), k
        assert run_fused[name + k].tobytes() == run_plain[name + k].tobytes(), k


@functools.lru_cache(maxsize=None)
def _solve_reference(name, lam):
    """fs.solve_reference for a graph of this module (it takes case names)."""
    g = build(name)
    H, grad = fs.dense_system(g)
    n = H.shape[0]
    A = H + lam * np.eye(n)
    ref = fs.ld_solve(fs.ld_cholesky(A), -grad)
    y = max(fs.rel_err(s(-grad), ref) for s in fs.yardstick_solvers(A, fs.plan_order(g)).values())
    H2, grad2 = fs.dense_system_c_oracle(g)
    y = max(y, fs.rel_err(fs.ld_solve(fs.ld_cholesky(H2 + lam * np.eye(n)), -grad2), ref))
    ref.setflags(write=False)
    return ref, y, n


@pytest.mark.gpu
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", list(NEW))
def test_new_cases_vs_longdouble(run_fused, name, lam):
    eps = np.finfo(np.longdouble).eps
    if not eps < 2e-19:
        pytest.skip(f"np.longdouble is no extended precision here (eps {eps:.3g}): no reference")
    ref, y, n = _solve_reference(name, lam)
    err = fs.rel_err(run_fused[name + "/solve%g" % lam].ravel(), ref)
    yy = max(y, n * 2.2e-16)
    print(f"fused_update solve {name} lambda {lam:g}: n {n} err {err:.3e} y {y:.3e} err/y {err / yy:.3f}")
    assert err <= fs.bound(y, n), (name, lam, err, y, err / yy)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NEW))
def test_new_cases_lanes_bitwise(run_fused, name):
    """Three lambda lanes are the one-lane trajectory bit for bit."""
    a, b = run_fused[name + "/lanes3/trace"], run_fused[name + "/lanes1/trace"]
    assert a.shape == b.shape and a.shape[0] > 0
    assert a.tobytes() == b.tobytes()
    assert run_fused[name + "/lanes3/poses"].tobytes() == run_fused[name + "/lanes1/poses"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NEW))
def test_new_cases_poisoned_workspace(run_fused, run_plain, name):
    """NaN in everything a factorisation must write before it reads it, between
    two optimizes: the second equals a clean run bit for bit, graph replay and
    eager.  A fused tile the gather did not cover would read the NaN (the class
    of failure that cost round 4 its first factorisation)."""
    for run in (run_fused, run_plain):
        for graphs in (1, 0):
            assert np.isfinite(run[name + "/clean/poses"]).all()
            for k in ("final", "poses"):
                assert run[name + f"/poison{graphs}/{k}"].tobytes() == run[name + f"/clean/{k}"].tobytes(), (graphs, k)
    assert run_fused[name + "/clean/poses"].tobytes() == run_plain[name + "/clean/poses"].tobytes()
