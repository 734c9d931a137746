"""The occupancy-grid map without a GPU: the line inline against the numpy twin
(tests/map_twin.py), every validation status, the PGM round trip, the
stand-alone sanitizer self-test of the inlines, the twin against the world it
maps, the symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import map_twin as mt
from graphslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mapper(pgo_lib):
    from graphslam_amd import mapper
    return mapper


def _status(fn, *a, **kw):
    from graphslam_amd.pose_graph import PgoError
    with pytest.raises(PgoError) as ei:
        fn(*a, **kw)
    return ei.value.status


def _line(L, x0, y0, x1, y1, cap=64):
    xy = (C.c_int * (2 * cap))()
    n = L.pgo_debug_map_line(x0, y0, x1, y1, xy, cap)
    return n, [(xy[2 * k], xy[2 * k + 1]) for k in range(min(n, cap))]


# ------------------------------------------------------------------ the line
def test_line_matches_twin_every_direction(pgo_lib):
    for dx in range(-9, 10):
        for dy in range(-9, 10):
            for x0, y0 in ((0, 0), (-4, 7)):
                n, cells = _line(pgo_lib, x0, y0, x0 + dx, y0 + dy)
                assert n == max(abs(dx), abs(dy)) + 1
                assert cells == mt.line(x0, y0, x0 + dx, y0 + dy), (dx, dy)
    n, cells = _line(pgo_lib, 0, 0, 100, 37, cap=8)     # the count does not stop at cap
    assert n == 101 and cells == mt.line(0, 0, 100, 37)[:8]
    assert pgo_lib.pgo_debug_map_line(0, 0, 5, 5, None, 0) == 6
    W = pgo_lib.pgo_debug_map_window()
    assert W >= 0 and W % 2 == 0


def test_twin_lockstep_equals_scalar_walk():
    grid, scans, poses, _, _ = mt.world_case(0.0, count=3, n_beams=90)
    small = mt.Grid(0.1, 3.0 - 0.037, 2.0 - 0.013, 90, 70)    # the scans reach far beyond it
    for g in (grid, small):
        for clear in (True, False):
            hit, miss, st = mt.render(g, scans, poses, clear)
            h2, m2 = mt.render_scalar(g, scans, poses, clear)
            assert np.array_equal(hit, h2) and np.array_equal(miss, m2)
            assert st["updates"] == hit.sum() + miss.sum() == st["updates_call"]
            assert st["beams"] == st["beams_return"] + st["beams_no_return"] + st["beams_skipped"] == 270


# ------------------------------------------------------------------ validation
def test_create_argument_checks(mapper):
    M = mapper.OccupancyGridMapper
    ok = M(0.05, (0.0, 0.0), 10, 10)
    assert ok.num_scans == 0
    for res in (0.0, -0.05, math.nan, math.inf):
        assert _status(M, res, (0.0, 0.0), 10, 10) == _lib.PGO_E_ARG
    assert _status(M, 0.05, (math.nan, 0.0), 10, 10) == _lib.PGO_E_ARG
    for w, h in ((0, 10), (10, 0), (-1, 10), (1 << 14, (1 << 14) + 1)):
        assert _status(M, 0.05, (0.0, 0.0), w, h) == _lib.PGO_E_ARG
    M(0.05, (0.0, 0.0), 1 << 14, 1 << 14).close()             # 2^28 cells: allowed (no device touched)
    assert _status(M, 0.05, (0.0, 0.0), 10, 10, l_min=1.0, l_max=0.5) == _lib.PGO_E_ARG
    M(0.05, (0.0, 0.0), 10, 10, l_min=0.5, l_max=0.5).close()
    p = mapper.default_params()
    assert (p.resolution, p.l_occ, p.l_free, p.l_min, p.l_max, p.clear_no_return) == (0.05, 0.85, -0.4, -2.0, 3.5, 1)
    assert pgo_lib_null_handles()


def pgo_lib_null_handles():
    L = _lib.lib()
    assert L.pgo_map_create(0, None) is None
    assert L.pgo_map_num_scans(None) == 0
    assert L.pgo_map_add_scan(None, 0, 1, None, 0.0, 0.0, 0.0, 1.0) == _lib.PGO_E_ARG
    assert L.pgo_map_render(None, 0, 0, None, 0, None) == _lib.PGO_E_ARG
    assert L.pgo_map_render_graph(None, None, 0, None) == _lib.PGO_E_ARG
    assert L.pgo_map_get_counts(None, None, None) == _lib.PGO_E_ARG
    assert L.pgo_map_get_occupancy(None, None) == _lib.PGO_E_ARG
    L.pgo_map_destroy(None)
    return True


def test_add_scan_argument_checks(mapper):
    m = mapper.OccupancyGridMapper(0.05, (0.0, 0.0), 10, 10)
    r = np.ones(8, np.float32)
    good = (-math.pi, 0.1, 0.05, 10.0)
    assert _status(m.add_scan, 1, np.zeros(0, np.float32), *good) == _lib.PGO_E_ARG
    assert _status(m.add_scan, 1, np.ones(4097, np.float32), *good) == _lib.PGO_E_ARG
    assert _status(m.add_scan, 1, r, -math.pi, 0.1, -0.01, 10.0) == _lib.PGO_E_ARG      # range_min < 0
    assert _status(m.add_scan, 1, r, -math.pi, 0.1, 10.0, 10.0) == _lib.PGO_E_ARG       # range_max <= range_min
    assert _status(m.add_scan, 1, r, -math.pi, 0.1, 0.05, 1638.5) == _lib.PGO_E_ARG     # > 32768 cells
    assert _status(m.add_scan, 1, r, -math.pi, 0.1, 0.05, math.inf) == _lib.PGO_E_ARG
    assert _status(m.add_scan, 1, r, math.nan, 0.1, 0.05, 10.0) == _lib.PGO_E_ARG
    assert _status(m.add_scan, 1, r, -math.pi, math.inf, 0.05, 10.0) == _lib.PGO_E_ARG
    assert m.num_scans == 0
    m.add_scan(1, r, -math.pi, 0.1, 0.05, 1638.4)                                       # exactly 32768 cells
    m.add_scan(2, np.ones(4096, np.float32), *good)
    m.add_scan(2 ** 64 - 2, np.array([math.nan, math.inf, -1.0], np.float32), *good)    # ranges may be anything
    assert m.num_scans == 3
    assert _status(m.add_scan, 2, r, *good) == _lib.PGO_E_DUP_KEY
    assert m.num_scans == 3
    # render's host-side checks come before any device work
    assert _status(m.render, np.zeros((4, 3))) == _lib.PGO_E_ARG                        # past the stored scans
    assert _status(m.render, np.zeros((1, 3)), first=3) == _lib.PGO_E_ARG
    for bad in (math.nan, math.inf, -math.inf):
        assert _status(m.render, [[0.0, 0.0, 0.0], [0.0, bad, 0.0]]) == _lib.PGO_E_NONFINITE
        assert _status(m.render, [[0.0, 0.0, bad]], first=2) == _lib.PGO_E_NONFINITE


@pytest.mark.parametrize("device", [99, -1])
def test_no_device_only_at_render_or_get(mapper, device):
    """Create and add_scan touch no device; the first render or read reports
    PGO_E_NO_DEVICE: an ordinal that no machine has (with a GPU: out of range;
    without one: no device at all).  The handle stays usable on the host."""
    m = mapper.OccupancyGridMapper(0.1, (0.0, 0.0), 20, 20, device=device)
    m.add_scan(1, np.ones(8, np.float32), -math.pi, 0.1, 0.05, 5.0)
    m.add_scan(2, np.ones(8, np.float32), -math.pi, 0.1, 0.05, 5.0)
    assert m.num_scans == 2
    assert _status(m.render, np.zeros((2, 3))) == _lib.PGO_E_NO_DEVICE
    assert _status(m.render, np.zeros((1, 3)), first=1, accumulate=True) == _lib.PGO_E_NO_DEVICE
    assert _status(m.render, np.zeros((0, 3))) == _lib.PGO_E_NO_DEVICE                  # (a render of no scan clears)
    assert _status(m.counts) == _lib.PGO_E_NO_DEVICE
    assert _status(m.occupancy) == _lib.PGO_E_NO_DEVICE
    assert m.stats is None
    # the host-side checks still come first
    assert _status(m.render, np.zeros((3, 3))) == _lib.PGO_E_ARG
    assert _status(m.render, [[0.0, math.nan, 0.0]]) == _lib.PGO_E_NONFINITE
    assert _status(m.add_scan, 2, np.ones(8, np.float32), -math.pi, 0.1, 0.05, 5.0) == _lib.PGO_E_DUP_KEY
    m.add_scan(3, np.ones(8, np.float32), -math.pi, 0.1, 0.05, 5.0)
    assert m.num_scans == 3
    st = _lib.PgoMapStats()
    assert _lib.lib().pgo_map_render(m._h, 0, 0, None, 0, C.byref(st)) == _lib.PGO_E_NO_DEVICE
    assert st.status == _lib.PGO_E_NO_DEVICE
    m.close()


def test_render_graph_checks_keys_and_device_first(mapper):
    """A scan key that is no vertex -> PGO_E_NO_KEY, a graph on another device ->
    PGO_E_ARG: both before any device work, so they show without a GPU."""
    from graphslam_amd.pose_graph import PoseGraph, ValuesKeyDoesNotExist
    pg = PoseGraph(device=0)
    pg.add_vertex(5, 1.0, 1.0, 0.0)
    m = mapper.OccupancyGridMapper(0.1, (0.0, 0.0), 20, 20)
    m.add_scan(5, np.ones(4, np.float32), 0.0, 0.1, 0.05, 5.0)
    m.add_scan(6, np.ones(4, np.float32), 0.0, 0.1, 0.05, 5.0)
    with pytest.raises(ValuesKeyDoesNotExist) as ei:
        m.render_graph(pg)
    assert ei.value.status == _lib.PGO_E_NO_KEY
    m2 = mapper.OccupancyGridMapper(0.1, (0.0, 0.0), 20, 20, device=1)
    m2.add_scan(5, np.ones(4, np.float32), 0.0, 0.1, 0.05, 5.0)
    assert _status(m2.render_graph, pg) == _lib.PGO_E_ARG


# ------------------------------------------------------------------ PGM
def test_pgm_round_trip(mapper, tmp_path):
    occ = np.full((5, 7), -1, np.int8)
    occ[0, :] = 100          # grid row 0: the bottom wall
    occ[1:4, 1:6] = 12       # free inside
    occ[2, 3] = 50           # the threshold itself is occupied
    occ[3, 3] = 49
    path = tmp_path / "map.pgm"
    mapper.write_pgm(path, occ)
    raw = path.read_bytes()
    assert raw.startswith(b"P5\n7 5\n255\n") and len(raw) == len(b"P5\n7 5\n255\n") + 35
    img = mapper.read_pgm(path)
    assert img.shape == (5, 7) and img.dtype == np.uint8
    assert np.all(img[4] == 0)                          # row 0 is at the bottom of the image
    assert np.all(img[0] == 205)                        # grid row 4: never seen
    assert img[4 - 2, 3] == 0 and img[4 - 3, 3] == 254 and img[4 - 1, 1] == 254 and img[4 - 1, 0] == 205
    back = np.full(occ.shape, -1, np.int8)
    back[img[::-1] == 0] = 100
    back[img[::-1] == 254] = 0
    assert np.array_equal(back == -1, occ == -1) and np.array_equal(back == 100, occ >= 50)
    assert set(np.unique(img)) == {0, 205, 254}


# ------------------------------------------------------------------ the host module under sanitizers
def test_map_inlines_under_asan_ubsan():
    """pgo_map.h driven by map_selftest.cpp under ASan + UBSan: a stand-alone host
    program, nothing preloaded."""
    b = subprocess.run(["make", "-s", "-C", "graphslam_amd/csrc", "asan-map"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "graphslam_amd", "csrc", "build", "map_selftest_asan")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "map_selftest: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ------------------------------------------------------------------ the twin on the world it maps
def _segment_distance(px, py, segs):
    """(n,) distance of every point to the nearest of the (m, 4) segments."""
    a, e = segs[:, :2], segs[:, 2:] - segs[:, :2]
    w = np.stack([px, py], axis=1)[:, None, :] - a[None]
    t = np.clip((w * e[None]).sum(-1) / (e * e).sum(-1)[None], 0.0, 1.0)
    return np.linalg.norm(w - t[..., None] * e[None], axis=-1).min(axis=1)


def test_twin_maps_the_world():
    grid, scans, poses, segs, rects = mt.world_case(0.0)
    assert len(scans) == 24 and mt.boundary_distance(grid, scans, poses) >= 1e-9
    hit, miss, st = mt.render(grid, scans, poses)
    res = grid.resolution
    cx = grid.origin_x + (np.arange(grid.width) + 0.5) * res
    cy = grid.origin_y + (np.arange(grid.height) + 0.5) * res
    X, Y = np.meshgrid(cx, cy)
    # every hit cell's centre within half a cell diagonal of a wall (the end point is in the cell)
    hy, hx = np.nonzero(hit)
    assert len(hx) > 500
    worst = _segment_distance(X[hy, hx], Y[hy, hx], segs).max()
    print(f"worst hit-cell centre to wall distance {worst:.4f} (bound {res * math.sqrt(2) / 2:.4f})")
    assert worst <= res * math.sqrt(2) / 2
    touched = (hit + miss) > 0
    for x0, y0, x1, y1 in rects:    # nothing deeper than one cell inside a box
        deep = (X > x0 + res) & (X < x1 - res) & (Y > y0 + res) & (Y < y1 - res)
        assert deep.any() and not (touched & deep).any()
    outside = (X < -res) | (X > 20.0 + res) | (Y < -res) | (Y > 12.0 + res)
    assert outside.any() and not (touched & outside).any()
    assert st["beams"] == 24 * 360 and st["beams_skipped"] == 0 and st["scans_skipped"] == 0
    assert st["beams_return"] == int(hit.sum()) and st["beams_no_return"] > 0
    # order independence: integer sums, one clamp at the end
    h2, m2, _ = mt.render(grid, scans[::-1], poses[::-1])
    assert np.array_equal(hit, h2) and np.array_equal(miss, m2)
    occ, _ = mt.occupancy(hit, miss)
    assert occ.min() == -1 and set(np.unique(occ[hit > 2 * miss + 1])) <= set(range(51, 101))
    # an origin on the walls' lattice puts end points on cell boundaries: not a fair exact test
    aligned = mt.Grid(0.1, -1.0, -1.0, 220, 140)
    assert mt.boundary_distance(aligned, scans, poses) < 1e-9


def test_symbols_declared_and_bound(pgo_lib):
    names = {"pgo_map_default_params", "pgo_map_create", "pgo_map_destroy", "pgo_map_last_error", "pgo_map_add_scan",
             "pgo_map_num_scans", "pgo_map_render", "pgo_map_render_graph", "pgo_map_get_counts",
             "pgo_map_get_occupancy", "pgo_map_debug_ms", "pgo_debug_map_line", "pgo_debug_map_window"}
    assert names <= set(_lib.declared_symbols())
    assert all(hasattr(pgo_lib, n) for n in names)
    assert _lib.PGO_MAP_ACCUMULATE == 1 and pgo_lib.pgo_abi_version() == 6
