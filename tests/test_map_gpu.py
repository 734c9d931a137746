"""The occupancy-grid map on the GPU against the numpy twin (tests/map_twin.py):
hit / miss counts exactly, the render's counters, the int8 grid.

An exact comparison is fair only away from rounding boundaries (device and host
sin / cos / exp may differ in the last bit): before any GPU call every case
computes, in the twin, the smallest distance of a sensor or end-point cell
coordinate to an integer and asserts it is >= 1e-9 cells; int8 cells whose
unrounded 100 p lies within 1e-6 of a half-integer need only be within 1, and
may be at most 0.1 % of the grid (map_twin.compare_occupancy)."""
import math

import numpy as np
import pytest

import map_twin as mt
from graphslam_amd import _lib, datasets

pytestmark = pytest.mark.gpu

MIN_BOUNDARY = 1e-9
STAT_KEYS = ("scans", "scans_skipped", "beams", "beams_return", "beams_no_return", "beams_skipped", "updates",
             "known_cells")


@pytest.fixture(scope="module")
def mapper(pgo_lib):
    from graphslam_amd import mapper
    return mapper


@pytest.fixture(scope="module")
def world():
    """Case 7's inputs, shared: the noisy world and the twin's planes of it."""
    grid, scans, poses, _, _ = mt.world_case(0.01)
    dist = mt.boundary_distance(grid, scans, poses)
    hit, miss, st = mt.render(grid, scans, poses)
    for a in (hit, miss):
        a.setflags(write=False)
    return grid, scans, poses, dist, hit, miss, st


def _make(mapper, grid, scans, keys=None, **params):
    m = mapper.OccupancyGridMapper(grid.resolution, (grid.origin_x, grid.origin_y), grid.width, grid.height, 0,
                                   **params)
    for k, sc in enumerate(scans):
        m.add_scan(k if keys is None else keys[k], *sc)
    return m


def _check(mapper, grid, scans, poses, clear=True):
    """Render on the GPU and compare everything with the twin; returns the
    handle, the GPU planes and the twin's stats."""
    dist = mt.boundary_distance(grid, scans, poses, clear)
    assert dist >= MIN_BOUNDARY, dist
    hit, miss, st = mt.render(grid, scans, poses, clear)
    m = _make(mapper, grid, scans, clear_no_return=int(clear))
    got = m.render(poses)
    gh, gm = m.counts()
    assert np.array_equal(gh, hit) and np.array_equal(gm, miss)
    assert {k: got[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}
    share = mt.compare_occupancy(m.occupancy(), hit, miss)
    print(f"boundary distance {dist:.3g} cells, updates {st['updates']}, exempt int8 share {share:.2g}, "
          f"render {got['ms_render']:.3f} ms, finalize {got['ms_finalize']:.3f} ms")
    return m, gh, gm, st


# ---------------------------------------------------------------- 1. directions
def _direction_scans():
    """One single-beam scan from the centre of cell (16, 16) to the centre of
    every cell of a 33 x 33 grid: all octants, slopes, ties and length 0."""
    scans, cells = [], []
    for cy in range(33):
        for cx in range(33):
            dx, dy = cx - 16, cy - 16
            scans.append(mt.make_scan([math.hypot(dx, dy)], math.atan2(dy, dx), 0.0, 0.0, 100.0))
            cells.append((dx, dy))
    return mt.Grid(1.0, 0.0, 0.0, 33, 33), scans, cells


def test_directions_all_in_one_call(mapper):
    grid, scans, _ = _direction_scans()
    poses = np.tile([16.5, 16.5, 0.0], (len(scans), 1))
    _, gh, gm, st = _check(mapper, grid, scans, poses)
    assert np.all(gh == 1) and st["beams_return"] == 1089          # every cell is some beam's end
    assert gm[16, 16] == 1088                                      # every beam but the zero-length one starts here


def test_directions_twelve_alone(mapper):
    grid, scans, cells = _direction_scans()
    chosen = [(7, 3), (3, 7), (-3, 7), (-7, 3), (-7, -3), (-3, -7), (3, -7), (7, -3),      # the eight octants
              (9, 0), (0, -9), (-8, 8), (0, 0)]                                          # two axes, a diagonal, length 0
    m = _make(mapper, grid, scans)
    pose = np.array([[16.5, 16.5, 0.0]])
    for c in chosen:
        k = cells.index(c)
        assert mt.boundary_distance(grid, [scans[k]], pose) >= MIN_BOUNDARY
        hit, miss, st = mt.render(grid, [scans[k]], pose)
        got = m.render(pose, first=k)
        gh, gm = m.counts()
        assert np.array_equal(gh, hit) and np.array_equal(gm, miss), c
        assert got["updates"] == max(abs(c[0]), abs(c[1])) + 1 == st["updates"]
        assert gh[16 + c[1], 16 + c[0]] == 1 and gh.sum() == 1


# ---------------------------------------------------------------- 2. clipping
def test_clipping(mapper):
    grid = mt.Grid(1.0, 0.0, 0.0, 16, 16)
    sensors = [(0.5, 0.5), (15.5, 0.5), (0.5, 15.5), (15.5, 15.5),            # the corner cells
               (-5.5, 7.5), (21.5, 7.5), (7.5, -5.5), (7.5, 21.5),            # outside each side
               (-5.5, -5.5), (21.5, -5.5), (-5.5, 21.5), (21.5, 21.5)]        # outside each diagonal
    lengths = np.array([2.3, 9.7, 40.1, 17.3, 5.9, 29.3, 3.1, 12.7], np.float32)   # wholly outside ... right through
    scans, poses = [], []
    for k, (x, y) in enumerate(sensors):
        scans.append(mt.make_scan(np.tile(lengths, 8), -math.pi + 0.0137, 2 * math.pi / 64, 0.05, 50.0))
        poses.append((x + 0.013 * k, y - 0.017 * k, 0.1 * k))
    # scans skipped whole, between the others: sensor cells at and beyond +-2^30 in x and in y (a host pose
    # must be finite, so the guard is the only way to one); their beams count nowhere
    for k, (x, y) in enumerate([(2.0 ** 30 + 0.5, 7.5), (7.5, -(2.0 ** 30) - 0.5), (-3.0e9, 3.0e9), (1.0e300, 0.5)]):
        scans.insert(3 * k + 1, mt.make_scan(np.tile(lengths, 8), -math.pi + 0.0137, 2 * math.pi / 64, 0.05, 50.0))
        poses.insert(3 * k + 1, (x, y, 0.3))
    # ... and the last cells inside the guard are rendered (wholly outside the grid: nothing to count)
    scans.append(mt.make_scan(np.tile(lengths, 8), -math.pi + 0.0137, 2 * math.pi / 64, 0.05, 50.0))
    poses.append((2.0 ** 30 - 0.5, -(2.0 ** 30) + 1.5, 0.3))       # cells 2^30 - 1 and -(2^30 - 1)
    _, gh, gm, st = _check(mapper, grid, scans, np.array(poses))
    assert st["scans"] == 17 and st["scans_skipped"] == 4
    assert st["beams"] == 13 * 64 and 0 < st["updates"] == int(gh.sum() + gm.sum())
    del scans[-1], poses[-1]
    for k in (3, 2, 1, 0):
        del scans[3 * k + 1], poses[3 * k + 1]
    # the outside sensors alone: beams through the grid from outside leave misses, and no hit cell is a start
    hit, miss, st2 = mt.render(grid, scans[4:], np.array(poses[4:]))
    assert miss.sum() > 0 and st2["updates"] < st["updates"]


# ---------------------------------------------------------------- 3. beam counts
@pytest.mark.parametrize("clear", [0, 1])
def test_beam_counts(mapper, clear, world):
    grid, _, wposes = world[:3]
    segs, _ = datasets.laser_world(7)
    rng = np.random.Generator(np.random.PCG64(11))
    scans, poses = [], []
    for k, n in enumerate((1, 63, 64, 65, 255, 256, 257, 1024, 4096)):
        scans.append(mt.make_scan(*datasets.simulate_scan(segs, wposes[k], n, 10.0, 0.01, rng)))
        poses.append(wposes[k])
    skipped = np.tile(np.array([math.nan, 0.01, -1.0, -math.inf], np.float32), 25)
    scans.append(mt.make_scan(skipped, -math.pi, 2 * math.pi / 100, 0.05, 10.0))      # every beam skipped
    poses.append(wposes[9])
    noret = np.tile(np.array([math.inf, 10.0, 11.0, 3.0e38], np.float32), 25)
    scans.append(mt.make_scan(noret, -math.pi, 2 * math.pi / 100, 0.05, 10.0))        # every beam a no-return
    poses.append(wposes[10])
    scans.append(scans[5])                                                            # skipped whole: cell 1e10
    poses.append(np.array([1.0e9, 0.0, 0.0]))
    _, gh, gm, st = _check(mapper, grid, scans, np.array(poses), bool(clear))
    assert st["scans_skipped"] == 1                                                   # ... and its 256 beams count nowhere
    assert st["beams"] == 1 + 63 + 64 + 65 + 255 + 256 + 257 + 1024 + 4096 + 200
    assert st["beams_skipped"] == 100 and st["beams_no_return"] >= 100
    # alone, the two special scans: nothing at all / misses only (or nothing without clear_no_return)
    m = _make(mapper, grid, scans, clear_no_return=clear)
    got = m.render(np.array(poses[9:10]), first=9)
    assert got["updates"] == 0 and got["known_cells"] == 0 and got["beams_skipped"] == 100
    assert np.all(m.occupancy() == -1)
    got = m.render(np.array(poses[10:11]), first=10)
    gh, gm = m.counts()
    assert gh.sum() == 0 and got["beams_no_return"] == 100 and (gm.sum() > 0) == bool(clear)
    assert got["updates"] == mt.render(grid, scans[10:11], poses[10:11], bool(clear))[2]["updates"]


# ---------------------------------------------------------------- 4. window edges
def test_window_edges(mapper, pgo_lib):
    W = pgo_lib.pgo_debug_map_window()
    half = W // 2
    G = 2 * W + 9
    grid = mt.Grid(1.0, 0.0, 0.0, G, G)
    # sensor cells whose window each grid border clips, alone and in pairs, and one whose window is whole
    cells = [(2, G // 2), (G - 3, G // 2), (G // 2, 2), (G // 2, G - 3), (1, 1), (G - 2, 1), (1, G - 2), (G - 2, G - 2),
             (G // 2, G // 2)]
    # beams along +x, +y, -x, -y: the window holds cells c - half .. c + half - 1, so ends at distance half - 1 / half
    # (+) and half / half + 1 (-) are its last cell and the first beyond; one cell longer puts a MISS there
    scans, poses = [], []
    for cx, cy in cells:
        for r in range(max(half - 2, 0), half + 4):
            scans.append(mt.make_scan([r, r, r, r], 0.0, math.pi / 2, 0.0, 1000.0))
            poses.append((cx + 0.5, cy + 0.5, 0.0))
        # and a sweep that crosses the window's edge in every direction, corners included
        scans.append(mt.make_scan(np.full(180, W + 2.5, np.float32), 0.003, 2 * math.pi / 180, 0.0, 1000.0))
        poses.append((cx + 0.37, cy + 0.61, 0.2))
    _, gh, gm, st = _check(mapper, grid, scans, np.array(poses))
    cx = cy = G // 2
    assert gh[cy, cx + half - 1] >= 1 and gh[cy, cx + half] >= 1 and gh[cy, cx - half] >= 1 and gh[cy, cx - half - 1] >= 1
    assert gm[cy, cx + half - 1] >= 1 and gm[cy, cx + half] >= 1 and gm[cy + half, cx] >= 1 and gm[cy - half - 1, cx] >= 1


# ---------------------------------------------------------------- 5. contention
def test_contention_same_pose(mapper, world):
    grid, scans, poses = world[:3]
    one = [scans[0]]
    assert mt.boundary_distance(grid, one, poses[:1]) >= MIN_BOUNDARY
    hit, miss, _ = mt.render(grid, one, poses[:1])
    m = _make(mapper, grid, [scans[0]] * 256)
    got = m.render(np.tile(poses[0], (256, 1)))
    gh, gm = m.counts()
    assert np.array_equal(gh, 256 * hit) and np.array_equal(gm, 256 * miss)
    assert got["updates"] == 256 * int(hit.sum() + miss.sum()) and gm.max() == 256 * 360
    m.render(poses[:1])
    h1, m1 = m.counts()
    assert np.array_equal(gh, 256 * h1) and np.array_equal(gm, 256 * m1)


def test_contention_subcell_offsets(mapper, world):
    grid, scans, poses = world[:3]
    rng = np.random.Generator(np.random.PCG64(5))
    p = np.tile(poses[0], (256, 1))
    p[:, :2] += rng.uniform(-0.35, 0.35, size=(256, 2)) * grid.resolution * 2      # a 3 x 3 block of sensor cells at most
    _check(mapper, grid, [scans[0]] * 256, p)


# ---------------------------------------------------------------- 6. state
def test_state(mapper, world):
    grid, scans, poses, dist, hit, miss, _ = world
    assert dist >= MIN_BOUNDARY
    n = len(scans)
    m = _make(mapper, grid, scans)
    m.render(poses)
    a = m.counts()
    occ_a = m.occupancy()
    m.render(poses)
    b = m.counts()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(occ_a, m.occupancy())
    assert np.array_equal(a[0], hit) and np.array_equal(a[1], miss)
    # render A (the first half) then B (the second) equals a fresh B
    m.render(poses[:n // 2])
    st_b = m.render(poses[n // 2:], first=n // 2)
    hb, mb = m.counts()
    fresh = _make(mapper, grid, scans)
    st_f = fresh.render(poses[n // 2:], first=n // 2)
    hf, mf = fresh.counts()
    assert np.array_equal(hb, hf) and np.array_equal(mb, mf) and st_b["updates"] == st_f["updates"]
    assert np.array_equal(m.occupancy(), fresh.occupancy())
    # the first half, then the second accumulated, equals the whole
    m.render(poses[:n // 2])
    st_acc = m.render(poses[n // 2:], first=n // 2, accumulate=True)
    hw, mw = m.counts()
    assert np.array_equal(hw, hit) and np.array_equal(mw, miss)
    assert st_acc["updates"] == int(hit.sum() + miss.sum()) and np.array_equal(m.occupancy(), occ_a)
    # a handle with the scans inserted in reverse
    rev = _make(mapper, grid, scans[::-1], keys=list(range(n))[::-1])
    rev.render(poses[::-1])
    hr, mr = rev.counts()
    assert np.array_equal(hr, hit) and np.array_equal(mr, miss) and np.array_equal(rev.occupancy(), occ_a)
    # a fresh handle reads as an empty map, and accumulating onto it is a plain render
    empty = _make(mapper, grid, scans)
    assert np.all(empty.occupancy() == -1) and empty.counts()[0].sum() == 0
    empty.render(poses, accumulate=True)
    assert np.array_equal(empty.counts()[1], miss)


# ---------------------------------------------------------------- 7. world
def test_world(mapper, world):
    grid, scans, poses, dist, hit, miss, st = world
    print(f"case 7: smallest cell-coordinate distance to an integer {dist:.3g}")
    _, raw = mt.occupancy(hit, miss)
    frac = (raw - np.floor(raw))[(hit + miss) > 0]
    print(f"case 7: smallest distance of 100 p to a half-integer {np.abs(frac - 0.5).min():.3g}")
    _check(mapper, grid, scans, poses)
    assert st["scans"] == 24 and st["beams"] == 24 * 360


# ---------------------------------------------------------------- 8. graph path
def test_graph_path(mapper, world):
    from graphslam_amd.pose_graph import PoseGraph, ValuesKeyDoesNotExist
    grid, scans, poses, dist, hit, miss, _ = world
    assert dist >= MIN_BOUNDARY
    keys = np.arange(100, 124, dtype=np.uint64)
    pg = PoseGraph(device=0)
    pg.add_vertices(keys[::-1].copy(), poses[::-1].copy())     # the graph's order is not the map's
    cov = np.diag([0.01, 0.01, 0.001])
    pg.add_prior(keys[0], poses[0], cov)
    pg.add_edges(keys[:-1], keys[1:], [datasets.between_xyt(poses[k], poses[k + 1]) for k in range(23)], cov)
    m = _make(mapper, grid, scans, keys=[int(k) for k in keys])
    st_g = m.render_graph(pg)
    hg, mg = m.counts()
    occ_g = m.occupancy()
    st_h = m.render(pg.poses(keys))
    hh, mh = m.counts()
    assert np.array_equal(hg, hh) and np.array_equal(mg, mh) and np.array_equal(occ_g, m.occupancy())
    assert {k: st_g[k] for k in STAT_KEYS} == {k: st_h[k] for k in STAT_KEYS}
    assert np.array_equal(hg, hit) and np.array_equal(mg, miss)
    # moved poses: the device values follow set_poses
    moved = poses + np.array([0.0213, -0.0171, 0.05])
    assert mt.boundary_distance(grid, scans, moved) >= MIN_BOUNDARY
    pg.set_poses(moved, keys)
    m.render_graph(pg)
    hg2, mg2 = m.counts()
    m.render(pg.poses(keys))
    hh2, mh2 = m.counts()
    assert np.array_equal(hg2, hh2) and np.array_equal(mg2, mh2) and not np.array_equal(hg2, hg)
    h2, m2, _ = mt.render(grid, scans, moved)
    assert np.array_equal(hg2, h2) and np.array_equal(mg2, m2)
    # accumulate through the graph path
    m.render_graph(pg, accumulate=True)
    assert np.array_equal(m.counts()[1], 2 * mg2)
    # a scan key that is no vertex
    m.add_scan(999, *scans[0])
    with pytest.raises(ValuesKeyDoesNotExist) as ei:
        m.render_graph(pg)
    assert ei.value.status == _lib.PGO_E_NO_KEY
    assert np.array_equal(m.counts()[1], 2 * mg2)               # the planes are untouched
