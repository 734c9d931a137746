"""Numpy / Python restatement of the occupancy-grid map's contract
(include/pgo.h, "occupancy-grid map from keyframe scans"), written from the
contract and not from the kernel: world -> cell by floor in float64, the beam
classes, the classic all-octant integer Bresenham line, integer hit / miss
counts, one clamp of the log odds at the end.

``line`` is the contract's loop, one cell at a time.  ``render`` runs the same
loop for all beams in lockstep (one numpy step per cell of the longest line);
``render_scalar`` walks beam by beam through ``line`` and pins the lockstep
form in tests/test_map_host.py."""
from collections import namedtuple

import numpy as np

Grid = namedtuple("Grid", "resolution origin_x origin_y width height")
Scan = namedtuple("Scan", "ranges angle_min angle_increment range_min range_max")
LOG_ODDS = dict(l_occ=0.85, l_free=-0.4, l_min=-2.0, l_max=3.5)
GUARD = 2.0 ** 30


def make_scan(ranges, angle_min, angle_increment, range_min, range_max):
    return Scan(np.asarray(ranges, dtype=np.float32), float(angle_min), float(angle_increment), float(range_min),
                float(range_max))


def line(x0, y0, x1, y1):
    """The cells of the line, both ends included: max(dx, dy) + 1 of them."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 > x0 else -1), (1 if y1 > y0 else -1)
    err = dx - dy
    x, y = x0, y0
    out = []
    while True:
        out.append((x, y))
        if (x, y) == (x1, y1):
            return out
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += sy


def _beams(grid, scans, poses, clear_no_return):
    """Per traced beam: sensor cell, end cell, whether it has a return, the real
    cell coordinates of its sensor and end point; and the stats."""
    res, ox, oy = grid.resolution, grid.origin_x, grid.origin_y
    st = dict(scans=len(scans), scans_skipped=0, beams=0, beams_return=0, beams_no_return=0, beams_skipped=0)
    cols = [[] for _ in range(9)]
    sensors = []
    for sc, (x, y, th) in zip(scans, np.asarray(poses, dtype=np.float64).reshape(-1, 3)):
        with np.errstate(all="ignore"):
            cu, cv = (x - ox) / res, (y - oy) / res
            u, v = np.floor(cu), np.floor(cv)
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(th)) or not (abs(u) < GUARD and abs(v) < GUARD):
            st["scans_skipped"] += 1
            continue
        sensors.append((cu, cv))
        r = sc.ranges.astype(np.float64)
        i = np.arange(len(r), dtype=np.float64)
        a = th + (sc.angle_min + i * sc.angle_increment)
        with np.errstate(invalid="ignore"):
            skipped = np.isnan(r) | (r < sc.range_min)
            noret = ~skipped & (r >= sc.range_max)
        ret = ~skipped & ~noret
        st["beams"] += len(r)
        st["beams_return"] += int(ret.sum())
        st["beams_no_return"] += int(noret.sum())
        st["beams_skipped"] += int(skipped.sum())
        traced = ret | (noret & bool(clear_no_return))
        d = np.where(ret, r, sc.range_max)[traced]
        eu = (x + d * np.cos(a[traced]) - ox) / res
        ev = (y + d * np.sin(a[traced]) - oy) / res
        n = int(traced.sum())
        for c, val in zip(cols, (np.full(n, u), np.full(n, v), np.floor(eu), np.floor(ev), ret[traced],
                                 np.full(n, cu), np.full(n, cv), eu, ev)):
            c.append(val)
    cat = [np.concatenate(c) if c else np.zeros(0) for c in cols]
    x0, y0, x1, y1 = (c.astype(np.int64) for c in cat[:4])
    return x0, y0, x1, y1, cat[4].astype(bool), cat[5:], sensors, st


def boundary_distance(grid, scans, poses, clear_no_return=True):
    """The smallest distance, in cells, of any sensor or traced end-point cell
    coordinate to an integer: an exact comparison with another implementation of
    sin / cos is fair only when this is well above the rounding error."""
    *_, real, sensors, _ = _beams(grid, scans, poses, clear_no_return)
    vals = np.concatenate([np.ravel(sensors)] + [np.ravel(r) for r in real[2:]])
    if len(vals) == 0:
        return np.inf
    return float(np.abs(vals - np.rint(vals)).min())


def render(grid, scans, poses, clear_no_return=True, hit=None, miss=None):
    """(hit, miss, stats): int64 (height, width) planes (added to the ones given)."""
    H, W = grid.height, grid.width
    hit = np.zeros((H, W), dtype=np.int64) if hit is None else hit.astype(np.int64)
    miss = np.zeros((H, W), dtype=np.int64) if miss is None else miss.astype(np.int64)
    x0, y0, x1, y1, ret, _, _, st = _beams(grid, scans, poses, clear_no_return)
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.where(x1 > x0, 1, -1), np.where(y1 > y0, 1, -1)
    err = dx - dy
    x, y = x0.copy(), y0.copy()
    idx = np.arange(len(x))
    h, m = hit.reshape(-1), miss.reshape(-1)
    updates = 0
    while len(idx):
        xa, ya = x[idx], y[idx]
        last = (xa == x1[idx]) & (ya == y1[idx])
        inside = (xa >= 0) & (xa < W) & (ya >= 0) & (ya < H)
        is_hit = inside & last & ret[idx]
        is_miss = inside & ~(last & ret[idx])
        cell = ya * W + xa
        h += np.bincount(cell[is_hit], minlength=H * W)
        m += np.bincount(cell[is_miss], minlength=H * W)
        updates += int(inside.sum())
        idx = idx[~last]
        e2 = 2 * err[idx]
        a, b = e2 > -dy[idx], e2 < dx[idx]
        err[idx] += np.where(b, dx[idx], 0) - np.where(a, dy[idx], 0)
        x[idx] += np.where(a, sx[idx], 0)
        y[idx] += np.where(b, sy[idx], 0)
    st["updates_call"] = updates
    st["updates"] = int(hit.sum() + miss.sum())
    st["known_cells"] = int(((hit + miss) > 0).sum())
    return hit, miss, st


def render_scalar(grid, scans, poses, clear_no_return=True):
    """The same planes beam by beam through ``line``."""
    H, W = grid.height, grid.width
    hit, miss = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    x0, y0, x1, y1, ret, _, _, _ = _beams(grid, scans, poses, clear_no_return)
    for b in range(len(x0)):
        cells = line(int(x0[b]), int(y0[b]), int(x1[b]), int(y1[b]))
        for k, (cx, cy) in enumerate(cells):
            if 0 <= cx < W and 0 <= cy < H:
                (hit if (k == len(cells) - 1 and ret[b]) else miss)[cy, cx] += 1
    return hit, miss


def occupancy(hit, miss, l_occ=0.85, l_free=-0.4, l_min=-2.0, l_max=3.5):
    """(int8 grid, unrounded 100 p): -1 where hit + miss == 0."""
    hit, miss = hit.astype(np.float64), miss.astype(np.float64)
    L = np.clip(l_occ * hit + l_free * miss, l_min, l_max)
    raw = 100.0 * (1.0 - 1.0 / (1.0 + np.exp(L)))
    occ = np.where(hit + miss == 0, -1, np.rint(raw)).astype(np.int8)
    return occ, raw


def compare_occupancy(got, hit, miss, **log_odds):
    """The int8 grid against the twin's: cells whose unrounded 100 p lies within
    1e-6 of a half-integer need only be within 1 (exp may differ in the last
    bit), and may be at most 0.1 % of the grid.  Returns the exempt share."""
    occ, raw = occupancy(hit, miss, **log_odds)
    known = (hit + miss) > 0
    frac = raw - np.floor(raw)
    exempt = known & (np.abs(frac - 0.5) <= 1e-6)
    assert np.array_equal(got[~exempt], occ[~exempt])
    assert np.all(np.abs(got[exempt].astype(np.int64) - occ[exempt]) <= 1)
    share = float(exempt.sum()) / got.size
    assert share <= 1e-3, share
    return share


def world_case(noise, count=24, seed=3, world_seed=7, n_beams=360, range_max=10.0):
    """The test world: datasets.laser_world(world_seed) scanned from `count` poses
    drawn from Generator(PCG64(seed)), rejected within 0.3 of a box; the grid is
    220 x 140 cells of 0.1 m from (-1.037, -1.013) -- NOT aligned with the walls,
    so no end point sits on a cell boundary."""
    from graphslam_amd import datasets
    segs, rects = datasets.laser_world(world_seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    poses = []
    while len(poses) < count:
        p = np.array([rng.uniform(1.5, 18.5), rng.uniform(1.5, 10.5), rng.uniform(-np.pi, np.pi)])
        if np.any((p[0] > rects[:, 0] - 0.3) & (p[0] < rects[:, 2] + 0.3) &
                  (p[1] > rects[:, 1] - 0.3) & (p[1] < rects[:, 3] + 0.3)):
            continue
        poses.append(p)
    scans = [make_scan(*datasets.simulate_scan(segs, p, n_beams, range_max, noise, rng if noise > 0 else None))
             for p in poses]
    return Grid(0.1, -1.037, -1.013, 220, 140), scans, np.array(poses), segs, rects
