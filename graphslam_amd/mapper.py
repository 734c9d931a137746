"""Occupancy-grid map rendered from keyframe laser scans on the GPU.

The reference keeps every keyframe's ``sensor_msgs/LaserScan`` beside its
optimised pose (``Keyframe.msg``: ``scan``, ``pose_opti``), publishes them on
``/graph/keyframes`` and leaves the overlay to rviz.  ``OccupancyGridMapper``
stores the scans keyed like the graph's vertices and ray-casts them into a
``nav_msgs/OccupancyGrid``-shaped grid (include/pgo.h, "occupancy-grid map") at
poses from the host, or straight from a ``PoseGraph``'s device-resident values
after a solve.  Every render runs in libpgo.so on the GPU (one workgroup per
scan; no CPU fallback).

    pg.optimize()
    mapper.render_graph(pg)          # all scans at the optimised poses
    mapper.to_pgm("map.pgm")         # what map_server / Stage read
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .pose_graph import _EXC, PgoError

PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205   # map_server's trinary image values


def default_params(**kw) -> L.PgoMapParams:
    p = L.PgoMapParams()
    L.lib().pgo_map_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"pgo_map_params has no field {k!r}")
        setattr(p, k, v)
    return p


class OccupancyGridMapper:
    """One pgo_map handle: a grid of ``width`` x ``height`` cells of
    ``resolution`` metres whose cell (0, 0) has its corner at ``origin`` (x, y).
    ``params``: l_occ, l_free, l_min, l_max, clear_no_return."""

    def __init__(self, resolution, origin, width, height, device: int = 0, **params):
        self._L = L.lib()
        self._h = None
        p = default_params(resolution=float(resolution), origin_x=float(origin[0]), origin_y=float(origin[1]),
                           width=int(width), height=int(height), **params)
        self.params = p
        self.resolution, self.origin = p.resolution, (p.origin_x, p.origin_y)
        self.width, self.height = p.width, p.height
        self.stats = None   # of the last render
        self._h = self._L.pgo_map_create(int(device), C.byref(p))
        if not self._h:
            raise PgoError(L.PGO_E_ARG, "pgo_map_create: resolution > 0, width and height >= 1, width * height "
                                        "<= 2^28, l_min <= l_max, all finite")

    @classmethod
    def fit(cls, poses, range_max, resolution=0.05, margin=1.0, device: int = 0, **params):
        """A grid around the poses' bounding box grown by range_max + margin on
        every side."""
        xy = np.asarray(poses, dtype=np.float64).reshape(-1, 3)[:, :2]
        pad = float(range_max) + float(margin)
        lo, hi = xy.min(axis=0) - pad, xy.max(axis=0) + pad
        width, height = (int(np.ceil((hi[k] - lo[k]) / resolution)) for k in (0, 1))
        return cls(resolution, (lo[0], lo[1]), max(width, 1), max(height, 1), device, **params)

    def close(self):
        if self._h:
            self._L.pgo_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise _EXC.get(rc, PgoError)(rc, self._L.pgo_map_last_error(self._h).decode())
        return rc

    @property
    def num_scans(self):
        return int(self._L.pgo_map_num_scans(self._h))

    def add_scan(self, key, ranges, angle_min, angle_increment, range_min, range_max):
        """Store one LaserScan (ranges as float32) under the vertex key."""
        r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(-1)
        self._check(self._L.pgo_map_add_scan(self._h, int(key), len(r), r.ctypes.data_as(C.POINTER(C.c_float)),
                                             float(angle_min), float(angle_increment), float(range_min),
                                             float(range_max)))

    def render(self, poses, first=0, accumulate=False):
        """Render scans [first, first + len(poses)) in insertion order at the
        (x, y, theta) rows of ``poses``; returns the stats."""
        xyt = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        st = L.PgoMapStats()
        rc = self._L.pgo_map_render(self._h, int(first), xyt.shape[0], L.dptr(xyt),
                                    L.PGO_MAP_ACCUMULATE if accumulate else 0, C.byref(st))
        self._check(rc)
        self.stats = st.as_dict()
        return self.stats

    def render_graph(self, pg, accumulate=False):
        """Render every scan at the pose of its key among ``pg``'s current values,
        read on the device."""
        st = L.PgoMapStats()
        rc = self._L.pgo_map_render_graph(self._h, pg._h, L.PGO_MAP_ACCUMULATE if accumulate else 0, C.byref(st))
        self._check(rc)
        self.stats = st.as_dict()
        return self.stats

    def counts(self):
        """(hit, miss): two (height, width) int32 arrays."""
        hit = np.zeros((self.height, self.width), dtype=np.int32)
        miss = np.zeros((self.height, self.width), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self._L.pgo_map_get_counts(self._h, hit.ctypes.data_as(ip), miss.ctypes.data_as(ip)))
        return hit, miss

    def occupancy(self):
        """(height, width) int8: -1 unknown, 0 .. 100 (nav_msgs/OccupancyGrid.data)."""
        out = np.zeros((self.height, self.width), dtype=np.int8)
        self._check(self._L.pgo_map_get_occupancy(self._h, out.ctypes.data_as(C.POINTER(C.c_int8))))
        return out

    def to_pgm(self, path, occupied_thresh=50):
        """Binary P5 as map_server and Stage read it: occupied (a known cell of
        value >= occupied_thresh) 0, free (any other known cell) 254, unknown
        205; the image's first row is the grid's top row, so grid row 0 is at
        the bottom."""
        write_pgm(path, self.occupancy(), occupied_thresh)


def occupancy_to_image(occ, occupied_thresh=50):
    occ = np.asarray(occ)
    img = np.full(occ.shape, PGM_UNKNOWN, dtype=np.uint8)
    img[occ >= 0] = PGM_FREE
    img[occ >= occupied_thresh] = PGM_OCCUPIED
    return img[::-1]


def write_pgm(path, occ, occupied_thresh=50):
    img = occupancy_to_image(occ, occupied_thresh)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def read_pgm(path):
    """The (height, width) uint8 image of a binary P5 file, first row on top."""
    data = open(path, "rb").read()
    fields, pos = [], 0
    while len(fields) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end
    if fields[0] != b"P5" or int(fields[3]) != 255:
        raise ValueError("not a binary 8-bit PGM")
    w, h = int(fields[1]), int(fields[2])
    return np.frombuffer(data, dtype=np.uint8, count=w * h, offset=pos + 1).reshape(h, w)
