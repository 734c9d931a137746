#!/usr/bin/env python3
"""Occupancy-grid render at a user's size: `--scans` keyframes x
`--beams` beams at `--resolution` m on datasets.laser_world scaled so that the
keyframes fit (the room grows with sqrt(scans), the boxes with it), poses and
scans from a seed.  Prints one JSON line: ms_render / ms_finalize / ms_clear
(device events, warmed, median of --reps), cell updates per second, the clear
and finalize passes' bytes over time, a CRC of the planes (equal across builds
and runs: the sums are integers).

  --workload FILE   load the workload from FILE, or generate and save it there
                    (the file map_selftest --bench reads: the C++ restatement
                    on one core)
  PGO_LIB_PATH      another build of libpgo.so (the A/B of the LDS window)
"""
import argparse
import json
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RANGE_MIN, RANGE_MAX = 0.05, 10.0


def make_workload(scans, beams, resolution, seed):
    from graphslam_amd import datasets
    scale = max(1.0, (scans / 24.0) ** 0.5 / 2.0)          # ~ 10 m^2 of floor per keyframe
    width, height = 20.0 * scale, 12.0 * scale
    segs, rects = datasets.laser_world(7, width, height, boxes=int(6 * scale * scale))
    rng = np.random.Generator(np.random.PCG64(seed))
    poses = []
    while len(poses) < scans:
        p = np.array([rng.uniform(1.5, width - 1.5), rng.uniform(1.5, height - 1.5), rng.uniform(-np.pi, np.pi)])
        if np.any((p[0] > rects[:, 0] - 0.3) & (p[0] < rects[:, 2] + 0.3) &
                  (p[1] > rects[:, 1] - 0.3) & (p[1] < rects[:, 3] + 0.3)):
            continue
        poses.append(p)
    poses = np.array(poses)
    ranges = np.stack([datasets.simulate_scan(segs, p, beams, RANGE_MAX, 0.01, rng)[0] for p in poses])
    ox, oy = -1.037, -1.013
    w, h = int(np.ceil((width + 2.074) / resolution)), int(np.ceil((height + 2.026) / resolution))
    return dict(scans=scans, beams=beams, width=w, height=h, resolution=resolution, origin=(ox, oy),
                angle_min=-np.pi, angle_increment=2 * np.pi / beams, poses=poses, ranges=ranges.astype(np.float32))


def save_workload(path, wl):
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", wl["scans"], wl["beams"], wl["width"], wl["height"]))
        f.write(struct.pack("<7d", wl["resolution"], wl["origin"][0], wl["origin"][1], wl["angle_min"],
                            wl["angle_increment"], RANGE_MIN, RANGE_MAX))
        f.write(np.ascontiguousarray(wl["poses"], dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(wl["ranges"], dtype="<f4").tobytes())


def load_workload(path):
    data = open(path, "rb").read()
    n, b, w, h = struct.unpack_from("<4i", data, 0)
    res, ox, oy, amin, ainc, _, _ = struct.unpack_from("<7d", data, 16)
    poses = np.frombuffer(data, "<f8", 3 * n, 72).reshape(n, 3)
    ranges = np.frombuffer(data, "<f4", n * b, 72 + 24 * n).reshape(n, b)
    return dict(scans=n, beams=b, width=w, height=h, resolution=res, origin=(ox, oy), angle_min=amin,
                angle_increment=ainc, poses=poses, ranges=ranges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4096)
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--generate-only", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.workload and os.path.exists(a.workload):
        wl = load_workload(a.workload)
    else:
        wl = make_workload(a.scans, a.beams, a.resolution, a.seed)
        if a.workload:
            save_workload(a.workload, wl)
    if a.generate_only:
        print(json.dumps({k: wl[k] for k in ("scans", "beams", "width", "height", "resolution")}))
        return
    import ctypes as C

    from graphslam_amd import _lib
    from graphslam_amd.mapper import OccupancyGridMapper
    m = OccupancyGridMapper(wl["resolution"], wl["origin"], wl["width"], wl["height"], 0)
    for k in range(wl["scans"]):
        m.add_scan(k, wl["ranges"][k], wl["angle_min"], wl["angle_increment"], RANGE_MIN, RANGE_MAX)
    rows = []
    clear = C.c_double()
    for rep in range(a.warmup + a.reps):
        st = m.render(wl["poses"])
        _lib.lib().pgo_map_debug_ms(m._h, C.byref(clear))
        if rep >= a.warmup:
            rows.append((st["ms_render"], st["ms_finalize"], clear.value, st["ms_upload"], st["ms_total"]))
    rows = np.array(rows)
    med = np.median(rows, axis=0)
    hit, miss = m.counts()
    cells = wl["width"] * wl["height"]
    out = dict(label=a.label, lib=os.path.basename(_lib.LIB_PATH), window=_lib.lib().pgo_debug_map_window(),
               scans=wl["scans"], beams=wl["beams"], width=wl["width"], height=wl["height"], reps=a.reps,
               ms_render=med[0], ms_render_min=rows[:, 0].min(), ms_render_max=rows[:, 0].max(),
               ms_finalize=med[1], ms_clear=med[2], ms_upload=med[3], ms_total=med[4],
               updates=st["updates"], known_cells=st["known_cells"], beams_return=st["beams_return"],
               beams_no_return=st["beams_no_return"],
               updates_per_s=st["updates"] / (med[0] * 1e-3),
               finalize_TBps=cells * 9 / (med[1] * 1e-3) / 1e12, clear_TBps=cells * 8 / (med[2] * 1e-3) / 1e12,
               crc=zlib.crc32(miss.tobytes(), zlib.crc32(hit.tobytes())))
    print(json.dumps({k: (float(v) if isinstance(v, np.floating) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
