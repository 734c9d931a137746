// Occupancy-grid mapping (pgo_map_*): the arithmetic of one laser beam -- the
// world -> cell conversion with its 2^30 guard, the beam classes, the all-octant
// integer Bresenham line, the counts -> occupancy conversion -- and the host-side
// validation, as host + device inlines.  The render and finalize kernels
// (pgo_map.hip) run the code the host tests pin; map_selftest.cpp and
// pgo_debug_map_line drive it without a device.  No HIP types.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pgo.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PGO_MAP_HD __host__ __device__
#else
#define PGO_MAP_HD
#endif

struct pgo_graph;

namespace pgo {

// Side, in cells, of the square near-field window of the miss plane that
// k_map_render keeps in LDS around the sensor cell (chosen by
// measurement).  0 makes every update a global atomic.
constexpr int kMapWindow = 32;
constexpr int kMapMaxBeams = 4096;                  // per scan
constexpr double kMapCellGuard = 1073741824.0;      // 2^30: sensor cells stay below it in magnitude
constexpr double kMapMaxRangeCells = 32768.0;       // range_max / resolution: bounds every beam's loop
constexpr long long kMapMaxCells = 1LL << 28;       // width * height

enum { kMapBeamSkip = 0, kMapBeamReturn = 1, kMapBeamNoReturn = 2 };

PGO_MAP_HD inline bool map_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// floor((w - origin) / resolution), in fp64
PGO_MAP_HD inline double map_cell_coord(double w, double origin, double res) { return floor((w - origin) / res); }

// The sensor's cell.  False: the scan is skipped whole (a non-finite pose, or a
// cell coordinate of magnitude >= 2^30), so that all cell arithmetic of the
// scans that are rendered stays in int32.
PGO_MAP_HD inline bool map_sensor_cell(double x, double y, double th, double ox, double oy, double res, int* cx,
                                       int* cy) {
  if (!map_finite(x) || !map_finite(y) || !map_finite(th)) return false;
  const double u = map_cell_coord(x, ox, res), v = map_cell_coord(y, oy, res);
  if (!(fabs(u) < kMapCellGuard) || !(fabs(v) < kMapCellGuard)) return false;
  *cx = (int)u;
  *cy = (int)v;
  return true;
}

// NaN or r < range_min: skipped; r >= range_max (+inf included): no return
PGO_MAP_HD inline int map_beam_class(double r, double range_min, double range_max) {
  if (r != r || r < range_min) return kMapBeamSkip;
  return r >= range_max ? kMapBeamNoReturn : kMapBeamReturn;
}

// The cell of beam i's end point at distance d along a = th + (angle_min + i
// angle_increment) from a sensor whose cell passed map_sensor_cell.  With d <=
// range_max <= 32768 cells the end cell is within 32770 cells of the sensor's.
// False (never with validated scans): the end point is not finite.
PGO_MAP_HD inline bool map_end_cell(double x, double y, double th, double angle_min, double angle_inc, int i, double d,
                                    double ox, double oy, double res, int* ex, int* ey) {
  const double a = th + (angle_min + i * angle_inc);
  const double u = map_cell_coord(x + d * cos(a), ox, res), v = map_cell_coord(y + d * sin(a), oy, res);
  if (!(fabs(u) < 2.0 * kMapCellGuard - 1.0) || !(fabs(v) < 2.0 * kMapCellGuard - 1.0)) return false;
  *ex = (int)u;
  *ey = (int)v;
  return true;
}

// The classic all-octant integer Bresenham line from (x0, y0) to (x1, y1):
// max(dx, dy) + 1 cells, both ends included.
struct MapLine {
  int x, y, x1, y1, dx, dy, sx, sy, err;
};
PGO_MAP_HD inline void map_line_begin(MapLine& l, int x0, int y0, int x1, int y1) {
  l.x = x0;
  l.y = y0;
  l.x1 = x1;
  l.y1 = y1;
  l.dx = x1 > x0 ? x1 - x0 : x0 - x1;
  l.dy = y1 > y0 ? y1 - y0 : y0 - y1;
  l.sx = x1 > x0 ? 1 : -1;
  l.sy = y1 > y0 ? 1 : -1;
  l.err = l.dx - l.dy;
}
PGO_MAP_HD inline bool map_line_last(const MapLine& l) { return l.x == l.x1 && l.y == l.y1; }
PGO_MAP_HD inline void map_line_step(MapLine& l) {
  const int e2 = 2 * l.err;
  if (e2 > -l.dy) {
    l.err -= l.dy;
    l.x += l.sx;
  }
  if (e2 < l.dx) {
    l.err += l.dx;
    l.y += l.sy;
  }
}

// One traced beam: visit(x, y, hit) for every cell of the line, hit only on the
// last cell of a beam with a return (every other visit is a miss).
template <class Visit>
PGO_MAP_HD inline void map_trace(int x0, int y0, int x1, int y1, bool is_return, Visit&& visit) {
  MapLine l;
  map_line_begin(l, x0, y0, x1, y1);
  for (;;) {
    const bool last = map_line_last(l);
    visit(l.x, l.y, last && is_return);
    if (last) break;
    map_line_step(l);
  }
}

// true: no cell of the line's bounding box lies in the grid (nothing to walk)
PGO_MAP_HD inline bool map_line_misses_grid(int x0, int y0, int x1, int y1, int width, int height) {
  const int xl = x0 < x1 ? x0 : x1, xh = x0 < x1 ? x1 : x0, yl = y0 < y1 ? y0 : y1, yh = y0 < y1 ? y1 : y0;
  return xh < 0 || xl >= width || yh < 0 || yl >= height;
}

// counts -> occupancy: -1 unknown, else rint(100 p) of the log odds clamped once
PGO_MAP_HD inline int map_occupancy(int hit, int miss, double l_occ, double l_free, double l_min, double l_max) {
  if ((long long)hit + miss == 0) return -1;
  double L = l_occ * hit + l_free * miss;
  L = L < l_min ? l_min : (L > l_max ? l_max : L);
  const double p = 1.0 - 1.0 / (1.0 + exp(L));
  return (int)rint(100.0 * p);
}

// ---- host-side validation (before any device work)
inline void map_default_params(pgo_map_params& p) {
  p.resolution = 0.05;
  p.origin_x = p.origin_y = 0.0;
  p.width = p.height = 0;
  p.l_occ = 0.85;
  p.l_free = -0.4;
  p.l_min = -2.0;
  p.l_max = 3.5;
  p.clear_no_return = 1;
}

// resolution finite and > 0, a finite origin, width and height >= 1 with width *
// height <= 2^28, finite log odds with l_min <= l_max
inline bool map_params_ok(const pgo_map_params& p) {
  if (!map_finite(p.resolution) || !(p.resolution > 0.0) || !map_finite(p.origin_x) || !map_finite(p.origin_y))
    return false;
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > kMapMaxCells) return false;
  if (!map_finite(p.l_occ) || !map_finite(p.l_free) || !map_finite(p.l_min) || !map_finite(p.l_max)) return false;
  return p.l_min <= p.l_max;
}

// n in 1..4096, 0 <= range_min < range_max, range_max / resolution <= 32768,
// finite angles (the last beam's included)
inline bool map_scan_ok(int n, const float* ranges, double angle_min, double angle_inc, double range_min,
                        double range_max, double res) {
  if (n < 1 || n > kMapMaxBeams || !ranges) return false;
  if (!(range_min >= 0.0) || !(range_max > range_min) || !(range_max / res <= kMapMaxRangeCells)) return false;
  return map_finite(angle_min) && map_finite(angle_inc) && map_finite(angle_min + (n - 1) * angle_inc);
}

// all scans of a handle hold at most 2^31 - 1 beams (beam offsets are int32)
inline bool map_beams_fit(size_t have, int n) { return have + (size_t)n <= (size_t)INT32_MAX; }

// ---- pgo_map_render_graph's view of a graph (defined in pgo_api.cpp)
// the insertion index of a key, -1 when it is no vertex; host only
long long graph_vertex_index(const pgo_graph* g, uint64_t key);
int graph_device_ordinal(const pgo_graph* g);
// Brings the graph's device values up to date and returns its double4 pose[]
// table (x, y, cos theta, sin theta per vertex, insertion order) and the vertex
// count.  The graph's stream is idle on return.
int graph_device_poses(pgo_graph* g, const void** pose, size_t* n);

}  // namespace pgo
