// Stand-alone host self-test of the occupancy-grid map's inlines (pgo_map.h):
// no device, no handle.  Built with ASan + UBSan by `make asan-map` and run by
// tests/test_map_host.py.  `map_selftest --bench FILE` (make map-bench, -O3)
// times the plain restatement below on a workload file of scripts/map_bench.py.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pgo_map.h"

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      failures++;                                                  \
    }                                                              \
  } while (0)

struct Scan {
  std::vector<float> r;
  double amin, ainc, rmin, rmax;
};

// The contract of include/pgo.h restated in plain C++, no pgo_map.h inline.
static long long render_plain(const pgo_map_params& p, const std::vector<Scan>& scans, const std::vector<double>& xyt,
                              std::vector<int>& hit, std::vector<int>& miss, long long* skipped) {
  long long updates = 0;
  for (size_t s = 0; s < scans.size(); s++) {
    const double x = xyt[3 * s], y = xyt[3 * s + 1], th = xyt[3 * s + 2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(th)) {
      ++*skipped;
      continue;
    }
    const double u = std::floor((x - p.origin_x) / p.resolution), v = std::floor((y - p.origin_y) / p.resolution);
    if (!(std::fabs(u) < 1073741824.0) || !(std::fabs(v) < 1073741824.0)) {
      ++*skipped;
      continue;
    }
    const Scan& sc = scans[s];
    for (size_t i = 0; i < sc.r.size(); i++) {
      const double r = (double)sc.r[i];
      if (std::isnan(r) || r < sc.rmin) continue;
      const bool no_return = r >= sc.rmax;
      if (no_return && !p.clear_no_return) continue;
      const double d = no_return ? sc.rmax : r, a = th + (sc.amin + (double)i * sc.ainc);
      int cx = (int)u, cy = (int)v;
      const int x1 = (int)std::floor((x + d * std::cos(a) - p.origin_x) / p.resolution);
      const int y1 = (int)std::floor((y + d * std::sin(a) - p.origin_y) / p.resolution);
      const int dx = std::abs(x1 - cx), dy = std::abs(y1 - cy), sx = x1 > cx ? 1 : -1, sy = y1 > cy ? 1 : -1;
      int err = dx - dy;
      for (;;) {
        const bool last = cx == x1 && cy == y1;
        if (cx >= 0 && cx < p.width && cy >= 0 && cy < p.height) {
          (last && !no_return ? hit : miss)[(size_t)cy * p.width + cx]++;
          updates++;
        }
        if (last) break;
        const int e2 = 2 * err;
        if (e2 > -dy) {
          err -= dy;
          cx += sx;
        }
        if (e2 < dx) {
          err += dx;
          cy += sy;
        }
      }
    }
  }
  return updates;
}

// The same render as the kernel composes it from the inlines (no window).
static long long render_inlines(const pgo_map_params& p, const std::vector<Scan>& scans, const std::vector<double>& xyt,
                                std::vector<int>& hit, std::vector<int>& miss, long long* skipped) {
  long long updates = 0;
  for (size_t s = 0; s < scans.size(); s++) {
    const double x = xyt[3 * s], y = xyt[3 * s + 1], th = xyt[3 * s + 2];
    int cx, cy;
    if (!pgo::map_sensor_cell(x, y, th, p.origin_x, p.origin_y, p.resolution, &cx, &cy)) {
      ++*skipped;
      continue;
    }
    const Scan& sc = scans[s];
    for (int i = 0; i < (int)sc.r.size(); i++) {
      const double r = (double)sc.r[i];
      const int cls = pgo::map_beam_class(r, sc.rmin, sc.rmax);
      if (cls == pgo::kMapBeamSkip || (cls == pgo::kMapBeamNoReturn && !p.clear_no_return)) continue;
      int ex, ey;
      if (!pgo::map_end_cell(x, y, th, sc.amin, sc.ainc, i, cls == pgo::kMapBeamReturn ? r : sc.rmax, p.origin_x,
                             p.origin_y, p.resolution, &ex, &ey))
        continue;
      if (pgo::map_line_misses_grid(cx, cy, ex, ey, p.width, p.height)) continue;
      pgo::map_trace(cx, cy, ex, ey, cls == pgo::kMapBeamReturn, [&](int px, int py, bool is_hit) {
        if ((unsigned)px >= (unsigned)p.width || (unsigned)py >= (unsigned)p.height) return;
        (is_hit ? hit : miss)[(size_t)py * p.width + px]++;
        updates++;
      });
    }
  }
  return updates;
}

// The workload file: int32 scans, beams per scan, width, height; double
// resolution, origin x, y, angle_min, angle_increment, range_min, range_max;
// the poses; the ranges.  False: short or out of range.
static bool read_workload(std::FILE* f, pgo_map_params& p, std::vector<double>& xyt, std::vector<Scan>& scans) {
  int hd[4];
  double dd[7];
  if (std::fread(hd, sizeof(int), 4, f) != 4 || std::fread(dd, sizeof(double), 7, f) != 7) return false;
  pgo::map_default_params(p);
  p.resolution = dd[0];
  p.origin_x = dd[1];
  p.origin_y = dd[2];
  p.width = hd[2];
  p.height = hd[3];
  if (hd[0] < 1 || hd[0] > (1 << 20) || hd[1] < 1 || hd[1] > pgo::kMapMaxBeams || !pgo::map_params_ok(p)) return false;
  xyt.resize(3 * (size_t)hd[0]);
  if (std::fread(xyt.data(), sizeof(double), xyt.size(), f) != xyt.size()) return false;
  scans.resize(hd[0]);
  for (auto& sc : scans) {
    sc.r.resize(hd[1]);
    sc.amin = dd[3];
    sc.ainc = dd[4];
    sc.rmin = dd[5];
    sc.rmax = dd[6];
    if (!pgo::map_scan_ok(hd[1], sc.r.data(), sc.amin, sc.ainc, sc.rmin, sc.rmax, p.resolution)) return false;
    if (std::fread(sc.r.data(), sizeof(float), sc.r.size(), f) != sc.r.size()) return false;
  }
  return true;
}

static int bench(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 2;
  }
  pgo_map_params p;
  std::vector<double> xyt;
  std::vector<Scan> scans;
  const bool ok = read_workload(f, p, xyt, scans);
  std::fclose(f);
  if (!ok) {
    std::printf("%s is no workload file\n", path);
    return 2;
  }
  const int hd[2] = {(int)scans.size(), (int)scans[0].r.size()};
  const size_t cells = (size_t)p.width * p.height;
  double best = 1e300;
  long long updates = 0;
  for (int rep = 0; rep < 5; rep++) {
    std::vector<int> hit(cells, 0), miss(cells, 0);
    long long skipped = 0;
    const auto t0 = std::chrono::steady_clock::now();
    updates = render_plain(p, scans, xyt, hit, miss, &skipped);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("rep %d: %.3f ms\n", rep, ms);
    if (ms < best) best = ms;
  }
  std::printf("map restatement: %d scans x %d beams, %lld updates, best of 5 %.3f ms, %.3g updates/s\n", hd[0], hd[1],
              updates, best, updates / (best * 1e-3));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--bench") == 0) return bench(argv[2]);
  // ---- the line: every (dx, dy) in [-9, 9]^2 from an offset start
  for (int dx = -9; dx <= 9; dx++)
    for (int dy = -9; dy <= 9; dy++) {
      const int x0 = 3, y0 = -2, x1 = x0 + dx, y1 = y0 + dy;
      std::vector<int> xs, ys, hits;
      pgo::map_trace(x0, y0, x1, y1, true, [&](int x, int y, bool h) {
        xs.push_back(x);
        ys.push_back(y);
        hits.push_back(h);
      });
      const int n = std::max(std::abs(dx), std::abs(dy)) + 1;
      CHECK((int)xs.size() == n);
      CHECK(xs.front() == x0 && ys.front() == y0 && xs.back() == x1 && ys.back() == y1);
      for (int k = 0; k < (int)xs.size(); k++) {
        CHECK(hits[k] == (k + 1 == (int)xs.size()));
        if (k) {   // 8-connected, never standing still, monotone towards the end
          const int ax = xs[k] - xs[k - 1], ay = ys[k] - ys[k - 1];
          CHECK(std::abs(ax) <= 1 && std::abs(ay) <= 1 && (ax || ay));
          CHECK(ax * dx >= 0 && ay * dy >= 0);
        }
        // within half a cell of the true segment along the minor axis
        if (std::abs(dx) >= std::abs(dy) && dx)
          CHECK(std::fabs((ys[k] - y0) - (double)dy * (xs[k] - x0) / dx) <= 0.5 + 1e-12);
        else if (dy)
          CHECK(std::fabs((xs[k] - x0) - (double)dx * (ys[k] - y0) / dy) <= 0.5 + 1e-12);
      }
      std::vector<int> again;
      pgo::map_trace(x0, y0, x1, y1, false, [&](int, int, bool h) { again.push_back(h); });
      CHECK((int)again.size() == n);
      for (int h : again) CHECK(!h);   // a no-return beam has no hit
    }
  {   // ties: a slope of exactly 1/2 steps as the classic loop does
    std::vector<int> ys;
    pgo::map_trace(0, 0, 4, 2, true, [&](int, int y, bool) { ys.push_back(y); });
    const int want[5] = {0, 0, 1, 1, 2};
    CHECK(ys.size() == 5);
    for (int k = 0; k < 5 && k < (int)ys.size(); k++) CHECK(ys[k] == want[k]);
  }
  {   // the longest line a validated scan can give
    int n = 0, lx = 0, ly = 0;
    pgo::map_trace(-7, 5, -7 + 32770, 5 - 32769, true, [&](int x, int y, bool) {
      n++;
      lx = x;
      ly = y;
    });
    CHECK(n == 32771 && lx == -7 + 32770 && ly == 5 - 32769);
  }
  CHECK(pgo::map_line_misses_grid(-5, 3, -1, 3, 10, 10) && pgo::map_line_misses_grid(10, 3, 12, 3, 10, 10));
  CHECK(pgo::map_line_misses_grid(3, -4, 3, -1, 10, 10) && pgo::map_line_misses_grid(3, 10, 3, 12, 10, 10));
  CHECK(!pgo::map_line_misses_grid(-5, 3, 0, 3, 10, 10) && !pgo::map_line_misses_grid(9, 9, 20, 20, 10, 10));
  CHECK(!pgo::map_line_misses_grid(-5, -5, 20, 20, 10, 10));

  // ---- world -> cell and the 2^30 guard
  CHECK(pgo::map_cell_coord(0.0, 0.0, 0.5) == 0.0 && pgo::map_cell_coord(-1e-9, 0.0, 0.5) == -1.0);
  CHECK(pgo::map_cell_coord(0.49, 0.0, 0.5) == 0.0 && pgo::map_cell_coord(0.5, 0.0, 0.5) == 1.0);
  CHECK(pgo::map_cell_coord(-1.2, -1.0, 0.1) == -2.0);
  {
    int cx = 7, cy = 7;
    const double g = 1073741824.0;
    CHECK(pgo::map_sensor_cell(g - 0.5, -(g - 1.0), 0.1, 0.0, 0.0, 1.0, &cx, &cy) && cx == (1 << 30) - 1 &&
          cy == -((1 << 30) - 1));
    CHECK(!pgo::map_sensor_cell(g, 0.0, 0.1, 0.0, 0.0, 1.0, &cx, &cy));
    CHECK(!pgo::map_sensor_cell(0.0, -g - 0.5, 0.1, 0.0, 0.0, 1.0, &cx, &cy));
    CHECK(!pgo::map_sensor_cell(1e300, 0.0, 0.1, 0.0, 0.0, 1e-300, &cx, &cy));   // the quotient overflows
    CHECK(!pgo::map_sensor_cell(NAN, 0.0, 0.0, 0.0, 0.0, 1.0, &cx, &cy));
    CHECK(!pgo::map_sensor_cell(0.0, INFINITY, 0.0, 0.0, 0.0, 1.0, &cx, &cy));
    CHECK(!pgo::map_sensor_cell(0.0, 0.0, -INFINITY, 0.0, 0.0, 1.0, &cx, &cy));
    int ex, ey;   // the farthest end cell from the guard's edge stays in int32
    CHECK(pgo::map_end_cell(g - 0.5, -(g - 1.0), 0.0, 0.0, 0.0, 0, 32768.0, 0.0, 0.0, 1.0, &ex, &ey) &&
          ex == (1 << 30) - 1 + 32768 && ey == -((1 << 30) - 1));
    CHECK(!pgo::map_end_cell(0.0, 0.0, 0.0, 0.0, 0.0, 0, INFINITY, 0.0, 0.0, 1.0, &ex, &ey));
  }

  // ---- beam classes
  CHECK(pgo::map_beam_class(NAN, 0.1, 10.0) == pgo::kMapBeamSkip);
  CHECK(pgo::map_beam_class(0.05, 0.1, 10.0) == pgo::kMapBeamSkip && pgo::map_beam_class(-INFINITY, 0.0, 10.0) == pgo::kMapBeamSkip);
  CHECK(pgo::map_beam_class(0.1, 0.1, 10.0) == pgo::kMapBeamReturn && pgo::map_beam_class(9.99, 0.1, 10.0) == pgo::kMapBeamReturn);
  CHECK(pgo::map_beam_class(10.0, 0.1, 10.0) == pgo::kMapBeamNoReturn && pgo::map_beam_class(INFINITY, 0.1, 10.0) == pgo::kMapBeamNoReturn);

  // ---- occupancy
  pgo_map_params p;
  pgo::map_default_params(p);
  CHECK(p.resolution == 0.05 && p.l_occ == 0.85 && p.l_free == -0.4 && p.l_min == -2.0 && p.l_max == 3.5 && p.clear_no_return == 1);
  CHECK(pgo::map_occupancy(0, 0, p.l_occ, p.l_free, p.l_min, p.l_max) == -1);
  CHECK(pgo::map_occupancy(1, 0, p.l_occ, p.l_free, p.l_min, p.l_max) == 70);     // 1 - 1 / (1 + e^0.85) = 0.7006
  CHECK(pgo::map_occupancy(0, 1, p.l_occ, p.l_free, p.l_min, p.l_max) == 40);     // e^-0.4: 0.4013
  CHECK(pgo::map_occupancy(100, 0, p.l_occ, p.l_free, p.l_min, p.l_max) == 97);   // clamped at 3.5: 0.9707
  CHECK(pgo::map_occupancy(0, 100, p.l_occ, p.l_free, p.l_min, p.l_max) == 12);   // clamped at -2: 0.1192
  CHECK(pgo::map_occupancy(2147483647, 2147483647, p.l_occ, p.l_free, p.l_min, p.l_max) == 97);
  CHECK(pgo::map_occupancy(8, 17, 0.85, -0.4, -2.0, 3.5) == 50);                   // L = 0

  // ---- parameter validation
  p.width = 220;
  p.height = 140;
  CHECK(pgo::map_params_ok(p));
  {
    pgo_map_params q = p;
    q.resolution = 0.0; CHECK(!pgo::map_params_ok(q)); q = p;
    q.resolution = -0.05; CHECK(!pgo::map_params_ok(q)); q = p;
    q.resolution = NAN; CHECK(!pgo::map_params_ok(q)); q = p;
    q.resolution = INFINITY; CHECK(!pgo::map_params_ok(q)); q = p;
    q.origin_x = NAN; CHECK(!pgo::map_params_ok(q)); q = p;
    q.origin_y = -INFINITY; CHECK(!pgo::map_params_ok(q)); q = p;
    q.width = 0; CHECK(!pgo::map_params_ok(q)); q = p;
    q.height = -3; CHECK(!pgo::map_params_ok(q)); q = p;
    q.width = 1 << 14; q.height = (1 << 14) + 1; CHECK(!pgo::map_params_ok(q));
    q.height = 1 << 14; CHECK(pgo::map_params_ok(q)); q = p;
    q.width = 2147483647; q.height = 2147483647; CHECK(!pgo::map_params_ok(q)); q = p;
    q.l_min = 1.0; q.l_max = 0.5; CHECK(!pgo::map_params_ok(q)); q = p;
    q.l_min = q.l_max = 0.0; CHECK(pgo::map_params_ok(q)); q = p;
    q.l_occ = NAN; CHECK(!pgo::map_params_ok(q)); q = p;
    q.l_max = INFINITY; CHECK(!pgo::map_params_ok(q));
  }
  // ---- scan validation
  {
    const float r[4] = {1.f, 2.f, 3.f, 4.f};
    CHECK(pgo::map_scan_ok(4, r, -3.14, 0.01, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(0, r, -3.14, 0.01, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4097, r, -3.14, 0.01, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, nullptr, -3.14, 0.01, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, -0.01, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, 10.0, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, NAN, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, 0.05, NAN, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, 0.05, INFINITY, 0.05));
    CHECK(pgo::map_scan_ok(4, r, -3.14, 0.01, 0.05, 1638.4, 0.05));     // exactly 32768 cells
    CHECK(!pgo::map_scan_ok(4, r, -3.14, 0.01, 0.05, 1638.5, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, NAN, 0.01, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, -3.14, INFINITY, 0.05, 10.0, 0.05));
    CHECK(!pgo::map_scan_ok(4, r, 1e308, 1e308, 0.05, 10.0, 0.05));     // the last beam's angle overflows
  }

  // the total over a handle: 2^31 - 1 beams (too many to store in a test)
  CHECK(pgo::map_beams_fit(0, 4096) && pgo::map_beams_fit(2147483647u - 4096u, 4096));
  CHECK(!pgo::map_beams_fit(2147483647u - 4095u, 4096) && !pgo::map_beams_fit(2147483647u, 1));
  CHECK(pgo::map_beams_fit(2147483646u, 1));

  // ---- a whole render: the plain restatement against the inlines, a grid the
  // scans reach beyond, every beam class, a pose outside, skipped scans
  for (int clear = 0; clear <= 1; clear++) {
    pgo_map_params q;
    pgo::map_default_params(q);
    q.resolution = 0.1;
    q.origin_x = -1.037;
    q.origin_y = -1.013;
    q.width = 97;
    q.height = 61;
    q.clear_no_return = clear;
    unsigned long long lcg = 12345;
    auto rnd = [&]() {
      lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
      return (double)(lcg >> 11) / 9007199254740992.0;
    };
    std::vector<Scan> scans(40);
    std::vector<double> xyt;
    for (size_t s = 0; s < scans.size(); s++) {
      Scan& sc = scans[s];
      const int n = s == 0 ? 1 : (s == 1 ? 4096 : 50 + (int)(rnd() * 400));
      sc.amin = -3.14159265358979323846;
      sc.ainc = 2.0 * 3.14159265358979323846 / n;
      sc.rmin = 0.05;
      sc.rmax = 6.0;
      for (int i = 0; i < n; i++) {
        const double t = rnd();
        sc.r.push_back(t < 0.03 ? NAN : t < 0.06 ? INFINITY : t < 0.09 ? 0.01f : t < 0.15 ? 7.0f : (float)(0.05 + 8.0 * rnd() * rnd()));
      }
      xyt.push_back(-3.0 + 15.0 * rnd());
      xyt.push_back(-3.0 + 11.0 * rnd());
      xyt.push_back(-4.0 + 8.0 * rnd());
    }
    xyt[3 * 5] = NAN;
    xyt[3 * 6 + 1] = 2e8;   // cell 2e9 >= 2^30
    xyt[3 * 7 + 2] = INFINITY;
    const size_t cells = (size_t)q.width * q.height;
    std::vector<int> h0(cells, 0), m0(cells, 0), h1(cells, 0), m1(cells, 0);
    long long s0 = 0, s1 = 0;
    const long long u0 = render_plain(q, scans, xyt, h0, m0, &s0), u1 = render_inlines(q, scans, xyt, h1, m1, &s1);
    CHECK(u0 == u1 && u0 > 10000 && s0 == 3 && s1 == 3);
    CHECK(h0 == h1 && m0 == m1);
    long long sum = 0;
    for (size_t c = 0; c < cells; c++) sum += h0[c] + m0[c];
    CHECK(sum == u0);
  }

  if (failures) {
    std::printf("map_selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("map_selftest: ok\n");
  return 0;
}
