// Occupancy-grid map rendered from keyframe laser scans on the GPU (pgo_map_*).
//
// The reference stores each keyframe's LaserScan beside its optimised pose
// (Keyframe.msg: scan, pose_opti) and leaves the overlay to rviz; this renders
// the scans into the hit / miss count planes of an occupancy grid whenever the
// poses move (after a loop closure: all of them).  The contract -- grid layout,
// beam classes, the Bresenham line, the one final clamp -- is in include/pgo.h;
// its arithmetic is the host + device inlines of pgo_map.h.
//
// MI355X layout.  k_map_render: one workgroup per scan, lanes over beams (a loop
// for scans of more beams than threads).  Every beam of a scan starts in the
// sensor's cell, so the miss updates pile up there and fall off within a few
// cells: the workgroup keeps a kMapWindow-square int32 window of the miss plane
// around the sensor cell in LDS (LDS integer atomics), and flushes it with one
// global no-return integer atomic per non-zero cell; cells beyond the window and
// all hits (end points are spread) go straight to global integer atomics.
// Integer sums: the planes do not depend on arrival order, launch shape or scan
// order.  k_map_clear zeroes the planes, k_map_finalize converts counts to int8
// occupancy and reduces `updates` / `known_cells`, both with 16-byte accesses.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "pgo.h"
#include "pgo_map.h"

namespace pgo {

constexpr int kMapThreads = 256;
constexpr int kMapFinalizeCells = 16;   // cells per thread of k_map_finalize: one 16-byte int8 store

struct MapScan {   // one stored scan, device layout
  double angle_min, angle_inc, range_min, range_max;
  int first, n;    // its beams: ranges[first .. first + n)
};

// device counters of one render
enum { kMapStSkipped = 0, kMapStBeams, kMapStReturn, kMapStNoReturn, kMapStBeamSkipped, kMapStUpdates, kMapStKnown,
       kMapStCount };

struct MapGrid {
  double res, ox, oy;
  int width, height;
};

// pose (x, y, cos, sin) of every scan's vertex -> (x, y, theta) per scan: theta
// as Rot2::theta() forms it (atan2(s, c)), what pgo_get_poses hands the host
__global__ void k_map_gather_poses(const double4* __restrict__ pose, const int* __restrict__ vidx, int n,
                                   double* __restrict__ xyt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double4 p = pose[vidx[i]];
  xyt[3 * i] = p.x;
  xyt[3 * i + 1] = p.y;
  xyt[3 * i + 2] = atan2(p.w, p.z);
}

__global__ __launch_bounds__(256) void k_map_clear(int4* __restrict__ planes, size_t n16) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) planes[i] = make_int4(0, 0, 0, 0);
}

// Block b renders scan first + b at pose xyt[3 b ..].
__global__ __launch_bounds__(kMapThreads) void k_map_render(MapGrid g, const MapScan* __restrict__ scans,
                                                            const float* __restrict__ ranges, int first,
                                                            const double* __restrict__ xyt, int clear_no_return,
                                                            int* __restrict__ hit, int* __restrict__ miss,
                                                            unsigned long long* __restrict__ stats) {
  constexpr int W = kMapWindow;
  __shared__ int win[W * W > 0 ? W * W : 1];
  __shared__ int cnt[3];
  const int tid = threadIdx.x;
  const MapScan sc = scans[first + blockIdx.x];
  const double x = xyt[3 * (size_t)blockIdx.x], y = xyt[3 * (size_t)blockIdx.x + 1], th = xyt[3 * (size_t)blockIdx.x + 2];
  int cx = 0, cy = 0;
  if (!map_sensor_cell(x, y, th, g.ox, g.oy, g.res, &cx, &cy)) {   // (uniform over the workgroup)
    if (tid == 0) atomicAdd(&stats[kMapStSkipped], 1ull);
    return;
  }
  const int wx0 = cx - W / 2, wy0 = cy - W / 2;   // the window's first cell (may lie outside the grid)
  for (int j = tid; j < W * W; j += kMapThreads) win[j] = 0;
  if (tid < 3) cnt[tid] = 0;
  __syncthreads();
  int n_ret = 0, n_noret = 0, n_skip = 0;
  for (int i = tid; i < sc.n; i += kMapThreads) {
    const double r = (double)ranges[sc.first + i];
    const int cls = map_beam_class(r, sc.range_min, sc.range_max);
    n_ret += cls == kMapBeamReturn;
    n_noret += cls == kMapBeamNoReturn;
    n_skip += cls == kMapBeamSkip;
    if (cls == kMapBeamSkip || (cls == kMapBeamNoReturn && !clear_no_return)) continue;
    const double d = cls == kMapBeamReturn ? r : sc.range_max;
    int ex, ey;
    if (!map_end_cell(x, y, th, sc.angle_min, sc.angle_inc, i, d, g.ox, g.oy, g.res, &ex, &ey)) continue;
    if (map_line_misses_grid(cx, cy, ex, ey, g.width, g.height)) continue;
    map_trace(cx, cy, ex, ey, cls == kMapBeamReturn, [&](int px, int py, bool is_hit) {
      if ((unsigned)px >= (unsigned)g.width || (unsigned)py >= (unsigned)g.height) return;
      const int cell = py * g.width + px;
      if (is_hit) {
        atomicAdd(&hit[cell], 1);
        return;
      }
      const unsigned ux = (unsigned)(px - wx0), uy = (unsigned)(py - wy0);
      if (ux < (unsigned)W && uy < (unsigned)W) atomicAdd(&win[uy * W + ux], 1);
      else atomicAdd(&miss[cell], 1);
    });
  }
  if (n_ret) atomicAdd(&cnt[0], n_ret);
  if (n_noret) atomicAdd(&cnt[1], n_noret);
  if (n_skip) atomicAdd(&cnt[2], n_skip);
  __syncthreads();
  // (only cells inside the grid were counted, so a non-zero cell is inside it)
  for (int j = tid; j < W * W; j += kMapThreads) {
    const int v = win[j];
    if (v) atomicAdd(&miss[(wy0 + j / (W > 0 ? W : 1)) * g.width + (wx0 + j % (W > 0 ? W : 1))], v);
  }
  if (tid == 0) {
    atomicAdd(&stats[kMapStBeams], (unsigned long long)sc.n);
    if (cnt[0]) atomicAdd(&stats[kMapStReturn], (unsigned long long)cnt[0]);
    if (cnt[1]) atomicAdd(&stats[kMapStNoReturn], (unsigned long long)cnt[1]);
    if (cnt[2]) atomicAdd(&stats[kMapStBeamSkipped], (unsigned long long)cnt[2]);
  }
}

// counts -> int8 occupancy, 16 cells per thread (four 16-byte loads per plane,
// one 16-byte store), and the integer reductions: sum of hit + miss, cells with
// any update
__global__ __launch_bounds__(256) void k_map_finalize(const int* __restrict__ hit, const int* __restrict__ miss, int n,
                                                      double l_occ, double l_free, double l_min, double l_max,
                                                      signed char* __restrict__ occ,
                                                      unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long red[2][256 / 64];
  const int base = (blockIdx.x * 256 + threadIdx.x) * kMapFinalizeCells;
  unsigned long long upd = 0, known = 0;
  if (base + kMapFinalizeCells <= n) {
    union {
      int4 q;
      signed char c[16];
    } o;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int4 h = *(const int4*)(hit + base + 4 * k), m = *(const int4*)(miss + base + 4 * k);
      const int hh[4] = {h.x, h.y, h.z, h.w}, mm[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        upd += (unsigned long long)((long long)hh[j] + mm[j]);
        known += (long long)hh[j] + mm[j] != 0;
        o.c[4 * k + j] = (signed char)map_occupancy(hh[j], mm[j], l_occ, l_free, l_min, l_max);
      }
    }
    *(int4*)(occ + base) = o.q;
  } else {
    for (int c = base; c < n; c++) {
      const int h = hit[c], m = miss[c];
      upd += (unsigned long long)((long long)h + m);
      known += (long long)h + m != 0;
      occ[c] = (signed char)map_occupancy(h, m, l_occ, l_free, l_min, l_max);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    upd += __shfl_down(upd, off, 64);
    known += __shfl_down(known, off, 64);
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  if (lane == 0) {
    red[0][wave] = upd;
    red[1][wave] = known;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    upd = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    known = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (upd) atomicAdd(&stats[kMapStUpdates], upd);
    if (known) atomicAdd(&stats[kMapStKnown], known);
  }
}

}  // namespace pgo

// ============================================================== C-ABI
struct pgo_map {
  int device = 0;
  pgo_map_params p;
  std::string last_error;
  // ---- host copy of the scans (insertion order) ----
  std::unordered_map<uint64_t, int32_t> index;
  std::vector<uint64_t> keys;
  std::vector<pgo::MapScan> scans;
  std::vector<float> ranges;
  // ---- device state (created by the first render or read) ----
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};                   // render start, render end, finalize end, clear start
  double ms_clear = 0.0;                   // device time of the last render's clear pass
  unsigned long long* h_stats = nullptr;   // pinned
  unsigned long long* d_stats = nullptr;
  int* d_planes = nullptr;                 // hit [0, cells), miss [plane, plane + cells); plane = cells rounded up to 64
  signed char* d_occ = nullptr;            // [plane]
  size_t cells = 0, plane = 0;
  // grow-only: the scans uploaded so far, the poses of one render
  pgo::MapScan* d_scans = nullptr;
  float* d_ranges = nullptr;
  size_t scans_cap = 0, ranges_cap = 0, dev_scans = 0;
  double* d_xyt = nullptr;
  int* d_vidx = nullptr;
  size_t xyt_cap = 0, vidx_cap = 0;
};

namespace {

int mfail(pgo_map* m, int code, const std::string& msg) {
  if (m) m->last_error = msg;
  return code;
}

#define MAP_HIP(m, expr)                                                                  \
  do {                                                                                    \
    const hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) return mfail(m, PGO_E_HIP, std::string("map: ") + hipGetErrorString(e_)); \
  } while (0)

int map_launch_clear(pgo_map* m) {
  const size_t n16 = 2 * m->plane / 4;
  const int blocks = (int)std::min<size_t>((n16 + 255) / 256, 4096);
  pgo::k_map_clear<<<blocks, 256, 0, m->stream>>>((int4*)m->d_planes, n16);
  MAP_HIP(m, hipGetLastError());
  return PGO_OK;
}

// stream, events, the planes (zeroed) and the occupancy (unknown)
int map_ensure_device(pgo_map* m) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return mfail(m, PGO_E_NO_DEVICE, "no HIP device available");
  if (m->device < 0 || m->device >= count) return mfail(m, PGO_E_NO_DEVICE, "device ordinal out of range");
  if (hipSetDevice(m->device) != hipSuccess) return mfail(m, PGO_E_NO_DEVICE, "hipSetDevice");
  if (m->d_occ) return PGO_OK;
  if (!m->stream) MAP_HIP(m, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  for (auto& e : m->ev)
    if (!e) MAP_HIP(m, hipEventCreate(&e));
  if (!m->h_stats) MAP_HIP(m, hipHostMalloc((void**)&m->h_stats, sizeof(unsigned long long) * pgo::kMapStCount));
  if (!m->d_stats) MAP_HIP(m, hipMalloc((void**)&m->d_stats, sizeof(unsigned long long) * pgo::kMapStCount));
  m->cells = (size_t)m->p.width * m->p.height;
  m->plane = (m->cells + 63) & ~(size_t)63;
  if (!m->d_planes && hipMalloc((void**)&m->d_planes, sizeof(int) * 2 * m->plane) != hipSuccess)
    return mfail(m, PGO_E_NOMEM, "map: count planes");
  signed char* occ = nullptr;
  if (hipMalloc((void**)&occ, m->plane) != hipSuccess) return mfail(m, PGO_E_NOMEM, "map: occupancy");
  const int rc = map_launch_clear(m);
  hipError_t e = rc == PGO_OK ? hipMemsetAsync(occ, 0xff, m->plane, m->stream) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  if (rc != PGO_OK || e != hipSuccess) {
    (void)hipFree(occ);
    return rc != PGO_OK ? rc : mfail(m, PGO_E_HIP, std::string("map: ") + hipGetErrorString(e));
  }
  m->d_occ = occ;
  return PGO_OK;
}

template <class T>
int map_grow(pgo_map* m, T** p, size_t& cap, size_t need) {
  if (cap >= need) return PGO_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  cap = 0;
  const size_t want = need * 3 / 2;
  if (hipMalloc((void**)p, sizeof(T) * want) != hipSuccess) return mfail(m, PGO_E_NOMEM, "map: device buffer");
  cap = want;
  return PGO_OK;
}

// the scans added since the last render (all of them when a buffer had to grow)
int map_upload_scans(pgo_map* m) {
  const size_t ns = m->scans.size();
  if (m->dev_scans == ns) return PGO_OK;
  if (m->scans_cap < ns || m->ranges_cap < m->ranges.size()) {
    m->dev_scans = 0;
    int rc = map_grow(m, &m->d_scans, m->scans_cap, ns);
    if (rc == PGO_OK) rc = map_grow(m, &m->d_ranges, m->ranges_cap, m->ranges.size());
    if (rc != PGO_OK) return rc;
  }
  const size_t s0 = m->dev_scans, b0 = (size_t)m->scans[s0].first;
  MAP_HIP(m, hipMemcpyAsync(m->d_scans + s0, m->scans.data() + s0, sizeof(pgo::MapScan) * (ns - s0), hipMemcpyHostToDevice,
                            m->stream));
  MAP_HIP(m, hipMemcpyAsync(m->d_ranges + b0, m->ranges.data() + b0, sizeof(float) * (m->ranges.size() - b0),
                            hipMemcpyHostToDevice, m->stream));
  MAP_HIP(m, hipStreamSynchronize(m->stream));   // (the host vectors may move at the next add_scan)
  m->dev_scans = ns;
  return PGO_OK;
}

double wall_ms(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Scans [first, first + n) at host poses xyt, or (vidx != NULL) at the poses
// gpose[vidx[.]] of a graph on this device.
int map_render(pgo_map* m, size_t first, size_t n, const double* xyt, const std::vector<int>* vidx, const void* gpose,
               int flags, pgo_map_stats* st) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc = map_ensure_device(m);
  if (rc != PGO_OK) return rc;
  hipStream_t s = m->stream;
  const auto tu = std::chrono::steady_clock::now();
  if ((rc = map_upload_scans(m)) != PGO_OK) return rc;
  if (n) {
    if ((rc = map_grow(m, &m->d_xyt, m->xyt_cap, 3 * n)) != PGO_OK) return rc;
    if (vidx) {
      if ((rc = map_grow(m, &m->d_vidx, m->vidx_cap, n)) != PGO_OK) return rc;
      MAP_HIP(m, hipMemcpyAsync(m->d_vidx, vidx->data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    } else {
      MAP_HIP(m, hipMemcpyAsync(m->d_xyt, xyt, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    }
  }
  MAP_HIP(m, hipMemsetAsync(m->d_stats, 0, sizeof(unsigned long long) * pgo::kMapStCount, s));
  MAP_HIP(m, hipStreamSynchronize(s));
  const double ms_upload = wall_ms(tu);
  MAP_HIP(m, hipEventRecord(m->ev[3], s));
  if (!(flags & PGO_MAP_ACCUMULATE) && (rc = map_launch_clear(m)) != PGO_OK) return rc;
  int* hit = m->d_planes;
  int* miss = m->d_planes + m->plane;
  MAP_HIP(m, hipEventRecord(m->ev[0], s));
  if (n) {
    if (vidx)
      pgo::k_map_gather_poses<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((const double4*)gpose, m->d_vidx, (int)n,
                                                                         m->d_xyt);
    const pgo::MapGrid g = {m->p.resolution, m->p.origin_x, m->p.origin_y, m->p.width, m->p.height};
    pgo::k_map_render<<<(unsigned)n, pgo::kMapThreads, 0, s>>>(g, m->d_scans, m->d_ranges, (int)first, m->d_xyt,
                                                               m->p.clear_no_return, hit, miss, m->d_stats);
    MAP_HIP(m, hipGetLastError());
  }
  MAP_HIP(m, hipEventRecord(m->ev[1], s));
  const int per_block = 256 * pgo::kMapFinalizeCells;
  pgo::k_map_finalize<<<(unsigned)((m->cells + per_block - 1) / per_block), 256, 0, s>>>(
      hit, miss, (int)m->cells, m->p.l_occ, m->p.l_free, m->p.l_min, m->p.l_max, m->d_occ, m->d_stats);
  MAP_HIP(m, hipGetLastError());
  MAP_HIP(m, hipEventRecord(m->ev[2], s));
  MAP_HIP(m, hipMemcpyAsync(m->h_stats, m->d_stats, sizeof(unsigned long long) * pgo::kMapStCount, hipMemcpyDeviceToHost,
                            s));
  MAP_HIP(m, hipStreamSynchronize(s));
  float ms_clear = 0.f;
  m->ms_clear = !(flags & PGO_MAP_ACCUMULATE) && hipEventElapsedTime(&ms_clear, m->ev[3], m->ev[0]) == hipSuccess
                    ? ms_clear
                    : 0.0;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    const unsigned long long* h = m->h_stats;
    st->status = PGO_OK;
    st->scans = (long long)n;
    st->scans_skipped = (long long)h[pgo::kMapStSkipped];
    st->beams = (long long)h[pgo::kMapStBeams];
    st->beams_return = (long long)h[pgo::kMapStReturn];
    st->beams_no_return = (long long)h[pgo::kMapStNoReturn];
    st->beams_skipped = (long long)h[pgo::kMapStBeamSkipped];
    st->updates = (long long)h[pgo::kMapStUpdates];
    st->known_cells = (long long)h[pgo::kMapStKnown];
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, m->ev[0], m->ev[1]) == hipSuccess) st->ms_render = ms;
    if (hipEventElapsedTime(&ms, m->ev[1], m->ev[2]) == hipSuccess) st->ms_finalize = ms;
    st->ms_upload = ms_upload;
    st->ms_total = wall_ms(t0);
  }
  return PGO_OK;
}

}  // namespace

extern "C" {

void pgo_map_default_params(pgo_map_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  pgo::map_default_params(*p);
}

pgo_map* pgo_map_create(int device, const pgo_map_params* p) {
  if (!p || !pgo::map_params_ok(*p)) return nullptr;
  pgo_map* m = new (std::nothrow) pgo_map();
  if (!m) return nullptr;
  m->device = device;
  m->p = *p;
  return m;
}

void pgo_map_destroy(pgo_map* m) {
  if (!m) return;
  if (m->stream) {
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    (void)hipStreamDestroy(m->stream);
    for (auto e : m->ev)
      if (e) (void)hipEventDestroy(e);
    if (m->h_stats) (void)hipHostFree(m->h_stats);
    for (void* q : {(void*)m->d_stats, (void*)m->d_planes, (void*)m->d_occ, (void*)m->d_scans, (void*)m->d_ranges,
                    (void*)m->d_xyt, (void*)m->d_vidx})
      if (q) (void)hipFree(q);
  }
  delete m;
}

const char* pgo_map_last_error(const pgo_map* m) { return m ? m->last_error.c_str() : "null handle or bad parameters"; }

int pgo_map_add_scan(pgo_map* m, uint64_t key, int n, const float* ranges, double angle_min, double angle_increment,
                     double range_min, double range_max) {
  if (!m) return PGO_E_ARG;
  if (!pgo::map_scan_ok(n, ranges, angle_min, angle_increment, range_min, range_max, m->p.resolution))
    return mfail(m, PGO_E_ARG,
                 "map: a scan holds 1 .. 4096 beams, 0 <= range_min < range_max, range_max / resolution <= 32768, "
                 "finite angles");
  if (!pgo::map_beams_fit(m->ranges.size(), n)) return mfail(m, PGO_E_ARG, "map: more than 2^31 - 1 beams");
  if (m->index.count(key)) return mfail(m, PGO_E_DUP_KEY, "map: scan key " + std::to_string(key) + " already stored");
  pgo::MapScan sc;
  sc.angle_min = angle_min;
  sc.angle_inc = angle_increment;
  sc.range_min = range_min;
  sc.range_max = range_max;
  sc.first = (int)m->ranges.size();
  sc.n = n;
  m->index.emplace(key, (int32_t)m->scans.size());
  m->keys.push_back(key);
  m->scans.push_back(sc);
  m->ranges.insert(m->ranges.end(), ranges, ranges + n);
  return PGO_OK;
}

size_t pgo_map_num_scans(const pgo_map* m) { return m ? m->scans.size() : 0; }

int pgo_map_render(pgo_map* m, size_t first, size_t n, const double* xyt, int flags, pgo_map_stats* st) {
  if (!m) return PGO_E_ARG;
  if (st) st->status = PGO_E_ARG;
  if (first > m->scans.size() || n > m->scans.size() - first || (n && !xyt))
    return mfail(m, PGO_E_ARG, "map: scan range past the stored scans, or no poses");
  for (size_t i = 0; i < 3 * n; i++)
    if (!pgo::map_finite(xyt[i])) {
      if (st) st->status = PGO_E_NONFINITE;
      return mfail(m, PGO_E_NONFINITE, "map: non-finite pose");
    }
  const int rc = map_render(m, first, n, xyt, nullptr, nullptr, flags, st);
  if (st) st->status = rc;
  return rc;
}

int pgo_map_render_graph(pgo_map* m, pgo_graph* g, int flags, pgo_map_stats* st) {
  if (!m || !g) return PGO_E_ARG;
  if (st) st->status = PGO_E_ARG;
  const size_t n = m->scans.size();
  std::vector<int> vidx(n);
  for (size_t i = 0; i < n; i++) {
    const long long v = pgo::graph_vertex_index(g, m->keys[i]);
    if (v < 0) {
      if (st) st->status = PGO_E_NO_KEY;
      return mfail(m, PGO_E_NO_KEY, "map: scan key " + std::to_string(m->keys[i]) + " is no vertex of the graph");
    }
    vidx[i] = (int)v;
  }
  if (pgo::graph_device_ordinal(g) != m->device) return mfail(m, PGO_E_ARG, "map: the graph lives on another device");
  const void* pose = nullptr;
  if (n) {
    size_t nv = 0;
    const int rc = pgo::graph_device_poses(g, &pose, &nv);
    if (rc != PGO_OK) {
      if (st) st->status = rc;
      return mfail(m, rc, std::string("map: the graph's device values: ") + pgo_last_error(g));
    }
    for (size_t i = 0; i < n; i++)
      if ((size_t)vidx[i] >= nv) return mfail(m, PGO_E_HIP, "map: the graph's device values are incomplete");
  }
  const int rc = map_render(m, 0, n, nullptr, &vidx, pose, flags, st);
  if (st) st->status = rc;
  return rc;
}

int pgo_map_get_counts(pgo_map* m, int32_t* hit, int32_t* miss) {
  if (!m) return PGO_E_ARG;
  const int rc = map_ensure_device(m);
  if (rc != PGO_OK) return rc;
  if (hit) MAP_HIP(m, hipMemcpyAsync(hit, m->d_planes, sizeof(int) * m->cells, hipMemcpyDeviceToHost, m->stream));
  if (miss)
    MAP_HIP(m, hipMemcpyAsync(miss, m->d_planes + m->plane, sizeof(int) * m->cells, hipMemcpyDeviceToHost, m->stream));
  MAP_HIP(m, hipStreamSynchronize(m->stream));
  return PGO_OK;
}

int pgo_map_get_occupancy(pgo_map* m, int8_t* out) {
  if (!m || !out) return PGO_E_ARG;
  const int rc = map_ensure_device(m);
  if (rc != PGO_OK) return rc;
  MAP_HIP(m, hipMemcpyAsync(out, m->d_occ, m->cells, hipMemcpyDeviceToHost, m->stream));
  MAP_HIP(m, hipStreamSynchronize(m->stream));
  return PGO_OK;
}

int pgo_map_debug_ms(const pgo_map* m, double* ms_clear) {
  if (!m || !ms_clear) return PGO_E_ARG;
  *ms_clear = m->ms_clear;
  return PGO_OK;
}

int pgo_debug_map_line(int x0, int y0, int x1, int y1, int* xy, int cap) {
  int k = 0;
  pgo::map_trace(x0, y0, x1, y1, false, [&](int x, int y, bool) {
    if (xy && k < cap) {
      xy[2 * k] = x;
      xy[2 * k + 1] = y;
    }
    k++;
  });
  return k;
}

int pgo_debug_map_window(void) { return pgo::kMapWindow; }

}  // extern "C"
