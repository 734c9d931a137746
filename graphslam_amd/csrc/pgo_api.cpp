// libpgo.so: host side of the C-ABI in include/pgo.h.
//
// Mirrors, call for call, what /root/reference/src/graph/src/graph.cpp does
// through GTSAM (insert / add / optimize / at / nrFactors), keeps the graph and
// its values resident in HBM between calls, and drives the device kernels of
// pgo_kernels.hip with GTSAM's Levenberg-Marquardt control logic
// (tryLambda / decreaseLambda / increaseLambda / checkConvergence, GTSAM 4.0
// defaults) running on host scalars read back once per lambda try.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <thread>
#include <vector>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "pgo.h"
#include "pgo_chol.h"
#include "pgo_plan_digest.h"
#include "pgo_comm.h"
#include "pgo_search.h"
#include "pgo_device.h"
#include "pgo_gnc.h"
#include "pgo_init.h"
#include "pgo_lm.h"
#include "pgo_map.h"
#include "pgo_structure.h"

using pgo::DevGraph;

// Lambda lane l >= 1 of a batched factorisation (lane 0 is the handle's own
// buffers): the Cholesky plan holds a numeric workspace per lane and every
// launch of the factor + solve carries the lanes as grid dimension y, so L
// consecutive lambda tries cost one pass over the (mostly latency-bound)
// schedule.  Per lane: candidate values, reduction partials and scalars of its
// try; the linearisation (D, V, g) and the current values are shared.
struct Lane {
  double4* pose_cand = nullptr;
  double* part = nullptr;
  double* scal = nullptr;
};

struct Staging {
  char* buf = nullptr;
  size_t cap = 0, used = 0;
  hipEvent_t done = nullptr;                // recorded after a batch's copies (stage_end)
};

struct pgo_graph {
  int device = 0;
  std::string last_error;
  // ---- host copy of the factor graph (insertion order) ----
  std::unordered_map<uint64_t, int32_t> index;
  std::vector<uint64_t> keys;
  std::vector<double> xyt;                  // current values (x, y, theta)
  std::vector<uint64_t> ek1, ek2;
  std::vector<double> ez;                   // 3 per between factor
  std::vector<double> eom;                  // 6 per factor: O00 O01 O02 O11 O12 O22
  std::vector<unsigned char> eloss;         // loss kind per between factor (PGO_LOSS_*)
  std::vector<double> ek;                   // ... and its parameter k (1 with PGO_LOSS_NONE)
  size_t n_robust = 0;                      // factors with a loss other than NONE: any -> the robust kernels
  size_t n_fixed = 0;                       // ... of which fixed weights below 1 (pgo::kLossFixed, ek the weight)
  std::vector<uint64_t> pk;
  std::vector<double> pz, pom;
  // ---- device state ----
  bool hip_ready = false;
  bool dev_structure = false;               // device graph matches host graph
  bool dev_values = false;                  // device pose == host xyt
  bool host_values = true;                  // host xyt == device pose
  DevGraph d;
  double* h_scal = nullptr;                 // pinned
  int* h_ctrl = nullptr;                    // pinned
  hipEvent_t ev[6] = {};
  static constexpr int kProfPairs = 64;     // sampled SpMV timings per read-back
  hipEvent_t pev[2 * kProfPairs] = {};
  int pk_iter[kProfPairs] = {};
  // ---- supernodal Cholesky (built on first use; structure-dependent) ----
  pgo::CholPlan chol;
  int ordering = pgo::kOrderNd;             // fill-reducing ordering (pgo_opts.ordering)
  int part_size = 1;                        // subtree partition the plan must have (PGO_MULTI_PARTITION)
  bool plan_stale = false;                  // the graph changed since the plan was built (kept, see ensure_chol)
  size_t plan_edges = 0;                    // between factors (user order) the plan holds: later ones are new
  int plan_update = 0;                      // how the last ensure_chol refreshed it (pgo_stats.plan_update)
  double plan_ms = 0.0;
  pgo::ExchangeHook hook;                   // the partitioned factorisation's all-gathers (comm)
  bool chol_ready = false;
  // pgo_marginal_covariances_all: where every between factor's cross block sits
  // in the fronts, kept while the plan (its SelPlan::serial) and the factors stay
  std::vector<int4> sel_etab;
  unsigned sel_etab_serial = 0;
  bool handoff_timeout = false;            // the last factorisation's in-launch hand-off gave up (retried once)
  // profiled factorisations (pgo_params.profile_every): every launch timed
  std::vector<hipEvent_t> sev;              // event pairs, one per launch
  std::vector<int> sev_fam;
  std::vector<double> sev_flops, sev_bytes;
  std::vector<int> sev_grid, sev_tag;
  hipEvent_t fev[4] = {};                   // factor start / end, solve end (profiled factorisation)
  double fam_ms[pgo::kFamCount] = {}, fam_flops[pgo::kFamCount] = {}, fam_bytes[pgo::kFamCount] = {};
  long long fam_launches[pgo::kFamCount] = {};
  std::vector<double> trace;                // per lambda try / GN step of the last optimize (kTraceCols each)
  long long factorizations = 0;
  hipGraphExec_t fac_exec[9] = {};          // captured factorisation, per lane count (1: d.x path)
  hipGraphExec_t sol_exec[9] = {};          // captured triangular solves, per lane count
  // graphs of a plan an incremental update replaced: destroyed only at the next
  // capture or with the device state (a destruction costs ~10 ms, on the first
  // live registration after a full optimize otherwise; on this thread only --
  // destroying them on a helper thread raced with the workspace re-allocation)
  std::vector<hipGraphExec_t> stale_exec;
  int graph_eager[9] = {};                  // eager factorisations of this plan before the capture
  int eager_first = 0;                      // ... how many (8 after an incremental plan update, else 0)
  double* h_lam = nullptr;                  // pinned lambda staging
  Staging stage;                            // pinned upload staging (append_structure)
  // ---- multi-GPU speculative lambda search (pgo_comm_*) ----
  pgo::Comm comm;
  // the partition group's communicator of the hybrid mode (pgo_comm_init_*_part:
  // the ranks that split one factorisation; comm then links one rank of every
  // group for the speculative search), and the communicator the partitioned
  // factorisation exchanges over (set per optimize: pcomm in the hybrid mode,
  // else comm)
  pgo::Comm pcomm;
  pgo::Comm* part_comm = &comm;
  // pcomm belongs to the main communicator set up right after it (the order
  // multi_gpu.attach_hybrid uses): pcomm_fresh = set since the last main init;
  // a main init binds a fresh pcomm and frees a stale one (round 6: a main
  // communicator replaced without pgo_comm_free no longer keeps the old group's)
  bool pcomm_fresh = false, pcomm_bound = false;
  std::vector<Lane> lanes;                  // lanes 1..L-1 (speculative tries on this GPU)
  double* xb = nullptr;                     // [L x 3n] solutions of a batched factor + solve
  size_t xb_n = 0;                          // ... allocated for this many vertices (capacity)
  double* h_lanes = nullptr;                // pinned [48]: 4 scalars per lane, lambdas at 32, flags at 40
  hipEvent_t lin_done = nullptr;            // linearisation complete
  int lane_cap = 8;                         // 1 after a lane allocation failed (reset per plan)
  // ---- incremental appends (append_structure, the live re-solve) ----
  pgo::GraphStructure gs;                   // the structure the device holds, host side (pgo_structure.h)
  size_t cap_n = 0, cap_ne = 0;             // device capacities in vertices / factors
  bool dev_complete = false;                // the device holds gs exactly (appendable)
  int last_upload = 0;                      // 1 full upload, 2 append (diagnostics)
  bool saved_valid = false;                 // d.pose_saved holds a snapshot of this structure (pgo_save_values)
  // ---- closest-keyframe search scratch ----
  double* s_d = nullptr;                    // [kMaxBlocks + 1] partial / final distances
  int* s_i = nullptr;                       // [kMaxBlocks + 1] partial / final indices
  double* sb_d = nullptr;                   // batched: per-query distance, index, query pose index
  int* sb_i = nullptr;
  int* sb_q = nullptr;
  double* sbp_d = nullptr;                  // batched: per (chunk, query) partials
  int* sbp_i = nullptr;
  size_t sb_cap = 0, sbp_cap = 0;
  hipEvent_t sev_scan[2] = {}, sev_batch[2] = {};
  bool scan_timed = false, batch_timed = false;
  // ---- linear initialisation (pgo_initialize_linear) ----
  double* init_tgt = nullptr;               // [ne + np] the stages' angle targets, device factor / prior order
  size_t init_tgt_cap = 0;
  // ---- graduated non-convexity (pgo_optimize_gnc) ----
  unsigned char* gnc_cand = nullptr;        // [cap_ne] 1: the device factor is a candidate (built per call)
  double4* gnc_pose = nullptr;              // [cap_n] the values before an inner solve (put back if it fails)
  size_t gnc_cand_cap = 0, gnc_pose_cap = 0;   // sized with the graph's capacity, freed with the device graph
  std::vector<double> gnc_trace;            // per inner solve of the last pgo_optimize_gnc (kGncTraceCols each)
};

namespace {
// roctx range over a host scope (rocprofv3 --marker-trace shows the LM
// structure: optimize > plan / linearisation > lambda rounds; a no-op without
// a profiler attached)
struct RoctxRange {
  explicit RoctxRange(const char* m) { roctxRangePush(m); }
  ~RoctxRange() { roctxRangePop(); }
  RoctxRange(const RoctxRange&) = delete;
  RoctxRange& operator=(const RoctxRange&) = delete;
};
}  // namespace

namespace {

constexpr int kProfLaunches = 4096;   // timed launches per profiled factorisation + solve
constexpr int kTraceCols = 8;         // pgo_get_trace row

int fail(pgo_graph* g, int code, const std::string& msg) {
  if (g) g->last_error = msg;
  return code;
}

#define HIP_TRY(g, expr)                                                                       \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(g, PGO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

// noiseModel::Gaussian::Covariance(Q) (graph.cpp:45,83,103) -> Omega upper 6.
// GTSAM's smart check: all |off-diagonal| <= 1e-9 -> Diagonal::Variances;
// otherwise Information(Q^-1) with R = LLT(Q^-1).matrixU(): the lower triangle
// of Q^-1 is what counts, mirrored.
int information(const double* q, double* om6) {
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(q[i])) return PGO_E_BAD_COV;
  bool full = false;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      if (i != j && std::fabs(q[3 * i + j]) > 1e-9) full = true;
  if (!full) {
    for (int i = 0; i < 3; i++)
      if (!(q[4 * i] > 0.0)) return PGO_E_BAD_COV;
    om6[0] = 1.0 / q[0]; om6[1] = 0; om6[2] = 0;
    om6[3] = 1.0 / q[4]; om6[4] = 0;
    om6[5] = 1.0 / q[8];
    return PGO_OK;
  }
  const double a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5], g = q[6], h = q[7], k = q[8];
  const double A = e * k - f * h, B = -(d * k - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return PGO_E_BAD_COV;
  // lower triangle of the inverse: (1,0)=B/det, (2,0)=C/det, (2,1)=-(a h - b g)/det
  const double l00 = A / det, l10 = B / det, l20 = C / det;
  const double l11 = (a * k - c * g) / det, l21 = -(a * h - b * g) / det, l22 = (a * e - b * d) / det;
  // LLT must succeed
  if (!(l00 > 0)) return PGO_E_BAD_COV;
  const double r00 = std::sqrt(l00), r10 = l10 / r00, r20 = l20 / r00;
  const double s11 = l11 - r10 * r10;
  if (!(s11 > 0)) return PGO_E_BAD_COV;
  const double r11 = std::sqrt(s11), r21 = (l21 - r20 * r10) / r11;
  if (!(l22 - r20 * r20 - r21 * r21 > 0)) return PGO_E_BAD_COV;
  om6[0] = l00; om6[1] = l10; om6[2] = l20; om6[3] = l11; om6[4] = l21; om6[5] = l22;
  return PGO_OK;
}


// The captured graphs are destroyed here, before the caller frees or
// re-allocates the memory they point to (destroying them on a helper thread
// while the workspaces were freed and re-allocated raced: an intermittent host
// segfault on rapid lane-count changes).  The callers have drained the stream.
void destroy_stale_graphs(pgo_graph* g) {
  for (hipGraphExec_t e : g->stale_exec) (void)hipGraphExecDestroy(e);
  g->stale_exec.clear();
}

// defer: keep the execs for destroy_stale_graphs (they are never launched again)
void drop_graphs(pgo_graph* g, bool defer = false) {
  for (int l = 0; l < 9; l++) {
    for (hipGraphExec_t* e : {&g->fac_exec[l], &g->sol_exec[l]}) {
      if (*e) {
        if (defer) g->stale_exec.push_back(*e);
        else (void)hipGraphExecDestroy(*e);
      }
      *e = nullptr;
    }
    g->graph_eager[l] = 0;
  }
  if (!defer) destroy_stale_graphs(g);
}

void free_lanes(pgo_graph* g) {
  if (g->d.stream) (void)hipStreamSynchronize(g->d.stream);
  for (Lane& ln : g->lanes) {
    void* ptrs[] = {ln.pose_cand, ln.part, ln.scal};
    for (void* q : ptrs)
      if (q) (void)hipFree(q);
  }
  g->lanes.clear();
  if (g->xb) (void)hipFree(g->xb);
  g->xb = nullptr;
  for (int l = 2; l < 9; l++)   // the batched graphs hold xb
    for (hipGraphExec_t* e : {&g->fac_exec[l], &g->sol_exec[l]}) {
      if (*e) (void)hipGraphExecDestroy(*e);
      *e = nullptr;
    }
}

void free_device(pgo_graph* g, bool keep_plan = false) {
  g->dev_complete = false;
  free_lanes(g);
  g->lane_cap = 8;
  DevGraph& d = g->d;
  void* ptrs[] = {d.eij, d.ez, d.eom, d.prior_ptr, d.prior_vtx, d.pz, d.pom, d.row_ptr, d.slot_edge, d.slot_col, d.V,
                  d.erow, d.brow, d.s1_ptr, d.s1pos, d.eside, d.Dc, d.W, d.eloss, d.ek, d.s1fac, d.D, d.g, d.pose, d.pose_cand, d.pose_saved, d.x, d.r, d.z, d.p, d.q, d.Minv, d.part, d.scal, d.ctrl};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (g->gnc_cand) (void)hipFree(g->gnc_cand);
  if (g->gnc_pose) (void)hipFree(g->gnc_pose);
  g->gnc_cand = nullptr;
  g->gnc_pose = nullptr;
  g->gnc_cand_cap = g->gnc_pose_cap = 0;
  hipStream_t s = d.stream;
  d = DevGraph();
  d.stream = s;
  g->dev_structure = false;
  g->dev_values = false;
  drop_graphs(g);
  if (keep_plan && g->chol_ready) {   // the structure changed: ensure_chol decides what to keep
    g->plan_stale = true;
    return;
  }
  if (g->chol_ready) pgo::chol_free(g->chol);
  g->chol_ready = false;
}

int ensure_hip(pgo_graph* g) {
  if (g->hip_ready) return PGO_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(g, PGO_E_NO_DEVICE, "no HIP device available");
  if (g->device < 0 || g->device >= count) return fail(g, PGO_E_NO_DEVICE, "device ordinal out of range");
  HIP_TRY(g, hipSetDevice(g->device));
  HIP_TRY(g, hipStreamCreateWithFlags(&g->d.stream, hipStreamNonBlocking));
  HIP_TRY(g, hipHostMalloc((void**)&g->h_scal, 16 * sizeof(double), hipHostMallocDefault));
  HIP_TRY(g, hipHostMalloc((void**)&g->h_ctrl, 4 * sizeof(int), hipHostMallocDefault));
  HIP_TRY(g, hipHostMalloc((void**)&g->h_lam, sizeof(double), hipHostMallocDefault));
  HIP_TRY(g, hipHostMalloc((void**)&g->h_lanes, 48 * sizeof(double), hipHostMallocDefault));
  for (auto& e : g->ev) HIP_TRY(g, hipEventCreate(&e));
  for (auto& e : g->pev) HIP_TRY(g, hipEventCreate(&e));
  HIP_TRY(g, hipEventCreateWithFlags(&g->lin_done, hipEventDisableTiming));
  g->sev.resize(2 * kProfLaunches);
  g->sev_fam.resize(kProfLaunches);
  g->sev_flops.resize(kProfLaunches);
  g->sev_bytes.resize(kProfLaunches);
  g->sev_grid.resize(kProfLaunches);
  g->sev_tag.resize(kProfLaunches);
  for (auto& e : g->sev) HIP_TRY(g, hipEventCreate(&e));
  for (auto& e : g->fev) HIP_TRY(g, hipEventCreate(&e));
  g->hip_ready = true;
  return PGO_OK;
}

template <class T>
int dev_alloc(pgo_graph* g, T** p, size_t count) {
  HIP_TRY(g, hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)));
  return PGO_OK;
}

template <class T>
int h2d(pgo_graph* g, T* dst, const T* src, size_t count) {
  if (count == 0) return PGO_OK;
  HIP_TRY(g, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, g->d.stream));
  return PGO_OK;
}

// Host -> device through the handle's pinned staging buffer (a bump region per
// batch of copies; stage_reset after the stream has drained): the live
// re-solve's per-registration uploads at pinned speed
// a batch of staged copies: wait until the previous batch's copies have read
// the buffer, then refill it from the start; stage_end marks the batch
int stage_begin(pgo_graph* g, Staging& st) {
  if (st.done) HIP_TRY(g, hipEventSynchronize(st.done));
  else HIP_TRY(g, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  st.used = 0;
  return PGO_OK;
}
int stage_end(pgo_graph* g, Staging& st) {
  HIP_TRY(g, hipEventRecord(st.done, g->d.stream));
  return PGO_OK;
}

template <class T>
int staged_h2d(pgo_graph* g, Staging& st, T* dst, const T* src, size_t count) {
  if (count == 0) return PGO_OK;
  const size_t bytes = count * sizeof(T), off = (st.used + 255) / 256 * 256;
  if (off + bytes > st.cap) return h2d(g, dst, src, count);   // (full: a pageable copy)
  std::memcpy(st.buf + off, src, bytes);
  st.used = off + bytes;
  HIP_TRY(g, hipMemcpyAsync(dst, st.buf + off, bytes, hipMemcpyHostToDevice, g->d.stream));
  return PGO_OK;
}

#define RC_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != PGO_OK) return rc_; \
  } while (0)

// Host values -> device pose (Pose2(x, y, theta): Rot2::fromAngle), vertices
// [first, n) (the ones before stay as they are on the device)
int upload_values(pgo_graph* g, size_t first = 0) {
  const size_t n = g->keys.size();
  std::vector<double4> h(n > first ? n - first : 0);
  for (size_t i = first; i < n; i++) {
    const double th = g->xyt[3 * i + 2];
    h[i - first] = make_double4(g->xyt[3 * i], g->xyt[3 * i + 1], std::cos(th), std::sin(th));
  }
  RC_TRY(h2d(g, g->d.pose + first, h.data(), n - std::min(n, first)));
  HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  g->dev_values = true;
  return PGO_OK;
}

// Device pose -> host values (Values::at<Pose2>(k).x()/y()/theta(), graph.cpp:123-125)
int download_values(pgo_graph* g) {
  if (g->host_values) return PGO_OK;
  // the device-resident vertices (vertices appended since keep their host values)
  const size_t n = std::min(g->keys.size(), (size_t)g->d.n);
  std::vector<double4> h(n);
  if (n) {
    HIP_TRY(g, hipMemcpyAsync(h.data(), g->d.pose, n * sizeof(double4), hipMemcpyDeviceToHost, g->d.stream));
    HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  }
  for (size_t i = 0; i < n; i++) {
    g->xyt[3 * i] = h[i].x;
    g->xyt[3 * i + 1] = h[i].y;
    g->xyt[3 * i + 2] = std::atan2(h[i].w, h[i].z);
  }
  g->host_values = true;
  return PGO_OK;
}

// Factors [first, ne) resolved to vertex indices (GTSAM raises
// ValuesKeyDoesNotExist at optimize time for a factor on an unknown key).
int resolve_edges(pgo_graph* g, size_t first, std::vector<int2>& eij) {
  const size_t ne = g->ek1.size();
  eij.resize(ne - first);
  for (size_t e = first; e < ne; e++) {
    auto a = g->index.find(g->ek1[e]), b = g->index.find(g->ek2[e]);
    if (a == g->index.end() || b == g->index.end()) {
      const uint64_t k = a == g->index.end() ? g->ek1[e] : g->ek2[e];
      return fail(g, PGO_E_NO_KEY, "between factor " + std::to_string(e) + " references key " +
                                       std::to_string(k) + " with no inserted value");
    }
    eij[e - first] = make_int2(a->second, b->second);
  }
  return PGO_OK;
}

// loss kind and parameter of `count` factors, out k from user factor order[k]
void gather_losses(const pgo_graph* g, const int* order, size_t count, std::vector<unsigned char>& hl,
                   std::vector<double>& hk) {
  hl.resize(count);
  hk.resize(count);
  for (size_t k = 0; k < count; k++) {
    hl[k] = g->eloss[order[k]];
    hk[k] = g->ek[order[k]];
  }
}

// The host structure of the whole graph (pgo_structure.h), keys resolved.
int build_structure(pgo_graph* g, pgo::GraphStructure& S) {
  const int np = (int)g->pk.size();
  std::vector<int2> eij_user;
  RC_TRY(resolve_edges(g, 0, eij_user));
  std::vector<int> pv(np);
  for (int q = 0; q < np; q++) {
    auto a = g->index.find(g->pk[q]);
    if (a == g->index.end())
      return fail(g, PGO_E_NO_KEY, "prior factor on key " + std::to_string(g->pk[q]) + " with no inserted value");
    pv[q] = a->second;
  }
  S.build((int)g->keys.size(), eij_user, std::move(pv), g->eom.data(), g->n_robust > 0);
  return PGO_OK;
}

// Build the device graph: the host structure, allocate with room for appends, copy.
int upload_structure(pgo_graph* g) {
  RC_TRY(ensure_hip(g));
  RC_TRY(download_values(g));
  pgo::GraphStructure& S = g->gs;
  RC_TRY(build_structure(g, S));
  const int n = S.n, ne = S.ne(), np = (int)S.pv.size(), ns = 2 * ne;
  std::vector<double4> hz(ne), hpz(np);
  std::vector<double2> hom(3 * (size_t)ne), hpom(3 * (size_t)np);
  pgo::pack_measurements(g->ez.data(), g->eom.data(), S.dorder.data(), ne, hz.data(), hom.data());
  pgo::pack_measurements(g->pz.data(), g->pom.data(), S.porder.data(), np, hpz.data(), hpom.data());
  // the values already resident stay bit for bit (no host atan2 -> cos / sin
  // round trip): vertices are append-only, so the first n_old keep their index
  // (freed on every exit path: an early error return below must not leak it)
  struct HipFree {
    void operator()(double4* p) const { (void)hipFree(p); }
  };
  std::unique_ptr<double4, HipFree> keep;
  const int n_old = g->dev_values && g->d.pose ? std::min(g->d.n, n) : 0;
  if (n_old > 0) {
    double4* k = nullptr;
    HIP_TRY(g, hipMalloc((void**)&k, sizeof(double4) * n_old));
    keep.reset(k);
    HIP_TRY(g, hipMemcpyAsync(keep.get(), g->d.pose, sizeof(double4) * n_old, hipMemcpyDeviceToDevice, g->d.stream));
  }
  free_device(g, true);
  DevGraph& d = g->d;
  d.n = n;
  d.ne = ne;
  d.np = np;
  d.nslots = ns;
  // room for appended vertices / factors (the live re-solve appends one
  // keyframe and a few factors per registration: append_structure)
  const size_t cn = (size_t)n + std::max<size_t>(1024, n / 8);
  const size_t ce = (size_t)ne + std::max<size_t>(4096, ne / 8), cs = 2 * ce;
  g->cap_n = cn;
  g->cap_ne = ce;
  {   // the appends' pinned staging (append_structure / bind_plan), sized for the
      // largest per-registration upload of this graph, allocated with the graph
    const size_t want = 8 * cs + 8 * ce + 80 * cn + ((size_t)1 << 20);
    if (g->stage.cap < want) {
      if (g->stage.done) HIP_TRY(g, hipEventSynchronize(g->stage.done));
      if (g->stage.buf) (void)hipHostFree(g->stage.buf);
      g->stage.buf = nullptr;
      g->stage.cap = 0;
      HIP_TRY(g, hipHostMalloc((void**)&g->stage.buf, want, hipHostMallocDefault));
      g->stage.cap = want;
    }
  }
  d.G = S.G;
  d.G1 = S.G1;
  d.nlb = (int)S.brow.size() - 1;
  RC_TRY(dev_alloc(g, &d.brow, cn + 1));
  RC_TRY(h2d(g, d.brow, S.brow.data(), S.brow.size()));
  RC_TRY(dev_alloc(g, &d.erow, cn + 1));
  RC_TRY(dev_alloc(g, &d.s1_ptr, cn + 1));
  RC_TRY(dev_alloc(g, &d.s1pos, ce));
  RC_TRY(dev_alloc(g, &d.Dc, 6 * cn));
  RC_TRY(dev_alloc(g, &d.W, ce));
  RC_TRY(h2d(g, d.erow, S.erow.data(), n + 1));
  RC_TRY(h2d(g, d.s1_ptr, S.s1_ptr.data(), n + 1));
  RC_TRY(h2d(g, d.s1pos, S.s1pos.data(), ne));
  RC_TRY(h2d(g, d.Dc, S.Dc.data(), 6 * (size_t)n));
  if (g->n_robust > 0) {   // robust losses: kind and k in device order, the side-1 lists' factors
    std::vector<unsigned char> hl;
    std::vector<double> hk;
    gather_losses(g, S.dorder.data(), ne, hl, hk);
    RC_TRY(dev_alloc(g, &d.eloss, ce));
    RC_TRY(dev_alloc(g, &d.ek, ce));
    RC_TRY(dev_alloc(g, &d.s1fac, ce));
    RC_TRY(h2d(g, d.eloss, hl.data(), ne));
    RC_TRY(h2d(g, d.ek, hk.data(), ne));
    RC_TRY(h2d(g, d.s1fac, S.s1fac.data(), ne));
    HIP_TRY(g, hipStreamSynchronize(d.stream));   // (the sources are locals)
  }
  RC_TRY(dev_alloc(g, &d.eij, ce));
  RC_TRY(dev_alloc(g, &d.ez, ce));
  RC_TRY(dev_alloc(g, &d.eom, 3 * ce));
  RC_TRY(dev_alloc(g, &d.prior_ptr, cn + 1));
  RC_TRY(dev_alloc(g, &d.prior_vtx, np));
  RC_TRY(dev_alloc(g, &d.pz, np));
  RC_TRY(dev_alloc(g, &d.pom, 3 * (size_t)np));
  RC_TRY(dev_alloc(g, &d.row_ptr, cn + 1));
  RC_TRY(dev_alloc(g, &d.slot_edge, cs));
  RC_TRY(dev_alloc(g, &d.slot_col, cs));
  RC_TRY(dev_alloc(g, &d.V, 9 * cs));
  RC_TRY(dev_alloc(g, &d.D, 6 * cn));
  RC_TRY(dev_alloc(g, &d.g, 3 * cn));
  RC_TRY(dev_alloc(g, &d.pose, cn));
  RC_TRY(dev_alloc(g, &d.pose_cand, cn));
  RC_TRY(dev_alloc(g, &d.x, 3 * cn));
  RC_TRY(dev_alloc(g, &d.r, 3 * cn));
  RC_TRY(dev_alloc(g, &d.z, 3 * cn));
  RC_TRY(dev_alloc(g, &d.p, 3 * cn));
  RC_TRY(dev_alloc(g, &d.q, 3 * cn));
  RC_TRY(dev_alloc(g, &d.Minv, 6 * cn));
  RC_TRY(dev_alloc(g, &d.part, (size_t)pgo::kMaxBlocks * pgo::kPartSlices));
  RC_TRY(dev_alloc(g, &d.scal, 16));
  RC_TRY(dev_alloc(g, &d.ctrl, 4));
  std::vector<int> pvs(np);
  for (int t = 0; t < np; t++) pvs[t] = S.pv[S.porder[t]];
  RC_TRY(h2d(g, d.eij, S.eij.data(), ne));
  RC_TRY(h2d(g, d.ez, hz.data(), ne));
  RC_TRY(h2d(g, d.eom, hom.data(), 3 * (size_t)ne));
  RC_TRY(h2d(g, d.prior_ptr, S.prior_ptr.data(), n + 1));
  RC_TRY(h2d(g, d.prior_vtx, pvs.data(), np));
  RC_TRY(h2d(g, d.pz, hpz.data(), np));
  RC_TRY(h2d(g, d.pom, hpom.data(), 3 * (size_t)np));
  RC_TRY(h2d(g, d.row_ptr, S.row_ptr.data(), n + 1));
  RC_TRY(h2d(g, d.slot_edge, S.codes().data(), ns));   // pre-plan codes throughout
  g->chol.asm_bound = false;   // (a new device factor order: the plan's bound sources are void)
  RC_TRY(h2d(g, d.slot_col, S.slot_col.data(), ns));
  HIP_TRY(g, hipMemsetAsync(d.part, 0, sizeof(double) * pgo::kMaxBlocks * pgo::kPartSlices, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  g->dev_structure = true;
  S.reserve(g->cap_n, g->cap_ne);   // room for in-place appends (append_structure), as the device arrays have
  g->dev_complete = true;
  g->last_upload = 1;
  if (n_old > 0) {
    HIP_TRY(g, hipMemcpyAsync(d.pose, keep.get(), sizeof(double4) * n_old, hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(g, hipStreamSynchronize(d.stream));
  }
  return upload_values(g, n_old);
}


// Appended vertices and between factors (pgo_add_vertex / pgo_add_edge after
// an upload -- the live re-solve, graph.cpp:180-200) extend the device graph in
// place when the device holds the previous structure, no prior was added,
// capacities suffice and GraphStructure::append takes them (a new keyframe's
// odometry and loop closures sort after the old factors); only what its delta
// names is uploaded.  Returns 1 when the full upload must run instead.
int append_structure(pgo_graph* g) {
  pgo::PhaseTimer phase("append_structure");
  DevGraph& d = g->d;
  pgo::GraphStructure& S = g->gs;
  const int n = (int)g->keys.size(), ne = (int)g->ek1.size(), np = (int)g->pk.size();
  if (!g->dev_complete || !g->hip_ready || np != d.np || S.n != d.n || S.ne() != d.ne || ne < d.ne ||
      (size_t)n > g->cap_n || (size_t)ne > g->cap_ne || getenv("PGO_NO_APPEND"))
    return 1;
  // the first robust factor on an all-Gaussian device graph: the full upload
  // allocates the loss arrays (and the kernels launched change with it)
  if ((g->n_robust > 0) != (d.eloss != nullptr)) return 1;
  std::vector<int2> new_ij;
  if (resolve_edges(g, d.ne, new_ij) != PGO_OK) return 1;   // the full path reports it
  pgo::StructureDelta dl;
  if (!S.append(n, new_ij, g->eom.data(), d.eloss != nullptr, &dl, &phase)) return 1;
  phase("per-row");
  const int n_old = dl.n_old, ne_old = dl.ne_old, ns = 2 * ne;
  const int* nd = S.dorder.data() + ne_old;   // the new factors, device order -> user index
  const size_t nn = (size_t)(ne - ne_old);
  // the device: new factors, per-row arrays, slots
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  phase("sync");
  if (g->xb && (size_t)n > g->xb_n) free_lanes(g);   // (else the lanes hold the grown graph too)
  drop_graphs(g, true);
  phase("drop graphs");
  g->saved_valid = false;   // (the snapshot holds the old structure's values; its buffer, sized
                            // for the capacity, is kept: a hipFree would wait for the device)
  phase("free");
  std::vector<double4> hz(nn);
  std::vector<double2> hom(3 * nn);
  pgo::pack_measurements(g->ez.data(), g->eom.data(), nd, nn, hz.data(), hom.data());
  // only what changed: the new factors; the row / slot arrays from the first
  // row with a new slot (earlier rows and their slots are unchanged); the
  // side-1 sums of the rows that gained side-1 terms; whole for the rest
  Staging& sg = g->stage;   // (allocated by upload_structure; staged_h2d falls back to pageable copies)
  RC_TRY(stage_begin(g, sg));
  RC_TRY(staged_h2d(g, sg, d.eij + ne_old, S.eij.data() + ne_old, nn));
  RC_TRY(staged_h2d(g, sg, d.ez + ne_old, hz.data(), hz.size()));
  RC_TRY(staged_h2d(g, sg, d.eom + 3 * (size_t)ne_old, hom.data(), hom.size()));
  RC_TRY(staged_h2d(g, sg, d.prior_ptr + n_old + 1, S.prior_ptr.data() + n_old + 1, n - n_old));
  RC_TRY(staged_h2d(g, sg, d.row_ptr + dl.r0 + 1, S.row_ptr.data() + dl.r0 + 1, n - dl.r0));
  RC_TRY(staged_h2d(g, sg, d.slot_edge + dl.k0, S.codes().data() + dl.k0, ns - dl.k0));
  RC_TRY(staged_h2d(g, sg, d.slot_col + dl.k0, S.slot_col.data() + dl.k0, ns - dl.k0));
  RC_TRY(staged_h2d(g, sg, d.erow + dl.x0 + 1, S.erow.data() + dl.x0 + 1, n - dl.x0));
  RC_TRY(staged_h2d(g, sg, d.s1_ptr + dl.y0 + 1, S.s1_ptr.data() + dl.y0 + 1, n - dl.y0));
  RC_TRY(staged_h2d(g, sg, d.s1pos, S.s1pos.data(), ne));
  std::vector<unsigned char> hl;   // (alive until the stream has drained below: a full staging
  std::vector<double> hk;          // buffer falls back to copies from these)
  if (d.eloss) {
    gather_losses(g, nd, nn, hl, hk);
    RC_TRY(staged_h2d(g, sg, d.eloss + ne_old, hl.data(), hl.size()));
    RC_TRY(staged_h2d(g, sg, d.ek + ne_old, hk.data(), hk.size()));
    RC_TRY(staged_h2d(g, sg, d.s1fac, S.s1fac.data(), S.s1fac.size()));
  }
  for (int y : dl.dc_rows) RC_TRY(staged_h2d(g, sg, d.Dc + 6 * (size_t)y, S.Dc.data() + 6 * (size_t)y, 6));
  RC_TRY(staged_h2d(g, sg, d.Dc + 6 * (size_t)n_old, S.Dc.data() + 6 * (size_t)n_old, 6 * (size_t)(n - n_old)));
  RC_TRY(staged_h2d(g, sg, d.brow, S.brow.data(), S.brow.size()));
  RC_TRY(stage_end(g, sg));
  d.n = n;
  d.ne = ne;
  d.nslots = ns;
  d.nlb = (int)S.brow.size() - 1;
  d.G = S.G;
  d.G1 = S.G1;
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  g->dev_structure = true;
  g->last_upload = 2;
  if (g->chol_ready) g->plan_stale = true;   // ensure_chol decides what to keep
  phase("upload");
  // the new vertices' values (the resident ones stay bit for bit, unless the
  // caller set values since: then all of them)
  return upload_values(g, g->dev_values ? n_old : 0);
}

int ensure_device(pgo_graph* g) {
  if (!g->dev_structure) {
    const int rc = append_structure(g);
    if (rc == 1) RC_TRY(upload_structure(g));
    else if (rc != PGO_OK) return rc;
  }
  else if (!g->dev_values) RC_TRY(upload_values(g));
  return PGO_OK;
}

int sync_scalars(pgo_graph* g, int count) {
  HIP_TRY(g, hipMemcpyAsync(g->h_scal, g->d.scal, count * sizeof(double), hipMemcpyDeviceToHost, g->d.stream));
  HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  return PGO_OK;
}

int device_error(pgo_graph* g, const double4* pose, double* err) {
  HIP_TRY(g, pgo::launch_error(g->d, pose, g->d.scal));
  RC_TRY(sync_scalars(g, 1));
  *err = g->h_scal[0];
  return PGO_OK;
}

struct PcgResult {
  int flag = pgo::kRunning;
  int iterations = 0;
};

double ms_between(hipEvent_t a, hipEvent_t b);

int exchange_allgather(void* ctx, const void* send, void* recv, size_t bytes, hipStream_t s) {
  pgo_graph* g = static_cast<pgo_graph*>(ctx);
  std::string why;
  const int rc = pgo::comm_allgather_device(g->part_comm, send, recv, bytes, s, &why);
  if (rc != PGO_OK) g->last_error = "partition exchange: " + why;
  return rc == PGO_OK ? 0 : -1;
}

int exchange_broadcast(void* ctx, void* buf, size_t bytes, int root, hipStream_t s) {
  pgo_graph* g = static_cast<pgo_graph*>(ctx);
  std::string why;
  const int rc = pgo::comm_broadcast_device_async(g->part_comm, buf, bytes, root, s, &why);
  if (rc != PGO_OK) g->last_error = "panel exchange: " + why;
  return rc == PGO_OK ? 0 : -1;
}

int exchange_group(void* ctx, int begin) {
  pgo_graph* g = static_cast<pgo_graph*>(ctx);
  std::string why;
  const int rc = pgo::comm_group(g->part_comm, begin, &why);
  if (rc != PGO_OK) g->last_error = "panel exchange group: " + why;
  return rc == PGO_OK ? 0 : -1;
}

int bind_plan(pgo_graph* g, bool full);

// Before a PCG linearisation: an in-place append after a Cholesky plan left
// the device owner bits (and their host mirror, GraphStructure::codes) half the
// plan's, half pre-plan; upload the pre-plan codes whole so every factor has
// exactly one `se & 2` slot.
int unmix_slot_codes(pgo_graph* g) {
  if (!g->gs.unbind()) return PGO_OK;
  RC_TRY(h2d(g, g->d.slot_edge, g->gs.codes().data(), g->gs.codes().size()));
  HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  return PGO_OK;
}

int ensure_chol(pgo_graph* g) {
  const int psz = g->part_size > 1 ? g->part_comm->size : 1, prk = psz > 1 ? g->part_comm->rank : 0;
  if (g->chol_ready && (g->chol.part_size != psz || g->chol.part_rank != prk)) {   // other partition: re-plan
    (void)hipStreamSynchronize(g->d.stream);
    free_lanes(g);
    drop_graphs(g);
    pgo::chol_free(g->chol);
    g->chol_ready = false;
    g->lane_cap = 8;
  }
  const auto t0 = std::chrono::steady_clock::now();
  auto timed = [&](int kind) {
    g->plan_update = kind;
    g->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  g->plan_update = 0;
  g->plan_ms = 0.0;
  std::vector<int> order_in;
  if (g->chol_ready && g->plan_stale) {
    // the graph grew since the plan (pgo_add_edge / pgo_add_vertex after an
    // optimize: the live per-registration re-solve, graph.cpp:180-200).  Factors
    // whose blocks fit the plan's fronts (a loop closure inside existing fill):
    // keep the plan, rebuild only the H assembly lists.  New vertices / fill:
    // re-plan on the previous ordering with the new poses inserted in front of
    // their earliest-eliminated neighbour (no new nested dissection) while the
    // appended part is small; otherwise a full analysis.
    pgo::CholPlan& P = g->chol;
    const int n = g->d.n;
    std::vector<int2> pairs;   // the factors added since the plan (vertex indices)
    for (size_t e = g->plan_edges; e < g->ek1.size(); e++)
      pairs.push_back(make_int2(g->index.at(g->ek1[e]), g->index.at(g->ek2[e])));
    if (n == P.n && pgo::chol_covers(P, pairs)) {
      pgo::chol_assembly(P, g->gs.row_ptr, g->gs.slot_col);
      RC_TRY(bind_plan(g, false));
      g->plan_stale = false;
      g->plan_edges = g->ek1.size();
      g->eager_first = 8;
      timed(1);
      return PGO_OK;
    }
    // appended poses: into the plan incrementally while the tail is short and
    // the factor has not grown much (then a re-plan below)
    constexpr int kMaxTail = 64;
    pgo::PhaseTimer phase("ensure_chol");
    if (!getenv("PGO_NO_PLAN_APPEND") && pgo::chol_append(P, n, g->gs.row_ptr, g->gs.slot_col, pairs, kMaxTail, 1.05)) {
      phase("chol_append");
      if (P.schedule_error) return fail(g, PGO_E_HIP, "internal: inconsistent panel schedule");
      drop_graphs(g, true);
      RC_TRY(bind_plan(g, true));
      g->plan_stale = false;
      g->plan_edges = g->ek1.size();
      g->eager_first = 8;
      timed(4);
      return PGO_OK;
    }
    if (n >= P.n && n - P.n <= std::max(256, P.n / 10)) {
      // (base, order): old pose k -> (iperm[k], 0); a new pose -> (min base of its
      // already-placed neighbours, -(index)), so it is eliminated just before that
      // neighbour, later new poses before earlier ones (leaves of the chain first)
      const int n0 = P.n;
      std::vector<long long> key(n);
      for (int k = 0; k < n0; k++) key[k] = (long long)P.iperm[k] << 32;
      for (int v = n0; v < n; v++) {
        long long base = n;
        for (int q = g->gs.row_ptr[v]; q < g->gs.row_ptr[v + 1]; q++) {
          const int u = g->gs.slot_col[q];
          if (u < v) base = std::min(base, key[u] >> 32);
        }
        key[v] = (base << 32) | (0x7fffffffLL - (v - n0 + 1));   // below the old pose's 0x7fffffff
      }
      for (int k = 0; k < n0; k++) key[k] |= 0x7fffffffLL;
      order_in.resize(n);
      for (int k = 0; k < n; k++) order_in[k] = k;
      std::stable_sort(order_in.begin(), order_in.end(), [&](int a, int b) { return key[a] < key[b]; });
    }
    (void)hipStreamSynchronize(g->d.stream);
    free_lanes(g);
    drop_graphs(g);
    pgo::chol_free(P);
    g->chol_ready = false;
    g->lane_cap = 8;
  }
  g->plan_stale = false;
  if (g->chol_ready) return PGO_OK;
  g->chol.ordering = g->ordering;
  g->chol.part_size = psz;
  g->chol.part_rank = prk;
  g->chol.order_in = order_in;
  g->hook.ctx = g;
  g->hook.allgather = exchange_allgather;
  g->hook.broadcast = exchange_broadcast;
  g->hook.group = exchange_group;
  pgo::chol_analyze(g->chol, g->d.n, g->gs.row_ptr, g->gs.slot_col);
  g->gs.order_changed();   // (a new order: every owner bit)
  if (g->chol.schedule_error) return fail(g, PGO_E_HIP, "internal: inconsistent panel schedule");
  const auto tb = std::chrono::steady_clock::now();
  RC_TRY(bind_plan(g, true));
  if (getenv("PGO_PLAN_TIMING"))
    fprintf(stderr, "ensure_chol bind_plan %8.2f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count());
  g->chol_ready = true;
  g->plan_edges = g->ek1.size();
  g->eager_first = 0;
  timed(order_in.empty() ? 3 : 2);
  return PGO_OK;
}

// Bind the plan to the device graph: owner slot of every factor := its block
// in the lower triangle of the permuted matrix (the one the assembly reads;
// with write_all = 0 the linearisation writes only these), the assembly's
// sources remapped slot -> factor, and the plan (full) or its assembly lists
// uploaded.
int bind_plan(pgo_graph* g, bool full) {
  pgo::PhaseTimer phase("bind_plan");
  const pgo::SlotRange up = g->gs.bind(g->chol.iperm);
  const std::vector<int>& slot_edge = g->gs.codes();
  const std::vector<unsigned char>& eside = g->gs.eside();
  std::vector<int>& src = g->chol.asm_src;
  pgo::host_parallel((int)src.size(), [&](int q0, int q1) {
    for (int q = q0; q < q1; q++)   // (~slot: not yet bound; kept ones are factor indices already)
      if (src[q] < 0) src[q] = slot_edge[~src[q]] >> 2;
  });
  g->chol.asm_bound = true;
  phase("owners");
  const hipError_t e = full ? pgo::chol_upload(g->chol, g->d.stream) : pgo::chol_upload_assembly(g->chol, g->d.stream);
  if (e != hipSuccess) {
    pgo::chol_free(g->chol);
    g->gs.order_changed();   // (the device never got these bits: the next bind uploads every slot)
    return fail(g, e == hipErrorOutOfMemory ? PGO_E_NOMEM : PGO_E_HIP,
                std::string("Cholesky plan upload: ") + hipGetErrorString(e));
  }
  phase("chol_upload");
  if (!g->d.eside) RC_TRY(dev_alloc(g, &g->d.eside, std::max<size_t>(g->cap_ne, g->d.ne)));
  if (g->stage.buf) {   // pinned staging: the copies (and the fronts' zeroing) run on unsynchronised
    RC_TRY(stage_begin(g, g->stage));
    RC_TRY(staged_h2d(g, g->stage, g->d.eside, eside.data(), eside.size()));
    RC_TRY(staged_h2d(g, g->stage, g->d.slot_edge + up.begin, slot_edge.data() + up.begin, (size_t)(up.end - up.begin)));
    RC_TRY(stage_end(g, g->stage));
  } else {
    RC_TRY(h2d(g, g->d.eside, eside.data(), eside.size()));
    RC_TRY(h2d(g, g->d.slot_edge + up.begin, slot_edge.data() + up.begin, (size_t)(up.end - up.begin)));
    HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  }
  phase("slots");
  return PGO_OK;
}

// PCG solve of (H + lambda I) x = -g at the current linearisation.  With
// profile_every = k > 0, every k-th SpMV launch is bracketed by HIP events on
// the handle's stream; launches that ran after convergence (early-exit no-ops)
// are not counted.
int pcg_solve(pgo_graph* g, const pgo_params& p, double lam, PcgResult* out, pgo_stats* st) {
  const DevGraph& d = g->d;
  HIP_TRY(g, pgo::launch_pcg_init(d, lam));
  const double tol2 = p.pcg_relative_tol * p.pcg_relative_tol;
  const int chk = std::max(1, p.pcg_check_interval);
  const int prof = st ? p.profile_every : 0;
  int k = 0;
  out->flag = pgo::kRunning;
  while (k < p.pcg_max_iterations) {
    const int stop = std::min(p.pcg_max_iterations, k + chk);
    int npairs = 0;
    for (; k < stop; k++) {
      const bool timed = prof > 0 && (k % prof) == 0 && npairs < pgo_graph::kProfPairs;
      if (timed) {
        HIP_TRY(g, pgo::launch_pcg_spmv(d, lam, g->pev[2 * npairs], g->pev[2 * npairs + 1]));
        g->pk_iter[npairs++] = k;
      } else {
        HIP_TRY(g, pgo::launch_pcg_spmv(d, lam));
      }
      HIP_TRY(g, pgo::launch_pcg_vec(d, k, tol2));
    }
    HIP_TRY(g, hipMemcpyAsync(g->h_ctrl, d.ctrl, 2 * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(g, hipStreamSynchronize(d.stream));
    for (int t = 0; t < npairs; t++)
      if (g->pk_iter[t] < g->h_ctrl[1] || (g->h_ctrl[0] == pgo::kRunning)) {
        st->kernel_spmv_ms += ms_between(g->pev[2 * t], g->pev[2 * t + 1]);
        st->kernel_spmv_count++;
      }
    if (g->h_ctrl[0] != pgo::kRunning) break;
  }
  out->flag = g->h_ctrl[0];
  out->iterations = g->h_ctrl[1];
  return PGO_OK;
}

// (H + lambda I) x = -g.  PCG runs to completion here (its convergence reads
// sync); the Cholesky path is only enqueued and its pivot flag is read back with
// the next scalars (*known = false).
struct SolveState {
  bool known = true, solved = true;
  bool profiled = false;
  bool graph = false;                       // factor / solve replayed from graphs (ev[5] between them)
  pgo::LaunchProfile prof;
};

// Replay of the captured factorisation and solve graphs for nb lanes (captured
// on first use; one graph launch each instead of ~1e3 kernel launches), with
// ev[5] recorded between them: the factorisation's device time is ev[2]..ev[5].
int graph_factor_solve(pgo_graph* g, int nb, double* x, long long xstride, bool capture_now) {
  DevGraph& d = g->d;
  // after an incremental plan update the first factorisations per lane count
  // run eagerly: capturing ~1e3 launches costs ~14 ms on C3 and destroying the
  // graphs ~10 ms, more than a few replays gain -- the live re-solve refreshes
  // the plan every registration and factors it ~4 times (eager_first)
  if (!capture_now && !g->fac_exec[nb] && g->graph_eager[nb] < g->eager_first) {
    g->graph_eager[nb]++;
    HIP_TRY(g, pgo::chol_factor(g->chol, d.D, d.V, d.g, -1.0, d.stream, nullptr, nb));
    HIP_TRY(g, hipEventRecord(g->ev[5], d.stream));
    HIP_TRY(g, pgo::chol_solve(g->chol, x, d.stream, nb, xstride));
    return PGO_OK;
  }
  auto capture = [&](hipGraphExec_t* exec, bool factor) -> int {
    if (*exec) return PGO_OK;
    pgo::PhaseTimer phase("graph_capture");
    destroy_stale_graphs(g);
    hipGraph_t graph = nullptr;
    HIP_TRY(g, hipStreamBeginCapture(d.stream, hipStreamCaptureModeThreadLocal));
    const hipError_t e1 = factor ? pgo::chol_factor(g->chol, d.D, d.V, d.g, -1.0, d.stream, nullptr, nb)
                                 : pgo::chol_solve(g->chol, x, d.stream, nb, xstride);
    HIP_TRY(g, hipStreamEndCapture(d.stream, &graph));
    HIP_TRY(g, e1);
    HIP_TRY(g, hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
    HIP_TRY(g, hipGraphDestroy(graph));
    phase(factor ? "factor" : "solve");
    return PGO_OK;
  };
  RC_TRY(capture(&g->fac_exec[nb], true));
  RC_TRY(capture(&g->sol_exec[nb], false));
  HIP_TRY(g, hipGraphLaunch(g->fac_exec[nb], d.stream));
  HIP_TRY(g, hipEventRecord(g->ev[5], d.stream));
  HIP_TRY(g, hipGraphLaunch(g->sol_exec[nb], d.stream));
  return PGO_OK;
}

int linear_solve(pgo_graph* g, const pgo_params& p, double lam, pgo_stats* st, SolveState* ss) {
  if (p.linear_solver == PGO_SOLVER_PCG) {
    PcgResult pr;
    RC_TRY(pcg_solve(g, p, lam, &pr, st));
    if (st) st->pcg_iterations += pr.iterations;
    ss->known = true;
    ss->solved = pr.flag != pgo::kBreakdown;
    return PGO_OK;
  }
  RC_TRY(ensure_chol(g));
  const DevGraph& d = g->d;
  ss->profiled = st && p.profile_every > 0 && (g->factorizations % p.profile_every) == 0;
  g->factorizations++;
  pgo::LaunchProfile* prof = nullptr;
  if (ss->profiled) {
    ss->prof.ev = g->sev.data();
    ss->prof.cap = kProfLaunches;
    ss->prof.used = 0;
    ss->prof.fam = g->sev_fam.data();
    ss->prof.flops = g->sev_flops.data();
    ss->prof.bytes = g->sev_bytes.data();
    ss->prof.grid = g->sev_grid.data();
    ss->prof.tag = g->sev_tag.data();
    prof = &ss->prof;
  }
  *g->h_lam = lam;
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lam, sizeof(double), hipMemcpyHostToDevice, d.stream));
  const bool part = g->chol.part_size > 1;
  if (prof || !p.use_graphs || part) {  // eager: a profiled factorisation times every launch; the
                                        // partitioned one runs its exchanges between the phases
    pgo::ExchangeHook* hook = part ? &g->hook : nullptr;
    g->hook.failed = false;
    if (prof) HIP_TRY(g, hipEventRecord(g->fev[0], d.stream));
    const hipError_t ef = pgo::chol_factor(g->chol, d.D, d.V, d.g, -1.0, d.stream, prof, 1, hook);
    if (g->hook.failed) return fail(g, PGO_E_COMM, g->last_error);
    HIP_TRY(g, ef);
    if (prof) HIP_TRY(g, hipEventRecord(g->fev[1], d.stream));
    const hipError_t es = pgo::chol_solve(g->chol, d.x, d.stream, 1, 0, prof, hook);
    if (g->hook.failed) return fail(g, PGO_E_COMM, g->last_error);
    HIP_TRY(g, es);
    if (prof) HIP_TRY(g, hipEventRecord(g->fev[2], d.stream));
  } else {
    RC_TRY(graph_factor_solve(g, 1, d.x, 0, false));
    ss->graph = true;
  }
  ss->known = false;
  return PGO_OK;
}

// after the stream has drained: pivot flag and profile of an enqueued Cholesky solve
int finish_solve(pgo_graph* g, pgo_stats* st, SolveState* ss) {
  if (ss->known) return PGO_OK;
  if (ss->graph && st) {
    st->ms_factor_graph += ms_between(g->ev[2], g->ev[5]);
    st->factor_graph_flops += g->chol.flops;
  }
  int flag = 0;
  HIP_TRY(g, hipMemcpy(&flag, g->chol.d_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (flag & 2) {
    g->handoff_timeout = true;
    return fail(g, PGO_E_HIP, "factorisation: an in-launch hand-off timed out");
  }
  ss->solved = flag == 0;
  ss->known = true;
  if (st) st->factor_flops = g->chol.flops;
  if (ss->profiled && st) {
    for (int u = 0; u < ss->prof.used; u++) {
      const int f = ss->prof.fam[u];
      const double ms = ms_between(ss->prof.ev[2 * u], ss->prof.ev[2 * u + 1]);
      g->fam_ms[f] += ms;
      g->fam_flops[f] += ss->prof.flops[u];
      g->fam_bytes[f] += ss->prof.bytes[u];
      g->fam_launches[f]++;
      if (f == pgo::kFamPanelSyrk || f == pgo::kFamPanelSyrk128) {
        st->kernel_syrk_ms += ms;
        st->kernel_syrk_launches++;
      }
    }
    st->kernel_syrk_count++;
    st->syrk_flops = g->chol.syrk_flops;
    if (getenv("PGO_STEP_STAMPS") && getenv("PGO_PROFILE_DUMP")) {   // top level's k_step stamps
      std::vector<unsigned long long> stp(10 * pgo::kMaxStampSlots);
      if (pgo::chol_step_stamps(stp.data(), pgo::kMaxStampSlots) == hipSuccess)
        if (FILE* f = fopen(getenv("PGO_PROFILE_DUMP"), "a")) {
          for (int q = 0; q < pgo::kMaxStampSlots; q++) {
            const unsigned long long* t = &stp[10 * q];
            if (!t[0] || !t[5]) continue;
            fprintf(f, "# stamp step %d:", q);
            for (int k = 1; k < 9; k++) fprintf(f, " %.2f", (double)((long long)(t[k] - t[0])) * 0.01);
            fprintf(f, "\n");
          }
          fclose(f);
        }
    }
    // PGO_PROFILE_DUMP=path: append the launch timeline of this factorisation
    // (family, level, panel step, workgroups, start and duration in ms from the
    // factorisation's first event, algorithmic flops, bytes)
    if (const char* path = getenv("PGO_PROFILE_DUMP")) {
      if (FILE* f = fopen(path, "a")) {
        fprintf(f, "# factorisation %lld\n", g->factorizations - 1);
        for (int u = 0; u < ss->prof.used; u++)
          fprintf(f, "%s %d %d %d %.4f %.4f %.4g %.4g\n", pgo::kernel_family_name(ss->prof.fam[u]),
                  ss->prof.tag[u] >> 16, ss->prof.tag[u] & 0xffff, ss->prof.grid[u],
                  ms_between(g->fev[0], ss->prof.ev[2 * u]), ms_between(ss->prof.ev[2 * u], ss->prof.ev[2 * u + 1]),
                  ss->prof.flops[u], ss->prof.bytes[u]);
        fclose(f);
      }
    }
    st->ms_factor_profiled += ms_between(g->fev[0], g->fev[1]);
    st->ms_solve_profiled += ms_between(g->fev[1], g->fev[2]);
  }
  return PGO_OK;
}

// Lanes 1..want-1 over the current Cholesky plan (numeric workspaces for want
// lanes); returns the lane count available (fewer when HBM runs out: each lane
// holds a full set of fronts).
int ensure_lanes(pgo_graph* g, int want) {
  want = std::max(1, std::min({want, 8, g->lane_cap}));
  if ((int)g->lanes.size() == want - 1 && g->chol.batch >= want) return want;
  free_lanes(g);
  const DevGraph& d = g->d;
  if (g->chol.batch != want) {
    // the captured graphs hold the old workspace pointers
    drop_graphs(g);
    if (pgo::chol_set_batch(g->chol, want, d.stream) != hipSuccess) {
      (void)hipGetLastError();
      g->lane_cap = 1;
      return 1;
    }
  }
  g->xb_n = std::max<size_t>({g->cap_n, (size_t)d.n, 1});   // appended vertices keep the lanes
  bool ok = hipMalloc((void**)&g->xb, sizeof(double) * 3 * g->xb_n * want) == hipSuccess;
  for (int l = 1; l < want && ok; l++) {
    g->lanes.emplace_back();
    Lane& ln = g->lanes.back();
    // (capacity, not n: an accepted lane's buffer becomes the handle's pose
    // array, which appended vertices extend in place)
    ok = hipMalloc((void**)&ln.pose_cand, sizeof(double4) * std::max<size_t>({g->cap_n, (size_t)d.n, 1})) ==
             hipSuccess &&
         hipMalloc((void**)&ln.part, sizeof(double) * pgo::kMaxBlocks * pgo::kPartSlices) == hipSuccess &&
         hipMalloc((void**)&ln.scal, sizeof(double) * 16) == hipSuccess &&
         hipMemsetAsync(ln.part, 0, sizeof(double) * pgo::kMaxBlocks * pgo::kPartSlices, d.stream) == hipSuccess;
  }
  if (ok) ok = hipStreamSynchronize(d.stream) == hipSuccess;
  if (!ok) {  // out of memory (or similar): one lane, and do not try again for this plan
    (void)hipGetLastError();
    free_lanes(g);
    drop_graphs(g);
    (void)pgo::chol_set_batch(g->chol, 1, d.stream);
    g->lane_cap = 1;
    return 1;
  }
  return want;
}

// The device view of lane l's try (lane 0: the handle's own buffers), solution in xb
DevGraph lane_view(const pgo_graph* g, int l) {
  DevGraph v = g->d;
  v.x = g->xb + (size_t)l * 3 * g->d.n;
  if (l == 0) return v;
  const Lane& ln = g->lanes[l - 1];
  v.pose_cand = ln.pose_cand;
  v.part = ln.part;
  v.scal = ln.scal;
  return v;
}

// nb >= 2 consecutive lambda tries in one batched factor + solve (captured
// graph per lane count), then per lane: model decrease, retract, error; one
// read-back.  out[l]: lane l's outcome.
int run_lanes(pgo_graph* g, const pgo_params& p, int nb, const double* lams, pgo::TryOutcome* out, pgo_stats* st) {
  DevGraph& d = g->d;
  hipEvent_t* ev = g->ev;
  g->factorizations++;
  for (int l = 0; l < nb; l++) g->h_lanes[4 * 8 + l] = lams[l];
  HIP_TRY(g, hipEventRecord(ev[2], d.stream));
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lanes + 4 * 8, nb * sizeof(double), hipMemcpyHostToDevice,
                            d.stream));
  const bool part = g->chol.part_size > 1;
  if (!p.use_graphs || part) {   // (partitioned: eager, the exchanges run between the phases)
    pgo::ExchangeHook* hook = part ? &g->hook : nullptr;
    g->hook.failed = false;
    const hipError_t ef = pgo::chol_factor(g->chol, d.D, d.V, d.g, -1.0, d.stream, nullptr, nb, hook);
    if (g->hook.failed) return fail(g, PGO_E_COMM, g->last_error);
    HIP_TRY(g, ef);
    const hipError_t es = pgo::chol_solve(g->chol, g->xb, d.stream, nb, 3LL * d.n, nullptr, hook);
    if (g->hook.failed) return fail(g, PGO_E_COMM, g->last_error);
    HIP_TRY(g, es);
  } else {
    RC_TRY(graph_factor_solve(g, nb, g->xb, 3LL * d.n, false));
  }
  HIP_TRY(g, hipEventRecord(ev[3], d.stream));
  for (int l = 0; l < nb; l++) {
    const DevGraph v = lane_view(g, l);
    HIP_TRY(g, pgo::launch_model_decrease(v, v.x, v.scal + 1));
    HIP_TRY(g, pgo::launch_retract(v, v.x));
    HIP_TRY(g, pgo::launch_error(v, v.pose_cand, v.scal));
    HIP_TRY(g, hipMemcpyAsync(g->h_lanes + 4 * l, v.scal, 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  }
  if (d.eloss)   // the linearised error of this linearisation (launch_error_lin), into lane 0's spare slot
    HIP_TRY(g, hipMemcpyAsync(g->h_lanes + 3, d.scal + 4, sizeof(double), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(g->h_lanes + 4 * 8 + 8, g->chol.d_flag, nb * sizeof(int), hipMemcpyDeviceToHost,
                            d.stream));
  HIP_TRY(g, hipEventRecord(ev[4], d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  int flags[8];
  std::memcpy(flags, g->h_lanes + 4 * 8 + 8, nb * sizeof(int));
  for (int l = 0; l < nb; l++)
    if (flags[l] & 2) {
      g->handoff_timeout = true;
      return fail(g, PGO_E_HIP, "factorisation: an in-launch hand-off timed out");
    }
  for (int l = 0; l < nb; l++)
    out[l] = {flags[l] == 0 ? 1.0 : 0.0, g->h_lanes[4 * l], g->h_lanes[4 * l + 1], g->h_lanes[4 * l + 2]};
  if (st) {
    st->ms_solve += ms_between(ev[2], ev[3]);
    st->ms_update += ms_between(ev[3], ev[4]);
    st->factor_flops = g->chol.flops;
    if (p.use_graphs && !part) {   // (ev[5] is recorded by the graph replay only)
      st->ms_factor_graph += ms_between(ev[2], ev[5]);
      st->factor_graph_flops += nb * g->chol.flops;
    }
  }
  return PGO_OK;
}

// scratch + timing events of the closest-keyframe search (first use)
int ensure_search(pgo_graph* g) {
  if (g->s_d) return PGO_OK;
  HIP_TRY(g, hipMalloc((void**)&g->s_i, sizeof(int) * (pgo::kMaxBlocks + 1)));
  for (hipEvent_t* e : {&g->sev_scan[0], &g->sev_scan[1], &g->sev_batch[0], &g->sev_batch[1]})
    HIP_TRY(g, hipEventCreate(e));
  HIP_TRY(g, hipMalloc((void**)&g->s_d, sizeof(double) * (pgo::kMaxBlocks + 1)));
  return PGO_OK;
}

double ms_between(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();   // (an unrecorded event must not surface as the next launch's error)
    return 0.0;
  }
  return ms;
}

}  // namespace

// ============================================================== C-ABI
extern "C" {

int pgo_abi_version(void) { return PGO_ABI_VERSION; }

const char* pgo_status_string(int s) {
  switch (s) {
    case PGO_OK: return "ok";
    case PGO_E_ARG: return "invalid argument";
    case PGO_E_DUP_KEY: return "ValuesKeyAlreadyExists: key already inserted";
    case PGO_E_NO_KEY: return "ValuesKeyDoesNotExist: key has no value";
    case PGO_E_BAD_COV: return "covariance is not symmetric positive definite";
    case PGO_E_INDETERMINANT: return "IndeterminantLinearSystemException: linear system is singular";
    case PGO_E_NONFINITE: return "non-finite value";
    case PGO_E_HIP: return "HIP runtime error";
    case PGO_E_NO_DEVICE: return "no HIP device";
    case PGO_E_NOMEM: return "out of memory";
    case PGO_E_BAD_EDGE: return "between factor connects a key to itself";
    case PGO_E_COMM: return "inter-rank exchange failed";
    case PGO_E_NOT_ENOUGH: return "not enough keyframes";
    case PGO_W_MAXITER: return "stopped at max_iterations";
    default: return "unknown status";
  }
}

void pgo_default_params(pgo_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 100;
  p->relative_error_tol = 1e-5;
  p->absolute_error_tol = 1e-5;
  p->error_tol = 0.0;
  p->lambda_initial = 1e-5;
  p->lambda_factor = 10.0;
  p->lambda_upper_bound = 1e5;
  p->lambda_lower_bound = 0.0;
  p->min_model_fidelity = 1e-3;
  p->use_fixed_lambda_factor = 1;
  p->algorithm = PGO_ALG_LM;
  p->linear_solver = PGO_SOLVER_CHOLESKY;
  p->pcg_relative_tol = 1e-10;
  p->pcg_max_iterations = 20000;
  p->pcg_check_interval = 32;
  p->max_outer = 0;
  p->profile_every = 0;
  p->use_graphs = 1;
  p->lambda_lanes = 1;
  p->multi_gpu = PGO_MULTI_SPECULATIVE;
}

pgo_graph* pgo_create(const pgo_opts* opts) {
  pgo_graph* g = new (std::nothrow) pgo_graph();
  if (!g) return nullptr;
  if (opts) {
    if (opts->ordering != PGO_ORDERING_ND && opts->ordering != PGO_ORDERING_AMD) {
      delete g;
      return nullptr;
    }
    g->device = opts->device;
    g->ordering = opts->ordering == PGO_ORDERING_AMD ? pgo::kOrderAmd : pgo::kOrderNd;
  }
  return g;
}

void pgo_destroy(pgo_graph* g) {
  if (!g) return;
  if (g->comm.nccl || g->comm.d_gather || g->pcomm.nccl || g->pcomm.d_gather) (void)hipSetDevice(g->device);
  pgo::comm_free(&g->comm);
  pgo::comm_free(&g->pcomm);
  if (g->hip_ready) {
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->d.stream);
    free_device(g);
    for (auto& e : g->ev)
      if (e) (void)hipEventDestroy(e);
    if (g->h_scal) (void)hipHostFree(g->h_scal);
    if (g->h_ctrl) (void)hipHostFree(g->h_ctrl);
    if (g->h_lam) (void)hipHostFree(g->h_lam);
    if (g->stage.buf) (void)hipHostFree(g->stage.buf);
    if (g->stage.done) (void)hipEventDestroy(g->stage.done);
    if (g->h_lanes) (void)hipHostFree(g->h_lanes);
    for (auto& e : g->pev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : g->sev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : g->fev)
      if (e) (void)hipEventDestroy(e);
    if (g->lin_done) (void)hipEventDestroy(g->lin_done);
    void* sp[] = {g->s_d, g->s_i, g->sb_d, g->sb_i, g->sb_q, g->sbp_d, g->sbp_i, g->init_tgt};
    for (void* q : sp)
      if (q) (void)hipFree(q);
    for (hipEvent_t e : {g->sev_scan[0], g->sev_scan[1], g->sev_batch[0], g->sev_batch[1]})
      if (e) (void)hipEventDestroy(e);
    if (g->d.stream) (void)hipStreamDestroy(g->d.stream);
  }
  delete g;
}

const char* pgo_last_error(const pgo_graph* g) { return g ? g->last_error.c_str() : "null handle"; }

int pgo_add_vertex(pgo_graph* g, uint64_t key, double x, double y, double theta) {
  if (!g) return PGO_E_ARG;
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(theta))
    return fail(g, PGO_E_NONFINITE, "non-finite initial value for key " + std::to_string(key));
  if (g->index.count(key)) return fail(g, PGO_E_DUP_KEY, "key " + std::to_string(key) + " already inserted");
  // (no download: the resident values stay on the device, the new one is host-side
  // until the next upload -- download_values reads back the resident ones only)
  g->index.emplace(key, (int32_t)g->keys.size());
  g->keys.push_back(key);
  g->xyt.insert(g->xyt.end(), {x, y, theta});
  g->dev_structure = false;
  return PGO_OK;
}

// Bulk adds leave 1/8 room in the host arrays (and the key index), as the device
// arrays have: the live node's first single appends after a bulk load then do
// not copy the whole graph (a 500k-factor graph: ~46 MB, ~9 ms).
static size_t with_room(size_t n) { return n + n / 8 + 64; }

int pgo_add_vertices(pgo_graph* g, size_t n, const uint64_t* keys, const double* xyt) {
  if (!g || (n && (!keys || !xyt))) return PGO_E_ARG;
  const size_t nv = with_room(g->keys.size() + n);
  if (g->keys.capacity() < g->keys.size() + n) {
    g->keys.reserve(nv);
    g->xyt.reserve(3 * nv);
    g->index.reserve(nv);
  }
  for (size_t i = 0; i < n; i++) RC_TRY(pgo_add_vertex(g, keys[i], xyt[3 * i], xyt[3 * i + 1], xyt[3 * i + 2]));
  return PGO_OK;
}

int pgo_add_prior(pgo_graph* g, uint64_t key, const double pose[3], const double cov[9]) {
  if (!g || !pose || !cov) return PGO_E_ARG;
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(pose[a])) return fail(g, PGO_E_NONFINITE, "non-finite prior pose");
  double om[6];
  if (information(cov, om) != PGO_OK) return fail(g, PGO_E_BAD_COV, "prior covariance not positive definite");
  g->pk.push_back(key);
  g->pz.insert(g->pz.end(), pose, pose + 3);
  g->pom.insert(g->pom.end(), om, om + 6);
  g->dev_structure = false;
  return PGO_OK;
}

int pgo_add_edge(pgo_graph* g, uint64_t k1, uint64_t k2, const double z[3], const double cov[9]) {
  if (!g || !z || !cov) return PGO_E_ARG;
  if (k1 == k2) return fail(g, PGO_E_BAD_EDGE, "between factor on key " + std::to_string(k1) + " and itself");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(z[a])) return fail(g, PGO_E_NONFINITE, "non-finite measurement");
  double om[6];
  if (information(cov, om) != PGO_OK)
    return fail(g, PGO_E_BAD_COV, "between factor covariance not positive definite");
  if (g->ek1.size() >= (size_t)(1 << 30)) return fail(g, PGO_E_NOMEM, "too many factors");
  g->ek1.push_back(k1);
  g->ek2.push_back(k2);
  g->ez.insert(g->ez.end(), z, z + 3);
  g->eom.insert(g->eom.end(), om, om + 6);
  g->eloss.push_back(PGO_LOSS_NONE);
  g->ek.push_back(1.0);
  g->dev_structure = false;
  return PGO_OK;
}

static int check_loss(pgo_graph* g, int loss, double k) {
  if (loss < PGO_LOSS_NONE || loss > PGO_LOSS_GEMAN_MCCLURE) return fail(g, PGO_E_ARG, "unknown robust loss");
  if (loss != PGO_LOSS_NONE && !(std::isfinite(k) && k > 0.0))
    return fail(g, PGO_E_ARG, "robust loss parameter k must be finite and positive");
  if (!std::isfinite(k)) return fail(g, PGO_E_ARG, "robust loss parameter k must be finite");
  return PGO_OK;
}

int pgo_add_edge_robust(pgo_graph* g, uint64_t k1, uint64_t k2, const double z[3], const double cov[9], int loss,
                        double k) {
  if (!g) return PGO_E_ARG;
  RC_TRY(check_loss(g, loss, k));
  RC_TRY(pgo_add_edge(g, k1, k2, z, cov));
  if (loss != PGO_LOSS_NONE) {
    g->eloss.back() = (unsigned char)loss;
    g->ek.back() = k;
    g->n_robust++;
  }
  return PGO_OK;
}

int pgo_add_edges_robust(pgo_graph* g, size_t n, const uint64_t* k1, const uint64_t* k2, const double* z,
                         const double* cov, int cov_stride, const int* loss, const double* k, int loss_stride) {
  if (!g || (n && (!k1 || !k2 || !z || !cov || !loss || !k)) || (cov_stride != 0 && cov_stride != 9) ||
      (loss_stride != 0 && loss_stride != 1))
    return PGO_E_ARG;
  for (size_t i = 0; i < (loss_stride ? n : std::min<size_t>(n, 1)); i++) RC_TRY(check_loss(g, loss[i], k[i]));
  if (g->ek1.capacity() < g->ek1.size() + n) {
    const size_t ne = with_room(g->ek1.size() + n);
    g->ek1.reserve(ne);
    g->ek2.reserve(ne);
    g->ez.reserve(3 * ne);
    g->eom.reserve(6 * ne);
    g->eloss.reserve(ne);
    g->ek.reserve(ne);
  }
  for (size_t i = 0; i < n; i++)
    RC_TRY(pgo_add_edge_robust(g, k1[i], k2[i], z + 3 * i, cov + (size_t)cov_stride * i,
                               loss[(size_t)loss_stride * i], k[(size_t)loss_stride * i]));
  return PGO_OK;
}

int pgo_get_edge_weights(pgo_graph* g, size_t first, size_t n, double* out) {
  if (!g || (n && !out)) return PGO_E_ARG;
  const size_t ne = g->ek1.size();
  if (first > ne || n > ne - first) return fail(g, PGO_E_ARG, "edge_weights: range past the last between factor");
  if (n == 0) return PGO_OK;
  if (g->n_robust == 0) {   // an all-Gaussian graph: every weight is 1
    std::fill(out, out + n, 1.0);
    return PGO_OK;
  }
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  const DevGraph& d = g->d;
  double* dw = nullptr;
  HIP_TRY(g, hipMalloc((void**)&dw, sizeof(double) * ne));
  std::vector<double> hw(ne);
  hipError_t e = pgo::launch_edge_weights(d, dw);
  if (e == hipSuccess) e = hipMemcpyAsync(hw.data(), dw, sizeof(double) * ne, hipMemcpyDeviceToHost, d.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  (void)hipFree(dw);
  HIP_TRY(g, e);
  for (size_t de = 0; de < ne; de++) {
    const size_t u = (size_t)g->gs.dorder[de];
    if (u >= first && u < first + n) out[u - first] = hw[de];
  }
  return PGO_OK;
}

int pgo_add_edges(pgo_graph* g, size_t n, const uint64_t* k1, const uint64_t* k2, const double* z,
                  const double* cov, int cov_stride) {
  if (!g || (n && (!k1 || !k2 || !z || !cov)) || (cov_stride != 0 && cov_stride != 9)) return PGO_E_ARG;
  if (g->ek1.capacity() < g->ek1.size() + n) {
    const size_t ne = with_room(g->ek1.size() + n);
    g->ek1.reserve(ne);
    g->ek2.reserve(ne);
    g->ez.reserve(3 * ne);
    g->eom.reserve(6 * ne);
    g->eloss.reserve(ne);
    g->ek.reserve(ne);
  }
  for (size_t i = 0; i < n; i++) RC_TRY(pgo_add_edge(g, k1[i], k2[i], z + 3 * i, cov + (size_t)cov_stride * i));
  return PGO_OK;
}

size_t pgo_num_factors(const pgo_graph* g) { return g ? g->ek1.size() + g->pk.size() : 0; }
size_t pgo_num_vertices(const pgo_graph* g) { return g ? g->keys.size() : 0; }

int pgo_get_pose(pgo_graph* g, uint64_t key, double out[3]) {
  if (!g || !out) return PGO_E_ARG;
  auto it = g->index.find(key);
  if (it == g->index.end()) return fail(g, PGO_E_NO_KEY, "key " + std::to_string(key) + " has no value");
  RC_TRY(download_values(g));
  std::memcpy(out, &g->xyt[3 * (size_t)it->second], 3 * sizeof(double));
  return PGO_OK;
}

int pgo_get_poses(pgo_graph* g, size_t n, const uint64_t* keys, double* out) {
  if (!g || (n && !out)) return PGO_E_ARG;
  RC_TRY(download_values(g));
  if (!keys) {
    if (n != g->keys.size()) return fail(g, PGO_E_ARG, "n must equal the number of vertices when keys is NULL");
    if (n) std::memcpy(out, g->xyt.data(), 3 * n * sizeof(double));
    return PGO_OK;
  }
  for (size_t i = 0; i < n; i++) {
    auto it = g->index.find(keys[i]);
    if (it == g->index.end()) return fail(g, PGO_E_NO_KEY, "key " + std::to_string(keys[i]) + " has no value");
    std::memcpy(out + 3 * i, &g->xyt[3 * (size_t)it->second], 3 * sizeof(double));
  }
  return PGO_OK;
}

int pgo_set_poses(pgo_graph* g, size_t n, const uint64_t* keys, const double* xyt) {
  if (!g || (n && !xyt)) return PGO_E_ARG;
  RC_TRY(download_values(g));
  for (size_t i = 0; i < 3 * n; i++)
    if (!std::isfinite(xyt[i])) return fail(g, PGO_E_NONFINITE, "non-finite value");
  if (!keys) {
    if (n != g->keys.size()) return fail(g, PGO_E_ARG, "n must equal the number of vertices when keys is NULL");
    if (n) std::memcpy(g->xyt.data(), xyt, 3 * n * sizeof(double));
  } else {
    for (size_t i = 0; i < n; i++) {
      auto it = g->index.find(keys[i]);
      if (it == g->index.end()) return fail(g, PGO_E_NO_KEY, "key " + std::to_string(keys[i]) + " has no value");
      std::memcpy(&g->xyt[3 * (size_t)it->second], xyt + 3 * i, 3 * sizeof(double));
    }
  }
  g->dev_values = false;
  return PGO_OK;
}

int pgo_save_values(pgo_graph* g) {
  if (!g) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  DevGraph& d = g->d;
  if (!d.pose_saved) RC_TRY(dev_alloc(g, &d.pose_saved, std::max<size_t>(g->cap_n, d.n)));
  if (d.n)
    HIP_TRY(g, hipMemcpyAsync(d.pose_saved, d.pose, d.n * sizeof(double4), hipMemcpyDeviceToDevice, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  g->saved_valid = true;
  return PGO_OK;
}

int pgo_restore_values(pgo_graph* g) {
  if (!g) return PGO_E_ARG;
  DevGraph& d = g->d;
  if (!g->dev_structure || !d.pose_saved || !g->saved_valid)
    return fail(g, PGO_E_ARG, "no saved values (graph changed or never saved)");
  if (d.n)
    HIP_TRY(g, hipMemcpyAsync(d.pose, d.pose_saved, d.n * sizeof(double4), hipMemcpyDeviceToDevice, d.stream));
  g->dev_values = true;
  g->host_values = false;
  return PGO_OK;
}

int pgo_marginal_covariances(pgo_graph* g, size_t n, const uint64_t* keys, double* out) {
  if (!g || (n && (!keys || !out))) return PGO_E_ARG;
  if (n == 0) return PGO_OK;
  std::vector<int> poses(n);
  for (size_t i = 0; i < n; i++) {
    auto it = g->index.find(keys[i]);
    if (it == g->index.end()) return fail(g, PGO_E_NO_KEY, "marginal of key " + std::to_string(keys[i]) + " with no inserted value");
    poses[i] = it->second;
  }
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  g->part_size = 1;   // the path solves walk every front: a one-rank plan
  RC_TRY(ensure_chol(g));
  DevGraph& d = g->d;
  d.write_all = 0;
  HIP_TRY(g, pgo::launch_linearize(d));
  *g->h_lam = 0.0;
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lam, sizeof(double), hipMemcpyHostToDevice, d.stream));
  HIP_TRY(g, pgo::chol_factor(g->chol, d.D, d.V, d.g, 0.0, d.stream, nullptr));
  int flag = 0;
  HIP_TRY(g, hipMemcpyAsync(&flag, g->chol.d_flag, sizeof(int), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  if (flag) return fail(g, PGO_E_INDETERMINANT, "marginals: the linearised system is not positive definite");
  // batches bound the per-workgroup scratch (6 x max front rows doubles each)
  const size_t B = 256;
  for (size_t b0 = 0; b0 < n; b0 += B) {
    const int nb = (int)std::min(B, n - b0);
    HIP_TRY(g, pgo::chol_marginals(g->chol, poses.data() + b0, nb, out + 9 * b0, d.stream));
  }
  return PGO_OK;
}

int pgo_marginal_covariances_all(pgo_graph* g, double* cov, double* edge_cross) {
  if (!g) return PGO_E_ARG;
  if (g->keys.empty()) return PGO_OK;
  if (!cov) return PGO_E_ARG;
  RC_TRY(ensure_device(g));   // (a factor on a key never inserted: PGO_E_NO_KEY)
  HIP_TRY(g, hipSetDevice(g->device));
  g->part_size = 1;   // the pass walks every front: a one-rank plan
  RC_TRY(ensure_chol(g));
  DevGraph& d = g->d;
  d.write_all = 0;
  HIP_TRY(g, pgo::launch_linearize(d));
  *g->h_lam = 0.0;
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lam, sizeof(double), hipMemcpyHostToDevice, d.stream));
  HIP_TRY(g, pgo::chol_factor(g->chol, d.D, d.V, d.g, 0.0, d.stream, nullptr));
  int flag = 0;
  HIP_TRY(g, hipMemcpyAsync(&flag, g->chol.d_flag, sizeof(int), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  if (flag) return fail(g, PGO_E_INDETERMINANT, "marginals: the linearised system is not positive definite");
  const size_t ne = edge_cross ? g->ek1.size() : 0;
  bool changed = false;
  if (ne && (g->sel_etab_serial != g->chol.sel.serial || g->sel_etab.size() != ne)) {
    std::vector<int2> pairs(ne);
    for (size_t e = 0; e < ne; e++) pairs[e] = make_int2(g->index.at(g->ek1[e]), g->index.at(g->ek2[e]));
    g->sel_etab.resize(ne);
    pgo::selinv_edge_table(g->chol, pairs.data(), (long long)ne, g->sel_etab.data());
    g->sel_etab_serial = 0;
    for (const int4& t : g->sel_etab)
      if (t.x < 0) return fail(g, PGO_E_HIP, "internal: a factor's block is not in the Cholesky plan's fronts");
    g->sel_etab_serial = g->chol.sel.serial;
    changed = true;
  }
  const hipError_t e = pgo::chol_selinv(g->chol, g->sel_etab.data(), (long long)ne, changed, cov, edge_cross, d.stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(g, e == hipErrorOutOfMemory ? PGO_E_NOMEM : PGO_E_HIP,
                std::string("selected inversion: ") + hipGetErrorString(e));
  }
  return PGO_OK;
}

int pgo_error(pgo_graph* g, double* err) {
  if (!g || !err) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  return device_error(g, g->d.pose, err);
}

// ---- linear initialisation (pgo_init.h / pgo_init.hip; DESIGN.md "Linear initialisation")

// The host tree of the graph as it stands (keys resolved; no device).
static int init_host_tree(pgo_graph* g, pgo::InitTree& T) {
  pgo::PhaseTimer phase("init_host_tree");
  std::vector<int2> eij;
  RC_TRY(resolve_edges(g, 0, eij));
  phase("resolve");
  const size_t ne = eij.size(), np = g->pk.size();
  std::vector<int> pv(np);
  for (size_t q = 0; q < np; q++) {
    auto a = g->index.find(g->pk[q]);
    if (a == g->index.end())
      return fail(g, PGO_E_NO_KEY, "prior factor on key " + std::to_string(g->pk[q]) + " with no inserted value");
    pv[q] = a->second;
  }
  static_assert(sizeof(int2) == 2 * sizeof(int), "int2 is two packed ints");
  const bool ok = pgo::init_tree((int)g->keys.size(), ne, reinterpret_cast<const int*>(eij.data()),
                                 ne ? g->ez.data() + 2 : nullptr, 3, np, pv.data(), np ? g->pz.data() + 2 : nullptr, 3,
                                 &T);
  phase("tree");
  if (!ok)
    return fail(g, PGO_E_INDETERMINANT, "linear initialisation: the connected component of key " +
                                            std::to_string(g->keys[T.free_vertex]) + " has no prior");
  return PGO_OK;
}

// delta_e + 2 pi k_e per device factor, then theta_q + 2 pi k_q per device prior
static int init_upload_targets(pgo_graph* g, const pgo::InitTree& T) {
  constexpr double kTwoPi = 6.283185307179586476925286766559;
  const pgo::GraphStructure& S = g->gs;
  const size_t ne = (size_t)S.ne(), np = S.pv.size();
  if (g->init_tgt_cap < ne + np) {
    HIP_TRY(g, hipStreamSynchronize(g->d.stream));
    if (g->init_tgt) (void)hipFree(g->init_tgt);
    g->init_tgt = nullptr;
    g->init_tgt_cap = 0;
    const size_t cap = std::max(ne + np, g->cap_ne + np);
    RC_TRY(dev_alloc(g, &g->init_tgt, cap));
    g->init_tgt_cap = cap;
  }
  std::vector<double> h(ne + np);
  for (size_t k = 0; k < ne; k++) {
    const int e = S.dorder[k];
    h[k] = T.delta[e] + kTwoPi * (double)T.k_edge[e];
  }
  for (size_t t = 0; t < np; t++) {
    const int q = S.porder[t];
    h[ne + t] = pgo::init_wrap(g->pz[3 * (size_t)q + 2]) + kTwoPi * (double)T.k_prior[q];
  }
  RC_TRY(h2d(g, g->init_tgt, h.data(), h.size()));
  HIP_TRY(g, hipStreamSynchronize(g->d.stream));   // (the source is a local)
  return PGO_OK;
}

// x = A^-1 b of the system in (d.D, d.V, d.g), undamped, eager launches; the
// stream is drained and the pivot flag read.  A hand-off that timed out (a
// workgroup starved on a time-sliced GPU) is reported as finish_solve reports
// it, never re-run unseen: the values stay as they were.
static int init_factor_solve(pgo_graph* g, const char* what) {
  DevGraph& d = g->d;
  *g->h_lam = 0.0;
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lam, sizeof(double), hipMemcpyHostToDevice, d.stream));
  HIP_TRY(g, pgo::chol_factor(g->chol, d.D, d.V, d.g, 1.0, d.stream, nullptr));
  HIP_TRY(g, pgo::chol_solve(g->chol, d.x, d.stream));
  int flag = 0;
  HIP_TRY(g, hipMemcpyAsync(&flag, g->chol.d_flag, sizeof(int), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  if (flag & 2) {
    g->handoff_timeout = true;
    return fail(g, PGO_E_HIP, "factorisation: an in-launch hand-off timed out");
  }
  if (flag)
    return fail(g, PGO_E_INDETERMINANT, std::string("linear initialisation: the ") + what +
                                            " system is not positive definite");
  return PGO_OK;
}

int pgo_initialize_linear(pgo_graph* g, pgo_init_stats* stats) {
  if (!g) return PGO_E_ARG;
  pgo_init_stats st;
  std::memset(&st, 0, sizeof(st));
  const auto T0 = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  auto done = [&](int rc) {
    st.status = rc;
    st.ms_total = ms_since(T0);
    if (stats) *stats = st;
    return rc;
  };
  if (g->keys.empty()) return done(PGO_OK);
  // the tree first: a component without a prior is reported before any device work
  pgo::InitTree T;
  int rc = init_host_tree(g, T);
  st.ms_tree = ms_since(T0);
  if (rc != PGO_OK) return done(rc);
  st.components = T.components;
  st.tree_depth = T.tree_depth;
  st.wraps = T.wraps;
  if ((rc = ensure_device(g)) != PGO_OK) return done(rc);
  DevGraph& d = g->d;
  auto run = [&]() -> int {
    HIP_TRY(g, hipSetDevice(g->device));
    g->part_size = 1;   // every rank solves the whole system: a one-rank plan
    RC_TRY(ensure_chol(g));
    d.write_all = 0;
    RC_TRY(device_error(g, d.pose, &st.error_before));
    RC_TRY(init_upload_targets(g, T));
    // the result is built in pose_cand and copied over the values at the end:
    // a failed solve leaves them as they were
    auto t = std::chrono::steady_clock::now();
    HIP_TRY(g, pgo::launch_init_orient(d, g->init_tgt, g->init_tgt + d.ne));
    RC_TRY(init_factor_solve(g, "orientation"));
    HIP_TRY(g, pgo::launch_init_write_orient(d, d.x, d.pose_cand));
    st.ms_orient = ms_since(t);
    t = std::chrono::steady_clock::now();
    HIP_TRY(g, pgo::launch_init_trans(d, d.pose_cand));
    RC_TRY(init_factor_solve(g, "position"));
    HIP_TRY(g, pgo::launch_init_write_trans(d, d.x, d.pose_cand));
    HIP_TRY(g, hipStreamSynchronize(d.stream));
    st.ms_trans = ms_since(t);
    RC_TRY(device_error(g, d.pose_cand, &st.error_after));
    if (!std::isfinite(st.error_after)) return fail(g, PGO_E_NONFINITE, "linear initialisation: non-finite result");
    HIP_TRY(g, hipMemcpyAsync(d.pose, d.pose_cand, d.n * sizeof(double4), hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(g, hipStreamSynchronize(d.stream));
    g->dev_values = true;
    g->host_values = false;
    return PGO_OK;
  };
  return done(run());
}

int pgo_debug_init_tree(pgo_graph* g, int* parent, long long* k_edge, long long* k_prior, size_t cap_v, size_t cap_e,
                        size_t cap_p) {
  if (!g || (cap_v && !parent) || (cap_e && !k_edge) || (cap_p && !k_prior)) return PGO_E_ARG;
  pgo::InitTree T;
  RC_TRY(init_host_tree(g, T));
  for (size_t v = 0; v < T.parent.size() && v < cap_v; v++) parent[v] = T.parent[v];
  for (size_t e = 0; e < T.k_edge.size() && e < cap_e; e++) k_edge[e] = T.k_edge[e];
  for (size_t q = 0; q < T.k_prior.size() && q < cap_p; q++) k_prior[q] = T.k_prior[q];
  return (int)g->keys.size();
}

int pgo_debug_init_system(pgo_graph* g, int stage, double* hdiag, double* hoff, double* rhs) {
  if (!g || (stage != 1 && stage != 2)) return PGO_E_ARG;
  if (g->keys.empty()) return PGO_OK;
  pgo::InitTree T;
  RC_TRY(init_host_tree(g, T));
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  DevGraph& d = g->d;
  g->part_size = 1;
  RC_TRY(ensure_chol(g));   // (the owner bits the sweeps write by)
  d.write_all = 0;
  if (stage == 1) {
    RC_TRY(init_upload_targets(g, T));
    HIP_TRY(g, pgo::launch_init_orient(d, g->init_tgt, g->init_tgt + d.ne));
  } else {
    HIP_TRY(g, pgo::launch_init_trans(d, d.pose));
  }
  std::vector<double> V(9 * (size_t)d.ne), D(6 * (size_t)d.n), G(3 * (size_t)d.n);
  if (d.ne) HIP_TRY(g, hipMemcpyAsync(V.data(), d.V, V.size() * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(D.data(), d.D, D.size() * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(G.data(), d.g, G.size() * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  if (hdiag)
    for (int i = 0; i < d.n; i++) {
      const double* s = &D[6 * (size_t)i];
      double* o = hdiag + 9 * (size_t)i;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
      o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
    }
  if (hoff)   // (both stages' blocks are symmetric: the owner's orientation does not matter)
    for (int e = 0; e < d.ne; e++) {
      const size_t de = (size_t)(g->gs.codes()[g->gs.edge_slot0[e]] >> 2);
      std::memcpy(hoff + 9 * (size_t)e, &V[9 * de], 9 * sizeof(double));
    }
  if (rhs) std::memcpy(rhs, G.data(), G.size() * 8);
  return PGO_OK;
}

int pgo_optimize(pgo_graph* g, const pgo_params* params, pgo_stats* stats) {
  RoctxRange range_opt("pgo_optimize");
  if (!g) return PGO_E_ARG;
  pgo_params p;
  if (params) p = *params;
  else pgo_default_params(&p);
  pgo_stats st;
  std::memset(&st, 0, sizeof(st));
  const auto T0 = std::chrono::steady_clock::now();
  auto upload0 = std::chrono::steady_clock::now();
  g->trace.clear();
  for (int f = 0; f < pgo::kFamCount; f++) {
    g->fam_ms[f] = g->fam_flops[f] = g->fam_bytes[f] = 0.0;
    g->fam_launches[f] = 0;
  }
  auto since_T0 = [&]() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
  };
  g->last_upload = 0;
  int rc = ensure_device(g);
  if (rc != PGO_OK) return rc;
  st.ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - upload0).count();
  st.upload_kind = g->last_upload;
  DevGraph& d = g->d;
  HIP_TRY(g, hipSetDevice(g->device));
  double err = 0.0;
  RC_TRY(device_error(g, d.pose, &err));
  st.initial_error = err;
  if (!std::isfinite(err)) {
    st.status = PGO_E_NONFINITE;
    if (stats) *stats = st;
    return fail(g, PGO_E_NONFINITE, "initial error is not finite");
  }
  if (p.algorithm == PGO_ALG_GN && g->gs.gauge_free && d.n > 0 && !(err <= p.error_tol)) {
    st.status = PGO_E_INDETERMINANT;
    if (stats) *stats = st;
    return fail(g, PGO_E_INDETERMINANT,
                "Gauss-Newton: a connected component has no prior, the linear system is singular");
  }
  hipEvent_t* ev = g->ev;
  // PGO_MULTI_PARTITION with ranks: every try's factorisation is split over
  // the ranks (each rank then walks the same, replicated LM control).
  // PGO_MULTI_HYBRID: split over the partition group (pcomm), and the groups
  // run the speculative search over comm (one rank of every group each)
  const bool chol_lm = p.linear_solver != PGO_SOLVER_PCG && p.algorithm != PGO_ALG_GN;
  // (a bound partition group of one rank is the speculative search alone)
  const bool hybrid = p.multi_gpu == PGO_MULTI_HYBRID && g->pcomm_bound && g->pcomm.size > 1 && chol_lm;
  if (p.multi_gpu == PGO_MULTI_HYBRID && !g->pcomm_bound && g->comm.size > 1 && chol_lm)
    return fail(g, PGO_E_ARG, "PGO_MULTI_HYBRID needs a partition-group communicator (pgo_comm_init_*_part, "
                              "set up before the main communicator)");
  g->part_comm = hybrid ? &g->pcomm : &g->comm;
  const bool partition = (hybrid || (p.multi_gpu == PGO_MULTI_PARTITION && g->comm.size > 1)) && chol_lm;
  g->part_size = partition ? g->part_comm->size : 1;
  // Cholesky: the plan (and the owner bits it assigns) first, then the
  // linearisation writes only the blocks the assembly reads
  if (p.linear_solver != PGO_SOLVER_PCG && d.n > 0) {
    RoctxRange range_plan("plan");
    RC_TRY(ensure_chol(g));
    st.plan_update = g->plan_update;
    st.ms_plan = g->plan_ms;
  }
  if (p.linear_solver == PGO_SOLVER_PCG) RC_TRY(unmix_slot_codes(g));
  d.write_all = p.linear_solver == PGO_SOLVER_PCG ? 1 : 0;
  // robust losses: GTSAM's guard against a vanishing model decrease compares it
  // with the linearised error sum 0.5 w r^2, which is no longer the error; it
  // is computed once per linearisation and read back with the first try
  const bool robust = d.eloss != nullptr;
  double lin_err = err;
  // One lambda try (GTSAM tryLambda): solve (H + lam I) delta = -g, retract into
  // pose_cand, error there and the linear model decrease; one read-back.
  bool first_try = true;
  auto account_linearize = [&]() {   // after the first try of a linearisation has synchronised
    if (!first_try) return;
    const double lin_ms = ms_between(ev[0], ev[1]);
    st.ms_linearize += lin_ms;
    if (p.profile_every > 0) {
      st.kernel_linearize_ms += lin_ms;
      st.kernel_linearize_count++;
    }
    first_try = false;
  };
  auto run_try_once = [&](double lam_try, pgo::TryOutcome* out) -> int {
    SolveState ss;
    HIP_TRY(g, hipEventRecord(ev[2], d.stream));
    RC_TRY(linear_solve(g, p, lam_try, &st, &ss));
    st.solves++;
    HIP_TRY(g, hipEventRecord(ev[3], d.stream));
    if (!ss.known || ss.solved) {
      if (p.algorithm != PGO_ALG_GN) HIP_TRY(g, pgo::launch_model_decrease(d, d.x, d.scal + 1));
      HIP_TRY(g, pgo::launch_retract(d, d.x));
      HIP_TRY(g, pgo::launch_error(d, d.pose_cand, d.scal));
    }
    HIP_TRY(g, hipEventRecord(ev[4], d.stream));
    RC_TRY(sync_scalars(g, robust ? 5 : 3));
    if (robust) lin_err = g->h_scal[4];
    RC_TRY(finish_solve(g, &st, &ss));
    account_linearize();
    st.ms_solve += ms_between(ev[2], ev[3]);
    st.ms_update += ms_between(ev[3], ev[4]);
    *out = {ss.solved ? 1.0 : 0.0, g->h_scal[0], g->h_scal[1], g->h_scal[2]};
    return PGO_OK;
  };
  // a try whose in-launch hand-off timed out (a workgroup starved on a shared
  // GPU) runs once more before the optimize fails (every rank of a partitioned
  // run sees the same flags, so all retry together)
  auto retried = [&](auto&& body) -> int {
    g->handoff_timeout = false;
    int rc = body();
    if (rc == PGO_E_HIP && g->handoff_timeout) {
      g->handoff_timeout = false;
      st.handoff_retries++;   // visible in pgo_stats / the bench's per_step (round 6)
      rc = body();
    }
    return rc;
  };
  auto run_try = [&](double lam_try, pgo::TryOutcome* out) -> int {
    return retried([&] { return run_try_once(lam_try, out); });
  };
  pgo::Comm& cm = g->comm;
  // the speculative search's ranks (a partitioned run is one search: P = 1
  // here; the hybrid's search runs over the groups, one rank of each in cm)
  const bool spec = !partition || hybrid;
  const int P = spec ? cm.size : 1, me = spec ? cm.rank : 0;
  const bool exchange = spec && (P > 1 || pgo::force_collectives(&cm));   // forced: 1-rank RCCL too
  st.ranks = hybrid ? cm.size * g->pcomm.size : cm.size;
  auto transport_of = [](const pgo::Comm& c) {
    return c.size <= 1 && !c.nccl ? PGO_TRANSPORT_NONE : (c.host ? PGO_TRANSPORT_HOST : PGO_TRANSPORT_RCCL);
  };
  st.transport = transport_of(cm);
  st.part_transport = hybrid ? transport_of(g->pcomm) : PGO_TRANSPORT_NONE;
  // lanes: concurrent tries on this GPU (Cholesky LM only)
  int L = 1;
  if (p.algorithm != PGO_ALG_GN && p.linear_solver != PGO_SOLVER_PCG && p.lambda_lanes > 1 && d.n > 0)
    L = ensure_lanes(g, p.lambda_lanes);
  // an exchange between the ranks: its wall time into ms_comm, a failure under the call's name
  auto comm_call = [&](const char* what, auto&& call) -> int {
    const auto c0 = std::chrono::steady_clock::now();
    std::string why;
    const int rc = call(&why);
    if (rc != PGO_OK) return fail(g, rc, std::string(what) + ": " + why);
    st.ms_comm += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    return PGO_OK;
  };
  // every rank must agree on the lanes per rank (a lane allocation may fail on
  // one); a partitioned run's ranks factor the same lanes together (the
  // hybrid: the minimum over the group, then over the groups)
  auto agree_lanes = [&](pgo::Comm& c) -> int {
    std::vector<double> all(c.size);
    const double mineL = L;
    RC_TRY(comm_call("lane count all-gather", [&](std::string* why) {
      return pgo::comm_allgather(&c, &mineL, 1, all.data(), d.stream, why);
    }));
    for (double v : all) L = std::min(L, (int)v);
    return PGO_OK;
  };
  if (partition && g->part_comm->size > 1) RC_TRY(agree_lanes(*g->part_comm));
  if (exchange && (!partition || hybrid)) RC_TRY(agree_lanes(cm));
  const int T = P * L;                       // tries per round
  std::vector<pgo::TryOutcome> outs(T);
  // the policy: which lambdas to try, how many lanes, what the outcomes mean (pgo_lm.h)
  static const int adapt_mode = getenv("PGO_LANES_ADAPT") ? atoi(getenv("PGO_LANES_ADAPT")) : 1;
  pgo::LmControl ctl(p, err, adapt_mode);
  // per-iteration record (pgo_get_trace): the control's rows + wall ms
  auto take_trace = [&]() {
    for (size_t r = g->trace.size() / kTraceCols; r < ctl.trace.size() / pgo::kLmTraceCols; r++) {
      const double* row = ctl.trace.data() + r * pgo::kLmTraceCols;
      g->trace.insert(g->trace.end(), row, row + pgo::kLmTraceCols);
      g->trace.push_back(since_T0());   // (a row's own stamp, as it is taken over)
    }
  };
  if (ctl.start() && d.n > 0) {
    for (;;) {
      RoctxRange range_lin("linearisation");
      HIP_TRY(g, pgo::launch_linearize(d, ev[0], ev[1]));
      if (robust) HIP_TRY(g, pgo::launch_error_lin(d, d.pose, d.scal + 3));
      HIP_TRY(g, hipEventRecord(g->lin_done, d.stream));
      ctl.begin_linearization();
      first_try = true;
      if (p.algorithm == PGO_ALG_GN) {  // one plain step; every rank computes the same one
        pgo::TryOutcome o;
        RC_TRY(run_try(0.0, &o));
        if (ctl.gn_step(o)) std::swap(d.pose, d.pose_cand);
        take_trace();
      } else {
        // Lambda rounds: try k of a round runs on rank k / L, lane k % L
        for (;;) {
          RoctxRange range_round("lambda_round");
          ctl.plan_round(T);
          const bool prof_next = p.profile_every > 0 && (g->factorizations % p.profile_every) == 0;
          const int Lr = ctl.round_lanes(L, prof_next, exchange);
          std::vector<pgo::TryOutcome> mine(L, pgo::kNoTry);   // (past the bound / lane idle: no try)
          int nb = 0;   // this rank's valid tries (a prefix of its lanes)
          while (nb < Lr && ctl.valid[me * L + nb]) nb++;
          if (nb == 1) {
            RC_TRY(run_try(ctl.lam_k[me * L], &mine[0]));
          } else if (nb > 1) {
            RC_TRY(retried([&] { return run_lanes(g, p, nb, &ctl.lam_k[me * L], mine.data(), &st); }));
            st.solves += nb;
            account_linearize();
            if (robust) lin_err = g->h_lanes[3];
          } else if (robust) {   // (a rank without a try this round still walks the outcomes)
            RC_TRY(sync_scalars(g, 5));
            lin_err = g->h_scal[4];
          }
          st.lambda_rounds++;
          if (exchange) {
            RC_TRY(comm_call("lambda round all-gather", [&](std::string* why) {
              return pgo::comm_allgather(&cm, &mine[0].solved, 4 * L, &outs[0].solved, d.stream, why);
            }));
          } else {
            outs = mine;
          }
          const pgo::LmWalk w = ctl.walk(outs.data(), robust ? lin_err : ctl.err);
          take_trace();
          if (w.winner >= 0) {
            const int wr = w.winner / L, wl = w.winner % L;
            // the accepted candidate values: lane wl's buffer on rank wr
            double4** cand = wr == me && wl > 0 ? &g->lanes[wl - 1].pose_cand : &d.pose_cand;
            if (exchange)
              RC_TRY(comm_call("accepted values broadcast", [&](std::string* why) {
                return pgo::comm_broadcast_device(&cm, *cand, sizeof(double4) * (size_t)d.n, wr, d.stream, why);
              }));
            std::swap(d.pose, *cand);
          }
          if (w.done) break;
        }
      }
      if (!ctl.next_linearization()) break;
    }
  }
  ctl.finish();
  g->host_values = false;
  st.status = ctl.status;
  st.stop_reason = ctl.stop_reason;
  st.linearizations = ctl.linearizations;
  st.iterations = ctl.iters;
  st.inner_iterations = ctl.inner;
  st.final_error = ctl.err;
  st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
  if (stats) *stats = st;
  if (ctl.status < 0) return fail(g, ctl.status, pgo_status_string(ctl.status));
  return ctl.status;
}

// ---- fixed weights and graduated non-convexity (pgo_gnc.h / pgo_gnc.hip)

namespace {

constexpr int kGncTraceCols = 8;   // pgo_get_gnc_trace row

// The host's loss kinds and parameters onto the device graph that is resident
// (its first d.ne factors; appended ones travel with append_structure): the
// loss arrays are allocated when the first factor gets a loss or a weight below
// 1 and released when the last one loses it, which switches the handle between
// the Gaussian and the robust kernel sets.  Values only: no structure, plan or
// captured graph depends on them.  Without a resident graph the next upload
// carries the host arrays.
int sync_device_losses(pgo_graph* g) {
  if (!g->dev_complete || !g->hip_ready) return PGO_OK;
  HIP_TRY(g, hipSetDevice(g->device));
  DevGraph& d = g->d;
  pgo::GraphStructure& S = g->gs;
  const size_t ne = (size_t)d.ne;
  const bool want = g->n_robust > 0;
  if (!want) {
    if (!d.eloss) return PGO_OK;
    HIP_TRY(g, hipStreamSynchronize(d.stream));
    (void)hipFree(d.eloss);
    (void)hipFree(d.ek);
    (void)hipFree(d.s1fac);
    d.eloss = nullptr;
    d.ek = nullptr;
    d.s1fac = nullptr;
    S.s1fac.clear();
    return PGO_OK;
  }
  if (!d.eloss) {
    S.s1fac.resize(ne);
    for (size_t e = 0; e < ne; e++) S.s1fac[S.s1pos[e]] = (int)e;
    unsigned char* dl = nullptr;
    double* dk = nullptr;
    int* df = nullptr;
    const size_t ce = std::max<size_t>(g->cap_ne, ne);
    hipError_t e = hipMalloc((void**)&dl, std::max<size_t>(ce, 1));
    if (e == hipSuccess) e = hipMalloc((void**)&dk, std::max<size_t>(ce, 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&df, std::max<size_t>(ce, 1) * sizeof(int));
    if (e == hipSuccess && ne)
      e = hipMemcpyAsync(df, S.s1fac.data(), ne * sizeof(int), hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) {
      if (dl) (void)hipFree(dl);
      if (dk) (void)hipFree(dk);
      if (df) (void)hipFree(df);
      S.s1fac.clear();
      HIP_TRY(g, e);
    }
    d.eloss = dl;
    d.ek = dk;
    d.s1fac = df;
  }
  std::vector<unsigned char> hl;
  std::vector<double> hk;
  gather_losses(g, S.dorder.data(), ne, hl, hk);
  RC_TRY(h2d(g, d.eloss, hl.data(), ne));
  RC_TRY(h2d(g, d.ek, hk.data(), ne));
  HIP_TRY(g, hipStreamSynchronize(d.stream));   // (the sources are locals)
  return PGO_OK;
}

// host side of a fixed weight on user factor u (kind NONE or fixed before)
void set_host_weight(pgo_graph* g, size_t u, double w) {
  const bool was = g->eloss[u] == pgo::kLossFixed, is = w != 1.0;
  g->eloss[u] = is ? (unsigned char)pgo::kLossFixed : (unsigned char)PGO_LOSS_NONE;
  g->ek[u] = w;
  if (is && !was) g->n_robust++, g->n_fixed++;
  if (!is && was) g->n_robust--, g->n_fixed--;
}

double wall_ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The candidates' bytes in device order (gnc_cand) and the values buffer, sized
// with the graph's capacity.
int gnc_upload_candidates(pgo_graph* g, const std::vector<size_t>& cand) {
  DevGraph& d = g->d;
  const size_t ne = (size_t)d.ne, ce = std::max<size_t>(g->cap_ne, ne), cn = std::max<size_t>(g->cap_n, d.n);
  if (g->gnc_cand_cap < ce) {
    if (g->gnc_cand) (void)hipFree(g->gnc_cand);
    g->gnc_cand = nullptr;
    g->gnc_cand_cap = 0;
    RC_TRY(dev_alloc(g, &g->gnc_cand, ce));
    g->gnc_cand_cap = ce;
  }
  if (g->gnc_pose_cap < cn) {
    if (g->gnc_pose) (void)hipFree(g->gnc_pose);
    g->gnc_pose = nullptr;
    g->gnc_pose_cap = 0;
    RC_TRY(dev_alloc(g, &g->gnc_pose, cn));
    g->gnc_pose_cap = cn;
  }
  std::vector<unsigned char> user(ne, 0), dev(ne);
  for (size_t u : cand) user[u] = 1;
  for (size_t e = 0; e < ne; e++) dev[e] = user[(size_t)g->gs.dorder[e]];
  RC_TRY(h2d(g, g->gnc_cand, dev.data(), ne));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  return PGO_OK;
}

// one sweep and its read-back: out5 as launch_gnc_weights
int gnc_sweep(pgo_graph* g, int loss, double mu, double c2, double wtol, int write, double* out5) {
  DevGraph& d = g->d;
  HIP_TRY(g, pgo::launch_gnc_weights(d, d.pose, g->gnc_cand, loss, mu, c2, wtol, write, d.scal));
  RC_TRY(sync_scalars(g, 5));
  std::memcpy(out5, g->h_scal, 5 * sizeof(double));
  return PGO_OK;
}

// the candidates idx[0..n) (NULL: all) as checked user indices
int gnc_candidates(pgo_graph* g, size_t n, const size_t* idx, std::vector<size_t>& cand) {
  const size_t ne = g->ek1.size();
  cand.clear();
  if (!idx) {
    cand.resize(ne);
    for (size_t e = 0; e < ne; e++) cand[e] = e;
  } else {
    std::vector<unsigned char> seen(ne, 0);
    cand.reserve(n);
    for (size_t i = 0; i < n; i++) {
      if (idx[i] >= ne) return fail(g, PGO_E_ARG, "gnc: candidate index past the last between factor");
      if (seen[idx[i]]) return fail(g, PGO_E_ARG, "gnc: duplicate candidate index");
      seen[idx[i]] = 1;
      cand.push_back(idx[i]);
    }
  }
  for (size_t u : cand)
    if (g->eloss[u] != PGO_LOSS_NONE && g->eloss[u] != pgo::kLossFixed)
      return fail(g, PGO_E_ARG, "gnc: a candidate factor has a robust loss");
  return PGO_OK;
}

// the candidates' weights from the device (d.ek) into the host arrays
int gnc_download_weights(pgo_graph* g, const std::vector<size_t>& cand) {
  DevGraph& d = g->d;
  const size_t ne = (size_t)d.ne;
  std::vector<double> hk(ne);
  if (ne) HIP_TRY(g, hipMemcpyAsync(hk.data(), d.ek, ne * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  std::vector<size_t> dpos(ne);
  for (size_t e = 0; e < ne; e++) dpos[(size_t)g->gs.dorder[e]] = e;
  for (size_t u : cand) set_host_weight(g, u, hk[dpos[u]]);
  return PGO_OK;
}

}  // namespace

int pgo_set_edge_weights(pgo_graph* g, size_t first, size_t n, const double* w) {
  if (!g || (n && !w)) return PGO_E_ARG;
  const size_t ne = g->ek1.size();
  if (first > ne || n > ne - first) return fail(g, PGO_E_ARG, "set_edge_weights: range past the last between factor");
  for (size_t i = 0; i < n; i++) {
    if (!(std::isfinite(w[i]) && w[i] >= 0.0 && w[i] <= 1.0))
      return fail(g, PGO_E_ARG, "set_edge_weights: a weight must be finite and in [0, 1]");
    if (g->eloss[first + i] != PGO_LOSS_NONE && g->eloss[first + i] != pgo::kLossFixed)
      return fail(g, PGO_E_ARG, "set_edge_weights: factor " + std::to_string(first + i) + " has a robust loss");
  }
  if (n == 0) return PGO_OK;
  for (size_t i = 0; i < n; i++) set_host_weight(g, first + i, w[i]);
  return sync_device_losses(g);
}

int pgo_get_gnc_trace(const pgo_graph* g, double* out, int cap) {
  if (!g || cap < 0 || (cap > 0 && !out)) return PGO_E_ARG;
  const int rows = (int)(g->gnc_trace.size() / kGncTraceCols);
  if (cap > 0 && rows > 0)
    std::memcpy(out, g->gnc_trace.data(), sizeof(double) * kGncTraceCols * std::min(rows, cap));
  return rows;
}

int pgo_optimize_gnc(pgo_graph* g, const pgo_params* inner, const pgo_gnc_params* gnc, size_t n, const size_t* idx,
                     pgo_gnc_stats* stats) {
  RoctxRange range_gnc("pgo_optimize_gnc");
  if (!g || (n && !idx && n != g->ek1.size())) return PGO_E_ARG;
  pgo_gnc_params gp;
  if (gnc) gp = *gnc;
  else pgo_gnc_default_params(&gp);
  pgo_gnc_stats st;
  std::memset(&st, 0, sizeof(st));
  st.mu_initial = st.mu_final = NAN;
  auto leave = [&](int rc) {
    st.status = rc;
    if (stats) *stats = st;
    return rc;
  };
  if (!pgo::gnc_params_ok(gp)) return leave(fail(g, PGO_E_ARG, "gnc: bad parameters"));
  if (g->comm.size > 1) return leave(fail(g, PGO_E_ARG, "gnc: one rank only (the handle has a communicator)"));
  if (g->n_robust > g->n_fixed)
    return leave(fail(g, PGO_E_ARG, "gnc: the graph has factors under a robust loss"));
  std::vector<size_t> cand;
  {
    const int rc = gnc_candidates(g, n, idx, cand);
    if (rc != PGO_OK) return leave(rc);
  }
  const auto T0 = std::chrono::steady_clock::now();
  g->gnc_trace.clear();
  st.candidates = (int)cand.size();
  const double c2 = gp.barc_sq;
  // the candidates' weights: all 1 on the host (kind NONE), then the device
  auto all_one = [&]() -> int {
    for (size_t u : cand) set_host_weight(g, u, 1.0);
    return sync_device_losses(g);
  };
  pgo_stats is;
  auto row = [&](double mu, double cost, double sw, double nonbin, double rmax) {
    const double r[kGncTraceCols] = {mu,   cost, sw, nonbin, rmax, (double)is.inner_iterations, (double)is.iterations,
                                     (double)is.stop_reason};
    g->gnc_trace.insert(g->gnc_trace.end(), r, r + kGncTraceCols);
  };
  auto inner_solve = [&]() -> int {
    const auto t = std::chrono::steady_clock::now();
    std::memset(&is, 0, sizeof(is));
    const int rc = pgo_optimize(g, inner, &is);
    st.ms_inner += wall_ms_since(t);
    st.inner_tries += is.inner_iterations;
    st.linearizations += is.linearizations;
    return rc;
  };
  auto finish = [&](int rc) {
    st.ms_total = wall_ms_since(T0);
    return leave(rc);
  };
  {
    const int rc = all_one();
    if (rc != PGO_OK) return finish(rc);
  }
  // row 0: exactly pgo_optimize(g, inner)
  {
    const int rc = inner_solve();
    st.initial_error = is.initial_error;
    st.final_cost = is.final_error;
    if (rc < 0) {
      st.stop_reason = PGO_GNC_STOP_ERROR;
      return finish(rc);
    }
  }
  if (cand.empty()) {
    row(NAN, is.final_error, 0.0, 0.0, 0.0);
    st.stop_reason = PGO_GNC_STOP_NO_CANDIDATES;
    return finish(PGO_OK);
  }
  HIP_TRY(g, hipSetDevice(g->device));
  DevGraph& d = g->d;
  // the candidates become fixed weights (1 so far): the robust kernel set from here on
  for (size_t u : cand) {
    if (g->eloss[u] != pgo::kLossFixed) g->n_robust++, g->n_fixed++;
    g->eloss[u] = (unsigned char)pgo::kLossFixed;
    g->ek[u] = 1.0;
  }
  // on any way out: the host arrays in step with what the call leaves behind
  auto settle = [&](bool keep) -> int {
    if (keep) RC_TRY(gnc_download_weights(g, cand));
    else
      for (size_t u : cand) set_host_weight(g, u, 1.0);
    return sync_device_losses(g);
  };
  auto bail = [&](int rc) {
    (void)settle(false);
    st.stop_reason = PGO_GNC_STOP_ERROR;
    return finish(rc);
  };
  {
    int rc = sync_device_losses(g);
    if (rc == PGO_OK) rc = gnc_upload_candidates(g, cand);
    if (rc != PGO_OK) return bail(rc);
  }
  double s5[5];
  auto sweep = [&](double mu, int write) -> int {
    const auto t = std::chrono::steady_clock::now();
    const int rc = gnc_sweep(g, gp.loss, mu, c2, gp.weights_tol, write, s5);
    st.ms_weights += wall_ms_since(t);
    return rc;
  };
  pgo::GncControl ctl(gp);
  {
    const int rc = sweep(1.0, 0);   // (read-only: the mu does not matter to the largest r^2)
    if (rc != PGO_OK) return bail(rc);
  }
  row(NAN, is.final_error, (double)cand.size(), 0.0, s5[0]);
  const bool iterate = ctl.start(is.final_error, s5[0]);
  st.mu_initial = ctl.mu_initial;
  if (iterate) {
    for (;;) {
      const double mu = ctl.mu;
      int rc = sweep(mu, 1);
      if (rc != PGO_OK) return bail(rc);
      const double rmax = s5[0], sw = s5[1], nonbin = s5[2];
      if (d.n) {
        const hipError_t e = hipMemcpyAsync(g->gnc_pose, d.pose, d.n * sizeof(double4), hipMemcpyDeviceToDevice, d.stream);
        if (e != hipSuccess) return bail(fail(g, PGO_E_HIP, hipGetErrorString(e)));
      }
      rc = inner_solve();
      if (rc < 0) {   // the values of the last successful inner solve, the candidates plain again
        const std::string why = g->last_error;
        if (d.n && g->dev_structure && d.pose) {
          (void)hipMemcpyAsync(d.pose, g->gnc_pose, d.n * sizeof(double4), hipMemcpyDeviceToDevice, d.stream);
          (void)hipStreamSynchronize(d.stream);
          g->dev_values = true;
          g->host_values = false;
        }
        (void)settle(false);
        g->last_error = why;
        st.stop_reason = PGO_GNC_STOP_ERROR;
        return finish(rc);
      }
      st.final_cost = is.final_error;
      st.mu_final = mu;
      row(mu, is.final_error, sw, nonbin, rmax);
      if (!ctl.step(is.final_error, nonbin)) break;
    }
  }
  st.outer_iterations = ctl.outer;
  st.stop_reason = ctl.stop_reason;
  {
    const int rc = sweep(std::isfinite(ctl.mu) ? ctl.mu : 1.0, 0);   // r^2 > c^2 at the final values
    if (rc != PGO_OK) return bail(rc);
    st.outliers = (int)s5[3];
  }
  {
    const int rc = settle(gp.keep_weights != 0);
    if (rc != PGO_OK) return finish(rc);
  }
  return finish(ctl.stop_reason == PGO_GNC_STOP_MAX_ITER ? PGO_W_MAXITER : PGO_OK);
}

int pgo_debug_gnc_sweep(pgo_graph* g, int loss, double mu, double barc_sq, size_t n, const size_t* idx, int write,
                        double* w_all, double* stats5) {
  if (!g || !stats5 || (loss != PGO_GNC_GM && loss != PGO_GNC_TLS) || !(barc_sq > 0.0) || !(mu > 0.0) ||
      !std::isfinite(mu) || !std::isfinite(barc_sq) || (n && !idx && n != g->ek1.size()))
    return PGO_E_ARG;
  if (g->n_robust > g->n_fixed) return fail(g, PGO_E_ARG, "gnc: the graph has factors under a robust loss");
  std::vector<size_t> cand;
  RC_TRY(gnc_candidates(g, n, idx, cand));
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  const size_t ne = g->ek1.size();
  // the candidates as fixed weights (their own, or 1) while the sweep runs
  const std::vector<unsigned char> loss0 = g->eloss;
  const std::vector<double> k0 = g->ek;
  const size_t nr0 = g->n_robust, nf0 = g->n_fixed;
  for (size_t u : cand) {
    if (g->eloss[u] != pgo::kLossFixed) g->n_robust++, g->n_fixed++, g->ek[u] = 1.0;
    g->eloss[u] = (unsigned char)pgo::kLossFixed;
  }
  auto restore = [&]() {
    g->eloss = loss0;
    g->ek = k0;
    g->n_robust = nr0;
    g->n_fixed = nf0;
    return sync_device_losses(g);
  };
  int rc = cand.empty() ? PGO_OK : sync_device_losses(g);
  if (rc == PGO_OK) rc = gnc_upload_candidates(g, cand);
  if (rc == PGO_OK && cand.empty()) {   // nothing marked: no loss arrays needed, nothing to write
    std::memset(stats5, 0, 5 * sizeof(double));
    if (w_all) std::fill(w_all, w_all + ne, 1.0);
    return restore();
  }
  if (rc == PGO_OK) rc = gnc_sweep(g, loss, mu, barc_sq, 1e-4, 1, stats5);
  std::vector<double> hk(ne);
  if (rc == PGO_OK && ne) {
    hipError_t e = hipMemcpyAsync(hk.data(), g->d.ek, ne * sizeof(double), hipMemcpyDeviceToHost, g->d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->d.stream);
    if (e != hipSuccess) rc = fail(g, PGO_E_HIP, hipGetErrorString(e));
  }
  if (rc != PGO_OK) {
    (void)restore();
    return rc;
  }
  if (w_all) {
    std::fill(w_all, w_all + ne, 1.0);
    std::vector<unsigned char> is_cand(ne, 0);
    for (size_t u : cand) is_cand[u] = 1;
    for (size_t e = 0; e < ne; e++) {
      const size_t u = (size_t)g->gs.dorder[e];
      if (is_cand[u]) w_all[u] = hk[e];
    }
  }
  if (!write) return restore();
  RC_TRY(gnc_download_weights(g, cand));
  return sync_device_losses(g);   // (a weight of exactly 1 is a plain factor again, on the device too)
}

int pgo_closest_keyframe(pgo_graph* g, double x, double y, int skip, uint64_t* key, double* dist) {
  if (!g || !key || !dist || skip < 0 || !std::isfinite(x) || !std::isfinite(y)) return PGO_E_ARG;
  const size_t n = g->keys.size();
  if (n <= (size_t)skip)
    return fail(g, PGO_E_NOT_ENOUGH, "closest_keyframe: not enough keyframes (" + std::to_string(n) + " <= skip " +
                                         std::to_string(skip) + ")");
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  const DevGraph& d = g->d;
  RC_TRY(ensure_search(g));
  const int limit = (int)(n - skip);
  HIP_TRY(g, pgo::launch_closest_scan(d.pose, limit, x, y, g->s_d, g->s_i, g->s_d + pgo::kMaxBlocks,
                                      g->s_i + pgo::kMaxBlocks, d.stream, g->sev_scan[0], g->sev_scan[1]));
  g->scan_timed = true;
  HIP_TRY(g, hipMemcpyAsync(g->h_scal, g->s_d + pgo::kMaxBlocks, sizeof(double), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(g->h_ctrl, g->s_i + pgo::kMaxBlocks, sizeof(int), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  const int idx = g->h_ctrl[0];
  if (idx < 0 || idx >= limit) return fail(g, PGO_E_NONFINITE, "closest_keyframe: no finite distance");
  *key = g->keys[idx];
  *dist = g->h_scal[0];
  return PGO_OK;
}

int pgo_closest_keyframes(pgo_graph* g, size_t q, const uint64_t* query_keys, int skip, uint64_t* keys_out,
                          double* dist_out) {
  if (!g || skip < 0 || (q && (!query_keys || !keys_out || !dist_out)) || q > (size_t)INT32_MAX) return PGO_E_ARG;
  if (q == 0) return PGO_OK;
  // queries sorted by vertex index: a workgroup's candidate ranges are then alike
  std::vector<std::pair<int, int>> order(q);
  for (size_t k = 0; k < q; k++) {
    auto it = g->index.find(query_keys[k]);
    if (it == g->index.end()) return fail(g, PGO_E_NO_KEY, "closest_keyframes: key " + std::to_string(query_keys[k]) + " has no value");
    order[k] = {it->second, (int)k};
  }
  std::stable_sort(order.begin(), order.end());
  std::vector<int> qv(q);
  for (size_t k = 0; k < q; k++) qv[k] = order[k].first;
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  const DevGraph& d = g->d;
  RC_TRY(ensure_search(g));
  const int max_limit = std::max(qv.back() + 1 - skip, 0);
  const size_t parts = q * (size_t)pgo::closest_batch_chunks(max_limit);
  if (g->sb_cap < q || g->sbp_cap < parts) {
    for (void* p : {(void*)g->sb_d, (void*)g->sb_i, (void*)g->sb_q, (void*)g->sbp_d, (void*)g->sbp_i})
      if (p) (void)hipFree(p);
    g->sb_d = g->sbp_d = nullptr;
    g->sb_i = g->sb_q = g->sbp_i = nullptr;
    g->sb_cap = g->sbp_cap = 0;
    HIP_TRY(g, hipMalloc((void**)&g->sb_d, sizeof(double) * q));
    HIP_TRY(g, hipMalloc((void**)&g->sb_i, sizeof(int) * q));
    HIP_TRY(g, hipMalloc((void**)&g->sb_q, sizeof(int) * q));
    HIP_TRY(g, hipMalloc((void**)&g->sbp_d, sizeof(double) * parts));
    HIP_TRY(g, hipMalloc((void**)&g->sbp_i, sizeof(int) * parts));
    g->sb_cap = q;
    g->sbp_cap = parts;
  }
  HIP_TRY(g, hipMemcpyAsync(g->sb_q, qv.data(), sizeof(int) * q, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(g, pgo::launch_closest_batch(d.pose, g->sb_q, (int)q, skip, max_limit, g->sbp_d, g->sbp_i, g->sb_d,
                                       g->sb_i, d.stream, g->sev_batch[0], g->sev_batch[1]));
  g->batch_timed = true;
  std::vector<double> hd(q);
  std::vector<int> hi(q);
  HIP_TRY(g, hipMemcpyAsync(hd.data(), g->sb_d, sizeof(double) * q, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(hi.data(), g->sb_i, sizeof(int) * q, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  for (size_t k = 0; k < q; k++) {
    const int o = order[k].second;
    keys_out[o] = hi[k] >= 0 ? g->keys[hi[k]] : PGO_NO_KEY;
    dist_out[o] = hi[k] >= 0 ? hd[k] : INFINITY;
  }
  return PGO_OK;
}

int pgo_debug_search_ms(pgo_graph* g, double* scan_ms, double* batch_ms) {
  if (!g || !scan_ms || !batch_ms) return PGO_E_ARG;
  *scan_ms = g->scan_timed ? ms_between(g->sev_scan[0], g->sev_scan[1]) : 0.0;
  *batch_ms = g->batch_timed ? ms_between(g->sev_batch[0], g->sev_batch[1]) : 0.0;
  return PGO_OK;
}

int pgo_comm_unique_id(void* out, size_t cap) {
  std::string why;
  return pgo::comm_unique_id(out, cap, &why);
}

// a main communicator (re)initialised: the partition group's communicator set
// up since the previous main init is bound to it, an older one is freed
static void bind_part_comm(pgo_graph* g) {
  if (!g->pcomm_fresh) {
    if (g->pcomm.nccl) (void)hipSetDevice(g->device);
    pgo::comm_free(&g->pcomm);
  }
  g->pcomm_bound = g->pcomm_fresh;
  g->pcomm_fresh = false;
}

int pgo_comm_init_rccl(pgo_graph* g, const void* unique_id, size_t id_bytes, int rank, int size) {
  if (!g) return PGO_E_ARG;
  RC_TRY(ensure_hip(g));
  HIP_TRY(g, hipSetDevice(g->device));
  std::string why;
  const int rc = pgo::comm_init_rccl(&g->comm, unique_id, id_bytes, rank, size, &why);
  bind_part_comm(g);
  return rc == PGO_OK ? rc : fail(g, rc, why);
}

int pgo_comm_init_host(pgo_graph* g, const pgo_host_comm* comm) {
  if (!g) return PGO_E_ARG;
  if (g->comm.nccl) (void)hipSetDevice(g->device);
  std::string why;
  const int rc = pgo::comm_init_host(&g->comm, comm, &why);
  bind_part_comm(g);
  return rc == PGO_OK ? rc : fail(g, rc, why);
}

int pgo_comm_free(pgo_graph* g) {
  if (!g) return PGO_E_ARG;
  if (g->comm.nccl || g->pcomm.nccl) (void)hipSetDevice(g->device);
  pgo::comm_free(&g->comm);
  pgo::comm_free(&g->pcomm);
  g->part_comm = &g->comm;
  g->pcomm_fresh = g->pcomm_bound = false;
  return PGO_OK;
}

int pgo_comm_init_rccl_part(pgo_graph* g, const void* unique_id, size_t id_bytes, int rank, int size) {
  if (!g) return PGO_E_ARG;
  RC_TRY(ensure_hip(g));
  HIP_TRY(g, hipSetDevice(g->device));
  std::string why;
  const int rc = pgo::comm_init_rccl(&g->pcomm, unique_id, id_bytes, rank, size, &why);
  g->pcomm_fresh = rc == PGO_OK;
  g->pcomm_bound = false;
  return rc == PGO_OK ? rc : fail(g, rc, why);
}

int pgo_comm_init_host_part(pgo_graph* g, const pgo_host_comm* comm) {
  if (!g) return PGO_E_ARG;
  if (g->pcomm.nccl) (void)hipSetDevice(g->device);
  std::string why;
  const int rc = pgo::comm_init_host(&g->pcomm, comm, &why);
  g->pcomm_fresh = rc == PGO_OK;
  g->pcomm_bound = false;
  return rc == PGO_OK ? rc : fail(g, rc, why);
}

int pgo_comm_part_rank(const pgo_graph* g, int* rank, int* size) {
  if (!g || !rank || !size) return PGO_E_ARG;
  *rank = g->pcomm.rank;
  *size = g->pcomm.size;
  return PGO_OK;
}

int pgo_comm_rank(const pgo_graph* g, int* rank, int* size) {
  if (!g || !rank || !size) return PGO_E_ARG;
  *rank = g->comm.rank;
  *size = g->comm.size;
  return PGO_OK;
}

int pgo_comm_selftest(pgo_graph* g) {
  if (!g) return PGO_E_ARG;
  pgo::Comm& c = g->comm;
  hipStream_t s = nullptr;
  if (!c.host) {
    RC_TRY(ensure_hip(g));
    HIP_TRY(g, hipSetDevice(g->device));
    s = g->d.stream;
  }
  const double mine[4] = {(double)c.rank, (double)c.size, (double)c.rank * c.rank, 1.0};
  std::vector<double> all(4 * (size_t)c.size);
  std::string why;
  int rc = pgo::comm_allgather(&c, mine, 4, all.data(), s, &why);
  if (rc != PGO_OK) return fail(g, rc, why);
  for (int r = 0; r < c.size; r++)
    if (all[4 * r] != r || all[4 * r + 1] != c.size || all[4 * r + 2] != (double)r * r || all[4 * r + 3] != 1.0)
      return fail(g, PGO_E_COMM, "all-gather returned wrong data for rank " + std::to_string(r));
  // broadcast from the last rank: 1000 doubles root * 1e6 + i
  const int root = c.size - 1, nb = 1000;
  std::vector<double> h(nb);
  for (int i = 0; i < nb; i++) h[i] = c.rank == root ? root * 1e6 + i : -1.0;
  if (c.host) {  // host transport: exercise the callback directly on host memory
    if (c.hc.broadcast(c.hc.ctx, h.data(), sizeof(double) * nb, root) != 0)
      return fail(g, PGO_E_COMM, "host broadcast callback failed");
  } else {
    double* dbuf = nullptr;
    HIP_TRY(g, hipMalloc((void**)&dbuf, sizeof(double) * nb));
    HIP_TRY(g, hipMemcpy(dbuf, h.data(), sizeof(double) * nb, hipMemcpyHostToDevice));
    rc = pgo::comm_broadcast_device(&c, dbuf, sizeof(double) * nb, root, s, &why);
    if (rc == PGO_OK) (void)hipMemcpy(h.data(), dbuf, sizeof(double) * nb, hipMemcpyDeviceToHost);
    (void)hipFree(dbuf);
    if (rc != PGO_OK) return fail(g, rc, why);
  }
  for (int i = 0; i < nb; i++)
    if (h[i] != root * 1e6 + i) return fail(g, PGO_E_COMM, "broadcast returned wrong data");
  return PGO_OK;
}

int pgo_get_trace(const pgo_graph* g, double* out, int cap) {
  if (!g || cap < 0 || (cap > 0 && !out)) return PGO_E_ARG;
  const int rows = (int)(g->trace.size() / kTraceCols);
  if (cap > 0 && rows > 0) std::memcpy(out, g->trace.data(), sizeof(double) * kTraceCols * std::min(rows, cap));
  return rows;
}

const char* pgo_kernel_family_name(int f) { return pgo::kernel_family_name(f); }

int pgo_get_kernel_profile(const pgo_graph* g, double* out, int cap) {
  if (!g || cap < 0 || (cap > 0 && !out)) return PGO_E_ARG;
  for (int f = 0; f < pgo::kFamCount && f < cap; f++) {
    double* o = out + 5 * (size_t)f;
    o[0] = (double)g->fam_launches[f];
    o[1] = g->fam_ms[f];
    o[2] = g->fam_flops[f];
    o[3] = g->fam_bytes[f];
    o[4] = 0.0;
  }
  return pgo::kFamCount;
}

// diagnostics: a plan of the host graph as it stands (no device state)
static int analyze_host_graph(pgo_graph* g, pgo::GraphStructure& S, pgo::CholPlan& P) {
  RC_TRY(download_values(g));
  RC_TRY(build_structure(g, S));
  P.ordering = g->ordering;
  pgo::chol_analyze(P, S.n, S.row_ptr, S.slot_col);
  return PGO_OK;
}

int pgo_debug_parents(pgo_graph* g, int* parent, int cap) {
  if (!g || cap < 0 || (cap > 0 && !parent)) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  for (int s = 0; s < P.ns && s < cap; s++) parent[s] = P.parent[s];
  return P.ns;
}

int pgo_debug_partition(pgo_graph* g, int size, int* owner, double* out, int cap) {
  if (!g || size < 1 || cap < 0 || (cap > 0 && (!owner || !out))) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  std::vector<double> rf;
  double top = 0;
  const std::vector<int> own = pgo::partition_subtrees(P, size, &rf, &top);
  for (int s = 0; s < P.ns && s < cap; s++) owner[s] = own[s];
  for (int r = 0; r < size && r < cap; r++) out[r] = rf[r];
  if (size < cap) out[size] = top;
  if (cap >= 2 * size + 2) {
    double rep = 0;
    const std::vector<double> df = pgo::distributed_rank_flops(P, size, &rep);
    for (int r = 0; r < size; r++) out[size + 1 + r] = df[r];
    out[2 * size + 1] = rep;
  }
  if (cap >= 2 * size + 4 && size > 1) {   // the exchanges of the distributed top (rank 0's plan: all ranks share them)
    pgo::CholPlan Q;
    Q.ordering = g->ordering;
    Q.part_size = size;
    Q.part_rank = 0;
    pgo::chol_analyze(Q, (int)g->keys.size(), H.row_ptr, H.slot_col);
    double pts = 0, dbl = 0;
    for (const pgo::XExchange& x : Q.xchg) {
      pts++;
      for (long long v : x.size) dbl += (double)v;
    }
    out[2 * size + 2] = pts;
    out[2 * size + 3] = dbl;
  }
  return P.ns;
}

int pgo_debug_ordering(pgo_graph* g, int32_t* perm, size_t n) {
  if (!g || (n && !perm) || n != g->keys.size()) return PGO_E_ARG;
  RC_TRY(download_values(g));
  if (g->chol_ready) {
    if (n) std::memcpy(perm, g->chol.perm.data(), n * sizeof(int32_t));
    return PGO_OK;
  }
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  if (n) std::memcpy(perm, P.perm.data(), n * sizeof(int32_t));
  return PGO_OK;
}

int pgo_debug_fronts(pgo_graph* g, int* w, int* m, int* level, int cap) {
  if (!g || cap < 0 || (cap > 0 && (!w || !m || !level))) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  for (int s = 0; s < P.ns && s < cap; s++) {
    w[s] = P.w[s];
    m[s] = P.m[s];
    level[s] = P.height[s];
  }
  return P.ns;
}

int pgo_debug_row_lanes(pgo_graph* g, int* G, int* G1) {
  if (!g || !G || !G1) return PGO_E_ARG;
  RC_TRY(download_values(g));
  pgo::GraphStructure H;   // the structure upload_structure would build (no plan, no device)
  RC_TRY(build_structure(g, H));
  *G = H.G;
  *G1 = H.G1;
  return PGO_OK;
}

int pgo_debug_plan(pgo_graph* g, double* out, int cap) {
  if (!g || !out || cap < 16) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  if (P.schedule_error) return fail(g, PGO_E_HIP, "internal: inconsistent panel schedule");
  // launches: factor = memsets, assembly, rhs permutation, per level extend-add
  // ranks + vector assembly + small classes + per panel diag/trsm/Schur (+look-ahead);
  // solve (backward only) = per level partials + init + steps, perm out
  long long lf = 5, ls = 1, trsm = 0, syrk = 0;
  int maxm = 0;
  for (int s = 0; s < P.ns; s++) maxm = std::max(maxm, P.m[s]);
  for (const auto& lv : P.levels) {
    lf += (long long)lv.ea_off.size() + 1 + lv.small.size();
    for (const auto& ps : lv.panels)
      lf += (ps.potrf_cnt > 0) + (ps.sdiag_cnt + ps.col_cnt + ps.prep_cnt + (ps.syrk_inline ? ps.syrk_cnt : 0) > 0) +
            (ps.syrk_cnt > 0 && !ps.syrk_inline) + (ps.far_cnt > 0);
    ls += (lv.bwd_part.cnt > 0) + (long long)lv.bwd.size();
    for (const auto& ps : lv.panels) {
      trsm += ps.fcol_cnt + ps.col_cnt;
      syrk += ps.syrk_cnt;
    }
  }
  for (int i = 0; i < cap; i++) out[i] = 0.0;
  out[0] = P.ns;
  out[1] = (double)P.levels.size();
  out[2] = P.nnzl;
  out[3] = P.flops;
  out[4] = P.syrk_flops;
  out[5] = (double)P.ftotal;
  out[6] = (double)lf;
  out[7] = (double)ls;
  out[8] = maxm;
  out[9] = (double)trsm;
  out[10] = (double)syrk;
  out[11] = (double)P.small_list.size();
  // fused update-matrix tiles (pgo_chol.h syrk_gather): all; with a child
  // rectangle; with more than one gather pass of them; clipped by the front's edge
  out[12] = (double)P.fused_tiles;
  out[13] = (double)P.fused_with_pairs;
  out[14] = (double)P.fused_multipass;
  out[15] = (double)P.fused_edge;
  int o = 16;
  for (const auto& lv : P.levels) {   // per level: fronts, max m, max blocks, panels, small fronts, syrk tiles
    if (o + 6 > cap) break;
    long long tiles = 0;
    int small = 0;
    for (const auto& ps : lv.panels) tiles += ps.syrk_cnt;
    for (const auto& sc : lv.small) small += sc.cnt;
    out[o++] = lv.front_cnt;
    out[o++] = lv.maxm;
    out[o++] = lv.maxblk;
    out[o++] = (double)lv.panels.size();
    out[o++] = small;
    out[o++] = (double)tiles;
  }
  return PGO_OK;
}

int pgo_debug_plan_digest(pgo_graph* g, int part_size, int part_rank, uint64_t* out, int cap) {
  if (!g || part_size < 1 || part_rank < 0 || part_rank >= part_size || cap < 0 || (cap > 0 && !out)) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  P.part_size = part_size;
  P.part_rank = part_rank;
  RC_TRY(analyze_host_graph(g, H, P));
  uint64_t v[pgo::kDigestSections + pgo::kBranchCounters];
  long long br[pgo::kBranchCounters];
  pgo::plan_digest(P, v);
  pgo::plan_branch_counters(P, br);
  for (int i = 0; i < pgo::kBranchCounters; i++) v[pgo::kDigestSections + i] = (uint64_t)br[i];
  for (int i = 0; i < cap && i < pgo::kDigestSections + pgo::kBranchCounters; i++) out[i] = v[i];
  return pgo::kDigestSections;
}

int pgo_debug_selinv_plan(pgo_graph* g, double* out, int cap) {
  if (!g || !out || cap < 4) return PGO_E_ARG;
  pgo::GraphStructure H;
  pgo::CholPlan P;
  RC_TRY(analyze_host_graph(g, H, P));
  if (P.schedule_error) return fail(g, PGO_E_HIP, "internal: inconsistent panel schedule");
  const pgo::SelPlan& Q = P.sel;
  for (int i = 0; i < cap; i++) out[i] = 0.0;
  out[0] = Q.launches;
  out[1] = pgo::selinv_flops(P);
  // Z in the fronts' layout, the panel scratch, the partial products, the read-out buffer
  out[2] = (double)P.ftotal + (double)Q.gmax + 4096.0 * (double)Q.pmax + 9.0 * ((double)P.n + (double)g->ek1.size());
  out[3] = (double)Q.levels.size();
  for (size_t L = 0; L < Q.levels.size() && 4 + (int)L < cap; L++) {   // launches per level, leaves first
    const pgo::SelLevel& sl = Q.levels[L];
    int n = (sl.small_cnt > 0) + (sl.gat_cnt > 0);
    for (const pgo::SelStep& st : sl.steps) n += 2 * (st.tile_cnt > 0) + 1;
    out[4 + L] = n;
  }
  return PGO_OK;
}

int pgo_debug_linearize(pgo_graph* g, double* hdiag, double* hoff, double* grad, double* err) {
  if (!g) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  DevGraph& d = g->d;
  d.write_all = 1;   // diagnostics read every block
  HIP_TRY(g, pgo::launch_linearize(d));
  HIP_TRY(g, pgo::launch_error(d, d.pose, d.scal));  // overwrites partial slice A
  std::vector<double> V(9 * (size_t)d.nslots), D(6 * (size_t)d.n), G(3 * (size_t)d.n);
  if (d.nslots) HIP_TRY(g, hipMemcpyAsync(V.data(), d.V, V.size() * 8, hipMemcpyDeviceToHost, d.stream));
  if (d.n) {
    HIP_TRY(g, hipMemcpyAsync(D.data(), d.D, D.size() * 8, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(g, hipMemcpyAsync(G.data(), d.g, G.size() * 8, hipMemcpyDeviceToHost, d.stream));
  }
  RC_TRY(sync_scalars(g, 1));
  if (err) *err = g->h_scal[0];
  if (hdiag)
    for (int i = 0; i < d.n; i++) {
      const double* s = &D[6 * (size_t)i];
      double* o = hdiag + 9 * (size_t)i;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
      o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
    }
  if (hoff)
    for (int e = 0; e < d.ne; e++)
      for (int q = 0; q < 9; q++) hoff[9 * (size_t)e + q] = V[q * (size_t)d.nslots + g->gs.edge_slot0[e]];
  if (grad && !G.empty()) std::memcpy(grad, G.data(), G.size() * 8);
  return PGO_OK;
}

// Same outputs from the Cholesky-mode linearisation (k_linearize_own +
// k_linearize_side1): owner blocks in factor order, transposed back to
// H_{k1,k2} where the owner is the factor's side-1 block.
int pgo_debug_linearize_cholesky(pgo_graph* g, double* hdiag, double* hoff, double* grad, double* err) {
  if (!g) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  DevGraph& d = g->d;
  if (d.n == 0) return PGO_OK;
  RC_TRY(ensure_chol(g));
  d.write_all = 0;
  HIP_TRY(g, pgo::launch_linearize(d));
  HIP_TRY(g, pgo::launch_error(d, d.pose, d.scal));
  std::vector<double> V(9 * (size_t)d.nslots), D(6 * (size_t)d.n), G(3 * (size_t)d.n);
  if (d.nslots) HIP_TRY(g, hipMemcpyAsync(V.data(), d.V, V.size() * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(D.data(), d.D, D.size() * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipMemcpyAsync(G.data(), d.g, G.size() * 8, hipMemcpyDeviceToHost, d.stream));
  RC_TRY(sync_scalars(g, 1));
  if (err) *err = g->h_scal[0];
  if (hdiag)
    for (int i = 0; i < d.n; i++) {
      const double* s = &D[6 * (size_t)i];
      double* o = hdiag + 9 * (size_t)i;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
      o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
    }
  if (hoff)
    for (int e = 0; e < d.ne; e++) {
      const int se = g->gs.codes()[g->gs.edge_slot0[e]];
      const size_t de = (size_t)(se >> 2);
      const bool side0_owner = (se & 2) != 0;
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
          hoff[9 * (size_t)e + 3 * r + c] = V[9 * de + (side0_owner ? 3 * r + c : 3 * c + r)];
    }
  if (grad && !G.empty()) std::memcpy(grad, G.data(), G.size() * 8);
  return PGO_OK;
}

int pgo_debug_spmv(pgo_graph* g, double lambda, const double* x, double* y) {
  if (!g || !x || !y) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  DevGraph& d = g->d;
  d.write_all = 1;   // diagnostics read every block
  HIP_TRY(g, pgo::launch_linearize(d));
  RC_TRY(h2d(g, d.p, x, 3 * (size_t)d.n));
  HIP_TRY(g, pgo::launch_spmv(d, lambda, d.p, d.q));
  if (d.n) HIP_TRY(g, hipMemcpyAsync(y, d.q, 3 * (size_t)d.n * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  return PGO_OK;
}

int pgo_debug_factor_time(pgo_graph* g, int lanes, int reps, double* ms) {
  if (!g || lanes < 1 || lanes > 8 || reps < 1 || !ms) return PGO_E_ARG;
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipSetDevice(g->device));
  DevGraph& d = g->d;
  if (d.n == 0) return fail(g, PGO_E_ARG, "empty graph");
  g->part_size = 1;
  RC_TRY(ensure_chol(g));
  d.write_all = 0;
  HIP_TRY(g, pgo::launch_linearize(d));
  const int L = lanes > 1 ? ensure_lanes(g, lanes) : 1;
  if (L < lanes) return fail(g, PGO_E_NOMEM, "not enough memory for the lambda lanes");
  for (int l = 0; l < L; l++) g->h_lanes[4 * 8 + l] = 1e-5 * std::pow(10.0, l);
  HIP_TRY(g, hipMemcpyAsync(g->chol.d_lambda, g->h_lanes + 4 * 8, L * sizeof(double), hipMemcpyHostToDevice,
                            d.stream));
  RC_TRY(graph_factor_solve(g, L, L > 1 ? g->xb : d.x, L > 1 ? 3LL * d.n : 0, true));   // capture + warm
  HIP_TRY(g, hipEventRecord(g->ev[0], d.stream));
  for (int r = 0; r < reps; r++) HIP_TRY(g, hipGraphLaunch(g->fac_exec[L], d.stream));
  HIP_TRY(g, hipEventRecord(g->ev[1], d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  *ms = ms_between(g->ev[0], g->ev[1]) / reps;
  return PGO_OK;
}

int pgo_debug_poison_fronts(pgo_graph* g) {
  if (!g) return PGO_E_ARG;
  if (!g->chol_ready || !g->chol.F) return fail(g, PGO_E_ARG, "no Cholesky workspace yet (optimize first)");
  HIP_TRY(g, hipSetDevice(g->device));
  HIP_TRY(g, pgo::chol_debug_poison(g->chol, g->d.stream));
  return PGO_OK;
}

int pgo_debug_solve(pgo_graph* g, double lambda, const pgo_params* params, double* delta, int* pcg_iterations) {
  if (!g || !delta) return PGO_E_ARG;
  pgo_params p;
  if (params) p = *params;
  else pgo_default_params(&p);
  RC_TRY(ensure_device(g));
  DevGraph& d = g->d;
  // the Cholesky assembly reads the owner blocks in factor order (k_linearize_own)
  g->part_size = 1;
  if (p.linear_solver != PGO_SOLVER_PCG && d.n > 0) RC_TRY(ensure_chol(g));
  if (p.linear_solver == PGO_SOLVER_PCG) RC_TRY(unmix_slot_codes(g));
  d.write_all = p.linear_solver == PGO_SOLVER_PCG ? 1 : 0;
  HIP_TRY(g, pgo::launch_linearize(d));
  pgo_stats st;
  std::memset(&st, 0, sizeof(st));
  SolveState ss;
  RC_TRY(linear_solve(g, p, lambda, &st, &ss));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  RC_TRY(finish_solve(g, nullptr, &ss));
  if (d.n) HIP_TRY(g, hipMemcpyAsync(delta, d.x, 3 * (size_t)d.n * 8, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(g, hipStreamSynchronize(d.stream));
  if (pcg_iterations) *pcg_iterations = (int)st.pcg_iterations;
  if (!ss.solved) return fail(g, PGO_E_INDETERMINANT, "linear system not positive definite");
  return PGO_OK;
}

}  // extern "C"

// ---- pgo_map_render_graph's view of a graph (pgo_map.h): the key -> index map
// and the device pose table; the pgo_graph calls are synchronous, so the table
// is at rest when the map's stream reads it
namespace pgo {

long long graph_vertex_index(const pgo_graph* g, uint64_t key) {
  const auto it = g->index.find(key);
  return it == g->index.end() ? -1 : (long long)it->second;
}

int graph_device_ordinal(const pgo_graph* g) { return g->device; }

int graph_device_poses(pgo_graph* g, const void** pose, size_t* n) {
  RC_TRY(ensure_device(g));
  HIP_TRY(g, hipStreamSynchronize(g->d.stream));
  *pose = g->d.pose;
  *n = (size_t)g->d.n;
  return PGO_OK;
}

}  // namespace pgo
