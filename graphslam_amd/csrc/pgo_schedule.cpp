// The panel scheduler of the GPU supernodal Cholesky (pgo_chol.h): from the
// plan's fronts, every launch list the factorisation, the solves, the selected
// inversion and the partitioned plans run from (chol_schedule, at the end,
// names the passes).  Host code, no HIP call.  A plan is a function of the
// fronts and the knobs alone, never of the thread count (pgo_plan_digest.h
// states "the same plan"; tests/test_plan_digest.py).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "pgo_chol.h"
#include "pgo_structure.h"

namespace pgo {

namespace {

long long env_ll(const char* name, long long dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; }

// The planner's knobs, read at the top of chol_schedule and nowhere below it.
struct ScheduleKnobs {
  // read at every schedule (tests change them in-process)
  bool lookahead = !getenv("PGO_NO_LOOKAHEAD");
  bool far_on = env_ll("PGO_FAR", 0) == 1;   // deferred far updates (off: PanelStep::far_cnt)
  int la_m = (int)env_ll("PGO_LOOKAHEAD_M", kLookaheadM);   // the look-ahead fronts' height threshold, a test knob
  bool dist_top = env_ll("PGO_DIST_TOP", 1) != 0;   // 0: the top fronts replicated on every rank (host self-test)
  bool fuse = env_ll("PGO_FUSE_UPDATE", 1) != 0;
  bool debug = getenv("PGO_SCHED_DEBUG") != nullptr;
  // read once per process
  long long big_min;   // PGO_BIGTILE_MIN: the 128-tile threshold, a tuning knob
  int asm_xcd;         // PGO_ASM_XCD: 0 keeps the assembly tiles' natural order, 2 orders every level
  bool timing;         // PGO_PLAN_TIMING
  ScheduleKnobs() {
    static const long long b = env_ll("PGO_BIGTILE_MIN", 4096);
    static const int x = (int)env_ll("PGO_ASM_XCD", 1);
    static const bool t = getenv("PGO_PLAN_TIMING") != nullptr;
    big_min = b, asm_xcd = x, timing = t;
  }
};

// Every schedule list that is built per level and appended to the plan's list
// of the same name (syrk_gather: one record per syrk task).
#define PGO_LEVEL_LISTS(X)                                                                                          \
  X(small_list) X(level_fronts) X(potrf_list) X(syrk_tasks) X(syrk_gather) X(sdiag_tasks) X(col_tasks) X(bwd_tasks) \
  X(bwdc_tasks) X(bwd_pref) X(bwd_part_tasks) X(ea_tasks) X(ea_pairs) X(xchg) X(xp_tasks) X(xp_loff) X(xp_lstride)

// One level's share of the schedule lists (chol_schedule builds the levels
// concurrently, then appends them to the plan's lists in level order).
struct LevelLists {
#define X(n) decltype(CholPlan::n) n;
  PGO_LEVEL_LISTS(X)
#undef X
  long long fused = 0, fused_with_pairs = 0, fused_multipass = 0, fused_edge = 0, xp_rslot = 0;
  int npart = 0;
  bool schedule_error = false;
  // empty again, capacity kept
  void reset() {
#define X(n) n.clear();
    PGO_LEVEL_LISTS(X)
#undef X
    fused = fused_with_pairs = fused_multipass = fused_edge = xp_rslot = npart = 0;
    schedule_error = false;
  }
};

struct ListBase {   // where a level's lists start in the plan's
#define X(n) size_t n = 0;
  PGO_LEVEL_LISTS(X)
#undef X
  int npart = 0;
};

// the schedule's update bookkeeping failed: the plan is unusable (PGO_SCHED_DEBUG: the level's first failure printed)
void sched_fail(LevelLists& S, const ScheduleKnobs& K, const char* fmt, ...) {
  if (K.debug && !S.schedule_error) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
  }
  S.schedule_error = true;
}

// dense Cholesky flops of the w pivot columns of an m-row front, plus the
// inverses of its diagonal blocks (what the small-front kernels form)
double front_flops(int m, int w) {
  double f = (double)w * w * w / 3.0;
  for (int k = 0; k < w; k++) {
    const double r = m - k - 1;
    f += 1 + r + r * (r + 1);
  }
  return f;
}

// tasks dealt round-robin from the 8 XCDs' queues into out[0..)
void deal(const std::vector<std::vector<int4>>& q, int4* out) {
  std::vector<size_t> pos(q.size(), 0);
  for (bool any = true; any;) {
    any = false;
    for (size_t x = 0; x < q.size(); x++)
      if (pos[x] < q[x].size()) {
        *out++ = q[x][pos[x]++];
        any = true;
      }
  }
}

}  // namespace

void xcd_order(std::vector<int4>& tasks, int tile) {
  constexpr int kXcd = 8, kBlk = 8;
  if ((int)tasks.size() < 4 * kXcd * kBlk) return;   // small launches: keep the natural order
  const int span = tile * kBlk;
  // (front, column block, row block) packed in the high bits, the task index in
  // the low 32: a plain sort of the keys is the stable sort by block
  // (block indices below 2^16: rows and columns below 2^20, span >= 512)
  using u128 = unsigned __int128;
  std::vector<u128> key(tasks.size());
  for (size_t i = 0; i < tasks.size(); i++) {
    const int4& t = tasks[i];
    const unsigned long long blk = (unsigned long long)(unsigned)t.x << 32 | (unsigned long long)(t.z / span) << 16 |
                                   (unsigned)((t.y & kRowMask) / span);
    key[i] = (u128)blk << 32 | i;
  }
  std::sort(key.begin(), key.end());
  std::vector<std::vector<int4>> q(kXcd);
  for (auto& v : q) v.reserve(tasks.size() / kXcd + 1);
  int blk = -1;
  unsigned long long prev = ~0ull;
  for (const u128 k : key) {
    if ((unsigned long long)(k >> 32) != prev) {
      blk++;
      prev = (unsigned long long)(k >> 32);
    }
    q[blk % kXcd].push_back(tasks[(size_t)(k & 0xffffffffu)]);
  }
  deal(q, tasks.data());
}

namespace {

// XCD-aware order of the Schur-update tiles [b, e) of one launch
void xcd_order_range(std::vector<int4>& tasks, int b, int e, int tile) {
  std::vector<int4> part(tasks.begin() + b, tasks.begin() + e);
  xcd_order(part, tile);
  std::copy(part.begin(), part.end(), tasks.begin() + b);
}

// XCD-aware order of a level's tile-assembly tasks [off, end): a child's
// update-matrix column lands on a parent column as one run of child rows that
// crosses the parent's row tiles, so vertically adjacent tiles read the same
// 128-byte lines at their run boundaries.  Blocks of kCols x kRows tiles of a
// front, column-major inside, are dealt round-robin to the 8 XCDs (blockIdx
// b -> XCD b % 8 as observed: speed only, each tile is computed alike
// wherever and whenever it runs).  mode (PGO_ASM_XCD) 0 keeps the natural
// order; 2 orders every level, however few its tiles (host self-test).
void ea_xcd_order(std::vector<int4>& tasks, size_t off, int mode) {
  constexpr int kXcd = 8, kCols = 4, kRows = 16;
  const size_t n = tasks.size() - off;
  if (mode == 0 || (mode == 1 && n < (size_t)4 * kXcd * kCols * kRows)) return;
  // key: (block of the front in order of first appearance, column, row), task index
  using u128 = unsigned __int128;
  std::vector<u128> key(n);
  int blk = -1, fprev = -1;
  std::vector<int> bid;   // the front's blocks: (tj / kCols, ti / kRows) -> block number
  int nbr = 0;
  for (size_t i = 0; i < n; i++) {
    const int4& t = tasks[off + i];
    const int ti = t.y >> 16, tj = t.y & 0xffff;
    if (t.x != fprev) {   // a front's tasks are contiguous (row-major lower triangle)
      fprev = t.x;
      int nt = 0;
      for (size_t k = i; k < n && tasks[off + k].x == t.x; k++) nt = std::max(nt, (tasks[off + k].y >> 16) + 1);
      nbr = (nt + kRows - 1) / kRows;
      bid.assign((size_t)((nt + kCols - 1) / kCols) * nbr, -1);
    }
    int& b = bid[(size_t)(tj / kCols) * nbr + ti / kRows];
    if (b < 0) b = ++blk;
    key[i] = (u128)((unsigned long long)b << 32 | (unsigned)tj << 16 | (unsigned)ti) << 32 | i;
  }
  std::sort(key.begin(), key.end());
  std::vector<std::vector<int4>> q(kXcd);
  for (const u128 k : key) q[(int)(k >> 64) % kXcd].push_back(tasks[off + (size_t)(k & 0xffffffffu)]);
  deal(q, tasks.data() + off);
}

// ---- multi-GPU subtree partition (part_size > 1, DESIGN.md "Multi-GPU"):
// rank part_rank factorises the fronts of its subtrees (phase 1), then every
// rank the replicated top fronts (phase 2), after the subtree roots' update
// matrices / vectors have been exchanged.  Storage only for the fronts this
// rank touches: its own, the top, and the other ranks' subtree roots (their
// update matrices arrive in the exchange).  One rank: everything is phase 1.
void partition_layout(CholPlan& P) {
  const int ns = P.ns, psz = std::max(P.part_size, 1), prk = P.part_rank;
  P.owner = partition_subtrees(P, psz);
  P.subtree_cnt.assign(ns, 1);
  for (int s = 0; s < ns; s++)
    if (P.parent[s] >= 0) P.subtree_cnt[P.parent[s]] += P.subtree_cnt[s];
  std::vector<char> need(ns, 0);
  P.xroot.clear(), P.xroot_rank.clear();
  for (int s = 0; s < ns; s++) {
    const bool root = P.owner[s] >= 0 && (P.parent[s] < 0 || P.owner[P.parent[s]] < 0);
    if (root) {
      P.xroot.push_back(s);
      P.xroot_rank.push_back(P.owner[s]);
    }
    need[s] = P.owner[s] == prk || P.owner[s] < 0 || (root && P.parent[s] >= 0);
  }
  if (psz > 1) {   // offsets over the needed fronts only
    for (int s = 0; s < ns; s++) {
      P.foff[s + 1] = P.foff[s] + (need[s] ? ((front_elems(P.m[s], P.w[s]) + 15) / 16) * 16 : 0);
      P.voff[s + 1] = P.voff[s] + (need[s] ? ((P.m[s] + 7) / 8) * 8 : 0);
      P.toff[s + 1] = P.toff[s] + (need[s] ? (long long)((P.w[s] + 63) / 64) * 4096 : 0);
    }
    P.ftotal = P.foff[ns], P.ttotal = P.toff[ns], P.vtotal = P.voff[ns];
  }
  // exchange layout: per rank its roots' payloads (packed lower update matrix,
  // then the update vector) back to back; the solve's: its subtrees' poses
  P.xroot_off.assign(P.xroot.size(), 0);
  P.xsize.assign(psz, 0), P.xsol_size.assign(psz, 0);
  P.xsol_ranges.clear();
  for (size_t q = 0; q < P.xroot.size(); q++) {
    const int sr = P.xroot[q], r = P.xroot_rank[q];
    const long long u = P.m[sr] - P.w[sr];
    P.xroot_off[q] = P.xsize[r];
    P.xsize[r] += u * (u + 1) / 2 + u;
    const int first = sr - P.subtree_cnt[sr] + 1;   // the subtree: postorder fronts [first, sr]
    P.xsol_ranges.push_back(make_int4(r, 3 * P.sfirst[first], 3 * P.sfirst[sr + 1], (int)P.xsol_size[r]));
    P.xsol_size[r] += 3LL * (P.sfirst[sr + 1] - P.sfirst[first]);
  }
  P.xmax = *std::max_element(P.xsize.begin(), P.xsize.end());
  P.xsol_max = *std::max_element(P.xsol_size.begin(), P.xsol_size.end());
}

// The levels' fronts: phase 1 (this rank's subtree fronts) then phase 2 (the
// top), by height; a height with no front of this rank is dropped.  Sets P.split.
std::vector<std::vector<int>> level_buckets(CholPlan& P) {
  std::vector<std::vector<int>> bylevel;
  for (int phase = 0; phase < 2; phase++) {
    auto in_phase = [&](int s) { return phase == 0 ? P.owner[s] == P.part_rank : P.owner[s] < 0; };
    int hmax = -1;
    for (int s = 0; s < P.ns; s++)
      if (in_phase(s)) hmax = std::max(hmax, P.height[s]);
    const size_t base = bylevel.size();
    bylevel.resize(base + hmax + 1);
    for (int s = 0; s < P.ns; s++)
      if (in_phase(s)) bylevel[base + P.height[s]].push_back(s);
    if (phase == 0) P.split = (int)bylevel.size();
  }
  std::vector<std::vector<int>> kept;
  int split = 0;
  for (size_t L = 0; L < bylevel.size(); L++)
    if (!bylevel[L].empty()) {
      kept.push_back(std::move(bylevel[L]));
      if ((int)L < P.split) split++;
    }
  P.split = split;
  return kept;
}

// Front (w, m) at its panel kb: the panel [kb, kn); the kKB block [.., be) the
// panel sits in (its Schur update is deferred by kKB-column blocks: inside a
// block -- inner -- only the block's remaining columns [kn, be) are updated,
// after the block's last panel the trailing columns [be, m) get the whole
// block's update: colend, the device's column clip); and, when the front has a
// panel after the next (kn2 < w), the column block [kn2, c2) the next step prepares.
struct PanelGeom {
  int nb, kn, be, colend, kn2, c2;
  bool inner;
  PanelGeom(int w, int m, int kb) {
    nb = std::min(kNB, w - kb), kn = kb + nb;
    be = std::min((kb & ~(kKB - 1)) + kKB, w);
    inner = kn < be;
    colend = inner ? be : m;
    kn2 = kn + kNB;
    const int be2 = std::min((kn & ~(kKB - 1)) + kKB, w);
    c2 = std::min(kn2 + kNB, kn2 < be2 ? be2 : m);
  }
};

// Look-ahead bookkeeping of a level's blocked fronts `big`.
// applied[i][j]: the first panel column whose Schur update column j of big
// front i has not received yet (every task updates whole columns: rows from the
// column down).  A step's tasks must find their columns uniform.
// touch[step][i]: the largest column the step's k_step tasks and near plain
// tiles touch; far0[step][piece][i]: the first column of the step's far plain
// tiles (deferred far updates: an apart step at a kKB block end; m = none), the
// far range cut at the kKB blocks (the update-matrix columns past w one piece),
// each piece joined on its own.
struct LookAhead {
  std::vector<std::vector<int>> applied, touch;
  std::vector<std::vector<std::vector<int>>> far0;
  bool apart_chain = false;   // once a step's plain tiles go to their own launch, the later ones do too
  LookAhead(const CholPlan& P, const std::vector<int>& big) : applied(big.size()) {
    for (size_t i = 0; i < big.size(); i++) applied[i].assign(P.m[big[i]], 0);
  }
  void begin_step() { touch.emplace_back(applied.size(), 0), far0.emplace_back(); }
  // columns [c0, c1) of front i must all stand at k0 (on_bad() if not, or if `bad`); they move to kn
  template <class F>
  void advance(size_t i, int c0, int c1, int k0, int kn, bool bad, F&& on_bad) {
    for (int j = c0; j < c1 && !bad; j++) bad = applied[i][j] != k0;
    if (bad) on_bad();
    std::fill(applied[i].begin() + c0, applied[i].begin() + c1, kn);
  }
  void touched(size_t i, int col) { touch.back()[i] = std::max(touch.back()[i], col); }
  // a far piece is joined before the first later step whose k_step tasks or
  // near plain tiles touch one of its columns (-1: at the level's end)
  void join_far(CholLevel& lv) const {
    for (size_t q = 0; q < lv.far_pieces.size(); q++) {
      int4& fp = lv.far_pieces[q];
      const int j = fp.x, g = (int)q - lv.panels[j].far_p0;
      const std::vector<int>& f0 = far0[j][g];
      fp.w = -1;
      for (size_t j2 = j + 1; j2 < lv.panels.size() && fp.w < 0; j2++)
        for (size_t i = 0; i < f0.size(); i++)
          if (touch[j2][i] > f0[i]) {
            fp.w = (int)j2;
            break;
          }
    }
  }
};

struct StepWork {   // one panel step being built
  PanelStep ps;
  std::vector<int4> xfirst, xstep;   // distributed top: panels factored by the first / the step launch
  std::vector<int4> plain;           // (front, first column, end column, k0): rows from the column down
  // ... the far part of an apart step's plain range (a kKB block end: the columns past the next block,
  // [be + kKB, m)): its own launch on a fourth stream, joined only before the first later step that touches them
  std::vector<std::vector<int4>> plain_far;   // [piece]: the ranges of every front's piece g
  std::vector<double> far_pflops;
  std::vector<int4> prep;            // prep tiles (front, r0, c0, k0), whole 64x64 tiles
  bool conflict = false;             // a front's next step reads this step's plain tiles
};

// One level's schedule into its own lists (offsets level-relative; merged in
// level order, so the plan is the same for any thread count).
//
// Distributed top (part_size > 1, dist): the top fronts' columns are dealt to
// the ranks instead of every rank factoring every top front.  A blocked top
// front's pivot columns go by 64-column panel, round robin (continuing over
// the fronts); its columns past the last whole panel (the update matrix) take
// the rank of the parent column they extend-add into, so a rank's share of a
// parent's columns is assembled from its own shares of the children's update
// matrices (no exchange of update matrices between top fronts).  Small top
// fronts (one workgroup / wavefront each) are computed by every rank (-1),
// and so are the update columns of their children.  Each column's updates
// are applied by its rank only, with the same tasks (same depths, same
// order) as the one-rank plan: bitwise the one-rank factor.  A rank receives
// every panel (broadcast by its owner right after it is factored) for its own
// columns' updates and the replicated backward solve.
struct LevelCtx {
  CholPlan& P;
  const ScheduleKnobs& K;
  const std::vector<int>& fronts;   // the level's fronts
  CholLevel& lv;
  LevelLists& S;
  bool dist;                        // a distributed top level: this rank generates only the tasks of its columns

  bool mine(int s, int col) const {
    if (!dist) return true;
    const int o = P.cown[P.cown_off[s] + col];
    return o < 0 || o == P.part_rank;
  }
  int cowner(int s, int col) const { return dist ? P.cown[P.cown_off[s] + col] : -1; }
  bool front_skip(int s) const { return K.lookahead && P.m[s] >= K.la_m; }
  // Prep (look-ahead fronts): the step also brings the column block after
  // the next one, [kn + 64, kn + 128), up to date with the panels before kn
  // (k_step workgroups beside the diagonal chain), so the next step's
  // diagonal and column tasks apply one panel only; the plain tiles skip
  // that block too.  Only for whole 64-column pivot blocks.
  bool has_prep(int s, int kn) const { return front_skip(s) && kn + 2 * kNB <= P.w[s]; }

  // part 0 (members of S and lv disjoint from part 1's: the two parts of a level run concurrently)
  void front_list(), bwd_init(), bwd_chain(), bwd_steps(), extend_add();
  // part 1: the small-front classes return the blocked fronts `big`, which the panel steps take
  std::vector<int> small_classes();
  void panel_steps(const std::vector<int>& big), first_panel(const std::vector<int>& big, StepWork& W);
  void plain_range(int s, const PanelGeom& g, int& cstart, int& cend) const;
  long long ntiles(const std::vector<int>& big, int kb, int T) const;
  void front_step(size_t i, int s, int kb, LookAhead& la, StepWork& W);
  void emit_tiles(const std::vector<int>& big, bool apart, LookAhead& la, StepWork& W);
  int add_exchange(const std::vector<int4>& items);
  void tail_exchange(const std::vector<int>& big), check_complete(const std::vector<int>& big, const LookAhead& la);
};

void LevelCtx::front_list() {
  lv.front_off = (int)S.level_fronts.size();
  lv.front_cnt = (int)fronts.size();
  for (int s : fronts) {
    S.level_fronts.push_back(s);
    lv.maxm = std::max(lv.maxm, P.m[s]);
    if (P.m[s] <= kSmallFront) lv.small_maxm = std::max(lv.small_maxm, P.m[s]);
    lv.maxblk = std::max(lv.maxblk, (P.w[s] + 63) / 64);
    // frontal vectors: own rows gathered from the permuted rhs, the children's
    // update vectors with their row maps, the vector written
    lv.vec_bytes += 8.0 * P.m[s] + (8.0 + 4.0 / 3.0) * P.w[s];
    for (int q = P.cptr[s]; q < P.cptr[s + 1]; q++) lv.vec_bytes += (8.0 + 4.0 / 3.0) * (P.m[P.children[q]] - P.w[P.children[q]]);
  }
}

// Blocked backward solve (64-column blocks of each front's pivot columns; the
// forward substitution is carried by the factorisation).  Init: all columns vs
// the rows below w -- partial products L21[r0:r0+kBwdRows, block]' x_below, one
// task each, reduced in fixed order by the init task of the block.
void LevelCtx::bwd_init() {
  SolveStep sp{(int)S.bwd_part_tasks.size(), 0};
  SolveStep st{(int)S.bwd_tasks.size(), 0};
  for (int s : fronts) {
    const int w = P.w[s], m = P.m[s], nblk = (w + 63) / 64;
    for (int b = 0; b < nblk; b++) {
      const int p0 = S.npart;
      for (int r0 = w; r0 < m; r0 += kBwdRows) S.bwd_part_tasks.push_back(make_int4(s, b * 64, r0, S.npart++));
      S.bwd_tasks.push_back(make_int4(s, b * 64, std::min(b * 64 + 64, w), b == nblk - 1 ? b : -1));
      S.bwd_pref.push_back(make_int2(p0, S.npart - p0));
    }
  }
  sp.cnt = (int)S.bwd_part_tasks.size() - sp.off;
  for (int q = sp.off; q < sp.off + sp.cnt; q++) {
    const int4 t = S.bwd_part_tasks[q];
    const double ncol = std::min(64, P.w[t.x] - t.y), rows = std::min(kBwdRows, P.m[t.x] - t.z);
    lv.bwd_part_flops += 2.0 * ncol * rows;
    // L rows x columns, x gathered per row (+ its pose index per 3 rows), the 64 partial sums out
    lv.bwd_part_bytes += 8.0 * ncol * rows + rows * (8.0 + 4.0 / 3.0) + 8.0 * 64;
  }
  st.cnt = (int)S.bwd_tasks.size() - st.off;
  for (int q = st.off; q < st.off + st.cnt; q++) {   // init: partials + y in, X_jj' z for the last block, x out
    const int4 t = S.bwd_tasks[q];
    const double n2 = t.z - t.y, np = S.bwd_pref[q].y;
    lv.bwd_init_bytes += 8.0 * n2 * (np + 2.0) + (t.w >= 0 ? 8.0 * n2 * (64.0 + 1.0) + 4.0 * n2 / 3.0 : 0.0);
  }
  lv.bwd_part = sp;
  lv.bwd.push_back(st);
}

// The backward steps as one chained launch (k_bwd_chain): block j of a front
// after the blocks above it, tasks ordered by distance from the last block so
// that every workgroup waits only on earlier-dispatched ones.
void LevelCtx::bwd_chain() {
  lv.bwdc.off = (int)S.bwdc_tasks.size();
  for (int d = 1; d < lv.maxblk; d++)
    for (int s : fronts) {
      const int w = P.w[s], nblk = (w + 63) / 64;
      if (d >= nblk) continue;
      const int j = nblk - 1 - d;
      S.bwdc_tasks.push_back(make_int4(s, j * 64, j * 64 + 64, j));
      // L[block b, block j] for every block b below j and its x_b, X_jj, z in, x out
      const double n2 = std::min(64, w - 64 * j);
      lv.bwd_chain_bytes += 8.0 * (w - 64.0 * (j + 1)) * (n2 + 1.0) + 8.0 * n2 * (64.0 + 3.0) + 4.0 * n2 / 3.0;
    }
  lv.bwdc.cnt = (int)S.bwdc_tasks.size() - lv.bwdc.off;
}

void LevelCtx::bwd_steps() {
  for (int b = lv.maxblk - 1; b >= 1; b--) {   // backward step b: columns left of block b
    SolveStep st{(int)S.bwd_tasks.size(), 0};
    for (int s : fronts) {
      if (b >= (P.w[s] + 63) / 64) continue;
      for (int c = 0; c < b; c++) {
        S.bwd_tasks.push_back(make_int4(s, c * 64, c * 64 + 64, c == b - 1 ? c : -1));
        S.bwd_pref.push_back(make_int2(0, 0));
      }
    }
    st.cnt = (int)S.bwd_tasks.size() - st.off;
    lv.bwd.push_back(st);
  }
}

// Assembly: one task per 64x64 tile of every front's lower triangle (the fused
// ones leave the list in fuse_level, which also orders the rest and sets
// ea_cnt), which it writes whole: its H entries (+ lambda on the diagonal),
// then the update-matrix elements of the front's children in order (fixed
// summation order, no atomics), each child contributing a rectangle of its
// update matrix (child rows [a0, a0+nr) x columns [b0, b0+nc), the rows /
// columns whose parent index falls in the tile).  No front is zeroed.
void LevelCtx::extend_add() {
  lv.ea_off.push_back((int)S.ea_tasks.size());
  std::vector<int> tcnt, tpos;
  std::vector<int4> runs;   // (child, tile, first child row, rows) of every child, children in order
  for (int sp : fronts) {
    const int nt = (P.m[sp] + 63) / 64;
    tcnt.assign((size_t)nt * (nt + 1) / 2, 0);
    runs.clear();
    std::vector<int> cr(1, 0);   // runs of child q: [cr[q], cr[q + 1])
    for (int q = P.cptr[sp]; q < P.cptr[sp + 1]; q++) {
      const int c = P.children[q];
      const int u = P.m[c] - P.w[c];
      const size_t r0 = runs.size();
      const int* rel = P.ea_rel.data() + P.ea_ptr[c];
      auto add = [&](int t, int a, int nr) {
        if (runs.size() == r0 || runs.back().y != t) runs.push_back(make_int4(c, t, a, 0));
        runs.back().w += nr;
      };
      // (row a of the update matrix: parent row 3 rel[a / 3] + a % 3; a pose's
      // three rows in one tile go as one)
      for (int a = 0; a < u; a += 3) {
        const int r = 3 * rel[a / 3];
        if ((r >> 6) == ((r + 2) >> 6) && a + 3 <= u) {
          add(r >> 6, a, 3);
        } else {
          for (int k = 0; k < 3 && a + k < u; k++) add((r + k) >> 6, a + k, 1);
        }
      }
      for (size_t i = r0; i < runs.size(); i++)   // a child's runs are in increasing tiles: one pair per tile
        for (size_t j = r0; j <= i; j++) tcnt[(size_t)runs[i].y * (runs[i].y + 1) / 2 + runs[j].y]++;
      cr.push_back((int)runs.size());
    }
    const int base = (int)S.ea_pairs.size();
    tpos.assign(tcnt.size(), 0);
    for (size_t k = 1; k < tcnt.size(); k++) tpos[k] = tpos[k - 1] + tcnt[k - 1];
    for (int ti = 0; ti < nt; ti++)
      for (int tj = 0; tj <= ti; tj++) {
        const size_t k = (size_t)ti * (ti + 1) / 2 + tj;
        S.ea_tasks.push_back(make_int4(sp, (ti << 16) | tj, base + tpos[k], tcnt[k]));
      }
    S.ea_pairs.resize(base + (tcnt.empty() ? 0 : tpos.back() + tcnt.back()));
    for (size_t q = 0; q + 1 < cr.size(); q++)   // children in order: their pairs in order within every tile
      for (int i = cr[q]; i < cr[q + 1]; i++)
        for (int j = cr[q]; j <= i; j++) {
          const size_t k = (size_t)runs[i].y * (runs[i].y + 1) / 2 + runs[j].y;
          S.ea_pairs[base + tpos[k]++] = make_int4(runs[i].x, runs[i].z, runs[j].z, runs[i].w | (runs[j].w << 8));
        }
  }
}

// Small fronts (not front_packed: m <= kSmallFront, w <= kWaveW): one wavefront
// each (the m x w panel in LDS, the rank-w Schur update streamed), by class
// m <= 64 (one row per lane) | 64 < m <= 128  x  w <= 8 | 16 | 32, largest
// first.  A front with more pivot columns takes the blocked path (64-column
// panels, every front of the level in the same launches -- a whole-front-in-LDS
// workgroup runs its w pivots one after the other at ~2 us each): returned.
// (The one-workgroup classes by size, wave 0, take what is neither: today nothing.)
std::vector<int> LevelCtx::small_classes() {
  const int classes[4] = {32, 64, 96, kSmallFront};
  std::vector<int> big, bucket[4], wave;
  for (int s : fronts) {
    if (front_packed(P.m[s], P.w[s])) {
      big.push_back(s);
    } else if (P.w[s] <= kWaveW) {
      wave.push_back(s);
    } else {
      int q = 0;
      while (P.m[s] > classes[q]) q++;
      bucket[q].push_back(s);
    }
  }
  auto add_class = [&](const std::vector<int>& part, int W) {
    if (part.empty()) return;
    SmallClass sc{(int)S.small_list.size(), (int)part.size(), 0, W};
    for (int s : part) {
      S.small_list.push_back(s);
      sc.mmax = std::max(sc.mmax, P.m[s]);
      sc.flops += front_flops(P.m[s], P.w[s]);
    }
    lv.small.push_back(sc);
  };
  for (int cls = 0; cls < 6; cls++) {
    const int rc = cls / 3, W = cls % 3 == 0 ? 8 : cls % 3 == 1 ? 16 : kWaveW;
    const int Wlo = cls % 3 == 0 ? 0 : W / 2;
    std::vector<int> part;
    for (int s : wave)
      if ((P.m[s] <= 64 ? 0 : 1) == rc && P.w[s] > Wlo && P.w[s] <= W) part.push_back(s);
    std::stable_sort(part.begin(), part.end(), [&](int a, int b) {
      const double wa = (double)P.m[a] * P.m[a] * P.w[a], wb = (double)P.m[b] * P.m[b] * P.w[b];
      return wa > wb;
    });
    add_class(part, W);
  }
  for (int q = 0; q < 4; q++) add_class(bucket[q], 0);
  return big;
}

// An exchange point: every panel / tail in `items` (front, kn, nb | kind << 16,
// owner) goes from its owner to every rank (one broadcast per sending rank).
int LevelCtx::add_exchange(const std::vector<int4>& items) {
  if (items.empty()) return -1;
  XExchange x;
  x.off = (int)S.xp_tasks.size();
  x.cnt = (int)items.size();
  x.size.assign(std::max(P.part_size, 1), 0);
  for (const int4& t : items) {
    const int s = t.x, kn = t.y, nb = t.z & 0xffff, kind = t.z >> 16, m = P.m[s];
    // kind 0: the L below the diagonal tile (the tile's own L is never stored),
    // the inverse, the frontal vector; kind 1: the tail columns whole
    const long long sz = kind == 0 ? (long long)(m - kn - nb) * nb + 4096 + (m - kn) : (long long)(m - kn) * nb;
    S.xp_tasks.push_back(t);
    S.xp_loff.push_back(x.size[t.w]);
    x.size[t.w] += sz;
  }
  for (int q = x.off; q < x.off + x.cnt; q++) S.xp_lstride.push_back(x.size[S.xp_tasks[q].w]);
  for (long long v : x.size) S.xp_rslot = std::max(S.xp_rslot, v);
  S.xchg.push_back(x);
  return (int)S.xchg.size() - 1;
}

// first panel of every front: k_panel_first (diagonal + trsm waiters)
void LevelCtx::first_panel(const std::vector<int>& big, StepWork& W) {
  for (int s : big) {
    if (P.w[s] <= 0) continue;
    const int nb = std::min(kNB, P.w[s]), m = P.m[s];
    if (dist) W.xfirst.push_back(make_int4(s, 0, nb, cowner(s, 0)));
    if (!mine(s, 0)) continue;
    S.potrf_list.push_back(s);
    W.ps.first_flops += 2.0 * nb * nb * (double)nb / 3.0 + (double)std::max(0, m - nb) * nb * nb;
    for (int r0 = kNB; r0 < m; r0 += kNB) S.col_tasks.push_back(make_int4(s, r0, 0, -1));
  }
}

// The columns [cstart, cend) of front s that the plain tiles of its panel g
// update.  With the plain tiles in their own launch (apart) the column block the
// next step prepares, [kn + 64, kn + 128), is skipped: the next step's
// diagonal / column tasks apply this panel's update with their own (depth 2
// panels, or the deferred block + 1 panel), so the next step does not wait for
// this step's plain tiles (joined one step later).  The skip is a property of
// the front alone (its size), never of the level it sits in: the update
// grouping -- hence the rounding -- of a front is the same in every plan (the
// partitioned plans' fronts are bit for bit the one-rank plan's).
void LevelCtx::plain_range(int s, const PanelGeom& g, int& cstart, int& cend) const {
  const int w = P.w[s];
  cend = g.colend;
  cstart = g.kn < w ? g.kn + kNB : g.kn;
  // the next step prepares [kn2, kn2 + 64): only when it covers all of it
  if (front_skip(s) && g.kn2 < w && g.c2 == g.kn2 + kNB && cstart + kNB <= cend) {
    cstart += kNB;
    if (has_prep(s, g.kn2)) cstart += kNB;   // the next step's prep block
  }
}

long long LevelCtx::ntiles(const std::vector<int>& big, int kb, int T) const {
  long long cnt = 0;
  for (int s : big) {
    if (P.w[s] <= kb) continue;
    int c0, c1;
    plain_range(s, PanelGeom(P.w[s], P.m[s], kb), c0, c1);
    for (int cc = c0; cc < c1; cc += T) cnt += (P.m[s] - cc + T - 1) / T;
  }
  return cnt;
}

// Panel kb of big front i = s: the next panel's diagonal and column tasks, the
// prep tiles, the plain ranges (near and far), with the look-ahead bookkeeping.
void LevelCtx::front_step(size_t i, int s, int kb, LookAhead& la, StepWork& W) {
  PanelStep& ps = W.ps;
  const int w = P.w[s], m = P.m[s];
  const PanelGeom g(w, m, kb);
  const int kn = g.kn;
  if (kn < w) {   // next panel: its diagonal tile and the tiles below it
    const int nb2 = std::min(kNB, w - kn), c1 = std::min(kn + kNB, g.colend);
    const int k0 = la.applied[i][kn];
    la.advance(i, kn, c1, k0, kn, false,
               [&] { sched_fail(S, K, "sched: sdiag front %d w %d m %d kb %d cols [%d,%d) k0 %d\n", s, w, m, kb, kn, c1, k0); });
    la.touched(i, c1);
    const int depth = kn - k0, kw = g.inner ? (k0 | (int)0x80000000) : k0;
    if (dist) W.xstep.push_back(make_int4(s, kn, nb2, cowner(s, kn)));
    const bool own = mine(s, kn);
    if (own) S.sdiag_tasks.push_back(make_int4(s, kn, kn, kw));
    const double fd = (double)depth * kNB * (kNB + 1) + 2.0 * nb2 * nb2 * (double)nb2 / 3.0 +
                      (double)std::min(kNB - nb2, m - kn - nb2) * nb2 * nb2;
    ps.step_flops += fd;
    ps.diag_flops += fd;
    for (int r0 = kn + kNB; r0 < m; r0 += kNB) {
      if (own) S.col_tasks.push_back(make_int4(s, r0, kn, kw));
      const int rows = std::min(kNB, m - r0);
      ps.step_flops += 2.0 * depth * rows * (c1 - kn) + (double)rows * nb2 * nb2;
      ps.colupd_flops += 2.0 * depth * rows * (c1 - kn);
      ps.trsm_flops += (double)rows * nb2 * nb2;
    }
    ps.syrk_flops += (double)depth * (c1 - kn) * (2.0 * m - kn - c1 + 1.0);
  }
  if (has_prep(s, kn)) {
    const int b0 = g.kn2, b1 = b0 + kNB, k0 = la.applied[i][b0];
    la.advance(i, b0, b1, k0, kn, k0 > kb,
               [&] { sched_fail(S, K, "sched: prep front %d w %d m %d kb %d cols [%d,%d) k0 %d\n", s, w, m, kb, b0, b1, k0); });
    la.touched(i, b1);
    if (mine(s, b0))
      for (int r0 = b0; r0 < m; r0 += kNB) W.prep.push_back(make_int4(s, r0, b0, k0));
    const double f = (double)(kn - k0) * kNB * (2.0 * m - b0 - b1 + 1.0);
    ps.step_flops += f;
    ps.colupd_flops += f;
    ps.syrk_flops += f;
  }
  int cstart, cend;
  plain_range(s, g, cstart, cend);
  // far split at a block end: columns past the next kKB block (the next
  // steps touch none of them until that block ends)
  // (PGO_FAR=1: measured within the replay noise on C3 -- 8.70 / 17.50 ms
  // at 1 / 3 lanes with and without, profiles/r04c_ab_far.txt -- while
  // the concurrent far tiles slow the k_step launches they overlap; off)
  const int nend = (!g.inner && cstart < cend && K.far_on) ? std::max(cstart, std::min(cend, std::min(g.be + kKB, w))) : cend;
  // the next step prepares [kn2, c2) of this front: this step's plain tiles feed it -> lag 1
  if (g.kn2 < w && cstart < nend && cstart < g.c2 && g.kn2 < nend) W.conflict = true;
  if (cstart >= cend) return;
  int k0 = la.applied[i][cstart];
  la.advance(i, cstart, cend, k0, kn, false, [&] {
    std::string at;
    for (int j = cstart; j < cend; j += 16) at += " " + std::to_string(la.applied[i][j]);
    sched_fail(S, K, "sched: plain front %d w %d m %d kb %d cols [%d,%d) k0 %d:%s\n", s, w, m, kb, cstart, cend, k0, at.c_str());
    k0 = kb;
  });
  const int depth = kn - k0, kw = g.inner ? (k0 | (int)0x80000000) : k0;
  for (int cc = cstart; cc < cend; cc++) ps.plain_flops += 2.0 * depth * (m - cc);
  if (cstart < nend) W.plain.push_back(make_int4(s, cstart, nend, kw));
  la.touched(i, nend);
  for (int c0 = nend, p = 0; c0 < cend; p++) {   // far pieces: a kKB block each, [w, m) one
    const int c1 = c0 < w ? std::min(std::min(cend, w), (c0 / kKB + 1) * kKB) : cend;
    if ((int)W.plain_far.size() <= p) {
      W.plain_far.emplace_back();
      W.far_pflops.push_back(0.0);
      la.far0.back().emplace_back(la.applied.size(), 0);
      for (size_t i2 = 0; i2 < la.applied.size(); i2++) la.far0.back()[p][i2] = (int)la.applied[i2].size();
    }
    W.plain_far[p].push_back(make_int4(s, c0, c1, kw));
    la.far0.back()[p][i] = c0;
    for (int cc = c0; cc < c1; cc++) W.far_pflops[p] += 2.0 * depth * (m - cc);
    c0 = c1;
  }
}

// Schur-update tile tasks of column ranges (front, first column, end column,
// k0), T x T.  A tile's columns stay inside one 64-column block of the packed
// front (pgo_chol.h front_packed): a range starting inside a block (the update
// matrix starts at w) opens with a narrow tile up to the block's end, clipped;
// a tile's elements are computed alike whatever its shape.
// (distributed top: 64-wide tiles, split where the column owner changes)
void gen_tiles(const LevelCtx& C, const std::vector<int4>& ranges, int T, std::vector<int4>& out) {
  for (const int4& u : ranges)
    for (int c0 = u.y; c0 < u.z;) {
      const int m = C.P.m[u.x];
      const int ce = (c0 & 63) ? std::min(u.z, (c0 + 63) & ~63) : std::min(u.z, c0 + T);
      // a tile narrower than T carries its width (the kernels clip its columns
      // there): a block's end inside the range, or the range's end -- which
      // is not the kernels' own column end where a step's range is split
      // into near and far parts
      const bool narrow = ce - c0 < T;
      if (!C.dist) {
        const int clip = narrow ? ce - c0 : 0;
        for (int r0 = c0; r0 < m; r0 += T) out.push_back(make_int4(u.x, r0 | (clip << kClipShift), c0, u.w));
      } else {
        for (int a = c0; a < ce;) {   // runs of one column owner: (a, b)
          int b = a + 1;
          while (b < ce && C.cowner(u.x, b) == C.cowner(u.x, a)) b++;
          if (C.mine(u.x, a)) {
            const int clip = (a == c0 && b == ce && !narrow) ? 0 : b - a;
            for (int r0 = c0; r0 < m; r0 += kTile) out.push_back(make_int4(u.x, r0 | (clip << kClipShift), a, u.w));
          }
          a = b;
        }
      }
      c0 = ce;
    }
}

// The step's tile size, its Schur-update tiles (near, then the far pieces, each
// in XCD order), inline or apart, the lag of an apart launch; the step is done.
void LevelCtx::emit_tiles(const std::vector<int>& big, bool apart, LookAhead& la, StepWork& W) {
  PanelStep& ps = W.ps;
  ps.syrk_flops += ps.plain_flops;
  ps.sdiag_cnt = (int)S.sdiag_tasks.size() - ps.sdiag_off;
  ps.col_cnt = (int)S.col_tasks.size() - ps.col_off - ps.fcol_cnt;
  S.col_tasks.insert(S.col_tasks.end(), W.prep.begin(), W.prep.end());
  ps.prep_cnt = (int)W.prep.size();
  // plain tiles: 128x128 (LDS-pipelined kernel) when there are many rounds of
  // them (measured: at <= ~500 tiles the 64x64 kernel's finer granularity
  // wins, scripts/ubench_syrk.hip), else 64x64; few 64-tiles ride in k_step,
  // many go to a concurrent launch (k_step's LDS request, sized for the
  // diagonal workgroups, halves their occupancy)
  long long cnt128 = 0;
  auto count128 = [&](const std::vector<int4>& ranges) {
    for (const int4& u : ranges)
      for (int c0 = u.y; c0 < u.z; c0 += kBigTile) cnt128 += (P.m[u.x] - c0 + kBigTile - 1) / kBigTile;
  };
  count128(W.plain);
  for (const auto& pl : W.plain_far) count128(pl);
  // (distributed top: a tile's elements are computed alike in either kernel,
  // so the split 64-wide tiles are bitwise the 128-tile update)
  ps.syrk_tile = cnt128 >= K.big_min && !dist ? kBigTile : kTile;
  gen_tiles(*this, W.plain, ps.syrk_tile, S.syrk_tasks);
  const int near_end = (int)S.syrk_tasks.size();
  std::vector<int> piece_end;
  for (const auto& pl : W.plain_far) {
    gen_tiles(*this, pl, ps.syrk_tile, S.syrk_tasks);
    piece_end.push_back((int)S.syrk_tasks.size());
  }
  ps.syrk_cnt = (int)S.syrk_tasks.size() - ps.syrk_off;
  ps.syrk_inline = !apart && ps.syrk_tile == kTile && ps.syrk_cnt <= kInlineTiles;
  ps.far_cnt = ps.syrk_inline ? 0 : (int)S.syrk_tasks.size() - near_end;
  if (ps.far_cnt == 0) {   // (inline, or nothing far: the far ranges' columns are this step's)
    for (const auto& pl : W.plain_far)
      for (const int4& u : pl)
        for (size_t i = 0; i < big.size(); i++)
          if (big[i] == u.x) la.touched(i, u.z);
    la.far0.back().clear();
    xcd_order_range(S.syrk_tasks, ps.syrk_off, ps.syrk_off + ps.syrk_cnt, ps.syrk_tile);
  } else {
    xcd_order_range(S.syrk_tasks, ps.syrk_off, near_end, ps.syrk_tile);
    ps.far_p0 = (int)lv.far_pieces.size();
    int b = near_end;
    for (size_t p = 0; p < W.plain_far.size(); p++) {   // (piece: first tile relative to syrk_off, count)
      xcd_order_range(S.syrk_tasks, b, piece_end[p], ps.syrk_tile);
      lv.far_pieces.push_back(make_int4((int)lv.panels.size(), b - ps.syrk_off, piece_end[p] - b, -1));
      lv.far_piece_flops.push_back(W.far_pflops[p]);   // (a piece may hold no tile of this rank)
      ps.far_flops += W.far_pflops[p];
      b = piece_end[p];
    }
    ps.far_np = (int)lv.far_pieces.size() - ps.far_p0;
  }
  // an apart launch no front's next step reads is joined before the step after next
  ps.plain_lag = ps.syrk_cnt > 0 && !ps.syrk_inline ? (W.conflict ? 1 : 2) : 0;
  // (an inline plain after a lag-2 apart one could touch its tiles at once)
  la.apart_chain = la.apart_chain || (ps.plain_lag == 2);
  if (ps.syrk_inline) ps.step_flops += ps.plain_flops;
  ps.xstep = add_exchange(W.xstep);
  lv.panels.push_back(ps);
}

// Blocked path, one step per 64-column panel kb of every big front of the
// level (right-looking, look-ahead 1, Schur updates of depth 64):
//   first step  k_panel_first: the front's first diagonal tile factored +
//               inverted, the rows below it solved (trsm) by workgroups that
//               wait for that inverse (in-launch hand-off)
//   each step   k_step: the next panel's diagonal tile updated with panel kb,
//               factored and inverted (sdiag); the tiles below it in the
//               next panel's column block updated, then solved against that
//               inverse (col); the other trailing tiles updated (syrk:
//               inline, or a concurrent k_panel_syrk_lds / 128 launch)
// A violation of the look-ahead bookkeeping marks the plan invalid (schedule_error).
void LevelCtx::panel_steps(const std::vector<int>& big) {
  int maxw = 0;
  for (int s : big) maxw = std::max(maxw, P.w[s]);
  LookAhead la(P, big);
  for (int kb = 0; kb < maxw; kb += kNB) {
    la.begin_step();
    StepWork W;
    PanelStep& ps = W.ps;
    ps.kb = kb;
    ps.syrk_flops = ps.plain_flops = ps.step_flops = ps.first_flops = 0;
    ps.col_off = (int)S.col_tasks.size(), ps.syrk_off = (int)S.syrk_tasks.size();
    ps.potrf_off = (int)S.potrf_list.size(), ps.sdiag_off = (int)S.sdiag_tasks.size();
    if (kb == 0) first_panel(big, W);
    ps.potrf_cnt = (int)S.potrf_list.size() - ps.potrf_off;
    ps.fcol_cnt = (int)S.col_tasks.size() - ps.col_off;
    ps.xfirst = add_exchange(W.xfirst);
    const int tile0 = ntiles(big, kb, kBigTile) >= K.big_min ? kBigTile : kTile;
    const bool apart = la.apart_chain || !(tile0 == kTile && ntiles(big, kb, kTile) <= kInlineTiles);
    for (size_t i = 0; i < big.size(); i++)
      if (P.w[big[i]] > kb) front_step(i, big[i], kb, la, W);
    emit_tiles(big, apart, la, W);
  }
  la.join_far(lv);
  tail_exchange(big);
  check_complete(big, la);
}

// distributed top: update columns past a front's last whole panel, factored with it, go to every rank
void LevelCtx::tail_exchange(const std::vector<int>& big) {
  if (!dist) return;
  std::vector<int4> tails;
  for (int s : big) {
    const int w = P.w[s], wr = std::min(P.m[s], (w + kNB - 1) / kNB * kNB);
    if (wr > w) tails.push_back(make_int4(s, w, (wr - w) | (1 << 16), cowner(s, w)));
  }
  lv.xtail = add_exchange(tails);
}

// every column has its updates: pivot columns up to their panel, the trailing ones from every panel
void LevelCtx::check_complete(const std::vector<int>& big, const LookAhead& la) {
  for (size_t i = 0; i < big.size(); i++) {
    const int s = big[i], w = P.w[s];
    for (int j = 0; j < P.m[s]; j++)
      if (la.applied[i][j] != (j < w ? (j / kNB) * kNB : w))
        sched_fail(S, K, "sched: end front %d w %d m %d col %d applied %d\n", s, w, P.m[s], j, la.applied[i][j]);
  }
}

// Fused update-matrix tiles (pgo_chol.h syrk_gather), once both parts of a
// level are there.  A tile (ti, tj) of a blocked front with 64 tj >= w rounded
// up to 64 holds no H entry (chol_assembly checks it).  Its columns' first
// Schur update is the task that finds applied == 0 and is not inner: k0 word
// 0.  Where that is a 64-tile task of a front that is not distributed, the
// task takes the tile's child rectangles and the tile leaves the assembly
// list; its pairs stay in ea_pairs.  Such a task (r0, c0) is assembly tile
// (r0 / 64, c0 / 64) exactly: gen_tiles aligns a range's tiles to the
// 64-column blocks after a narrow opening tile (the block straddling w: not
// fused), rows run from the column down in steps of 64, and the range ends
// at m.  Asserted here (schedule_error).  A later update of the same columns
// (a wide front's next kKB block end: k0 > 0) stays a plain read-modify-write,
// and so does every tile of a 128-tile step.  Then the XCD order of what is
// left, as before (PGO_FUSE_UPDATE=0: all of it).
void fuse_level(const CholPlan& P, const ScheduleKnobs& K, CholLevel& lv, LevelLists& S, bool dist) {
  const size_t e0 = (size_t)lv.ea_off.back();
  S.syrk_gather.assign(S.syrk_tasks.size(), make_int2(-1, 0));
  if (K.fuse && !dist && !S.syrk_tasks.empty()) {
    // a front's tile tasks: contiguous from its tile (0, 0), tile (ti, tj) at ti (ti + 1) / 2 + tj
    std::vector<std::pair<int, int>> fstart;
    for (size_t q = e0; q < S.ea_tasks.size(); q++)
      if (S.ea_tasks[q].y == 0) fstart.emplace_back(S.ea_tasks[q].x, (int)q);
    std::sort(fstart.begin(), fstart.end());
    std::vector<char> gone(S.ea_tasks.size(), 0);
    for (PanelStep& ps : lv.panels) {
      if (ps.syrk_tile != kTile) continue;
      for (int q = ps.syrk_off; q < ps.syrk_off + ps.syrk_cnt; q++) {
        const int4 t = S.syrk_tasks[q];
        const int s = t.x, r0 = t.y & kRowMask, clip = t.y >> kClipShift, c0 = t.z, m = P.m[s];
        if (t.w != 0 || c0 < ((P.w[s] + 63) & ~63)) continue;
        const auto it = std::lower_bound(fstart.begin(), fstart.end(), std::make_pair(s, 0));
        const int ti = r0 >> 6, tj = c0 >> 6;
        const size_t e = it == fstart.end() ? S.ea_tasks.size() : (size_t)it->second + (size_t)ti * (ti + 1) / 2 + tj;
        const bool whole = !(r0 & 63) && !(c0 & 63) && std::min(m, c0 + (clip ? clip : kTile)) == std::min(m, c0 + 64);
        if (!whole || e >= S.ea_tasks.size() || S.ea_tasks[e].x != s || S.ea_tasks[e].y != ((ti << 16) | tj) || gone[e]) {
          sched_fail(S, K, "sched: fused tile front %d w %d m %d task (%d, %d) clip %d\n", s, P.w[s], m, r0, c0, clip);
          continue;
        }
        gone[e] = 1;
        for (int k = 0; k < S.ea_tasks[e].w; k++) {
          const int4 pr = S.ea_pairs[S.ea_tasks[e].z + k];
          const long long nr = pr.w & 0xff, ncl = pr.w >> 8, d = pr.y - pr.z + 1;
          ps.gather_bytes += 8.0 * (double)(ramp_sum(d + nr - 1, ncl) - ramp_sum(d - 1, ncl));
        }
        S.syrk_gather[q] = make_int2(S.ea_tasks[e].z, S.ea_tasks[e].w);
        S.fused++;
        S.fused_with_pairs += S.ea_tasks[e].w > 0;
        S.fused_multipass += S.ea_tasks[e].w > 16;   // (kAsmPairs rectangles per gather pass)
        S.fused_edge += r0 + 64 > m || c0 + 64 > m;
      }
    }
    size_t o = e0;
    for (size_t q = e0; q < S.ea_tasks.size(); q++)
      if (!gone[q]) S.ea_tasks[o++] = S.ea_tasks[q];
    S.ea_tasks.resize(o);
  }
  ea_xcd_order(S.ea_tasks, e0, K.asm_xcd);
  lv.ea_cnt.push_back((int)S.ea_tasks.size() - lv.ea_off.back());
}

// Merge: level-relative offsets and indices made absolute; the level lists
// copied into place level by level on the pool (offsets from a serial pass).
void merge_levels(CholPlan& P, std::vector<LevelLists>& out, int nl) {
  std::vector<ListBase> base(nl + 1);
  for (int L = 0; L < nl; L++) {
    base[L + 1] = base[L];
#define X(n) base[L + 1].n += out[L].n.size();
    PGO_LEVEL_LISTS(X)
#undef X
    base[L + 1].npart += out[L].npart;
  }
#define X(n) resize_room(P.n, base[nl].n);
  PGO_LEVEL_LISTS(X)
#undef X
  P.npart = base[nl].npart;
  plan_parallel(nl, [&](int L) {
    LevelLists& S = out[L];
    CholLevel& lv = P.levels[L];
    const ListBase& b = base[L];
    const int bx = (int)b.xchg, npart0 = b.npart;
    lv.front_off += (int)b.level_fronts;
    lv.bwd_part.off += (int)b.bwd_part_tasks;
    for (int4& t : S.bwd_part_tasks) t.w += npart0;
    for (int q = lv.bwd[0].off; q < lv.bwd[0].off + lv.bwd[0].cnt; q++) S.bwd_pref[q].x += npart0;   // init tasks
    for (SolveStep& st : lv.bwd) st.off += (int)b.bwd_tasks;
    lv.bwdc.off += (int)b.bwdc_tasks;
    for (int& o : lv.ea_off) o += (int)b.ea_tasks;
    for (int4& t : S.ea_tasks) t.z += (int)b.ea_pairs;
    for (int2& g : S.syrk_gather)
      if (g.x >= 0) g.x += (int)b.ea_pairs;
    for (SmallClass& sc : lv.small) sc.off += (int)b.small_list;
    for (PanelStep& ps : lv.panels) {
      ps.potrf_off += (int)b.potrf_list;
      ps.col_off += (int)b.col_tasks;
      ps.syrk_off += (int)b.syrk_tasks;
      ps.sdiag_off += (int)b.sdiag_tasks;
      if (ps.xfirst >= 0) ps.xfirst += bx;
      if (ps.xstep >= 0) ps.xstep += bx;
    }
    if (lv.xtail >= 0) lv.xtail += bx;
    for (XExchange& x : S.xchg) x.off += (int)b.xp_tasks;
#define X(n) std::copy(S.n.begin(), S.n.end(), P.n.begin() + b.n);
    PGO_LEVEL_LISTS(X)
#undef X
  });
  P.syrk_flops = 0, P.fused_tiles = P.fused_with_pairs = P.fused_multipass = P.fused_edge = P.xp_rslot = 0;
  for (int L = 0; L < nl; L++) {
    P.fused_tiles += out[L].fused, P.fused_with_pairs += out[L].fused_with_pairs;
    P.fused_multipass += out[L].fused_multipass, P.fused_edge += out[L].fused_edge;
    for (const PanelStep& ps : P.levels[L].panels) P.syrk_flops += ps.plain_flops;
    P.xp_rslot = std::max(P.xp_rslot, out[L].xp_rslot);
    P.schedule_error = P.schedule_error || out[L].schedule_error;
  }
}

// The selected-inversion pass's launch lists (pgo_chol.h SelPlan) from the
// level lists: rebuilt with every schedule, so a re-plan and an incremental
// append carry them too.  A partitioned plan has none (the pass walks every
// front: pgo_marginal_covariances_all plans for one rank).
void selinv_schedule(CholPlan& P) {
  SelPlan& Q = P.sel;
  Q.levels.clear(), Q.gather.clear(), Q.tiles.clear(), Q.diag.clear();
  Q.goff.assign(P.ns, 0);
  Q.gmax = Q.pmax = Q.launches = 0;
  static std::atomic<unsigned> serial{0};   // (unique over plans: a handle's edge table is keyed by it)
  Q.serial = ++serial;
  if (P.part_size > 1) return;
  Q.levels.resize(P.levels.size());
  Q.launches = 1;   // the read-out
  std::vector<int> big;   // the level's blocked fronts, in level order
  for (size_t L = 0; L < P.levels.size(); L++) {
    const CholLevel& lv = P.levels[L];
    SelLevel& sl = Q.levels[L];
    const int* fr = P.level_fronts.data() + lv.front_off;
    // (every front that is not packed is in one of the level's wavefront
    // classes, and those sit back to back in small_list)
    sl.small_off = lv.small.empty() ? 0 : lv.small.front().off;
    for (const SmallClass& sc : lv.small) sl.small_cnt += sc.cnt;
    sl.gat_off = (int)Q.gather.size();
    long long g = 0;
    int maxblk = 0;
    big.clear();
    for (int q = 0; q < lv.front_cnt; q++) {
      const int s = fr[q], m = P.m[s], w = P.w[s];
      if (!front_packed(m, w)) continue;
      big.push_back(s);
      Q.goff[s] = g;
      g += 64LL * fpad(m);
      maxblk = std::max(maxblk, (w + 63) / 64);
      if (m > w)
        for (int cb = w / 64; 64 * cb < m; cb++) Q.gather.push_back(make_int2(s, cb));
    }
    Q.gmax = std::max(Q.gmax, g);
    sl.gat_cnt = (int)Q.gather.size() - sl.gat_off;
    Q.launches += (sl.small_cnt > 0) + (sl.gat_cnt > 0);
    for (int b = maxblk - 1; b >= 0; b--) {
      SelStep st{b, (int)Q.tiles.size(), 0, (int)Q.diag.size(), 0};
      int slot = 0;
      for (int s : big) {
        const int m = P.m[s], w = P.w[s], c0 = 64 * b;
        if (c0 >= w) continue;
        const int rs = c0 + std::min(64, w - c0), p0 = slot;
        for (int r0 = rs; r0 < m; r0 += 64) Q.tiles.push_back(make_int4(s, r0, c0, slot++));
        Q.diag.push_back(make_int4(s, c0, p0, slot - p0));
      }
      st.tile_cnt = (int)Q.tiles.size() - st.tile_off;
      st.diag_cnt = (int)Q.diag.size() - st.diag_off;
      Q.pmax = std::max<long long>(Q.pmax, slot);
      Q.launches += 2 * (st.tile_cnt > 0) + 1;
      sl.steps.push_back(st);
    }
  }
}

}  // namespace

// The plan's schedules from its fronts (chol_analyze's second half; the
// incremental append re-runs it on the updated fronts), in passes:
//   partition_layout  owners, a partitioned plan's storage, the root exchange's layout
//   level_buckets     the fronts by phase and height, empty levels dropped, the split
//   LevelCtx          one level's lists, two tasks per level on the planner's pool
//   fuse_level        the fused update-matrix tiles, the assembly tiles' XCD order
//   merge_levels      the level lists appended to the plan's, offsets made absolute
// then the selected-inversion lists and the H assembly lists.
void chol_schedule(CholPlan& P, const std::vector<int>& row_ptr, const std::vector<int>& slot_col) {
  const ScheduleKnobs K;
  PhaseTimer phase("chol_schedule");
  phase.on = K.timing;
  P.schedule_error = false;
  partition_layout(P);
  phase("partition");
  const std::vector<std::vector<int>> bylevel = level_buckets(P);
  const int nl = (int)bylevel.size();
  const bool dtop = P.part_size > 1 && K.dist_top;
  P.cown_off.assign(P.ns, -1), P.cown.clear();
  if (dtop) column_owners(P, P.owner, P.part_size, P.cown_off, P.cown);
  P.levels.assign(nl, CholLevel());
  // the level lists keep their storage from one schedule to the next in the
  // plan (a live plan refresh rebuilds them all: fresh allocations cost it the
  // page faults of ~tens of MB); chol_free releases them with the plan
  if (!P.sched_scratch.p) P.sched_scratch.p = std::make_shared<std::vector<LevelLists>>();
  std::vector<LevelLists>& out = *static_cast<std::vector<LevelLists>*>(P.sched_scratch.p.get());
  if ((int)out.size() < nl) out.resize(nl);
  for (int L = 0; L < nl; L++) out[L].reset();
  std::vector<double> lms(2 * nl, 0.0);
  plan_parallel(2 * nl, [&](int t) {   // two tasks per level
    const auto t0 = std::chrono::steady_clock::now();
    const int L = t >> 1;
    LevelCtx C{P, K, bylevel[L], P.levels[L], out[L], dtop && L >= P.split};
    if ((t & 1) == 0) C.front_list(), C.bwd_init(), C.bwd_chain(), C.bwd_steps(), C.extend_add();
    else C.panel_steps(C.small_classes());
    lms[t] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
  if (K.timing)
    for (int L = 0; L < nl; L++)
      fprintf(stderr, "  level %d: %.2f + %.2f ms (%zu fronts)\n", L, lms[2 * L], lms[2 * L + 1], bylevel[L].size());
  phase("levels");
  plan_parallel(nl, [&](int L) { fuse_level(P, K, P.levels[L], out[L], dtop && L >= P.split); });
  phase("fuse");
  merge_levels(P, out, nl);
  phase("schedule");
  selinv_schedule(P);
  phase("selinv");
  chol_assembly(P, row_ptr, slot_col);
  phase("assembly");
}

}  // namespace pgo
