// Host self-test of the solver's planning code (test infrastructure, not part
// of libpgo.so): drives the symbolic analysis on synthetic pose graphs so a host
// AddressSanitizer / UndefinedBehaviorSanitizer build (`make -C
// graphslam_amd/csrc asan-host`) exercises its memory accesses --
// nested-dissection and AMD orderings, supernodes, level schedule, panel steps,
// the assembly lists, the subtree partition for 2 and 4 ranks, the incremental
// paths (chol_covers / chol_assembly, a caller-given ordering) -- and the graph
// structure module (pgo_structure.cpp): the plan's sources bound through its
// bind, in-place appends against rebuilds, the owner-bit transitions.  No GPU calls.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <random>
#include <string>
#include <vector>

#include "pgo_chol.h"
#include "pgo_lm.h"
#include "pgo_plan_digest.h"
#include "pgo_structure.h"

namespace {

struct Pattern {
  int n = 0;
  std::vector<int> row_ptr, col;
};

// block pattern of H for a chain of n poses with `lc` random loop closures;
// `dups` of the loop closures (every lc / dups-th) repeated as a parallel
// factor: the same block listed twice in both rows, as the library's block-CSR
// lists parallel factors (one slot each, in device order)
Pattern make_pattern(int n, int lc, unsigned seed, const std::vector<std::pair<int, int>>& extra = {}, int dups = 0) {
  std::mt19937 rng(seed);
  std::vector<std::pair<int, int>> e;
  for (int i = 0; i + 1 < n; i++) e.emplace_back(i, i + 1);
  for (int q = 0; q < lc; q++) {
    const int a = 20 + (int)(rng() % (unsigned)(n - 20));
    e.emplace_back(a, (int)(rng() % (unsigned)(a - 10)));
  }
  e.insert(e.end(), extra.begin(), extra.end());
  Pattern P;
  P.n = n;
  std::vector<std::vector<int>> adj(n);
  for (auto& [a, b] : e) {
    adj[a].push_back(b);
    adj[b].push_back(a);
  }
  for (int i = 0; i < n; i++) {
    adj[i].push_back(i);
    std::sort(adj[i].begin(), adj[i].end());
    adj[i].erase(std::unique(adj[i].begin(), adj[i].end()), adj[i].end());
  }
  for (int q = 0; dups > 0 && q < lc; q += std::max(1, lc / dups)) {
    const auto [a, b] = e[n - 1 + q];
    if (a == b) continue;
    adj[a].push_back(b);
    adj[b].push_back(a);
  }
  P.row_ptr.assign(1, 0);
  for (int i = 0; i < n; i++) {
    std::sort(adj[i].begin(), adj[i].end());
    P.col.insert(P.col.end(), adj[i].begin(), adj[i].end());
    P.row_ptr.push_back((int)P.col.size());
  }
  return P;
}

// block pattern of H for n poses tied pairwise by `e`
Pattern pattern_of(int n, const std::vector<std::pair<int, int>>& e) {
  std::vector<std::vector<int>> adj(n);
  for (const auto& [a, b] : e) adj[a].push_back(b), adj[b].push_back(a);
  Pattern G;
  G.n = n;
  G.row_ptr.assign(1, 0);
  for (int i = 0; i < n; i++) {
    adj[i].push_back(i);
    std::sort(adj[i].begin(), adj[i].end());
    adj[i].erase(std::unique(adj[i].begin(), adj[i].end()), adj[i].end());
    G.col.insert(G.col.end(), adj[i].begin(), adj[i].end());
    G.row_ptr.push_back((int)G.col.size());
  }
  return G;
}

// a side x side grid of poses, each tied to its right and lower neighbour
Pattern make_grid(int side) {
  std::vector<std::pair<int, int>> e;
  for (int y = 0; y < side; y++)
    for (int x = 0; x < side; x++) {
      if (x + 1 < side) e.emplace_back(y * side + x, y * side + x + 1);
      if (y + 1 < side) e.emplace_back(y * side + x, (y + 1) * side + x);
    }
  return pattern_of(side * side, e);
}

// `leaves` cliques of 3 poses, each tied to every pose of a middle clique of 25
// and of a top clique of 30; a second middle clique of 25 tied to the top alone
// (it keeps the first from merging into the top); numbered in that order.
// Eliminated as numbered, the first middle front gets a rectangle from every
// leaf it has not absorbed in the tiles of its update matrix.
Pattern make_fan(int leaves) {
  const int m0 = 3 * leaves, m1 = m0 + 25, t0 = m1 + 25, n = t0 + 30;
  auto middle = [&](int a) { return a >= m0 && a < m1; };
  std::vector<std::pair<int, int>> e;
  for (int a = m0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (!middle(a) || b < m1 || b >= t0) e.emplace_back(a, b);
  for (int l = 0; l < leaves; l++)
    for (int a = 3 * l; a < 3 * l + 3; a++)
      for (int b = a + 1; b < n; b++)
        if (b < 3 * l + 3 || middle(b) || b >= t0) e.emplace_back(a, b);
  return pattern_of(n, e);
}

// the pattern restricted to poses [0, n)
Pattern restrict_pattern(const Pattern& G, int n) {
  Pattern R;
  R.n = n;
  R.row_ptr.assign(1, 0);
  for (int i = 0; i < n; i++) {
    for (int k = G.row_ptr[i]; k < G.row_ptr[i + 1]; k++)
      if (G.col[k] < n) R.col.push_back(G.col[k]);
    R.row_ptr.push_back((int)R.col.size());
  }
  return R;
}

int fail(const char* m) {
  std::fprintf(stderr, "host_selftest: %s\n", m);
  return 1;
}

// Task coverage of one top level / panel step: (kind, front, row tile, column,
// depth) -> how often.  Plain tiles count per (64-row tile, column) they
// update (128-tiles split), clipped as the kernels clip them.
using Key = std::tuple<int, int, int, int, int>;
void step_keys(const pgo::CholPlan& P, const pgo::PanelStep& ps, std::map<Key, int>& out) {
  for (int q = ps.syrk_off; q < ps.syrk_off + ps.syrk_cnt; q++) {
    const int4 t = P.syrk_tasks[q];
    const int s = t.x, row0 = t.y & pgo::kRowMask, clip = t.y >> pgo::kClipShift, c0 = t.z, m = P.m[s], w = P.w[s];
    const int T = ps.syrk_tile;
    int colend = t.w < 0 ? std::min((ps.kb & ~(pgo::kKB - 1)) + pgo::kKB, w) : m;
    const int cend = std::min({colend, c0 + (clip ? clip : T), m});
    for (int r0 = row0; r0 < std::min(row0 + T, m); r0 += 64)
      for (int col = c0; col < cend; col++)
        if (col <= r0 + 63) out[Key(0, s, r0, col, t.w)]++;
  }
  for (int q = ps.sdiag_off; q < ps.sdiag_off + ps.sdiag_cnt; q++) {
    const int4 t = P.sdiag_tasks[q];
    out[Key(1, t.x, t.y, t.z, t.w)]++;
  }
  for (int q = ps.col_off; q < ps.col_off + ps.fcol_cnt + ps.col_cnt + ps.prep_cnt; q++) {
    const int4 t = P.col_tasks[q];
    out[Key(2, t.x, t.y, t.z, t.w)]++;
  }
  for (int q = ps.potrf_off; q < ps.potrf_off + ps.potrf_cnt; q++) out[Key(3, P.potrf_list[q], 0, 0, 0)]++;
}

// The distributed top (part_size > 1): every rank's top tasks together are the
// replicated plan's (PGO_DIST_TOP=0), each task on its column's rank (every
// rank for the replicated columns); every factored panel is exchanged.
int check_distributed(const Pattern& G, int ordering, int size) {
  std::vector<pgo::CholPlan> D(size), R(size);
  for (int r = 0; r < size; r++) {
    for (int dist : {1, 0}) {
      pgo::CholPlan& Q = dist ? D[r] : R[r];
      if (!dist) setenv("PGO_DIST_TOP", "0", 1);
      Q.ordering = ordering;
      Q.part_size = size;
      Q.part_rank = r;
      pgo::chol_analyze(Q, G.n, G.row_ptr, G.col);
      unsetenv("PGO_DIST_TOP");
      if (Q.schedule_error) return fail("distributed: schedule");
    }
  }
  const pgo::CholPlan& A = R[0];
  long long tasks = 0, exch = 0;
  for (size_t L = A.split; L < A.levels.size(); L++)
    for (size_t j = 0; j < A.levels[L].panels.size(); j++) {
      std::map<Key, int> full;
      step_keys(A, A.levels[L].panels[j], full);
      std::vector<std::map<Key, int>> got(size);
      for (int r = 0; r < size; r++) {
        const pgo::CholPlan& Q = D[r];
        const size_t LQ = Q.split + (L - A.split);
        if (LQ >= Q.levels.size() || Q.levels[LQ].panels.size() != A.levels[L].panels.size())
          return fail("distributed: top levels differ");
        step_keys(Q, Q.levels[LQ].panels[j], got[r]);
        const pgo::PanelStep& ps = Q.levels[LQ].panels[j];
        for (int xi : {ps.xfirst, ps.xstep})
          if (xi >= 0) exch += Q.xchg[xi].cnt;
      }
      for (const auto& [k, cnt] : full) {
        const int kind = std::get<0>(k), s = std::get<1>(k);
        const int col = kind == 0 ? std::get<3>(k) : kind == 1 ? std::get<2>(k) : kind == 2 ? std::get<3>(k) : 0;
        const int o = D[0].cown[D[0].cown_off[s] + col];
        for (int r = 0; r < size; r++) {
          const auto it = got[r].find(k);
          const int want = (o < 0 || o == r) ? cnt : 0;
          if ((it == got[r].end() ? 0 : it->second) != want) {
            std::fprintf(stderr, "kind %d front %d row %d col %d depth %d: rank %d has %d, owner %d\n", kind, s,
                         std::get<2>(k), std::get<3>(k), std::get<4>(k), r, it == got[r].end() ? 0 : it->second, o);
            return fail("distributed: task coverage");
          }
          if (it != got[r].end()) got[r].erase(it);
        }
        tasks++;
      }
      for (int r = 0; r < size; r++)
        if (!got[r].empty()) return fail("distributed: a rank has a task the replicated plan lacks");
    }
  std::printf("distributed top, %d ranks: %lld task keys checked, %lld panels exchanged\n", size, tasks, exch);
  return 0;
}

// The tile lists of the H assembly (at_iptr / at_items): every tile task of
// every front this rank assembles lists exactly the front's off-diagonal
// targets, then its diagonal blocks, with an element in the tile, in order.
int check_assembly(const pgo::CholPlan& P) {
  std::vector<std::vector<int>> tg(P.ns);
  for (size_t g = 0; g < P.asm_front.size(); g++) tg[P.asm_front[g]].push_back((int)g);
  auto touches = [](int r0, int c0, int ti, int tj) {
    return r0 / 64 <= ti && ti <= (r0 + 2) / 64 && c0 / 64 <= tj && tj <= (c0 + 2) / 64;
  };
  for (size_t q = 0; q < P.ea_tasks.size(); q++) {
    const int4 t = P.ea_tasks[q];
    const int s = t.x, ti = t.y >> 16, tj = t.y & 0xffff;
    std::vector<int> want;
    for (int g : tg[s])
      if (touches(3 * P.asm_li[g], 3 * P.asm_lj[g], ti, tj)) want.push_back(g);
    for (int j = P.sfirst[s]; j < P.sfirst[s + 1]; j++)
      if (touches(3 * P.dg_loc[j], 3 * P.dg_loc[j], ti, tj)) want.push_back(~j);
    const int2 it = P.at_iptr[q];
    if (it.y != (int)want.size() || !std::equal(want.begin(), want.end(), P.at_items.begin() + it.x))
      return fail("assembly: a tile's H entries");
  }
  return 0;
}

// Who writes a front first.  Every 64x64 lower tile of every front this rank
// assembles (so every lower-trapezoid element: both kinds of task write their
// tile whole) is written whole exactly once before any task reads it: by its
// assembly tile (k_assemble_tile), or by a fused Schur task (syrk_gather: the
// 64-tile task that is the first update of an update-matrix tile and forms it
// from the children itself).  A fused task is tile-aligned and covers the
// tile's columns, sits at or past w rounded up to 64, and no Schur task of an
// earlier step or earlier in its step's list touches its tile; a plain Schur
// task only touches tiles already written.  Both kinds list exactly the child
// rectangles that land on their tile, children in order (brute force from the
// extend-add maps).
int check_first_writes(const pgo::CholPlan& P) {
  if (P.syrk_gather.size() != P.syrk_tasks.size()) return fail("fused: gather records");
  // 0: unwritten, 1: written by its assembly tile, 2: by its fused task, 3: updated since
  std::vector<std::vector<char>> st(P.ns);
  auto tile = [&](int s, int ti, int tj) -> char& {
    const int nt = (P.m[s] + 63) / 64;
    if (st[s].empty()) st[s].assign((size_t)nt * (nt + 1) / 2, 0);
    return st[s][(size_t)ti * (ti + 1) / 2 + tj];
  };
  auto check_pairs = [&](int s, int ti, int tj, int first, int cnt) {
    std::vector<int4> want;
    for (int q = P.cptr[s]; q < P.cptr[s + 1]; q++) {
      const int c = P.children[q], u = P.m[c] - P.w[c];
      int ra = -1, rn = 0, ca = -1, cn = 0;
      for (int a = 0; a < u; a++) {
        const int r = 3 * P.ea_rel[P.ea_ptr[c] + a / 3] + a % 3;
        if (r / 64 == ti && rn++ == 0) ra = a;
        if (r / 64 == tj && cn++ == 0) ca = a;
      }
      if (rn && cn) want.push_back(make_int4(c, ra, ca, rn | (cn << 8)));
    }
    if (cnt != (int)want.size() || first < 0 || (size_t)first + cnt > P.ea_pairs.size()) return false;
    for (int k = 0; k < cnt; k++) {
      const int4 a = P.ea_pairs[first + k], b = want[k];
      if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) return false;
    }
    return true;
  };
  long long fused = 0, fused_pairs = 0;
  for (const auto& lv : P.levels) {
    for (int q = lv.ea_off[0]; q < lv.ea_off[0] + lv.ea_cnt[0]; q++) {
      const int4 t = P.ea_tasks[q];
      const int s = t.x, ti = t.y >> 16, tj = t.y & 0xffff, nt = (P.m[s] + 63) / 64;
      if (ti >= nt || tj > ti) return fail("assembly: a tile outside its front's lower triangle");
      char& k = tile(s, ti, tj);
      if (k) return fail("assembly: a tile listed twice");
      k = 1;
      if (!check_pairs(s, ti, tj, t.z, t.w)) return fail("assembly: a tile's child rectangles");
    }
    for (const auto& ps : lv.panels)
      for (int q = ps.syrk_off; q < ps.syrk_off + ps.syrk_cnt; q++) {
        const int4 t = P.syrk_tasks[q];
        const int2 g = P.syrk_gather[q];
        const int s = t.x, row0 = t.y & pgo::kRowMask, clip = t.y >> pgo::kClipShift, c0 = t.z, m = P.m[s], w = P.w[s];
        const int T = ps.syrk_tile;
        const int colend = t.w < 0 ? std::min((ps.kb & ~(pgo::kKB - 1)) + pgo::kKB, w) : m;
        const int cend = std::min({colend, c0 + (clip ? clip : T), m});
        if (g.x >= 0) {
          if (T != pgo::kTile || t.w != 0 || (row0 & 63) || (c0 & 63) || c0 < ((w + 63) & ~63) ||
              cend != std::min(m, c0 + 64) || !pgo::front_packed(m, w))
            return fail("fused: a task that is not a whole update-matrix 64-tile's first update");
          char& k = tile(s, row0 / 64, c0 / 64);
          if (k) return fail("fused: the tile was written or updated before its fused task");
          k = 2;
          if (!check_pairs(s, row0 / 64, c0 / 64, g.x, g.y)) return fail("fused: a tile's child rectangles");
          fused++;
          fused_pairs += g.y > 0;
          continue;
        }
        for (int r0 = row0; r0 < std::min(row0 + T, m); r0 += 64)
          for (int cb = c0 / 64; cb <= (cend - 1) / 64 && cb <= r0 / 64; cb++) {
            char& k = tile(s, r0 / 64, cb);
            if (!k) return fail("a Schur task reads a tile nothing has written");
            k = 3;
          }
      }
  }
  if (fused != P.fused_tiles || fused_pairs != P.fused_with_pairs) return fail("fused: the plan's counts");
  for (const int4& t : P.ea_tasks)   // (a front's tile (0, 0) is never fused: the fronts this rank assembles)
    if (t.y == 0)
      for (char k : st[t.x])
        if (!k) return fail("a front's tile is written by no task");
  return 0;
}

// The assembly's targets and sources against the pattern: every target (j, i)
// of the permuted lower triangle (i > j) lists exactly the slots of one end of
// the block -- as many as row perm[i] holds to column perm[j] -- and every
// slot of the lower triangle is listed once.
// (sources: ~slot unbound; bound ones -- device factor indices, bound through
// `S`, the structure the pattern came from -- checked against the block's
// poses, and a target's parallel factors ascending: their slot order, the
// summation order.  With as many sources as the block has slots that is every
// factor of the pose pair, in device order.)
int check_sources(const pgo::CholPlan& P, const std::vector<int>& row_ptr, const std::vector<int>& col,
                  const pgo::GraphStructure* S = nullptr) {
  long long total = 0, want = 0;
  for (size_t g = 0; g < P.asm_front.size(); g++) {
    const int s = P.asm_front[g], j = P.sfirst[s] + P.asm_lj[g], i = P.rows[P.rptr[s] + P.asm_li[g]];
    if (i <= j) return fail("assembly: a target above the diagonal");
    const int a = P.perm[i], b = P.perm[j];
    int cnt = 0;
    for (int k = row_ptr[a]; k < row_ptr[a + 1]; k++) cnt += col[k] == b;
    if (P.asm_ptr[g + 1] - P.asm_ptr[g] != cnt) return fail("assembly: a target's source count");
    for (int q = P.asm_ptr[g]; q < P.asm_ptr[g + 1]; q++) {
      if (P.asm_src[q] >= 0) {   // bound: the factor id
        if (!S || P.asm_src[q] >= S->ne()) return fail("assembly: a bound source that is no factor");
        const int2 f = S->eij[P.asm_src[q]];
        if (std::min(f.x, f.y) != std::min(a, b) || std::max(f.x, f.y) != std::max(a, b))
          return fail("assembly: a bound source off its block");
        if (q > P.asm_ptr[g] && (P.asm_src[q - 1] < 0 || P.asm_src[q] <= P.asm_src[q - 1]))
          return fail("assembly: parallel factors out of slot order");
        continue;
      }
      const int k = ~P.asm_src[q];
      const int r = (int)(std::upper_bound(row_ptr.begin(), row_ptr.end(), k) - row_ptr.begin()) - 1;
      if (!((r == a && col[k] == b) || (r == b && col[k] == a))) return fail("assembly: a source off its block");
    }
    total += cnt;
  }
  for (int r = 0; r + 1 < (int)row_ptr.size(); r++)
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) want += P.iperm[r] > P.iperm[col[k]];
  if (total != want || P.asm_ptr.back() != want) return fail("assembly: sources of the lower triangle");
  return 0;
}

// Packed fronts: no Schur tile's columns straddle a 64-column block (the
// kernels address a tile's columns from one block base).
int check_tiles(const pgo::CholPlan& P) {
  for (const auto& lv : P.levels)
    for (const auto& ps : lv.panels)
      for (int q = ps.syrk_off; q < ps.syrk_off + ps.syrk_cnt; q++) {
        const int4 t = P.syrk_tasks[q];
        const int clip = t.y >> pgo::kClipShift, c0 = t.z, T = ps.syrk_tile;
        const int c1 = std::min(c0 + (clip ? clip : T), P.m[t.x]);
        if (T == pgo::kTile && (c0 >> 6) != ((c1 - 1) >> 6)) return fail("a 64-tile straddles two column blocks");
        if (T == pgo::kBigTile && (c0 & 63) && (c0 >> 6) != ((c1 - 1) >> 6))
          return fail("an unaligned 128-tile straddles two column blocks");
      }
  return 0;
}

// ---- the graph structure module (pgo_structure.h) and the plan bound through it ----

// A pose graph as the library's handle holds it: factors in user order with
// their information (values of mixed magnitude, so the order of Dc's sums shows).
struct TestGraph {
  int n = 0;
  std::vector<int2> e;
  std::vector<int> pv;
  std::vector<double> eom;
  void add(int a, int b) {
    e.push_back(make_int2(a, b));
    for (int q = 0; q < 6; q++) eom.push_back(1.0 / (3.0 + (double)(eom.size() % 97)) + 1e-7 * (double)eom.size());
  }
};

pgo::GraphStructure built(const TestGraph& g) {
  pgo::GraphStructure S;
  S.build(g.n, g.e, g.pv, g.eom.data(), true);
  return S;
}

// the factors of make_pattern's graph (odometry i -> i + 1, closures a -> b < a,
// every lc / dups-th closure twice: a parallel factor)
TestGraph make_edges(int n, int lc, unsigned seed, int dups) {
  std::mt19937 rng(seed);
  TestGraph g;
  g.n = n;
  for (int i = 0; i + 1 < n; i++) g.add(i, i + 1);
  for (int q = 0; q < lc; q++) {
    const int a = 20 + (int)(rng() % (unsigned)(n - 20));
    g.add(a, (int)(rng() % (unsigned)(a - 10)));
  }
  for (int q = 0; dups > 0 && q < lc; q += std::max(1, lc / dups)) g.add(g.e[n - 1 + q].x, g.e[n - 1 + q].y);
  return g;
}

// As bind_plan does: owner bits through the module, then every unbound source
// ~slot becomes its factor's device index.
void remap_sources(pgo::CholPlan& P, const pgo::GraphStructure& S) {
  for (int& x : P.asm_src)
    if (x < 0) x = S.codes()[~x] >> 2;
  P.asm_bound = true;
}

// The spliced assembly targets of an append equal a rebuild of the same plan,
// once both are bound.
int check_splice(const pgo::CholPlan& P, const pgo::GraphStructure& S) {
  pgo::CholPlan R = P;
  R.asm_splice = false;
  pgo::chol_assembly(R, S.row_ptr, S.slot_col);
  remap_sources(R, S);
  pgo::CholPlan Q = P;
  remap_sources(Q, S);
  if (Q.asm_front != R.asm_front || Q.asm_li != R.asm_li || Q.asm_lj != R.asm_lj || Q.asm_ptr != R.asm_ptr ||
      Q.asm_src != R.asm_src || Q.at_items != R.at_items || Q.at_iptr.size() != R.at_iptr.size())
    return fail("append: spliced assembly lists differ from a rebuild");
  for (size_t q = 0; q < Q.at_iptr.size(); q++)
    if (Q.at_iptr[q].x != R.at_iptr[q].x || Q.at_iptr[q].y != R.at_iptr[q].y) return fail("append: spliced tile items");
  return 0;
}

// The incremental symbolic update (chol_append): poses appended one at a time
// to a plan of the first n0 poses, the structure appended in place and the plan
// bound through it as the library does.  After each: the schedule is
// consistent, every front's below rows sit in its parent at the extend-add
// map's index, the sizes match the row lists, and the structure holds the exact
// fill of the plan's own ordering (a fresh analysis on P.perm) and the whole pattern.
int check_append(const TestGraph& G, int n_all, int n0, int ordering, pgo::CholPlan* keep = nullptr) {
  auto upto = [&](int lo, int hi) {   // the factors whose later pose is in [lo, hi)
    TestGraph g;
    for (const int2& f : G.e)
      if (std::max(f.x, f.y) >= lo && std::max(f.x, f.y) < hi) g.add(f.x, f.y);
    g.n = hi;
    return g;
  };
  TestGraph B = upto(0, n0);
  pgo::GraphStructure S = built(B);
  pgo::CholPlan P;
  P.ordering = ordering;
  pgo::chol_analyze(P, n0, S.row_ptr, S.slot_col);
  S.bind(P.iperm);
  remap_sources(P, S);
  {   // the growth limit applies to the plan after the append: no headroom refuses the first one
    pgo::CholPlan Q;
    Q.ordering = ordering;
    pgo::chol_analyze(Q, n0, S.row_ptr, S.slot_col);
    TestGraph B1 = upto(0, n0 + 1);
    const pgo::GraphStructure S1 = built(B1);
    std::vector<int2> pairs;
    for (int k = S1.row_ptr[n0]; k < S1.row_ptr[n0 + 1]; k++) pairs.push_back(make_int2(n0, S1.slot_col[k]));
    if (pgo::chol_append(Q, n0 + 1, S1.row_ptr, S1.slot_col, pairs, 1 << 30, 1.0)) return fail("append: growth limit not applied");
    if (Q.n != n0) return fail("append: a refused append changed the plan");
  }
  for (int n = n0 + 1; n <= n_all; n++) {
    const TestGraph add = upto(n - 1, n);
    for (const int2& f : add.e) B.add(f.x, f.y);
    B.n = n;
    pgo::StructureDelta dl;
    if (!S.append(n, add.e, B.eom.data(), true, &dl)) return fail("append: the structure refused a new pose");
    std::vector<int2> pairs;
    for (int k = S.row_ptr[n - 1]; k < S.row_ptr[n]; k++) pairs.push_back(make_int2(n - 1, S.slot_col[k]));
    if (!pgo::chol_append(P, n, S.row_ptr, S.slot_col, pairs, 1 << 30, 1e30)) return fail("append: refused");
    if (P.schedule_error) return fail("append: panel schedule bookkeeping");
    if (check_assembly(P) || check_first_writes(P) || check_sources(P, S.row_ptr, S.slot_col, &S)) return 1;
    S.bind(P.iperm);   // (the old poses keep their order: the new slots only)
    if (check_splice(P, S)) return 1;
    remap_sources(P, S);   // (the next append splices)
    if (check_sources(P, S.row_ptr, S.slot_col, &S)) return 1;
    if (P.n != n || !pgo::chol_covers(P, n, S.row_ptr, S.slot_col)) return fail("append: pattern not covered");
    for (int s = 0; s < P.ns; s++) {
      const int wp = P.sfirst[s + 1] - P.sfirst[s], nr = P.rptr[s + 1] - P.rptr[s];
      if (P.m[s] != 3 * nr || P.w[s] != 3 * wp || P.ea_ptr[s + 1] - P.ea_ptr[s] != nr - wp)
        return fail("append: front sizes");
      const int p = P.parent[s];
      for (int t = 0; t < nr - wp; t++) {
        const int r = P.rows[P.rptr[s] + wp + t];
        if (t > 0 && r <= P.rows[P.rptr[s] + wp + t - 1]) return fail("append: rows unsorted");
        if (p < 0 || P.rows[P.rptr[p] + P.ea_rel[P.ea_ptr[s] + t]] != r) return fail("append: extend-add map");
      }
    }
    pgo::CholPlan Q;
    Q.order_in = P.perm;
    pgo::chol_analyze(Q, n, S.row_ptr, S.slot_col);
    for (int q = 0; q < Q.ns; q++)
      for (int a = Q.rptr[q]; a < Q.rptr[q + 1]; a++)
        for (int j = Q.sfirst[q]; j < Q.sfirst[q + 1]; j++) {
          const int i = Q.rows[a];
          if (i > j) {
            std::vector<int2> one{make_int2(Q.perm[i], Q.perm[j])};
            if (!pgo::chol_covers(P, one)) return fail("append: fill of the ordering not covered");
          }
        }
  }
  {   // the structure after ten in-place appends and incremental binds: a rebuild, bound whole
    pgo::GraphStructure F = built(B);
    F.bind(P.iperm);
    if (S.codes() != F.codes() || S.eside() != F.eside() || S.row_ptr != F.row_ptr || S.slot_col != F.slot_col)
      return fail("append: the structure differs from a rebuild");
  }
  if (keep) *keep = P;
  else std::printf("append: %d poses onto %d, %d fronts, flops %.3g\n", n_all - n0, n0, P.ns, P.flops);
  return 0;
}

// What the device holds: the uploader's copies replayed on host arrays (the
// ranges pgo_api.cpp copies after build / append / bind / unbind, nothing more).
struct DeviceCopy {
  std::vector<int2> eij;
  std::vector<int> prior_ptr, row_ptr, code, col, erow, s1_ptr, s1pos, s1fac, brow;
  std::vector<unsigned char> eside;
  std::vector<double> Dc;
  template <class T>
  static void put(std::vector<T>& dst, const std::vector<T>& src, size_t first, size_t end) {
    if (dst.size() < src.size()) dst.resize(src.size());
    std::copy(src.begin() + first, src.begin() + end, dst.begin() + first);
  }
  void upload(const pgo::GraphStructure& S) {
    eij = S.eij, prior_ptr = S.prior_ptr, row_ptr = S.row_ptr, code = S.codes(), col = S.slot_col;
    erow = S.erow, s1_ptr = S.s1_ptr, s1pos = S.s1pos, s1fac = S.s1fac, brow = S.brow, Dc = S.Dc;
  }
  void append(const pgo::GraphStructure& S, const pgo::StructureDelta& d) {
    const size_t n = S.n, ne = S.ne();
    put(eij, S.eij, d.ne_old, ne);
    put(prior_ptr, S.prior_ptr, d.n_old + 1, n + 1);
    put(row_ptr, S.row_ptr, d.r0 + 1, n + 1);
    put(code, S.codes(), d.k0, 2 * ne);
    put(col, S.slot_col, d.k0, 2 * ne);
    put(erow, S.erow, d.x0 + 1, n + 1);
    put(s1_ptr, S.s1_ptr, d.y0 + 1, n + 1);
    s1pos = S.s1pos, s1fac = S.s1fac, brow = S.brow;
    for (int y : d.dc_rows) put(Dc, S.Dc, 6 * (size_t)y, 6 * (size_t)y + 6);
    put(Dc, S.Dc, 6 * (size_t)d.n_old, 6 * n);
  }
  void bind(const pgo::GraphStructure& S, pgo::SlotRange r) {
    put(code, S.codes(), r.begin, r.end);
    eside = S.eside();
  }
};

template <class T>
bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// S (appended in place) and D (the device after the delta's copies) against F,
// a fresh build of the grown graph: array for array, Dc bitwise; the owner bits apart
int same_structure(pgo::GraphStructure& S, const DeviceCopy& D, pgo::GraphStructure& F) {
  if (S.n != F.n || !same_bits(S.eij, F.eij) || S.dorder != F.dorder || S.pv != F.pv || S.prior_ptr != F.prior_ptr ||
      S.porder != F.porder || S.row_ptr != F.row_ptr || S.slot_col != F.slot_col || S.edge_slot0 != F.edge_slot0 ||
      S.erow != F.erow || S.s1_ptr != F.s1_ptr || S.s1pos != F.s1pos || S.s1fac != F.s1fac || S.brow != F.brow ||
      !same_bits(S.Dc, F.Dc) || S.G != F.G || S.G1 != F.G1 || S.gauge_free != F.gauge_free)
    return fail("structure: an in-place append differs from a rebuild");
  for (size_t k = 0; k < S.codes().size(); k++)
    if ((S.codes()[k] | 2) != (F.codes()[k] | 2)) return fail("structure: slot codes differ from a rebuild");
  for (int v = 1; v < S.n; v++)
    if (S.same_component(0, v) != F.same_component(0, v) || S.same_component(v - 1, v) != F.same_component(v - 1, v))
      return fail("structure: components differ from a rebuild");
  if (!same_bits(D.eij, F.eij) || D.prior_ptr != F.prior_ptr || D.row_ptr != F.row_ptr || D.col != F.slot_col ||
      D.erow != F.erow || D.s1_ptr != F.s1_ptr || D.s1pos != F.s1pos || D.s1fac != F.s1fac || D.brow != F.brow ||
      !same_bits(D.Dc, F.Dc) || D.code != S.codes())
    return fail("structure: the append's delta does not cover what changed");
  return 0;
}

// owner slots of every factor in `code` (device factor -> count, side of the last)
bool one_owner_each(const std::vector<int>& code, int ne, std::vector<unsigned char>* side = nullptr) {
  std::vector<int> cnt(ne, 0);
  if (side) side->assign(ne, 0);
  for (int c : code)
    if (c & 2) {
      cnt[c >> 2]++;
      if (side) (*side)[c >> 2] = (unsigned char)(c & 1);
    }
  return std::all_of(cnt.begin(), cnt.end(), [](int c) { return c == 1; });
}

// a chain of 48 poses, 10 closures (none from the last pose), 4 of them twice
// (parallel factors, apart in user order); optionally a second component of 8
// poses and a prior on pose 0
TestGraph small_graph(bool prior, bool second_component) {
  TestGraph g = make_edges(47, 10, 11, 0);
  g.add(47 - 1, 47);
  g.n = 48;
  for (int q = 0; q < 10; q += 3) g.add(g.e[46 + q].x, g.e[46 + q].y);
  if (second_component) {
    for (int i = 48; i + 1 < 56; i++) g.add(i, i + 1);
    g.n = 56;
  }
  if (prior) g.pv.push_back(0);
  return g;
}

// the append shapes; k counts the applications to one graph
enum { kPoseToRow0, kMiddleRow, kParallel, kThreePoses, kJoin, kShapes };
TestGraph append_shape(int kind, const pgo::GraphStructure& S, int k) {
  const int n = S.n;
  TestGraph a;
  a.n = n;
  switch (kind) {
    case kPoseToRow0: a.n = n + 1, a.add(n - 1, n), a.add(n, 0); break;
    case kMiddleRow: a.add(n - 1, 20 + k); break;
    case kParallel: a.add(S.eij.back().x, S.eij.back().y); break;
    case kThreePoses: a.n = n + 3, a.add(n - 1, n), a.add(n, n + 1), a.add(n + 1, n + 2), a.add(n + 2, 7 + k); break;
    case kJoin: a.n = n + 1, a.add(n - 1, n), a.add(n, 5 + k); break;   // (n - 1: the second component's end)
  }
  return a;
}

// One shape applied `reps` times in a row.  Pre-plan: every result equals a
// rebuild, codes included.  Bound first (random order `seed`): no bind between
// the appends (the second meets the first's new-slot list), each leaves the old
// slots' bits and one owner slot per factor on the device unless kMixed, then
// the incremental bind equals a full bind of a rebuild under the same order,
// unbind gives the rebuild's pre-plan codes, a changed order binds whole.
int check_shape(const TestGraph& g0, int kind, int reps, bool bound, unsigned seed) {
  TestGraph g = g0;
  pgo::GraphStructure S = built(g);
  DeviceCopy D;
  D.upload(S);
  std::mt19937 rng(seed);
  std::vector<int> iperm(g.n);
  for (int i = 0; i < g.n; i++) iperm[i] = i;
  std::shuffle(iperm.begin(), iperm.end(), rng);
  if (bound) {
    const pgo::SlotRange r = S.bind(iperm);
    if (r.begin != 0 || r.end != S.nslots() || S.slot_codes() != pgo::GraphStructure::kBound || S.bind_row0() != S.n)
      return fail("owner bits: the first bind's range");
    D.bind(S, r);
    std::vector<unsigned char> side;
    if (!one_owner_each(D.code, S.ne(), &side) || side != D.eside) return fail("owner bits: bind after a build");
    for (int r2 = 0; r2 < S.n; r2++)
      for (int k = S.row_ptr[r2]; k < S.row_ptr[r2 + 1]; k++)
        if (((D.code[k] & 2) != 0) != (iperm[r2] > iperm[S.slot_col[k]])) return fail("owner bits: not the lower triangle");
  }
  int k0_min = S.nslots();
  for (int k = 0; k < reps; k++) {
    const TestGraph a = append_shape(kind, S, k);
    const std::vector<int> before = D.code;
    const int n_old = S.n, ne_old = S.ne();
    for (const int2& f : a.e) g.add(f.x, f.y);
    g.n = a.n;
    pgo::StructureDelta dl;
    if (!S.append(g.n, a.e, g.eom.data(), true, &dl)) return fail("structure: an append in device order refused");
    D.append(S, dl);
    pgo::GraphStructure F = built(g);
    if (same_structure(S, D, F)) return 1;
    if (dl.n_old != n_old || dl.ne_old != ne_old || dl.k0 != S.row_ptr[dl.r0] || (kind == kPoseToRow0 && dl.r0 != 0) ||
        (kind == kMiddleRow && dl.r0 != 20 + k))
      return fail("structure: the append's delta");
    k0_min = std::min(k0_min, dl.k0);
    if (!bound) {
      if (S.codes() != F.codes() || S.slot_codes() != pgo::GraphStructure::kPrePlan) return fail("structure: pre-plan codes");
      continue;
    }
    if (S.slot_codes() != (k0_min > 0 ? pgo::GraphStructure::kMixed : pgo::GraphStructure::kBound) || S.bind_row0() > dl.r0)
      return fail("owner bits: the state after an append");
    if (k == 0) {   // every old slot bound, still (the merge keeps them, in order), the new ones pre-plan
      size_t o = 0;
      for (size_t q = 0; q < D.code.size(); q++) {
        if ((D.code[q] >> 2) < ne_old ? (o >= before.size() || D.code[q] != before[o++]) : D.code[q] != F.codes()[q])
          return fail("owner bits: an append moved or changed a bound slot");
      }
      if (o != before.size() || !one_owner_each(D.code, S.ne())) return fail("owner bits: per factor after an append");
    } else {   // the first append's list is stale: pre-plan codes from the first changed slot on
      if (!std::equal(D.code.begin() + dl.k0, D.code.end(), F.codes().begin() + dl.k0))
        return fail("owner bits: a second append before a bind left bound codes in its tail");
    }
  }
  if (kind == kJoin && (g0.pv.empty() ? !S.gauge_free : S.gauge_free)) return fail("structure: gauge after joining components");
  if (!bound) return 0;
  for (int v = (int)iperm.size(); v < g.n; v++) iperm.push_back(v);
  pgo::GraphStructure F = built(g);
  {   // append -> unbind on a copy: the rebuild's pre-plan codes, whole
    pgo::GraphStructure U = S;
    DeviceCopy DU = D;
    const bool up = U.unbind();
    if (up != (k0_min > 0)) return fail("owner bits: unbind without mixed codes, or none with them");
    if (up) DU.code = U.codes();
    if (!one_owner_each(DU.code, U.ne()) || (up && (DU.code != F.codes() || U.slot_codes() != pgo::GraphStructure::kPrePlan)))
      return fail("owner bits: unbind after an append");
  }
  const pgo::SlotRange r = S.bind(iperm);
  if (r.begin != k0_min || r.end != S.nslots()) return fail("owner bits: the incremental bind's range");
  D.bind(S, r);
  F.bind(iperm);
  if (S.codes() != F.codes() || D.code != F.codes() || S.eside() != F.eside())
    return fail("owner bits: an incremental bind differs from a full bind of a rebuild");
  std::shuffle(iperm.begin(), iperm.end(), rng);
  S.order_changed();
  const pgo::SlotRange r2 = S.bind(iperm);
  D.bind(S, r2);
  pgo::GraphStructure F2 = built(g);
  F2.bind(iperm);
  if (r2.begin != 0 || D.code != F2.codes() || S.eside() != F2.eside()) return fail("owner bits: bind after a changed order");
  return 0;
}

int check_structure() {
  const TestGraph base = small_graph(true, false);
  for (int kind = 0; kind < kJoin; kind++)
    for (int reps : {1, 2})
      for (bool bound : {false, true})
        if (check_shape(base, kind, reps, bound, 100 + kind)) return 1;
  for (bool prior : {false, true})   // a second component joined: anchored by the prior, or gauge-free still
    for (bool bound : {false, true})
      if (check_shape(small_graph(prior, true), kJoin, 2, bound, 7)) return 1;
  {   // refusals leave the structure untouched
    pgo::GraphStructure S = built(base), F = built(base);
    S.bind(std::vector<int>(base.n, 0)), F.bind(std::vector<int>(base.n, 0));
    DeviceCopy D;
    D.upload(S);
    TestGraph g = base;
    g.add(3, 30);   // sorts before (46, 47)
    pgo::StructureDelta dl;
    if (S.append(g.n, {g.e.back()}, g.eom.data(), true, &dl)) return fail("structure: a factor before the last old one appended");
    if (S.append(base.n, {}, base.eom.data(), true, &dl)) return fail("structure: nothing new appended");
    if (S.append(base.n - 1, {}, base.eom.data(), true, &dl)) return fail("structure: a shrunk graph appended");
    if (same_structure(S, D, F) || S.codes() != F.codes() || S.bind_row0() != F.bind_row0() || S.slot_codes() != F.slot_codes())
      return fail("structure: a refused append changed the structure");
    TestGraph v;   // vertices only: no factor to sort after
    v.n = 3;
    pgo::GraphStructure E = built(v);
    v.add(0, 1);
    if (E.append(3, v.e, v.eom.data(), true, &dl) || E.n != 3 || E.ne() != 0 || E.row_ptr != std::vector<int>(4, 0))
      return fail("structure: an append onto no factors");
  }
  {   // packing: (x, y, theta) -> (x, y, cos, sin), six doubles -> three double2, through `order`
    const double pi = 3.14159265358979323846;
    const double z[] = {1.5, -2.25, pi, 0.0, 1e-300, -pi, -7.0, 3.0, 0.3, 4.0, 5.0, -0.0};
    double om[24];
    for (int q = 0; q < 24; q++) om[q] = 0.5 + q * 1.25;
    const int order[] = {2, 0, 3, 1};
    double4 hz[4];
    double2 hom[12];
    pgo::pack_measurements(z, om, order, 4, hz, hom);
    for (int k = 0; k < 4; k++) {
      const int e = order[k];
      const double th = z[3 * e + 2];
      const double want[4] = {z[3 * e], z[3 * e + 1], std::cos(th), std::sin(th)};
      const double got[4] = {hz[k].x, hz[k].y, hz[k].z, hz[k].w};
      if (std::memcmp(want, got, sizeof(want))) return fail("packing: a measurement");
      for (int q = 0; q < 3; q++)
        if (hom[3 * k + q].x != om[6 * e + 2 * q] || hom[3 * k + q].y != om[6 * e + 2 * q + 1]) return fail("packing: information");
    }
  }
  std::printf("structure module: append shapes, refusals, owner bits, packing ok\n");
  return 0;
}

// ---- the optimiser's control (pgo_lm.h) against GTSAM's loop, one try at a time ----

struct ScriptTry {
  double solved, new_e, lin_change;
};

// Scripted outcomes: try k of linearisation i, whatever lambda it runs at.
// Past a linearisation's listed tries (and past the listed linearisations):
// `rest`, a solved try that doubles the error.
struct LmCase {
  const char* name;
  pgo_params p;
  double err0 = 100.0;
  std::vector<std::vector<ScriptTry>> lins;
  std::vector<double> lin_err;   // per listed linearisation (the robust guard's scale); empty: the error
  ScriptTry at(int i, int k) const {
    if (i < (int)lins.size() && k < (int)lins[i].size()) return lins[i][k];
    return {1.0, 2.0 * err0, 1.0};
  }
};

struct RefRun {
  std::vector<double> trace;   // 7 columns
  int iters = 0, inner = 0, lins = 0, status = PGO_OK, stop_reason = PGO_STOP_CONVERGED;
  double lam = 0, factor = 0, err = 0;
  std::vector<int> tries;      // per linearisation: tries made
  std::vector<int> accepted;   // per linearisation: the accepted try, -1 none
};

bool ref_converged(const pgo_params& p, double cur, double nw) {
  if (nw <= p.error_tol) return true;
  const double absd = cur - nw, reld = absd / cur;
  return (p.relative_error_tol != 0.0 && reld <= p.relative_error_tol) || absd <= p.absolute_error_tol;
}

// LevenbergMarquardtOptimizer::iterate / tryLambda and NonlinearOptimizer::
// defaultOptimize as the C oracle states them, sequentially; the stop reason
// as include/pgo.h defines it.
RefRun lm_reference(const LmCase& c) {
  const pgo_params& prm = c.p;
  RefRun R;
  double err = c.err0, lam = prm.lambda_initial, factor = prm.lambda_factor;
  int iters = 0, inner = 0, rc = PGO_OK, how = PGO_STOP_CONVERGED;
  auto row = [&](double a, double b, double s, double lc, double e, double f, double acc) {
    for (double v : {a, b, s, lc, e, f, acc}) R.trace.push_back(v);
  };
  if (!(err <= prm.error_tol) && iters < prm.max_iterations) {
    double new_err = err;
    for (;;) {
      const double cur_err = new_err;
      const int i = R.lins++;
      R.tries.push_back(0);
      R.accepted.push_back(-1);
      if (prm.algorithm == PGO_ALG_GN) {
        const ScriptTry s = c.at(i, R.tries[i]++);
        if (s.solved == 0.0) {
          rc = PGO_E_INDETERMINANT;
          break;
        }
        R.accepted[i] = 0;
        err = s.new_e;
        iters++;
        inner++;
        row(iters, 0, 1, NAN, err, 0, 1);
      } else {
        for (;;) {  // tryLambda
          double fidelity = 0.0, new_e = INFINITY, lin_change = NAN;
          int success = 0, stop = 0;
          const ScriptTry s = c.at(i, R.tries[i]++);
          const int solved = s.solved == 1.0;
          if (solved) {
            const double old_lin = i < (int)c.lin_err.size() ? c.lin_err[i] : err;
            lin_change = s.lin_change;
            if (lin_change >= 0) {
              new_e = s.new_e;
              const double cost_change = err - new_e;
              if (lin_change > 2.220446049250313e-16 * old_lin) {
                fidelity = cost_change / lin_change;
                success = fidelity > prm.min_model_fidelity;
              }
              if (std::fabs(cost_change) < prm.relative_error_tol * err) stop = 1;
            }
          }
          row(iters, lam, solved, lin_change, new_e, fidelity, success);
          if (success) {
            if (prm.use_fixed_lambda_factor) lam /= prm.lambda_factor;
            else {
              const double q = 2.0 * fidelity - 1.0;
              const double f = 1.0 - q * q * q;
              lam *= f > 1.0 / 3.0 ? f : 1.0 / 3.0;
              factor *= 2.0;
            }
            if (lam < prm.lambda_lower_bound) lam = prm.lambda_lower_bound;
            R.accepted[i] = R.tries[i] - 1;
            err = new_e;
            iters++;
            inner++;
            how = PGO_STOP_CONVERGED;
            break;
          }
          if (!stop) {
            lam *= factor;
            inner++;
            if (!prm.use_fixed_lambda_factor) factor *= 2.0;
            if (lam >= prm.lambda_upper_bound) {
              how = PGO_STOP_LAMBDA_BOUND;
              break;
            }
            continue;
          }
          how = PGO_STOP_SMALL_CHANGE;
          break;
        }
      }
      new_err = err;
      if (prm.max_outer > 0 && R.lins >= prm.max_outer) {
        how = PGO_STOP_MAX_OUTER;
        break;
      }
      if (!(iters < prm.max_iterations && !ref_converged(prm, cur_err, new_err) && std::isfinite(cur_err))) break;
    }
  }
  R.iters = iters, R.inner = inner, R.lam = lam, R.factor = factor, R.err = err;
  R.status = rc != PGO_OK ? rc : (iters >= prm.max_iterations && prm.max_iterations > 0 ? PGO_W_MAXITER : PGO_OK);
  R.stop_reason = rc < 0                                                       ? PGO_STOP_ERROR
                  : how == PGO_STOP_MAX_OUTER || R.status != PGO_W_MAXITER ? how
                                                                               : PGO_STOP_MAX_ITER;
  return R;
}

// The lane rule written out (the comment at LmControl::round_lanes): lanes a
// rank runs in a round, given the tries the previous linearisation walked and
// those of this one walked so far.
struct LaneRow {
  int mode, prev_walked, walked, L, profiled, exchange, Lr;
};
const LaneRow kLaneTable[] = {
    // mode 0: every round runs all lanes
    {0, 0, 0, 3, 0, 0, 3}, {0, 1, 0, 3, 0, 0, 3}, {0, 4, 1, 8, 0, 0, 8}, {0, 2, 0, 3, 1, 0, 1},
    // mode 1: the first linearisation and one after a first-try acceptance expect 1 try
    {1, 0, 0, 3, 0, 0, 1}, {1, 0, 1, 3, 0, 0, 3}, {1, 1, 0, 3, 0, 0, 1}, {1, 1, 1, 3, 0, 0, 3}, {1, 1, 4, 3, 0, 0, 3},
    // after k >= 2 tries: 2 expected, not k
    {1, 2, 0, 3, 0, 0, 2}, {1, 5, 0, 3, 0, 0, 2}, {1, 5, 1, 3, 0, 0, 1}, {1, 5, 2, 3, 0, 0, 3}, {1, 5, 0, 1, 0, 0, 1},
    {1, 7, 0, 8, 0, 0, 2}, {1, 7, 2, 8, 0, 0, 8},
    // a profiled factorisation runs alone; ranks that exchange run every lane
    {1, 5, 0, 3, 1, 0, 1}, {1, 5, 2, 3, 1, 0, 1}, {1, 0, 0, 3, 0, 1, 3}, {1, 5, 0, 3, 0, 1, 3}, {1, 5, 0, 3, 1, 1, 1},
    // mode 2: the previous linearisation's count, all lanes first
    {2, 0, 0, 3, 0, 0, 3}, {2, 1, 0, 3, 0, 0, 1}, {2, 3, 0, 4, 0, 0, 3}, {2, 3, 1, 4, 0, 0, 2}, {2, 3, 3, 4, 0, 0, 4},
    {2, 6, 0, 4, 0, 0, 4}, {2, 3, 0, 4, 0, 1, 4},
    // mode 3: mode 1's rule, all lanes first
    {3, 0, 0, 3, 0, 0, 3}, {3, 1, 0, 3, 0, 0, 1}, {3, 4, 0, 3, 0, 0, 2}, {3, 4, 1, 3, 0, 0, 1}, {3, 4, 2, 3, 0, 0, 3},
    {3, 0, 0, 3, 1, 0, 1},
};

pgo_params lm_params() {
  pgo_params p;
  std::memset(&p, 0, sizeof(p));
  p.max_iterations = 100;
  p.relative_error_tol = p.absolute_error_tol = 1e-5;
  p.lambda_initial = 1e-5, p.lambda_factor = 10.0, p.lambda_upper_bound = 1e5;
  p.min_model_fidelity = 1e-3;
  p.use_fixed_lambda_factor = 1;
  p.algorithm = PGO_ALG_LM;
  return p;
}

std::vector<LmCase> lm_cases() {
  const ScriptTry rej = {1.0, 200.0, 1.0}, bad = {0.0, 0.0, NAN};
  // a step from `from` to `to` at model fidelity fid
  auto acc = [](double from, double to, double fid = 1.0) { return ScriptTry{1.0, to, (from - to) / fid}; };
  // a solved try that barely moves: not accepted, the small cost change stops the linearisation
  auto still = [](double at) { return ScriptTry{1.0, at - at * 1e-9, 1.0}; };
  std::vector<LmCase> cs;
  auto add = [&](const char* name, std::vector<std::vector<ScriptTry>> lins) -> LmCase& {
    cs.push_back({name, lm_params(), 100.0, std::move(lins), {}});
    return cs.back();
  };
  // accepted at once; the last step both negligible and accepted, then converged
  add("first try", {{acc(100, 50)}, {acc(50, 25)}, {acc(25, 25 * (1 - 1e-7))}});
  {   // accepted at try k = 2 .. 10: past a round boundary at every T, past a whole rejected round at T = 8
    std::vector<std::vector<ScriptTry>> lins;
    for (int k = 2; k <= 10; k++) {
      lins.emplace_back(k - 1, rej);
      lins.back().push_back(acc(100 - 10 * (k - 2), 90 - 10 * (k - 2)));
    }
    lins.push_back({acc(10, 10 - 1e-7)});
    // (linearisation k leaves lambda k - 2 decades higher: 1e31 by the last)
    add("try k", lins).p.lambda_upper_bound = 1e300;
  }
  add("bad pivot", {{bad, bad, acc(100, 50)}, {rej, bad, acc(50, 49)}, {still(49)}});
  add("model increase", {{{1.0, 50.0, -1.0}, acc(100, 60)}, {{1.0, 10.0, -1e-30}, rej, acc(60, 59.9999999)}});
  {   // the guard eps * lin_err: a decrease under it with lin_err >> err (the error's own scale
      // would let it through and accept), one over it with lin_err << err (the error's would block it)
    LmCase& c = add("robust guard", {{{1.0, 50.0, 1e-11}, acc(100, 60)}, {{1.0, 59.0, 1e-15}}, {still(59)}});
    c.lin_err = {1e6, 1e-3, 59.0};
    c.p.min_model_fidelity = 1e-3;
  }
  add("small change", {{rej, {1.0, 100.0 * (1 - 1e-9), 1.0}}});
  for (int n = 1; n <= 9; n++) {   // n rejections reach the bound exactly: mid-round, at k = T - 1, at k = T
    LmCase& c = add("upper bound", {});
    c.p.lambda_factor = 2.0;
    c.p.lambda_upper_bound = 131072.0;
    c.p.lambda_initial = std::ldexp(1.0, 17 - n);
  }
  {   // an acceptance after the bound's last try but one, then the bound again
    LmCase& c = add("upper bound, accepted before", {{rej, rej, acc(100, 50)}});
    c.p.lambda_factor = 2.0, c.p.lambda_upper_bound = 131072.0, c.p.lambda_initial = std::ldexp(1.0, 14);
  }
  add("lower bound", {{acc(100, 50)}, {acc(50, 25)}, {rej, acc(25, 12)}, {still(12)}}).p.lambda_lower_bound = 1e-6;
  {   // the factor doubling: rejections and acceptances at fidelities on both sides of the 1/3 floor
    LmCase& c = add("doubling factor", {{rej, rej, acc(100, 50, 0.7)}, {rej, acc(50, 40, 0.05)}, {acc(40, 30, 0.5)},
                                        {rej, rej, rej, acc(30, 29, 0.999)}, {still(29)}});
    c.p.use_fixed_lambda_factor = 0;
    c.p.lambda_lower_bound = 1e-7;
    c.p.lambda_upper_bound = 1e30;   // (the doubled factor reaches 1e5 within the rejections of the fourth linearisation)
  }
  add("max_outer", {{acc(100, 50)}, {rej, acc(50, 25)}, {acc(25, 12)}}).p.max_outer = 2;
  add("max_outer, rejected", {{acc(100, 50)}}).p.max_outer = 2;
  add("max_iterations", {{acc(100, 50)}, {rej, acc(50, 25)}, {acc(25, 12)}}).p.max_iterations = 2;
  add("max_iterations 0", {{acc(100, 50)}}).p.max_iterations = 0;
  {
    LmCase& c = add("max_outer and max_iterations", {{acc(100, 50)}, {rej, rej, acc(50, 25)}, {acc(25, 12)}});
    c.p.max_outer = 2, c.p.max_iterations = 2;
  }
  add("error_tol at entry", {{acc(100, 50)}}).p.error_tol = 1e3;
  add("error_tol reached", {{acc(100, 50)}, {acc(50, 5)}, {acc(5, 1)}}).p.error_tol = 10.0;
  {
    LmCase& c = add("gn", {{acc(100, 50)}, {acc(50, 25)}, {acc(25, 25 - 1e-9)}});
    c.p.algorithm = PGO_ALG_GN;
  }
  {   // a Gauss-Newton step takes whatever error it lands on: the loop ends on the non-finite one
    LmCase& c = add("gn non-finite", {{acc(100, 50)}, {{1.0, NAN, NAN}}, {acc(50, 5)}, {acc(5, 1)}});
    c.p.algorithm = PGO_ALG_GN;
  }
  {
    LmCase& c = add("gn failed solve", {{acc(100, 50)}, {bad}, {acc(50, 5)}});
    c.p.algorithm = PGO_ALG_GN;
  }
  {
    LmCase& c = add("gn max_iterations", {{acc(100, 50)}, {acc(50, 25)}, {acc(25, 12)}});
    c.p.algorithm = PGO_ALG_GN, c.p.max_iterations = 2;
  }
  return cs;
}

bool same_double(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int check_lm() {
  for (const LaneRow& r : kLaneTable) {   // the lane rule on its own
    pgo::LmControl c(lm_params(), 100.0, r.mode);
    c.prev_walked = r.prev_walked, c.walked = r.walked;
    if (c.round_lanes(r.L, r.profiled != 0, r.exchange != 0) != r.Lr) {
      std::fprintf(stderr, "mode %d prev %d walked %d L %d profiled %d exchange %d: not %d lanes\n", r.mode,
                   r.prev_walked, r.walked, r.L, r.profiled, r.exchange, r.Lr);
      return fail("lm: the lane rule");
    }
  }
  const int splits[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 3}, {3, 1}, {1, 4}, {2, 2}, {4, 1}, {1, 6},
                           {2, 3}, {3, 2}, {6, 1}, {1, 8}, {2, 4}, {4, 2}, {8, 1}};
  long long runs = 0, rejected = 0;
  for (const LmCase& c : lm_cases()) {
    const RefRun R = lm_reference(c);
    // what the reference walked is what a device would have recorded; the rest is speculative
    pgo::LmScript S;
    S.lin_ptr.assign(1, 0);
    for (int i = 0; i < R.lins; i++) {
      for (int k = 0; k < R.tries[i]; k++) {
        const ScriptTry s = c.at(i, k);
        for (double v : {s.solved, s.new_e, s.lin_change}) S.tries.push_back(v);
      }
      S.lin_ptr.push_back(S.lin_ptr.back() + R.tries[i]);
      if (!c.lin_err.empty()) S.lin_err.push_back(i < (int)c.lin_err.size() ? c.lin_err[i] : NAN);
    }
    for (size_t r = 0; r < R.trace.size() / 7; r++) rejected += R.trace[7 * r + 6] == 0.0;
    for (const auto& pl : splits)
      for (int mode = 0; mode < 4; mode++)
        for (int every : {0, 1, 3}) {
          const int P = pl[0], L = pl[1], T = P * L;
          pgo_params p = c.p;
          p.profile_every = every;
          pgo::LmReplay rep;
          const pgo::LmControl C = pgo::lm_replay(p, c.err0, mode, P, L, every, S, &rep);
          // where the sequential loop's accepted tries fall: the accepting
          // round resumed after `base` walked tries and holds try base + k at
          // rank k / L, lane k % L
          std::vector<int> want;
          size_t w = 0;
          bool based = true;
          for (int i = 0; i < R.lins; i++) {
            if (R.accepted[i] < 0) continue;
            const int base = w < rep.winner_base.size() ? rep.winner_base[w] : -1;
            w++;
            const int k = R.accepted[i] - base;
            based = based && base >= 0 && k >= 0 && k < T && (c.p.algorithm != PGO_ALG_GN || base == 0);
            want.push_back(k / L);
            want.push_back(k % L);
          }
          if (c.p.algorithm == PGO_ALG_GN) want.clear(), based = rep.winner_base.empty();
          based = based && (c.p.algorithm == PGO_ALG_GN || w == rep.winner_base.size());
          const bool same = C.trace.size() == R.trace.size() &&
                            (R.trace.empty() || !std::memcmp(C.trace.data(), R.trace.data(), R.trace.size() * sizeof(double))) &&
                            C.iters == R.iters && C.inner == R.inner && C.linearizations == R.lins &&
                            same_double(C.lam, R.lam) && same_double(C.factor, R.factor) && same_double(C.err, R.err) &&
                            C.status == R.status && C.stop_reason == R.stop_reason && !rep.exhausted &&
                            rep.winners == want && based;
          if (!same) {
            std::fprintf(stderr,
                         "lm case '%s' (lambda0 %g), %d ranks x %d lanes, adapt %d, profiled every %d:\n"
                         "  control: %zu rows, iters %d inner %d lins %d lam %.17g factor %g err %.17g status %d stop %d "
                         "rounds %d winners %zu%s\n"
                         "  GTSAM  : %zu rows, iters %d inner %d lins %d lam %.17g factor %g err %.17g status %d stop %d "
                         "winners %zu\n",
                         c.name, c.p.lambda_initial, P, L, mode, every, C.trace.size() / 7, C.iters, C.inner,
                         C.linearizations, C.lam, C.factor, C.err, C.status, C.stop_reason, rep.rounds,
                         rep.winners.size() / 2, rep.exhausted ? " (script exhausted)" : "", R.trace.size() / 7, R.iters,
                         R.inner, R.lins, R.lam, R.factor, R.err, R.status, R.stop_reason, want.size() / 2);
            return fail("lm: the control differs from the sequential loop");
          }
          runs++;
        }
  }
  // what the cases are there to reach
  auto ref_of = [](const char* name, int nth = 0) {
    for (const LmCase& c : lm_cases())
      if (!std::strcmp(c.name, name) && nth-- == 0) return lm_reference(c);
    return RefRun();
  };
  const RefRun guard = ref_of("robust guard"), outer2 = ref_of("max_outer and max_iterations"), tryk = ref_of("try k");
  const std::pair<const char*, bool> reached[] = {
      {"robust guard", guard.trace.size() >= 21 && guard.trace[6] == 0.0 && guard.trace[5] == 0.0 && guard.trace[14 + 6] == 1.0},
      {"try k", tryk.iters == 10 && tryk.stop_reason == PGO_STOP_CONVERGED &&
                    tryk.accepted == std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8, 9, 0}},
      {"small change", ref_of("small change").stop_reason == PGO_STOP_SMALL_CHANGE},
      {"upper bound", ref_of("upper bound", 4).inner == 5 && ref_of("upper bound", 4).stop_reason == PGO_STOP_LAMBDA_BOUND},
      {"lower bound", ref_of("lower bound").lam == 1e-6},
      {"max_outer", ref_of("max_outer").stop_reason == PGO_STOP_MAX_OUTER},
      {"max_iterations", ref_of("max_iterations").status == PGO_W_MAXITER && ref_of("max_iterations").stop_reason == PGO_STOP_MAX_ITER},
      {"max_outer and max_iterations", outer2.status == PGO_W_MAXITER && outer2.stop_reason == PGO_STOP_MAX_OUTER},
      {"error_tol at entry", ref_of("error_tol at entry").lins == 0},
      {"max_iterations 0", ref_of("max_iterations 0").status == PGO_OK && ref_of("max_iterations 0").lins == 0},
      {"gn non-finite", ref_of("gn non-finite").lins == 3},
      {"gn failed solve", ref_of("gn failed solve").status == PGO_E_INDETERMINANT && ref_of("gn failed solve").stop_reason == PGO_STOP_ERROR},
      {"doubling factor", ref_of("doubling factor").factor == 10.0 * 1024.0},
  };
  for (const auto& [name, ok] : reached)
    if (!ok) {
      std::fprintf(stderr, "lm case '%s'\n", name);
      return fail("lm: a scripted case does not reach what it is there for");
    }
  std::printf("lm control: %lld runs against the sequential loop (%lld rejected tries per pass), lane rule ok\n", runs,
              rejected);
  return 0;
}

// --digest: one line per built-in case -- the case, the plan's section digests
// (pgo_plan_digest.h), the branch counters.  The planner's knobs come from the
// environment (scripts/plan_digests.py runs the set, a fresh process each).
void digest_line(const std::string& name, const pgo::CholPlan& P) {
  uint64_t d[pgo::kDigestSections];
  long long br[pgo::kBranchCounters];
  pgo::plan_digest(P, d);
  pgo::plan_branch_counters(P, br);
  std::printf("%s", name.c_str());
  for (uint64_t v : d) std::printf(" %016llx", (unsigned long long)v);
  std::printf(" |");
  for (long long v : br) std::printf(" %lld", v);
  std::printf("\n");
}

int digest_cases() {
  std::printf("# case");
  for (const char* s : pgo::kDigestSectionNames) std::printf(" %s", s);
  std::printf(" |");
  for (const char* s : pgo::kBranchCounterNames) std::printf(" %s", s);
  std::printf("\n");
  const std::pair<const char*, Pattern> graphs[] = {{"tiny5", restrict_pattern(make_pattern(40, 0, 3), 5)},
                                                    {"chain3000", make_pattern(3000, 400, 7)},
                                                    {"grid60", make_grid(60)},
                                                    {"grid100", make_grid(100)}};
  for (const auto& [gname, G] : graphs)
    for (int ordering : {pgo::kOrderNd, pgo::kOrderAmd})
      for (int size : {1, 2, 4, 8})
        for (int r = 0; r < size; r++) {
          pgo::CholPlan P;
          P.ordering = ordering;
          P.part_size = size;
          P.part_rank = r;
          pgo::chol_analyze(P, G.n, G.row_ptr, G.col);
          if (P.schedule_error) return fail("digest: panel schedule bookkeeping");
          digest_line(std::string(gname) + (ordering == pgo::kOrderNd ? "/nd/" : "/amd/") + std::to_string(size) + "r" +
                          std::to_string(r),
                      P);
        }
  {   // a given ordering: the fan's poses as numbered
    const Pattern G = make_fan(40);
    pgo::CholPlan P;
    P.order_in.resize(G.n);
    for (int k = 0; k < G.n; k++) P.order_in[k] = k;
    pgo::chol_analyze(P, G.n, G.row_ptr, G.col);
    if (P.schedule_error || check_first_writes(P)) return fail("digest: fan");
    digest_line("fan40/given/1r0", P);
  }
  for (int ordering : {pgo::kOrderNd, pgo::kOrderAmd}) {
    pgo::CholPlan P;
    if (check_append(make_edges(1500, 200, 9, 40), 1500, 1490, ordering, &P)) return 1;
    digest_line(std::string("append1490+10/") + (ordering == pgo::kOrderNd ? "nd" : "amd"), P);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--digest")) return digest_cases();
  if (check_lm()) return 1;
  if (check_structure()) return 1;
  for (int n : {1, 2, 5}) {   // graphs smaller than the planner's thread count
    const Pattern G = restrict_pattern(make_pattern(40, 0, 3), n);
    pgo::CholPlan P;
    pgo::chol_analyze(P, G.n, G.row_ptr, G.col);
    if (P.schedule_error || !pgo::chol_covers(P, G.n, G.row_ptr, G.col)) return fail("tiny graph");
  }
  // every front a look-ahead front (the skip and prep bookkeeping on small ones too), then the default
  // (PGO_SELFTEST_QUICK=1: the default only -- a second pass under another planner knob)
  const bool quick = getenv("PGO_SELFTEST_QUICK") && atoi(getenv("PGO_SELFTEST_QUICK")) == 1;
  for (const char* la : {"64", "1000000000", ""}) {
  if (quick && *la) continue;
  if (*la) setenv("PGO_LOOKAHEAD_M", la, 1);
  else unsetenv("PGO_LOOKAHEAD_M");
  for (int ordering : {pgo::kOrderNd, pgo::kOrderAmd}) {
    const Pattern G = make_pattern(3000, 400, 7);
    pgo::CholPlan P;
    P.ordering = ordering;
    pgo::chol_analyze(P, G.n, G.row_ptr, G.col);
    if (P.ns <= 0 || P.flops <= 0) return fail("analysis");
    if (P.schedule_error) return fail("panel schedule bookkeeping");
    if (!pgo::chol_covers(P, G.n, G.row_ptr, G.col)) return fail("plan does not cover its own pattern");
    if (check_assembly(P) || check_first_writes(P) || check_tiles(P) || check_sources(P, G.row_ptr, G.col)) return 1;
    for (int size : {2, 4}) {
      std::vector<double> rf;
      double top = 0;
      const auto own = pgo::partition_subtrees(P, size, &rf, &top);
      if ((int)own.size() != P.ns) return fail("partition size");
      for (int r = 0; r < size; r++) {
        pgo::CholPlan Q;
        Q.ordering = ordering;
        Q.part_size = size;
        Q.part_rank = r;
        pgo::chol_analyze(Q, G.n, G.row_ptr, G.col);
        if (Q.ns != P.ns || Q.schedule_error) return fail("partitioned plan");
        if (check_assembly(Q) || check_first_writes(Q) || check_tiles(Q)) return 1;
      }
    }
    // a loop closure inside the existing fill: same fronts, new assembly lists
    const Pattern G2 = make_pattern(3000, 400, 7, {{2, 0}});
    if (pgo::chol_covers(P, G2.n, G2.row_ptr, G2.col)) pgo::chol_assembly(P, G2.row_ptr, G2.col);
    // appended poses re-planned on a given ordering
    const Pattern G3 = make_pattern(3010, 400, 7, {{3009, 5}});
    pgo::CholPlan R;
    R.ordering = ordering;
    R.order_in.resize(G3.n);
    for (int k = 0; k < G3.n; k++) R.order_in[k] = G3.n - 1 - k;
    pgo::chol_analyze(R, G3.n, G3.row_ptr, G3.col);
    if (!pgo::chol_covers(R, G3.n, G3.row_ptr, G3.col) || R.schedule_error) return fail("given ordering");
    // appended poses: the incremental symbolic update
    if (check_append(make_edges(1500, 200, 9, 40), 1500, 1490, ordering)) return 1;
  }
  {   // a 2-D grid of poses: nested dissection gives big separator fronts (many
      // panels, kKB block boundaries, partial last panels) -- the look-ahead
      // schedule's bookkeeping is checked on them
    const Pattern G = make_grid(60);
    pgo::CholPlan P;
    pgo::chol_analyze(P, G.n, G.row_ptr, G.col);
    if (check_tiles(P) || check_first_writes(P)) return 1;
    {   // PGO_FUSE_UPDATE=0: every tile back in the assembly lists, the same Schur tasks
      setenv("PGO_FUSE_UPDATE", "0", 1);
      pgo::CholPlan Q;
      pgo::chol_analyze(Q, G.n, G.row_ptr, G.col);
      unsetenv("PGO_FUSE_UPDATE");
      if (P.fused_tiles <= 0 || P.fused_with_pairs <= 0 || Q.fused_tiles != 0 || Q.schedule_error ||
          check_first_writes(Q) || Q.ea_tasks.size() != P.ea_tasks.size() + (size_t)P.fused_tiles ||
          Q.syrk_tasks.size() != P.syrk_tasks.size() || Q.ea_pairs.size() != P.ea_pairs.size())
        return fail("grid: the fused tiles against PGO_FUSE_UPDATE=0");
    }
    for (int size : {2, 3, 4, 8})
      if (check_distributed(G, pgo::kOrderNd, size)) return 1;
    int maxw = 0;
    for (int s2 = 0; s2 < P.ns; s2++) maxw = std::max(maxw, P.w[s2]);
    if (P.schedule_error) return fail("grid: panel schedule bookkeeping");
    std::printf("grid plan (look-ahead threshold %s): %d fronts, widest %d pivot columns\n", *la ? la : "default",
                P.ns, maxw);
  }
  }
  std::printf("host selftest ok\n");
  return 0;
}
