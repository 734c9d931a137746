// Stand-alone driver of the linear initialisation's host module (pgo_init.cpp)
// for the AddressSanitizer + UndefinedBehaviorSanitizer build (make asan-init):
// designed graphs with known trees and 2 pi integers, and seeded random graphs
// against a plain O(V E) restatement of the search.  Host only, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#include "pgo_init.h"

namespace {

constexpr double kPi = 3.14159265358979323846, kTwoPi = 2.0 * kPi;
int g_fail = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
      g_fail++;                                                            \
    }                                                                      \
  } while (0)

struct Graph {
  int n = 0;
  std::vector<int> eij;      // 2 per between factor
  std::vector<double> ez;    // measured angle per between factor
  std::vector<int> pv;
  std::vector<double> pz;
  void edge(int i, int j, double th) {
    eij.push_back(i);
    eij.push_back(j);
    ez.push_back(th);
  }
  void prior(int v, double th) {
    pv.push_back(v);
    pz.push_back(th);
  }
  bool tree(pgo::InitTree* T) const {
    return pgo::init_tree(n, ez.size(), eij.data(), ez.data(), 1, pv.size(), pv.data(), pz.data(), 1, T);
  }
};

bool near(double a, double b, double tol = 1e-12) { return std::fabs(a - b) <= tol; }

// the definition again, the slow way: every popped vertex scans all factors
void reference_tree(const Graph& g, std::vector<int>& parent, std::vector<double>& theta, int* depth_out) {
  const int ne = (int)g.ez.size();
  parent.assign(g.n, -1);
  theta.assign(g.n, 0.0);
  std::vector<int> depth(g.n, -1), comp(g.n, -1);
  int nc = 0;
  for (int s = 0; s < g.n; s++) {   // components by flooding
    if (comp[s] >= 0) continue;
    comp[s] = nc;
    for (bool grew = true; grew;) {
      grew = false;
      for (int e = 0; e < ne; e++) {
        const int i = g.eij[2 * e], j = g.eij[2 * e + 1];
        if ((comp[i] == nc) != (comp[j] == nc)) {
          comp[i] = comp[j] = nc;
          grew = true;
        }
      }
    }
    nc++;
  }
  *depth_out = 0;
  for (int c = 0; c < nc; c++) {
    int root = -1;
    for (int v = 0; v < g.n && root < 0; v++) {
      if (comp[v] != c) continue;
      for (size_t q = 0; q < g.pv.size(); q++)
        if (g.pv[q] == v) {
          root = v;
          theta[v] = pgo::init_wrap(g.pz[q]);
          break;
        }
    }
    if (root < 0) continue;
    std::deque<int> fifo{root};
    depth[root] = 0;
    while (!fifo.empty()) {
      const int u = fifo.front();
      fifo.pop_front();
      for (int e = 0; e < ne; e++) {
        const int i = g.eij[2 * e], j = g.eij[2 * e + 1];
        if (i != u && j != u) continue;
        const int v = i == u ? j : i;
        if (depth[v] >= 0) continue;
        const double dl = pgo::init_wrap(g.ez[e]);
        depth[v] = depth[u] + 1;
        if (depth[v] > *depth_out) *depth_out = depth[v];
        parent[v] = u;
        theta[v] = i == u ? theta[u] + dl : theta[u] - dl;
        fifo.push_back(v);
      }
    }
  }
}

void check_chain() {
  Graph g;
  g.n = 4;
  g.edge(0, 1, 0.3);
  g.edge(1, 2, -0.2);
  g.edge(2, 3, 0.5);
  g.prior(0, 0.1);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  CHECK(T.components == 1 && T.tree_depth == 3 && T.wraps == 0 && T.free_vertex == -1);
  CHECK(T.parent == std::vector<int>({-1, 0, 1, 2}));
  CHECK(T.theta[0] == pgo::init_wrap(0.1));
  CHECK(T.theta[1] == T.theta[0] + pgo::init_wrap(0.3));
  CHECK(T.theta[3] == (T.theta[1] + pgo::init_wrap(-0.2)) + pgo::init_wrap(0.5));
  for (long long k : T.k_edge) CHECK(k == 0);
  CHECK(T.k_prior.size() == 1 && T.k_prior[0] == 0);
  // the root in the middle, one factor inserted (later, earlier): it is walked backwards
  Graph h;
  h.n = 4;
  h.edge(0, 1, 0.3);
  h.edge(2, 1, 0.2);     // (later, earlier)
  h.edge(2, 3, 0.5);
  h.prior(2, 7.0);       // not wrapped on entry
  h.prior(2, 0.0);       // a second prior of the root: not the tree's angle, k from the tree
  h.prior(3, 1.0);       // a later vertex's prior does not move the root
  CHECK(h.tree(&T));
  CHECK(T.parent == std::vector<int>({1, 2, -1, 2}) && T.tree_depth == 2);
  CHECK(T.theta[2] == pgo::init_wrap(7.0));
  CHECK(T.theta[1] == T.theta[2] + pgo::init_wrap(0.2));
  CHECK(T.theta[0] == T.theta[1] - pgo::init_wrap(0.3));
  CHECK(T.theta[3] == T.theta[2] + pgo::init_wrap(0.5));
  CHECK(T.k_prior[0] == 0 && T.k_prior[1] == 0 && T.k_prior[2] == 0);
  // single vertex, and no vertex at all
  Graph s;
  s.n = 1;
  s.prior(0, -4.0);
  CHECK(s.tree(&T) && T.components == 1 && T.tree_depth == 0 && T.parent[0] == -1);
  CHECK(T.theta[0] == pgo::init_wrap(-4.0));
  Graph z;
  CHECK(z.tree(&T) && T.components == 0 && T.parent.empty());
}

void check_square_full_turn() {
  Graph g;
  g.n = 4;
  for (int k = 0; k < 4; k++) g.edge(k, (k + 1) % 4, kPi / 2);   // the turns sum to 2 pi
  g.prior(0, 0.0);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  // 0 scans (0,1) then (3,0); 1 reaches 2 before 3 could
  CHECK(T.parent == std::vector<int>({-1, 0, 1, 0}) && T.tree_depth == 2);
  CHECK(near(T.theta[1], kPi / 2) && near(T.theta[3], -kPi / 2) && near(T.theta[2], kPi));
  CHECK(T.k_edge == std::vector<long long>({0, 0, -1, 0}) && T.wraps == 1);
  // a ring of 8 whose turns sum to three full turns: the one non-tree factor carries all three
  Graph r;
  r.n = 8;
  for (int k = 0; k < 8; k++) r.edge(k, (k + 1) % 8, 3 * kPi / 4);
  r.prior(0, 0.0);
  CHECK(r.tree(&T));
  CHECK(T.parent == std::vector<int>({-1, 0, 1, 2, 3, 6, 7, 0}) && T.tree_depth == 4);
  CHECK(T.k_edge == std::vector<long long>({0, 0, 0, 0, -3, 0, 0, 0}) && T.wraps == 3);
}

void check_star() {
  Graph g;
  const int spokes = 9;
  g.n = spokes + 1;
  for (int k = 1; k <= spokes; k++) {
    if (k & 1) g.edge(0, k, 0.1 * k);
    else g.edge(k, 0, 0.1 * k);   // the hub as k2
  }
  g.prior(0, 0.25);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  CHECK(T.tree_depth == 1 && T.wraps == 0);
  for (int k = 1; k <= spokes; k++) {
    CHECK(T.parent[k] == 0);
    const double d = pgo::init_wrap(0.1 * k);
    CHECK(T.theta[k] == ((k & 1) ? T.theta[0] + d : T.theta[0] - d));
  }
}

void check_components() {
  Graph g;
  g.n = 6;
  g.edge(0, 1, 0.1);
  g.edge(3, 4, 0.2);
  g.edge(1, 2, 0.3);
  g.edge(5, 4, 0.4);
  g.prior(4, 1.0);
  g.prior(1, -1.0);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  CHECK(T.components == 2 && T.tree_depth == 1);
  CHECK(T.parent == std::vector<int>({1, -1, 1, 4, -1, 4}));
  CHECK(T.theta[0] == pgo::init_wrap(-1.0) - pgo::init_wrap(0.1));
  CHECK(T.theta[5] == pgo::init_wrap(1.0) - pgo::init_wrap(0.4));
  // the second component loses its prior
  g.pv.erase(g.pv.begin());
  g.pz.erase(g.pz.begin());
  CHECK(!g.tree(&T) && T.free_vertex == 3);
  // an isolated vertex without a prior
  Graph h;
  h.n = 2;
  h.prior(0, 0.0);
  CHECK(!h.tree(&T) && T.free_vertex == 1);
  h.prior(1, 0.5);
  CHECK(h.tree(&T) && T.components == 2);
}

void check_duplicates() {
  Graph g;
  g.n = 3;
  g.edge(0, 1, 0.4);
  g.edge(0, 1, 0.4 + 3 * kTwoPi);   // a parallel duplicate, three turns on: the same delta
  g.edge(1, 0, -0.4);               // and one the other way round
  g.edge(1, 2, 3.0);
  g.edge(1, 2, -3.0);               // an inconsistent duplicate: 6 rad apart, nearest turn is one
  g.prior(0, 0.0);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  CHECK(T.parent == std::vector<int>({-1, 0, 1}));
  CHECK(near(T.delta[1], 0.4, 1e-12));
  CHECK(T.k_edge == std::vector<long long>({0, 0, 0, 0, 1}) && T.wraps == 1);
}

// Measurements taken from true unwrapped angles, each shifted by whole turns:
// every k is forced -- with it the factor's residual vanishes, any other
// integer leaves a whole turn -- and the tree reproduces the true angles up to
// whole turns and one constant per component.  The search itself against the
// slow restatement.
void check_consistent_random() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> ang(-20.0, 20.0);
  for (int trial = 0; trial < 20; trial++) {
    Graph g;
    g.n = 30 + 7 * trial;
    std::vector<double> phi(g.n);
    for (double& p : phi) p = ang(rng);
    auto measure = [&](int i, int j) { g.edge(i, j, phi[j] - phi[i] + kTwoPi * (double)((int)(rng() % 7) - 3)); };
    const int half = g.n / 2;   // two components: [0, half) and [half, n)
    for (int v = 1; v < g.n; v++) {
      if (v == half) continue;
      const int lo = v < half ? 0 : half;
      const int u = lo + (int)(rng() % (unsigned)(v - lo));
      if (rng() & 1) measure(u, v);
      else measure(v, u);
    }
    for (int x = 0; x < g.n; x++) {   // closures inside each component, duplicates allowed
      const int lo = (rng() & 1) ? 0 : half, sz = lo ? g.n - half : half;
      const int a = lo + (int)(rng() % (unsigned)sz), b = lo + (int)(rng() % (unsigned)sz);
      if (a != b) measure(a, b);
    }
    const int r0 = (int)(rng() % (unsigned)half), r1 = half + (int)(rng() % (unsigned)(g.n - half));
    g.prior(r1, phi[r1]);
    g.prior(r0, phi[r0] + kTwoPi);
    if (r0 + 1 < half) g.prior(r0 + 1, phi[r0 + 1] - 2 * kTwoPi);   // a second prior in the component
    pgo::InitTree T;
    CHECK(g.tree(&T));
    CHECK(T.components == 2);
    std::vector<int> parent;
    std::vector<double> theta;
    int depth = 0;
    reference_tree(g, parent, theta, &depth);
    CHECK(parent == T.parent && theta == T.theta && depth == T.tree_depth);
    long long wraps = 0;
    for (size_t e = 0; e < g.ez.size(); e++) {
      const int i = g.eij[2 * e], j = g.eij[2 * e + 1];
      CHECK(near(T.theta[j] - T.theta[i] - T.delta[e] - kTwoPi * (double)T.k_edge[e], 0.0, 1e-9));
      if (T.parent[j] == i || T.parent[i] == j) {
        // (a duplicate of a tree factor is consistent with it: 0 as well)
        CHECK(T.k_edge[e] == 0);
      }
      wraps += std::llabs(T.k_edge[e]);
    }
    CHECK(wraps == T.wraps);
    for (size_t q = 0; q < g.pv.size(); q++)
      CHECK(near(T.theta[g.pv[q]] - pgo::init_wrap(g.pz[q]) - kTwoPi * (double)T.k_prior[q], 0.0, 1e-9));
    for (int v = 0; v < g.n; v++) {   // the true angles up to whole turns and one constant per component
      const int root = v < half ? r0 : r1;
      const double off = (T.theta[v] - phi[v]) - (T.theta[root] - phi[root]);
      CHECK(near(off, kTwoPi * std::round(off / kTwoPi), 1e-9));
    }
  }
}

// A chain long enough for the measured angles to be wrapped on several host
// threads: every element is what one thread computes.
void check_long_chain() {
  Graph g;
  g.n = 100001;
  for (int k = 0; k + 1 < g.n; k++) g.edge(k, k + 1, 0.37 * k - 900.0);
  g.prior(0, 0.5);
  pgo::InitTree T;
  CHECK(g.tree(&T));
  CHECK(T.components == 1 && T.tree_depth == g.n - 1);
  double th = pgo::init_wrap(0.5);
  int bad = T.theta[0] != th;
  for (int k = 0; k + 1 < g.n; k++) {
    const double d = pgo::init_wrap(0.37 * k - 900.0);
    th += d;
    bad += T.delta[k] != d || T.parent[k + 1] != k || T.theta[k + 1] != th || T.k_edge[k] != 0;
  }
  CHECK(bad == 0);
}

}  // namespace

int main() {
  check_long_chain();
  check_chain();
  check_square_full_turn();
  check_star();
  check_components();
  check_duplicates();
  check_consistent_random();
  if (g_fail) {
    std::printf("init selftest FAILED (%d)\n", g_fail);
    return 1;
  }
  std::printf("init selftest ok\n");
  return 0;
}
