// The spanning tree and the 2 pi integers of the linear initialisation
// (pgo_init.h).  Host only.
#include "pgo_init.h"

#include <algorithm>
#include <cmath>
#include <thread>

namespace pgo {

namespace {
constexpr double kTwoPi = 6.283185307179586476925286766559;
}

double init_wrap(double t) { return std::atan2(std::sin(t), std::cos(t)); }

bool init_tree(int n, size_t ne, const int* eij, const double* ez_theta, size_t ez_stride, size_t np, const int* pv,
               const double* pz_theta, size_t pz_stride, InitTree* out) {
  InitTree& T = *out;
  T = InitTree();
  T.parent.assign(n, -1);
  T.theta.assign(n, 0.0);
  T.delta.resize(ne);
  T.k_edge.assign(ne, 0);
  T.k_prior.assign(np, 0);
  // three libm calls per factor -- most of the host time on a large graph --
  // over a few host threads (each element on its own: the same bits)
  {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nth = std::max<size_t>(1, std::min<size_t>({16, hw, ne / 32768}));
    auto chunk = [&](size_t t) {
      for (size_t e = ne * t / nth; e < ne * (t + 1) / nth; e++) T.delta[e] = init_wrap(ez_theta[e * ez_stride]);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nth; t++) th.emplace_back(chunk, t);
    chunk(0);
    for (std::thread& x : th) x.join();
  }
  // the between factors of every vertex, insertion order, either end: the
  // factor (<< 1 | this vertex is its first end) and the other end (ne < 2^31)
  struct Adj {
    unsigned code;
    int v;
  };
  std::vector<size_t> adj_ptr((size_t)n + 1, 0);
  for (size_t e = 0; e < ne; e++) {
    adj_ptr[eij[2 * e] + 1]++;
    adj_ptr[eij[2 * e + 1] + 1]++;
  }
  for (int v = 0; v < n; v++) adj_ptr[v + 1] += adj_ptr[v];
  std::vector<Adj> adj(2 * ne);
  {
    std::vector<size_t> fill(adj_ptr.begin(), adj_ptr.end() - 1);
    for (size_t e = 0; e < ne; e++) {
      const int i = eij[2 * e], j = eij[2 * e + 1];
      adj[fill[i]++] = {(unsigned)(e << 1) | 1u, j};
      adj[fill[j]++] = {(unsigned)(e << 1), i};
    }
  }
  std::vector<long long> first_prior(n, -1);
  for (size_t q = 0; q < np; q++)
    if (first_prior[pv[q]] < 0) first_prior[pv[q]] = (long long)q;
  // Breadth first from every vertex with a prior that no earlier root reached:
  // in insertion order that is the first such vertex of its component.
  std::vector<int> depth(n, -1), queue;
  queue.reserve(n);
  for (int r = 0; r < n; r++) {
    if (first_prior[r] < 0 || depth[r] >= 0) continue;
    T.components++;
    T.theta[r] = init_wrap(pz_theta[(size_t)first_prior[r] * pz_stride]);
    depth[r] = 0;
    queue.clear();
    queue.push_back(r);
    for (size_t h = 0; h < queue.size(); h++) {
      const int u = queue[h];
      for (size_t a = adj_ptr[u]; a < adj_ptr[u + 1]; a++) {
        const int v = adj[a].v;
        if (depth[v] >= 0) continue;
        const double dl = T.delta[adj[a].code >> 1];
        depth[v] = depth[u] + 1;
        T.tree_depth = std::max(T.tree_depth, depth[v]);
        T.parent[v] = u;
        T.theta[v] = (adj[a].code & 1) ? T.theta[u] + dl : T.theta[u] - dl;
        queue.push_back(v);
      }
    }
  }
  // a vertex no root reached: its component has no prior
  for (int v = 0; v < n; v++)
    if (depth[v] < 0) {
      T.free_vertex = v;
      return false;
    }
  for (size_t e = 0; e < ne; e++) {
    const double d = T.theta[eij[2 * e + 1]] - T.theta[eij[2 * e]] - T.delta[e];
    T.k_edge[e] = std::llrint(d / kTwoPi);
    T.wraps += T.k_edge[e] < 0 ? -T.k_edge[e] : T.k_edge[e];
  }
  for (size_t q = 0; q < np; q++)
    T.k_prior[q] = std::llrint((T.theta[pv[q]] - init_wrap(pz_theta[q * pz_stride])) / kTwoPi);
  return true;
}

}  // namespace pgo
