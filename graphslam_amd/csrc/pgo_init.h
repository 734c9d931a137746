// Host side of the two-stage linear initialisation (pgo_initialize_linear,
// internal to libpgo.so): the connected components and their roots, the
// breadth-first spanning tree, the tree orientations and the integers that fix
// the 2 pi ambiguity of every factor.  Pure host code -- no HIP call, no HIP
// type -- so init_selftest.cpp drives it under ASan / UBSan.  DESIGN.md,
// "Linear initialisation".
#pragma once
#include <cstddef>
#include <vector>

namespace pgo {

// atan2(sin t, cos t): an angle as Rot2::theta() reports it
double init_wrap(double t);

struct InitTree {
  int components = 0;
  int tree_depth = 0;              // edges on the longest root-to-vertex tree path
  long long wraps = 0;             // sum |k_edge|
  int free_vertex = -1;            // first vertex of a component without a prior (-1: none)
  std::vector<int> parent;         // tree parent per vertex, -1 for a root
  std::vector<double> theta;       // tree orientation per vertex (not wrapped)
  std::vector<double> delta;       // init_wrap(z_theta) per between factor
  std::vector<long long> k_edge;   // rint((theta[j] - theta[i] - delta) / 2 pi) per between factor
  std::vector<long long> k_prior;  // rint((theta[v] - init_wrap(prior theta)) / 2 pi) per prior
};

// n vertices; ne between factors (i, j) = eij[2 e], eij[2 e + 1] with measured
// angle ez_theta[e * ez_stride]; np priors on vertices pv[q] with angle
// pz_theta[q * pz_stride]; everything in insertion order.
//
// Per component the root is its first vertex (insertion order) that carries a
// prior, with theta[root] = init_wrap(angle of that vertex's first prior).  The
// search is a FIFO breadth-first one; a vertex scans its between factors in
// insertion order, whichever end it is: a newly reached v over e = (i, j) gets
// theta[u] + delta_e from u = i and theta[u] - delta_e from u = j (one add or
// subtract: a numpy twin reproduces it bitwise).
//
// False with free_vertex set when a component has no prior (nothing else is
// then meaningful); true otherwise.
bool init_tree(int n, size_t ne, const int* eij, const double* ez_theta, size_t ez_stride, size_t np, const int* pv,
               const double* pz_theta, size_t pz_stride, InitTree* out);

}  // namespace pgo
