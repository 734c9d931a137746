// Host side of the graph structure the device holds (internal to libpgo.so):
// device factor order, block-CSR rows, priors by vertex, the Cholesky-mode sweep
// structure and the owner bits of the slot codes.  Pure host code -- no HIP
// runtime call, only the HIP vector types -- so host_selftest.cpp drives it
// under ASan / UBSan.  pgo_api.cpp turns what build / append / bind report into
// allocations and copies.  DESIGN.md, "The structure module".
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pgo_chol.h"

namespace pgo {

// fn(begin, end) over contiguous chunks of [0, n) on the planner's host threads
// (the live re-solve's per-registration host work; chunk results independent)
template <class F>
void host_parallel(int n, F&& fn) {
  static const int hw = (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  const int nth = std::max(1, std::min(hw, n / 16384));
  plan_parallel(nth, [&](int t) { fn((int)((long long)n * t / nth), (int)((long long)n * (t + 1) / nth)); });
}

// PGO_PLAN_TIMING: phase times of the plan / append paths on stderr
struct PhaseTimer {
  const char* who;
  bool on = getenv("PGO_PLAN_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  explicit PhaseTimer(const char* w) : who(w) {}
  void operator()(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "%s %-14s %8.2f ms\n", who, what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// Measurements and information of `count` factors or priors in device layout:
// out k reads source order[k]; (x, y, theta) -> (x, y, cos theta, sin theta)
// (Pose2 stores Rot2(c, s)), the six doubles of Omega's upper triangle -> three double2
void pack_measurements(const double* z3, const double* om6, const int* order, size_t count, double4* z, double2* om);

// What an in-place append changed (GraphStructure::append): the uploader copies
// the new factors [ne_old, ne), row_ptr / the slot arrays from row r0 / slot k0,
// erow from row x0, s1_ptr from row y0, Dc of dc_rows and of the new rows, and
// prior_ptr of the new rows; s1pos, brow (and s1fac) whole.
struct StructureDelta {
  int n_old = 0, ne_old = 0;
  int r0 = 0, k0 = 0;             // first row with a new slot (<= n_old), its first slot
  int x0 = 0, y0 = 0;             // first rows of erow / s1_ptr that change
  std::vector<int> dc_rows;       // old rows whose Dc changed, sorted, unique
};

struct SlotRange {
  int begin = 0, end = 0;
};

// Slot codes are (device factor << 2) | (owner << 1) | side; every factor has a
// side-0 slot in row ei and a side-1 slot in row ej.
//
// Owner bits.  codes() is the host mirror of the device slot_edge: what the last
// upload of a slot range put there (the uploader copies exactly the ranges
// build / append / bind / unbind return).  Pre-plan, side 0 owns; bind() gives
// the owner bit to the slot in the lower triangle of the plan's permuted matrix
// (iperm[row] > iperm[column]).  The state, in one place:
//
//   slot_codes()  kPrePlan  every slot pre-plan (after build, after unbind)
//                 kBound    bound by the last bind; slots of rows >= bind_row0
//                           may be pre-plan again (an append whose first changed
//                           row is row 0) -- each factor still has one owner slot
//                 kMixed    as kBound, and an append left rows < bind_row0 bound
//                           while later rows may have been reset to pre-plan
//                           whole: a factor across the two halves can have two
//                           owner slots or none.  A PCG linearisation (it counts
//                           owner slots) needs unbind() first; the Cholesky path
//                           always binds before it linearises.
//   bind_row0     rows >= bind_row0 need their bits (re)computed by the next
//                 bind: n after a bind, the first changed row after an append,
//                 0 after build / unbind / order_changed
//   mirror_bound  every slot but new_slots carries the last bind's bit (new_slots:
//                 the slots of one append, pre-plan).  With bind_row0 > 0 the next
//                 bind sets only those.  A second append before a bind voids the
//                 list (slots move): mirror_bound off, the tail from its first
//                 changed slot reset to pre-plan, bind recomputes from bind_row0.
//
// Only build / append / bind / unbind / order_changed write this state.
class GraphStructure {
 public:
  enum SlotCodes { kPrePlan, kBound, kMixed };

  int n = 0;
  std::vector<int2> eij;           // factor endpoints, device order (sorted by (ei, ej), stable)
  std::vector<int> dorder;         // device factor -> user factor index
  std::vector<int> pv;             // prior -> vertex (user order)
  std::vector<int> prior_ptr, porder;   // priors CSR by vertex: position -> user prior index
  std::vector<int> row_ptr, slot_col;   // block-CSR rows, each sorted by (column, code)
  std::vector<int> edge_slot0;     // user factor -> its side-0 slot
  // Cholesky-mode sweep structure: the side-0 factors of row i are the device
  // range [erow[i], erow[i+1]); the side-1 factors of row j take positions
  // s1_ptr[j].. in device order (s1pos; s1fac its inverse, robust graphs only).
  // Dc[6 j..] is the sum of Omega over row j's side-1 factors, in device order.
  std::vector<int> erow, s1_ptr, s1pos, s1fac;
  std::vector<double> Dc;
  // k_linearize_own blocks: whole rows, greedily packed to <= kThreads side-0
  // factors and <= kThreads rows (a row with more factors is a block alone)
  std::vector<int> brow;
  int G = 4, G1 = 4;               // lanes per row: smallest power of two >= mean degree, in [4, 32]
  bool gauge_free = false;         // some connected component has no prior

  int ne() const { return (int)eij.size(); }
  int nslots() const { return (int)slot_code_.size(); }
  const std::vector<int>& codes() const { return slot_code_; }
  const std::vector<unsigned char>& eside() const { return eside_; }   // owner side per device factor (bind)
  SlotCodes slot_codes() const { return state_; }
  int bind_row0() const { return bind_row0_; }
  bool same_component(int a, int b) { return find(a) == find(b); }

  // Everything from scratch: `eij_user` the resolved endpoints and `eom` the
  // information (6 per factor) in user order, `pv` the priors' vertices.
  void build(int n, const std::vector<int2>& eij_user, std::vector<int> pv, const double* eom, bool robust);
  // Room for in-place appends up to these sizes (as the device arrays have).
  void reserve(size_t cap_n, size_t cap_ne);
  // Vertices [n, n_new) and the user-order factors [ne(), ne() + new_ij.size())
  // appended in place; leaves exactly what build() of the grown graph leaves
  // (owner state aside).  False, with nothing changed: nothing new, no factor
  // yet, or a new factor that sorts before the last old one in device order --
  // the caller rebuilds.  `eom` as for build (the whole user-order array).
  bool append(int n_new, const std::vector<int2>& new_ij, const double* eom, bool robust, StructureDelta* delta,
              PhaseTimer* phase = nullptr);
  // Owner bits for the plan with this inverse permutation; the slot range to upload (with eside()).
  SlotRange bind(const std::vector<int>& iperm);
  // Pre-plan codes whole, if a PCG linearisation needs them (kMixed): true -> upload codes() whole.
  bool unbind();
  // The plan's order changed: the next bind recomputes every bit.
  void order_changed() { bind_row0_ = 0; }

 private:
  int find(int x);
  void gauge_scan();               // gauge_free from uf_ and pv
  void row_blocks();               // brow, G, G1 from erow

  std::vector<int> slot_code_;
  std::vector<unsigned char> eside_;
  SlotCodes state_ = kPrePlan;
  int bind_row0_ = 0;
  bool mirror_bound_ = false;
  std::vector<int> new_slots_;
  std::vector<int> uf_;            // union-find parents over the vertices (gauge check)
  std::vector<int> spare_rp_, spare_sc_, spare_se_;   // the previous block-CSR arrays, reused by the next append
};

}  // namespace pgo
