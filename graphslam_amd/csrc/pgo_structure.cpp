// GraphStructure: see pgo_structure.h.
#include "pgo_structure.h"

#include <cmath>

#include "pgo_device.h"

namespace pgo {

namespace {

bool before(const int2& a, const int2& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; }

// device order of the factors: sorted by (ei, ej), so that the side-0 slots
// of a row read consecutive factors (coalesced factor loads in k_linearize)
std::vector<int> device_order(const std::vector<int2>& ij) {
  std::vector<int> o(ij.size());
  for (size_t q = 0; q < o.size(); q++) o[q] = (int)q;
  std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return before(ij[a], ij[b]); });
  return o;
}

int lanes_for(double mean) {
  int G = 4;
  while (G < 32 && G < mean) G *= 2;
  return G;
}

// side 0 owns until a Cholesky plan re-assigns it
int pre_plan(int code) { return (code & ~2) | ((code & 1) ? 0 : 2); }

}  // namespace

void pack_measurements(const double* z3, const double* om6, const int* order, size_t count, double4* z, double2* om) {
  for (size_t k = 0; k < count; k++) {
    const size_t e = (size_t)order[k];
    const double th = z3[3 * e + 2];
    z[k] = make_double4(z3[3 * e], z3[3 * e + 1], std::cos(th), std::sin(th));
    const double* o = &om6[6 * e];
    om[3 * k] = make_double2(o[0], o[1]);
    om[3 * k + 1] = make_double2(o[2], o[3]);
    om[3 * k + 2] = make_double2(o[4], o[5]);
  }
}

int GraphStructure::find(int x) {
  while (uf_[x] != x) x = uf_[x] = uf_[uf_[x]];
  return x;
}

// connected components without a prior leave H singular (3-dof gauge):
// GTSAM's Cholesky throws IndeterminantLinearSystemException there (GN);
// LM's damping keeps it solvable.
void GraphStructure::gauge_scan() {
  std::vector<char> anchored(n, 0);
  for (int v : pv) anchored[find(v)] = 1;
  gauge_free = false;
  for (int i = 0; i < n; i++)
    if (!anchored[find(i)]) gauge_free = true;
}

void GraphStructure::row_blocks() {
  brow.assign(1, 0);
  for (int r = 0; r < n;) {
    int r1 = r + 1;
    while (r1 < n && r1 - r < kThreads && erow[r1 + 1] - erow[r] <= kThreads) r1++;
    brow.push_back(r1);
    r = r1;
  }
  G = lanes_for(n ? 2.0 * ne() / n : 0.0);
  G1 = lanes_for(n ? (double)ne() / n : 0.0);
}

void GraphStructure::build(int n_, const std::vector<int2>& eij_user, std::vector<int> pv_, const double* eom,
                           bool robust) {
  n = n_;
  const int ne = (int)eij_user.size(), np = (int)pv_.size(), ns = 2 * ne;
  pv = std::move(pv_);
  dorder = device_order(eij_user);
  eij.resize(ne);
  for (int e = 0; e < ne; e++) eij[e] = eij_user[dorder[e]];
  // block-CSR rows: every factor owns a slot in row ei (side 0) and row ej (side 1)
  row_ptr.assign(n + 1, 0);
  for (int e = 0; e < ne; e++) {
    row_ptr[eij[e].x + 1]++;
    row_ptr[eij[e].y + 1]++;
  }
  for (int i = 0; i < n; i++) row_ptr[i + 1] += row_ptr[i];
  slot_code_.resize(ns);
  slot_col.resize(ns);
  {
    std::vector<int> fillp(row_ptr.begin(), row_ptr.end() - 1);
    for (int e = 0; e < ne; e++) {
      const int s0 = fillp[eij[e].x]++;
      slot_code_[s0] = (e << 2) | 2;
      slot_col[s0] = eij[e].y;
      const int s1 = fillp[eij[e].y]++;
      slot_code_[s1] = (e << 2) | 1;
      slot_col[s1] = eij[e].x;
    }
  }
  // order each row by column (locality of the x gathers), then code
  std::vector<std::pair<int, int>> tmp;
  for (int i = 0; i < n; i++) {
    const int b = row_ptr[i], en = row_ptr[i + 1];
    if (en - b < 2) continue;
    tmp.clear();
    for (int k = b; k < en; k++) tmp.emplace_back(slot_col[k], slot_code_[k]);
    std::sort(tmp.begin(), tmp.end());
    for (int k = b; k < en; k++) {
      slot_col[k] = tmp[k - b].first;
      slot_code_[k] = tmp[k - b].second;
    }
  }
  edge_slot0.assign(ne, -1);
  for (int k = 0; k < ns; k++)
    if ((slot_code_[k] & 1) == 0) edge_slot0[dorder[slot_code_[k] >> 2]] = k;
  uf_.resize(n);
  for (int i = 0; i < n; i++) uf_[i] = i;
  for (int e = 0; e < ne; e++) {
    const int a = find(eij[e].x), b = find(eij[e].y);
    if (a != b) uf_[a] = b;
  }
  gauge_scan();
  // priors CSR by vertex
  prior_ptr.assign(n + 1, 0);
  for (int q = 0; q < np; q++) prior_ptr[pv[q] + 1]++;
  for (int i = 0; i < n; i++) prior_ptr[i + 1] += prior_ptr[i];
  porder.resize(np);
  {
    std::vector<int> f(prior_ptr.begin(), prior_ptr.end() - 1);
    for (int q = 0; q < np; q++) porder[f[pv[q]]++] = q;
  }
  // the sweep structure
  erow.assign(n + 1, 0);
  s1_ptr.assign(n + 1, 0);
  s1pos.resize(ne);
  Dc.assign(6 * (size_t)n, 0.0);
  for (int e = 0; e < ne; e++) {
    erow[eij[e].x + 1]++;
    s1_ptr[eij[e].y + 1]++;
  }
  for (int i = 0; i < n; i++) {
    erow[i + 1] += erow[i];
    s1_ptr[i + 1] += s1_ptr[i];
  }
  {
    std::vector<int> f(s1_ptr.begin(), s1_ptr.end() - 1);
    for (int e = 0; e < ne; e++) {
      const int j = eij[e].y;
      s1pos[e] = f[j]++;
      const double* o = &eom[6 * (size_t)dorder[e]];
      for (int q = 0; q < 6; q++) Dc[6 * (size_t)j + q] += o[q];
    }
  }
  s1fac.clear();
  if (robust) {
    s1fac.resize(ne);
    for (int e = 0; e < ne; e++) s1fac[s1pos[e]] = e;
  }
  row_blocks();
  eside_.clear();
  state_ = kPrePlan;
  bind_row0_ = 0;
  mirror_bound_ = false;
  new_slots_.clear();
}

void GraphStructure::reserve(size_t cap_n, size_t cap_ne) {
  const size_t rn = cap_n + 1, re = cap_ne, rs = 2 * cap_ne;
  eij.reserve(re);
  dorder.reserve(re);
  erow.reserve(rn);
  s1_ptr.reserve(rn);
  s1pos.reserve(re);
  prior_ptr.reserve(rn);
  uf_.reserve(rn);
  edge_slot0.reserve(re);
  row_ptr.reserve(rn);
  slot_col.reserve(rs);
  slot_code_.reserve(rs);
  Dc.reserve(6 * rn);
  eside_.reserve(re);
}

bool GraphStructure::append(int n_new, const std::vector<int2>& new_ij, const double* eom, bool robust,
                            StructureDelta* delta, PhaseTimer* phase) {
  const int n_old = n, ne_old = ne(), ne_new = ne_old + (int)new_ij.size();
  if (n_new < n_old || ne_old == 0 || (n_new == n_old && new_ij.empty()) || (int)erow.size() != n_old + 1 ||
      (int)s1pos.size() != ne_old)
    return false;
  // the new factors in device order
  const std::vector<int> o = device_order(new_ij);
  std::vector<int> nd(o.size());
  std::vector<int2> nij(o.size());
  for (size_t q = 0; q < o.size(); q++) {
    nd[q] = ne_old + o[q];
    nij[q] = new_ij[o[q]];
  }
  if (!nij.empty() && before(nij.front(), eij.back())) return false;   // not an append in device order
  if (phase) (*phase)("resolve");
  n = n_new;
  eij.insert(eij.end(), nij.begin(), nij.end());
  dorder.insert(dorder.end(), nd.begin(), nd.end());
  std::vector<int> add(n, 0);
  for (const int2& ij : nij) {
    add[ij.x]++;
    add[ij.y]++;
  }
  const int ns = 2 * ne_new;
  // (into the previous append's arrays: their pages are mapped already;
  // every element is written below)
  std::vector<int>& rp = spare_rp_;
  std::vector<int>& sc = spare_sc_;
  std::vector<int>& se = spare_se_;
  rp.resize(n + 1);
  sc.resize(ns);
  se.resize(ns);
  rp[0] = 0;
  for (int i = 0; i < n; i++) rp[i + 1] = rp[i] + (i < n_old ? row_ptr[i + 1] - row_ptr[i] : 0) + add[i];
  // the new slots (row, column, code), by row then (column, code): merged into
  // the old rows (sorted by (column, code); two slots of a row to one column
  // belong to different factors -- no self-edges -- so the factor index
  // decides, never the owner bits the old codes may carry)
  std::vector<int3> extra;
  extra.reserve(2 * nij.size());
  for (size_t q = 0; q < nij.size(); q++) {
    const int de = ne_old + (int)q;
    extra.push_back(make_int3(nij[q].x, nij[q].y, (de << 2) | 2));
    extra.push_back(make_int3(nij[q].y, nij[q].x, (de << 2) | 1));
  }
  std::sort(extra.begin(), extra.end(), [](const int3& a, const int3& b) {
    return a.x != b.x ? a.x < b.x : a.y != b.y ? a.y < b.y : a.z < b.z;
  });
  // the old slots keep their codes (the merge keeps their order); with every one
  // of them bound the new ones are listed for bind, else bind recomputes rows
  if (!new_slots_.empty()) mirror_bound_ = false;   // (an earlier append not bound yet: its list is stale now)
  if (!mirror_bound_) new_slots_.clear();
  int prev = 0;   // rows [prev, r) copied whole
  auto copy_rows = [&](int r) {
    if (prev >= n_old) return;
    const int b = row_ptr[prev], e0 = row_ptr[std::min(r, n_old)];
    if (e0 > b) {
      std::copy(slot_col.begin() + b, slot_col.begin() + e0, sc.begin() + rp[prev]);
      std::copy(slot_code_.begin() + b, slot_code_.begin() + e0, se.begin() + rp[prev]);
    }
  };
  for (size_t q = 0; q < extra.size();) {
    const int i = extra[q].x;
    size_t q1 = q;
    while (q1 < extra.size() && extra[q1].x == i) q1++;
    copy_rows(i);
    const int b = i < n_old ? row_ptr[i] : 0, e0 = i < n_old ? row_ptr[i + 1] : 0;
    int w = rp[i], k = b;
    for (size_t t = q; t < q1; t++) {   // merge: old slots to the same column stay first (earlier factors)
      while (k < e0 && slot_col[k] <= extra[t].y) {
        sc[w] = slot_col[k];
        se[w++] = slot_code_[k++];
      }
      if (mirror_bound_) new_slots_.push_back(w);
      sc[w] = extra[t].y;
      se[w++] = extra[t].z;
    }
    for (; k < e0; k++) {
      sc[w] = slot_col[k];
      se[w++] = slot_code_[k];
    }
    prev = i + 1;
    q = q1;
  }
  copy_rows(n);
  row_ptr.swap(rp);
  slot_col.swap(sc);
  slot_code_.swap(se);
  // rows before r0 (the first with a new slot) and their slots are unchanged
  const int r0 = extra.empty() ? n_old : std::min(extra.front().x, n_old);
  const int k0 = row_ptr[r0];
  if (!mirror_bound_)   // pre-plan codes from the first changed slot on
    for (int k = k0; k < ns; k++) slot_code_[k] = pre_plan(slot_code_[k]);
  // gauge: the new factors join components; anchored roots from the priors
  uf_.resize(n);
  for (int i = n_old; i < n; i++) uf_[i] = i;
  for (const int2& ij : nij) {
    const int a = find(ij.x), b = find(ij.y);
    if (a != b) uf_[a] = b;
  }
  gauge_scan();
  prior_ptr.resize(n + 1, prior_ptr.back());
  if (phase) (*phase)("rows");
  edge_slot0.resize(ne_new, -1);
  for (int k = k0; k < ns; k++)
    if ((slot_code_[k] & 1) == 0) edge_slot0[dorder[slot_code_[k] >> 2]] = k;
  // the sweep structure: the new factors come last in device order, so an old
  // factor keeps its rank among its row's side-1 factors and moves by its
  // row's shift of s1_ptr
  int x0 = n_old, y0 = n_old;   // first rows of erow / s1_ptr that change (the new rows always)
  for (const int2& ij : nij) {
    x0 = std::min(x0, ij.x);
    y0 = std::min(y0, ij.y);
  }
  {
    std::vector<int> ecnt(n, 0), scnt(n, 0);   // new factors per row, by side
    for (const int2& ij : nij) {
      ecnt[ij.x]++;
      scnt[ij.y]++;
    }
    erow.resize(n + 1, erow.back());
    s1_ptr.resize(n + 1, s1_ptr.back());
    for (int i = x0, c = 0; i < n; i++) erow[i + 1] += (c += ecnt[i]);
    std::vector<int> dy(n + 1, 0);   // new side-1 factors in rows < j
    for (int j = y0, c = 0; j < n; j++) {
      dy[j] = c;
      s1_ptr[j + 1] += (c += scnt[j]);
    }
    for (int e = 0; e < ne_old; e++) {
      const int y = eij[e].y;
      if (y > y0) s1pos[e] += dy[y];
    }
    s1pos.resize(ne_new);
    std::vector<int> f(n, 0);   // the new factors after the old ones of their row
    for (size_t q = 0; q < nij.size(); q++) {
      const int y = nij[q].y;
      s1pos[ne_old + q] = s1_ptr[y + 1] - scnt[y] + f[y]++;
    }
  }
  if (robust) {
    s1fac.resize(ne_new);
    for (int e = 0; e < ne_new; e++) s1fac[s1pos[e]] = e;
  }
  Dc.resize(6 * (size_t)n, 0.0);
  delta->dc_rows.clear();
  for (size_t q = 0; q < nij.size(); q++) {   // new side-1 terms, in device order after the old ones
    const double* om = &eom[6 * (size_t)nd[q]];
    for (int c = 0; c < 6; c++) Dc[6 * (size_t)nij[q].y + c] += om[c];
    if (nij[q].y < n_old) delta->dc_rows.push_back(nij[q].y);
  }
  std::sort(delta->dc_rows.begin(), delta->dc_rows.end());
  delta->dc_rows.erase(std::unique(delta->dc_rows.begin(), delta->dc_rows.end()), delta->dc_rows.end());
  row_blocks();
  if (state_ != kPrePlan && k0 > 0) state_ = kMixed;   // rows < r0 keep the plan's bits
  bind_row0_ = std::min(bind_row0_, r0);
  delta->n_old = n_old;
  delta->ne_old = ne_old;
  delta->r0 = r0;
  delta->k0 = k0;
  delta->x0 = x0;
  delta->y0 = y0;
  return true;
}

SlotRange GraphStructure::bind(const std::vector<int>& iperm) {
  const int r0 = std::min(std::max(bind_row0_, 0), n), k0 = row_ptr[r0];
  eside_.resize(ne(), 0);
  // Cholesky-mode linearisation writes each factor's owner block at its
  // device factor index (one 72-byte record per factor), so the assembly reads V[9 e + q]
  auto own_bit = [&](int r, int k) {
    const bool own = iperm[r] > iperm[slot_col[k]];
    slot_code_[k] = (slot_code_[k] & ~2) | (own ? 2 : 0);
    if (own) eside_[slot_code_[k] >> 2] = (unsigned char)(slot_code_[k] & 1);   // one owner slot per factor
  };
  if (r0 > 0 && mirror_bound_) {   // the order kept and every other slot bound: the new slots only
    for (int k : new_slots_) {
      const int r = (int)(std::upper_bound(row_ptr.begin(), row_ptr.begin() + n + 1, k) - row_ptr.begin()) - 1;
      own_bit(r, k);
    }
  } else {
    host_parallel(n - r0, [&](int a, int b) {
      for (int r = r0 + a; r < r0 + b; r++)
        for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) own_bit(r, k);
    });
  }
  state_ = kBound;
  bind_row0_ = n;
  mirror_bound_ = true;
  new_slots_.clear();
  return SlotRange{k0, nslots()};
}

bool GraphStructure::unbind() {
  if (state_ != kMixed) return false;
  for (int& c : slot_code_) c = pre_plan(c);
  state_ = kPrePlan;
  bind_row0_ = 0;
  mirror_bound_ = false;
  new_slots_.clear();
  return true;
}

}  // namespace pgo
