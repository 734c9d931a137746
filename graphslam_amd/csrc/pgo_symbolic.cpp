// Host-side symbolic analysis for the GPU supernodal Cholesky (pgo_chol.h).
// Runs once per graph structure (GTSAM recomputes COLAMD every solve).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pgo_chol.h"
#include "pgo_structure.h"

namespace pgo {

// Approximate minimum degree on the quotient graph (Amestoy, Davis & Duff):
// eliminated pivots become elements that absorb their adjacent elements;
// external degrees are bounded by |A_i| + |L_p \ i| + sum_e |L_e \ L_p|,
// with |L_e \ L_p| from the w(e) counters; aggressive element absorption.
std::vector<int> order_amd(int n, const std::vector<int>& xadj, const std::vector<int>& adj) {
  std::vector<std::vector<int>> var(n), elem(n), members(n);
  std::vector<char> state(n, 0);  // 0 variable, 1 element, 2 absorbed
  std::vector<int> deg(n), w(n, 0), wstamp(n, -1), mark(n, -1);
  std::vector<int> head(n + 1, -1), nxt(n, -1), prv(n, -1);
  auto unlink = [&](int i) {
    if (prv[i] >= 0) nxt[prv[i]] = nxt[i];
    else head[deg[i]] = nxt[i];
    if (nxt[i] >= 0) prv[nxt[i]] = prv[i];
  };
  auto link = [&](int i) {
    nxt[i] = head[deg[i]];
    prv[i] = -1;
    if (head[deg[i]] >= 0) prv[head[deg[i]]] = i;
    head[deg[i]] = i;
  };
  for (int i = 0; i < n; i++) {
    for (int k = xadj[i]; k < xadj[i + 1]; k++)
      if (adj[k] != i) var[i].push_back(adj[k]);
    deg[i] = (int)var[i].size();
  }
  for (int i = n - 1; i >= 0; i--) link(i);
  std::vector<int> order(n);
  int mindeg = 0;
  for (int k = 0; k < n; k++) {
    while (head[mindeg] < 0) mindeg++;
    const int p = head[mindeg];
    unlink(p);
    order[k] = p;
    std::vector<int> Lp;
    mark[p] = k;
    for (int j : var[p])
      if (state[j] == 0 && mark[j] != k) {
        mark[j] = k;
        Lp.push_back(j);
      }
    for (int e : elem[p]) {
      if (state[e] != 1) continue;
      for (int j : members[e])
        if (state[j] == 0 && mark[j] != k) {
          mark[j] = k;
          Lp.push_back(j);
        }
      state[e] = 2;
      std::vector<int>().swap(members[e]);
    }
    state[p] = 1;
    std::vector<int>().swap(var[p]);
    std::vector<int>().swap(elem[p]);
    for (int i : Lp) unlink(i);
    for (int i : Lp)
      for (int e : elem[i]) {
        if (state[e] != 1) continue;
        if (wstamp[e] != k) {
          wstamp[e] = k;
          w[e] = (int)members[e].size();
        }
        w[e]--;
      }
    const int left = n - k - 1;
    const int lp = (int)Lp.size();
    for (int i : Lp) {
      long ext = 0;
      auto& ei = elem[i];
      size_t m = 0;
      for (int e : ei) {
        if (state[e] != 1) continue;
        if (w[e] == 0) {  // aggressive absorption: L_e inside L_p
          state[e] = 2;
          std::vector<int>().swap(members[e]);
          continue;
        }
        ei[m++] = e;
        ext += w[e];
      }
      ei.resize(m);
      ei.push_back(p);
      auto& vi = var[i];
      m = 0;
      for (int j : vi)
        if (state[j] == 0 && mark[j] != k) vi[m++] = j;
      vi.resize(m);
      long d = (long)vi.size() + (lp - 1) + ext;
      d = std::min<long>(d, (long)deg[i] + lp - 1);
      d = std::min<long>(d, left - 1);
      deg[i] = (int)std::max<long>(d, 0);
      link(i);
      mindeg = std::min(mindeg, deg[i]);
    }
    members[p] = std::move(Lp);
  }
  return order;
}

// Column owners of the distributed top (see chol_analyze): per top front s
// (owner[s] < 0) its m columns at cown[off[s] ..]: rank, or -1 (every rank).
void column_owners(const CholPlan& P, const std::vector<int>& owner, int psz, std::vector<int>& off,
                          std::vector<int>& cown) {
  const int ns = P.ns;
  off.assign(ns, -1);
  cown.clear();
  int rr = 0;   // round-robin position over the panels of the top fronts
  for (int s = ns - 1; s >= 0; s--) {   // parents before children
    if (owner[s] >= 0) continue;
    const int m = P.m[s], w = P.w[s], p = P.parent[s];
    off[s] = (int)cown.size();
    cown.resize(cown.size() + m, -1);
    int* own = cown.data() + off[s];
    const bool blk = front_packed(m, w);   // the blocked path (64-column panels)
    const int wr = blk ? std::min(m, (w + kNB - 1) / kNB * kNB) : 0;
    for (int col = 0; col < wr; col += kNB, rr++)
      for (int j = col; j < std::min(col + kNB, wr); j++) own[j] = rr % psz;
    for (int col = std::max(wr, w); col < m; col++) {
      const int t = col - w;
      own[col] = p >= 0 ? cown[off[p] + 3 * P.ea_rel[P.ea_ptr[s] + t / 3] + t % 3] : -1;
    }
    if (!blk)
      for (int j = 0; j < m; j++) own[j] = -1;
  }
}

std::vector<double> distributed_rank_flops(const CholPlan& P, int size, double* replicated) {
  std::vector<double> rf;
  double top = 0;
  const std::vector<int> owner = partition_subtrees(P, size, &rf, &top);
  std::vector<int> off, cown;
  column_owners(P, owner, size, off, cown);
  double rep = 0;
  for (int s = 0; s < P.ns; s++) {
    if (owner[s] >= 0) continue;
    const int m = P.m[s], w = P.w[s];
    for (int j = 0; j < m; j++) {
      // column j: its scaling as a pivot, its update by every earlier pivot
      const double f = 2.0 * std::min(j, w) * (m - j) + (j < w ? (double)(m - j) : 0.0);
      const int o = cown[off[s] + j];
      if (o < 0) rep += f;
      else rf[o] += f;
    }
  }
  for (double& v : rf) v += rep;
  if (replicated) *replicated = rep;
  return rf;
}

// Front storage offsets (F, Tinv, frontal vectors) and the factor's flops /
// nonzeros from the fronts' sizes m, w.
static void size_fronts(CholPlan& P) {
  const int ns = P.ns;
  P.foff.assign(ns + 1, 0);
  P.toff.assign(ns + 1, 0);
  P.voff.assign(ns + 1, 0);
  P.flops = 0;
  P.nnzl = 0;
  for (int s = 0; s < ns; s++) {
    P.foff[s + 1] = P.foff[s] + ((front_elems(P.m[s], P.w[s]) + 15) / 16) * 16;   // 128-byte aligned fronts
    P.voff[s + 1] = P.voff[s] + ((P.m[s] + 7) / 8) * 8;
    P.toff[s + 1] = P.toff[s] + (long long)((P.w[s] + 63) / 64) * 4096;
    for (int k = 0; k < P.w[s]; k++) {
      const double r = P.m[s] - k - 1;
      P.flops += 1 + r + r * (r + 1);
      P.nnzl += r + 1;
    }
  }
  P.ftotal = P.foff[ns];
  P.ttotal = P.toff[ns];
  P.vtotal = P.voff[ns];
}

// Threads of the host planning (PGO_PLAN_THREADS, default: the hardware's, at
// most 16), kept in a pool for the process (a plan refresh runs ~10 parallel
// passes: spawning threads per pass cost more than some passes).
static int plan_threads() {
  static const int t = [] {
    if (const char* e = getenv("PGO_PLAN_THREADS")) return std::max(1, atoi(e));
    return (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  }();
  return t;
}

namespace {
class PlanPool {
 public:
  explicit PlanPool(int workers) {
    for (int i = 0; i < workers; i++) th_.emplace_back([this] { work(); });
  }
  ~PlanPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(t) for t in [0, ntask), on the workers and the caller; one job at a time
  void run(int ntask, const std::function<void(int)>& fn) {
    if (ntask <= 1 || th_.empty()) {
      for (int t = 0; t < ntask; t++) fn(t);
      return;
    }
    std::lock_guard<std::mutex> job(job_m_);
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn;
      ntask_ = ntask;
      next_ = 0;
      busy_ = (int)th_.size();
      gen_++;
    }
    cv_.notify_all();
    for (int t; (t = next_.fetch_add(1)) < ntask;) fn(t);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [&] { return busy_ == 0; });
  }

 private:
  void work() {
    unsigned long seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      const std::function<void(int)>* fn = fn_;
      const int n = ntask_;
      lk.unlock();
      for (int t; (t = next_.fetch_add(1)) < n;) (*fn)(t);
      lk.lock();
      if (--busy_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_, job_m_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* fn_ = nullptr;
  int ntask_ = 0, busy_ = 0;
  std::atomic<int> next_{0};
  unsigned long gen_ = 0;
  bool stop_ = false;
};

PlanPool& plan_pool() {
  static PlanPool pool(plan_threads() - 1);
  return pool;
}
}  // namespace

void plan_parallel(int ntask, const std::function<void(int)>& fn) { plan_pool().run(ntask, fn); }

// fn(t, begin, end) on nth contiguous chunks of [0, n), chunk t by index (the
// results are independent of which thread runs it and of nth)
template <class F>
static void parallel_chunks(int n, int nth, F&& fn) {
  nth = std::max(1, std::min(nth, n));
  plan_parallel(nth, [&](int t) { fn(t, (int)((long long)n * t / nth), (int)((long long)n * (t + 1) / nth)); });
}

double selinv_flops(const CholPlan& P) {
  double f = 0;
  for (int s = 0; s < P.ns; s++)
    for (int c0 = 0; c0 < P.w[s]; c0 += 64) {   // G, Z_Rb, G' Z_Rb, X'X per pivot block
      const double nb = std::min(64, P.w[s] - c0), nr = P.m[s] - c0 - nb;
      f += nr * nb * nb + 2.0 * nr * nr * nb + 2.0 * nr * nb * nb + nb * nb * nb / 3.0;
    }
  return f;
}

void selinv_edge_table(const CholPlan& P, const int2* pairs, long long ne, int4* out) {
  const int nth = ne >= 4096 ? 16 : 1;
  plan_parallel(nth, [&](int t) {
    for (long long e = ne * t / nth; e < ne * (t + 1) / nth; e++) {
      const int q1 = P.iperm[pairs[e].x], q2 = P.iperm[pairs[e].y];
      const int a = std::min(q1, q2), b = std::max(q1, q2);   // a is eliminated first: b is a row of a's front
      const int s = P.dg_front[a];
      const int* r0 = P.rows.data() + P.rptr[s];
      const int* r1 = P.rows.data() + P.rptr[s + 1];
      const int* at = std::find(r0, r1, b);
      // (a factor's poses always share the front of the earlier one; a miss
      // would be a plan that does not cover the graph: flagged with front -1)
      out[e] = at == r1 ? make_int4(-1, 0, 0, 0) : make_int4(s, 3 * (int)(at - r0), 3 * P.dg_loc[a], q1 < q2);
    }
  });
}

void chol_analyze(CholPlan& P, int n, const std::vector<int>& row_ptr, const std::vector<int>& slot_col) {
  PhaseTimer phase("chol_analyze");
  P.nslots = (long long)slot_col.size();
  P.n = n;
  // ---- pose adjacency (old index), unique, no self loops
  std::vector<int> xadj(n + 1, 0), adj;
  adj.reserve(slot_col.size());
  {
    std::vector<int> stamp(n, -1);
    for (int i = 0; i < n; i++) {
      stamp[i] = i;
      for (int k = row_ptr[i]; k < row_ptr[i + 1]; k++) {
        const int j = slot_col[k];
        if (stamp[j] != i) {
          stamp[j] = i;
          adj.push_back(j);
        }
      }
      xadj[i + 1] = (int)adj.size();
    }
  }
  // a caller-given ordering (the incremental re-plan: the previous ordering
  // with the appended poses inserted) skips the fill-reducing ordering
  const std::vector<int> order0 = (int)P.order_in.size() == n ? P.order_in
                                  : P.ordering == kOrderAmd ? order_amd(n, xadj, adj) : order_nd(n, xadj, adj);
  std::vector<int> ip0(n);
  for (int k = 0; k < n; k++) ip0[order0[k]] = k;
  phase("ordering");
  // ---- elimination tree of the permuted pattern (Liu, path compression)
  std::vector<int> et(n, -1), anc(n, -1);
  for (int j = 0; j < n; j++) {
    const int oj = order0[j];
    for (int k = xadj[oj]; k < xadj[oj + 1]; k++) {
      int r = ip0[adj[k]];
      if (r >= j) continue;
      while (anc[r] != -1 && anc[r] != j) {
        const int t = anc[r];
        anc[r] = j;
        r = t;
      }
      if (anc[r] == -1) {
        anc[r] = j;
        et[r] = j;
      }
    }
  }
  phase("etree");
  // ---- postorder (children in increasing order)
  std::vector<int> chead(n, -1), cnext(n, -1), post;
  post.reserve(n);
  for (int j = n - 1; j >= 0; j--)
    if (et[j] >= 0) {
      cnext[j] = chead[et[j]];
      chead[et[j]] = j;
    }
  {
    std::vector<int> stack;
    for (int r = 0; r < n; r++) {
      if (et[r] != -1) continue;
      stack.push_back(r);
      while (!stack.empty()) {
        const int j = stack.back();
        const int c = chead[j];
        if (c == -1) {
          stack.pop_back();
          post.push_back(j);
        } else {
          chead[j] = cnext[c];
          stack.push_back(c);
        }
      }
    }
  }
  P.perm.resize(n);
  P.iperm.resize(n);
  std::vector<int> pos(n), par(n);
  for (int k = 0; k < n; k++) {
    P.perm[k] = order0[post[k]];
    pos[post[k]] = k;
  }
  for (int k = 0; k < n; k++) P.iperm[P.perm[k]] = k;
  for (int k = 0; k < n; k++) par[k] = et[post[k]] >= 0 ? pos[et[post[k]]] : -1;
  phase("postorder");
  // ---- column counts (off-diagonal pose rows) via row subtrees
  std::vector<int> cc(n, 0), mark(n, -1), nch(n, 0);
  for (int i = 0; i < n; i++) {
    mark[i] = i;
    const int oi = P.perm[i];
    for (int k = xadj[oi]; k < xadj[oi + 1]; k++) {
      int j = P.iperm[adj[k]];
      if (j >= i) continue;
      while (mark[j] != i) {
        cc[j]++;
        mark[j] = i;
        j = par[j];
      }
    }
  }
  for (int j = 0; j < n; j++)
    if (par[j] >= 0) nch[par[j]]++;
  phase("colcounts");
  // ---- fundamental supernodes, then relaxed amalgamation of a child that
  // immediately precedes its parent when it adds few explicit zeros
  std::vector<int> fs;
  for (int j = 0; j < n; j++) {
    if (j > 0 && par[j - 1] == j && nch[j] == 1 && cc[j - 1] == cc[j] + 1) continue;
    fs.push_back(j);
  }
  fs.push_back(n);
  std::vector<int> of, ol;
  std::vector<double> onz;
  // merge rule: a chain of W poses is kept together when W <= r[0], or
  // W <= r[1] with explicit-zero share z < r[2], W <= r[3] with z < r[4], or
  // z < r[5] (PGO_RELAX="r0,r1,r2,r3,r4,r5": a tuning knob)
  double rx[6] = {4, 8, 0.8, 24, 0.2, 0.05};   // (measured: C3 replays -4 % at 1 lane, -2 % at 3 lanes against {2, 6, 0.8, 16, 0.1, 0.05})
  if (const char* e = getenv("PGO_RELAX"))   // (separated by ',' or ';')
    for (int q = 0; q < 6 && *e; q++) {
      char* end = nullptr;
      rx[q] = strtod(e, &end);
      if (end == e) break;
      e = *end ? end + 1 : end;
    }
  for (size_t s = 0; s + 1 < fs.size(); s++) {
    int f = fs[s];
    const int l = fs[s + 1];
    const int wd = l - f, nb = cc[l - 1];
    double nz = 0.5 * wd * (wd + 1.0) + (double)wd * nb;
    while (!of.empty()) {
      const size_t t = of.size() - 1;
      if (ol[t] != f) break;
      const int lastc = ol[t] - 1;
      if (par[lastc] < f || par[lastc] >= l) break;
      const int W = l - of[t];
      const double tot = 0.5 * W * (W + 1.0) + (double)W * nb;
      const double tnz = nz + onz[t];
      const double z = (tot - tnz) / tot;
      const bool ok = (W <= rx[0]) || (W <= rx[1] && z < rx[2]) || (W <= rx[3] && z < rx[4]) || (z < rx[5]);
      if (!ok) break;
      f = of[t];
      nz = tnz;
      of.pop_back();
      ol.pop_back();
      onz.pop_back();
    }
    of.push_back(f);
    ol.push_back(l);
    onz.push_back(nz);
  }
  const int ns = (int)of.size();
  P.ns = ns;
  P.sfirst.assign(of.begin(), of.end());
  P.sfirst.push_back(n);
  std::vector<int> snode(n);
  for (int s = 0; s < ns; s++)
    for (int j = P.sfirst[s]; j < P.sfirst[s + 1]; j++) snode[j] = s;
  P.parent.assign(ns, -1);
  for (int s = 0; s < ns; s++) {
    const int lc = P.sfirst[s + 1] - 1;
    P.parent[s] = par[lc] >= 0 ? snode[par[lc]] : -1;
  }
  P.cptr.assign(ns + 1, 0);
  for (int s = 0; s < ns; s++)
    if (P.parent[s] >= 0) P.cptr[P.parent[s] + 1]++;
  for (int s = 0; s < ns; s++) P.cptr[s + 1] += P.cptr[s];
  P.children.assign(P.cptr[ns], 0);
  {
    std::vector<int> f(P.cptr.begin(), P.cptr.end() - 1);
    for (int s = 0; s < ns; s++)
      if (P.parent[s] >= 0) P.children[f[P.parent[s]]++] = s;
  }
  phase("supernodes");
  // ---- front rows: own poses then sorted below rows (A's pattern + children's rows)
  std::vector<std::vector<int>> below(ns);
  std::fill(mark.begin(), mark.end(), -1);
  for (int s = 0; s < ns; s++) {
    const int f = P.sfirst[s], l = P.sfirst[s + 1];
    auto& b = below[s];
    for (int j = f; j < l; j++) {
      const int oj = P.perm[j];
      for (int k = xadj[oj]; k < xadj[oj + 1]; k++) {
        const int i = P.iperm[adj[k]];
        if (i >= l && mark[i] != s) {
          mark[i] = s;
          b.push_back(i);
        }
      }
    }
    for (int q = P.cptr[s]; q < P.cptr[s + 1]; q++)
      for (int i : below[P.children[q]])
        if (i >= l && mark[i] != s) {
          mark[i] = s;
          b.push_back(i);
        }
    std::sort(b.begin(), b.end());
  }
  P.rptr.assign(ns + 1, 0);
  P.m.resize(ns);
  P.w.resize(ns);
  for (int s = 0; s < ns; s++) {
    const int wp = P.sfirst[s + 1] - P.sfirst[s];
    P.w[s] = 3 * wp;
    P.m[s] = 3 * (wp + (int)below[s].size());
    P.rptr[s + 1] = P.rptr[s] + wp + (int)below[s].size();
  }
  size_fronts(P);
  P.rows.resize(P.rptr[ns]);
  for (int s = 0; s < ns; s++) {
    int q = P.rptr[s];
    for (int j = P.sfirst[s]; j < P.sfirst[s + 1]; j++) P.rows[q++] = j;
    for (int i : below[s]) P.rows[q++] = i;
  }
  auto local_of = [&](int s, int i) {  // local pose index of new pose i in front s
    const int f = P.sfirst[s], l = P.sfirst[s + 1];
    if (i < l) return i - f;
    const auto& b = below[s];
    return (l - f) + (int)(std::lower_bound(b.begin(), b.end(), i) - b.begin());
  };
  phase("frontrows");
  // ---- extend-add maps: each below row of s -> local pose index in parent's front
  P.ea_ptr.assign(ns + 1, 0);
  for (int s = 0; s < ns; s++) P.ea_ptr[s + 1] = P.ea_ptr[s] + (int)below[s].size();
  P.ea_rel.resize(P.ea_ptr[ns]);
  for (int s = 0; s < ns; s++) {
    const int p = P.parent[s];
    for (size_t t = 0; t < below[s].size(); t++)
      P.ea_rel[P.ea_ptr[s] + t] = p >= 0 ? local_of(p, below[s][t]) : -1;
  }
  // ---- heights (leaves 0)
  P.height.assign(ns, 0);
  for (int s = 0; s < ns; s++)  // children precede parents (postorder)
    if (P.parent[s] >= 0) P.height[P.parent[s]] = std::max(P.height[P.parent[s]], P.height[s] + 1);
  P.dg_front.resize(n);
  P.dg_loc.resize(n);
  for (int j = 0; j < n; j++) {
    P.dg_front[j] = snode[j];
    P.dg_loc[j] = j - P.sfirst[snode[j]];
  }
  P.n_analyzed = n;
  P.flops_analyzed = P.flops;
  chol_schedule(P, row_ptr, slot_col);
}

// The targets after an append (chol_append): the columns in P.asm_dirty (the
// append's factors' columns and the new poses') get their entry lists rebuilt
// from the pattern, as chol_assembly builds every column; the other columns'
// targets and bound sources are kept (an append adds rows at the end of its
// fronts' row lists, so their local indices stand) and moved past the rebuilt
// ones.  Same lists as a rebuild once bound (host_selftest: check_append).
static void assembly_splice(CholPlan& P, const std::vector<int>& row_ptr, const std::vector<int>& slot_col) {
  std::vector<int>& dc = P.asm_dirty;
  std::sort(dc.begin(), dc.end());
  dc.erase(std::unique(dc.begin(), dc.end()), dc.end());
  const int ntg0 = (int)P.asm_front.size(), ne0 = P.asm_ptr[ntg0];
  auto colof = [&](int g) { return P.sfirst[P.asm_front[g]] + P.asm_lj[g]; };
  // old target range of each dirty column (targets are by column)
  std::vector<int> glo(dc.size()), ghi(dc.size());
  for (size_t d = 0; d < dc.size(); d++) {
    int lo = 0, hi = ntg0;
    while (lo < hi) {   // first g with colof(g) >= dc[d]
      const int mid = (lo + hi) / 2;
      if (colof(mid) < dc[d]) lo = mid + 1; else hi = mid;
    }
    glo[d] = lo;
    int g = lo;
    while (g < ntg0 && colof(g) == dc[d]) g++;
    ghi[d] = g;
  }
  // the dirty columns' new lists
  struct Col { std::vector<int> front, li, lj, cnt, src; };
  std::vector<Col> nc(dc.size());
  for (size_t d = 0; d < dc.size(); d++) {
    const int j = dc[d], r = P.perm[j];
    std::vector<int2> eik;
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      const int i = P.iperm[slot_col[k]];
      if (i > j) eik.push_back(make_int2(i, k));
    }
    std::sort(eik.begin(), eik.end(), [](const int2& x, const int2& y) { return x.x != y.x ? x.x < y.x : x.y < y.y; });
    const int s = P.dg_front[j], f = P.sfirst[s], l = P.sfirst[s + 1];
    const int* b0 = P.rows.data() + P.rptr[s] + (l - f);
    const int* b1 = P.rows.data() + P.rptr[s + 1];
    const int* cur = b0;
    Col& c = nc[d];
    for (size_t q = 0; q < eik.size(); q++) {
      const int i = eik[q].x;
      if (q == 0 || i != eik[q - 1].x) {
        int li;
        if (i < l) {
          li = i - f;
        } else {
          cur = std::lower_bound(cur, b1, i);
          li = (l - f) + (int)(cur - b0);
        }
        c.front.push_back(s);
        c.li.push_back(li);
        c.lj.push_back(j - f);
        c.cnt.push_back(0);
      }
      c.cnt.back()++;
      c.src.push_back(~eik[q].y);
    }
  }
  // splice in place: the kept segments between the dirty columns' old ranges
  // move up by the targets / entries the dirty columns before them gained (an
  // append only adds to the pattern: shifts >= 0), last segment first, then the
  // dirty columns' new lists are written into the gaps
  const int D = (int)dc.size();
  std::vector<long long> tshift(D + 1, 0), eshift(D + 1, 0);   // shift of kept segment d (after dirty d - 1)
  std::vector<int> plo(D), phi(D);                             // old entry pointers at glo / ghi
  for (int d = 0; d < D; d++) {
    plo[d] = P.asm_ptr[glo[d]];
    phi[d] = P.asm_ptr[ghi[d]];
    tshift[d + 1] = tshift[d] + (long long)nc[d].front.size() - (ghi[d] - glo[d]);
    eshift[d + 1] = eshift[d] + (long long)nc[d].src.size() - (phi[d] - plo[d]);
  }
  bool grows = true;
  for (int d = 0; d <= D; d++) grows = grows && tshift[d] >= 0 && eshift[d] >= 0;
  if (!grows) {   // (not an append: the caller's rebuild)
    dc.clear();
    P.asm_bound = false;
    return;
  }
  const long long ntg = ntg0 + tshift[D], ne = ne0 + eshift[D];
  auto grow = [](auto& v, long long n) {   // (room for the next appends too)
    if ((long long)v.capacity() < n) v.reserve(n + n / 16 + 1024);
    v.resize(n);
  };
  grow(P.asm_front, ntg);
  grow(P.asm_li, ntg);
  grow(P.asm_lj, ntg);
  grow(P.asm_ptr, ntg + 1);
  grow(P.asm_src, ne);
  for (int d = D; d >= 1; d--) {   // kept segment d: old targets [ghi[d-1], glo[d] or ntg0)
    const int a0 = ghi[d - 1], a1 = d < D ? glo[d] : ntg0;
    const int e0 = phi[d - 1], e1 = d < D ? plo[d] : ne0;
    const long long ts = tshift[d], es = eshift[d];
    if (ts == 0 && es == 0) continue;
    std::copy_backward(P.asm_src.begin() + e0, P.asm_src.begin() + e1, P.asm_src.begin() + e1 + es);
    std::copy_backward(P.asm_front.begin() + a0, P.asm_front.begin() + a1, P.asm_front.begin() + a1 + ts);
    std::copy_backward(P.asm_li.begin() + a0, P.asm_li.begin() + a1, P.asm_li.begin() + a1 + ts);
    std::copy_backward(P.asm_lj.begin() + a0, P.asm_lj.begin() + a1, P.asm_lj.begin() + a1 + ts);
    for (int g = a1 - 1; g >= a0; g--) P.asm_ptr[g + ts] = P.asm_ptr[g] + (int)es;
  }
  for (int d = 0; d < D; d++) {   // dirty column d's list: targets from glo[d] + tshift[d], entries from plo[d] + eshift[d]
    const Col& c = nc[d];
    const long long g0 = glo[d] + tshift[d];
    long long e = plo[d] + eshift[d];
    std::copy(c.src.begin(), c.src.end(), P.asm_src.begin() + e);
    for (size_t t = 0; t < c.front.size(); t++) {
      P.asm_front[g0 + t] = c.front[t];
      P.asm_li[g0 + t] = c.li[t];
      P.asm_lj[g0 + t] = c.lj[t];
      P.asm_ptr[g0 + t] = (int)e;
      e += c.cnt[t];
    }
  }
  P.asm_ptr[ntg] = (int)ne;
  dc.clear();
}

// Assembly of H into the plan's fronts (k_assemble_tile's H entries): the
// targets (lower 3x3 blocks H_{i,j}, i > j, of the permuted pattern: front,
// local row, local column, and their block-CSR slots -- parallel factors summed
// in slot order) and, per tile task, the targets and diagonal blocks with an
// element in the tile.  Depends on the pattern and the plan's fronts only: the
// incremental path re-runs it alone when appended factors fit the fronts.
void chol_assembly(CholPlan& P, const std::vector<int>& row_ptr, const std::vector<int>& slot_col) {
  const int n = P.n, ns = P.ns;
  const int nth = std::max(1, std::min(plan_threads(), n));   // (the chunks over the n poses: one per thread)
  PhaseTimer lap("chol_assembly");
  P.nslots = (long long)slot_col.size();
  const bool splice = P.asm_splice && P.asm_bound && !P.asm_ptr.empty();
  P.asm_splice = false;
  if (splice) {
    assembly_splice(P, row_ptr, slot_col);
    lap("splice");
  } else {
  // entries (j, i, k) of the permuted lower triangle (new indices i > j), by
  // (j, i, k).  Column j's entries are read from row perm[j]: its slots whose
  // column comes later, i.e. the mirror slot of each block (i, j).  Both slots
  // of a factor carry its device index, the only thing bind_plan keeps of k,
  // and a row's slots to one column are in the factors' device order whichever
  // end the row is: the same sources in the same order as from row perm[i].
  // Each column's few entries then sorted by (i, k) and its targets (distinct
  // (j, i)) counted per chunk of columns, then written.
  std::vector<int> jcnt(n + 1, 0);
  parallel_chunks(n, nth, [&](int, int r0, int r1) {   // (rows in their order: streamed)
    for (int r = r0; r < r1; r++) {
      const int j = P.iperm[r];
      int c = 0;
      for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) c += P.iperm[slot_col[k]] > j;
      jcnt[j + 1] = c;
    }
  });
  for (int j = 0; j < n; j++) jcnt[j + 1] += jcnt[j];
  lap("count");
  std::vector<int2> eik(jcnt[n]);   // (i, k) per entry, bucketed by j
  parallel_chunks(n, 8 * nth, [&](int, int r0, int r1) {
    for (int r = r0; r < r1; r++) {
      const int j = P.iperm[r];
      int q = jcnt[j];
      for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
        const int i = P.iperm[slot_col[k]];
        if (i > j) eik[q++] = make_int2(i, k);
      }
    }
  });
  lap("bucket");
  // (column chunks: 8 per thread, dealt dynamically -- the columns' work varies)
  const int nck = std::max(1, std::min(n, 8 * nth));
  std::vector<int> tstart(nck + 1, 0);
  parallel_chunks(n, nck, [&](int t, int j0, int j1) {
    int cnt = 0;
    for (int j = j0; j < j1; j++) {
      std::sort(eik.begin() + jcnt[j], eik.begin() + jcnt[j + 1],
                [](const int2& x, const int2& y) { return x.x != y.x ? x.x < y.x : x.y < y.y; });
      for (int q = jcnt[j]; q < jcnt[j + 1]; q++) cnt += (q == jcnt[j] || eik[q].x != eik[q - 1].x);
    }
    tstart[t + 1] = cnt;
  });
  lap("sort");
  for (int t = 0; t < nck; t++) tstart[t + 1] += tstart[t];
  const int ntg = tstart[nck];
  {   // (room for the live path's spliced appends: no regrowth on the first one)
    const size_t rt = ntg + ntg / 16 + 1024, re = eik.size() + eik.size() / 16 + 1024;
    P.asm_front.reserve(rt);
    P.asm_li.reserve(rt);
    P.asm_lj.reserve(rt);
    P.asm_ptr.reserve(rt + 1);
    P.asm_src.reserve(re);
  }
  P.asm_front.resize(ntg);
  P.asm_li.resize(ntg);
  P.asm_lj.resize(ntg);
  P.asm_ptr.resize(ntg + 1);
  P.asm_src.resize(eik.size());
  parallel_chunks(n, nck, [&](int t, int j0, int j1) {
    int g = tstart[t];
    for (int j = j0; j < j1; j++) {
      const int s = P.dg_front[j], f = P.sfirst[s], l = P.sfirst[s + 1];
      const int* b0 = P.rows.data() + P.rptr[s] + (l - f);
      const int* b1 = P.rows.data() + P.rptr[s + 1];
      const int* cur = b0;   // the bucket's rows come in increasing order: a forward scan finds them
      for (int q = jcnt[j]; q < jcnt[j + 1]; q++) {
        const int i = eik[q].x;
        if (q == jcnt[j] || i != eik[q - 1].x) {
          P.asm_ptr[g] = q;
          P.asm_front[g] = s;
          P.asm_lj[g] = j - f;
          int li;
          if (i < l) {
            li = i - f;
          } else {
            cur = std::lower_bound(cur, b1, i);
            li = (l - f) + (int)(cur - b0);
          }
          P.asm_li[g++] = li;
        }
        P.asm_src[q] = ~eik[q].y;
      }
    }
  });
  P.asm_bound = false;
  lap("targets");
  P.asm_ptr[ntg] = (int)eik.size();
  if (ntg == 0) P.asm_ptr.assign(1, 0);
  }
  const int ntg = (int)P.asm_front.size();
  // H entries by front tile: every 64x64 lower tile of a front lists the 3x3
  // blocks of H (off-diagonal targets t >= 0, diagonal blocks ~pose) with an
  // element in it (a block can straddle tile boundaries); items of a tile in
  // the order they are added (off-diagonal targets, then diagonal blocks).
  // Per front (its targets are contiguous: columns sorted), tiles in key order
  // ti (ti + 1) / 2 + tj -- the order of the front's tile tasks in ea_tasks.
  // targets of front s: [fg[s], fg[s + 1]) -- asm_front is nondecreasing (targets
  // by column, a front's columns contiguous and in front order): binary searches
  std::vector<int> fg(ns + 1, 0);
  parallel_chunks(ns + 1, nth, [&](int, int s0, int s1) {
    for (int s = s0; s < s1; s++)
      fg[s] = (int)(std::lower_bound(P.asm_front.begin(), P.asm_front.begin() + ntg, s) - P.asm_front.begin());
  });
  auto for_item = [](int r0, int c0, auto&& fn) {
    for (int ti = r0 / 64; ti <= (r0 + 2) / 64; ti++)
      for (int tj = c0 / 64; tj <= (c0 + 2) / 64; tj++)
        if (ti >= tj) fn(ti * (ti + 1) / 2 + tj);
  };
  std::vector<long long> fitems(ns + 1, 0);   // items of front s (counted, then its offset)
  // per front: item count per tile key, then its start (flat: front s at kbase[s], nt (nt + 1) / 2 + 1 keys)
  std::vector<long long> kbase(ns + 1, 0);
  for (int s = 0; s < ns; s++) {
    const long long nt = (P.m[s] + 63) / 64;
    kbase[s + 1] = kbase[s] + nt * (nt + 1) / 2 + 1;
  }
  std::vector<int> fcnt(kbase[ns], 0);
  parallel_chunks(ns, 8 * nth, [&](int, int s0, int s1) {
    for (int s = s0; s < s1; s++) {
      int* c = fcnt.data() + kbase[s];
      const long long nk = kbase[s + 1] - kbase[s];
      for (int g = fg[s]; g < fg[s + 1]; g++) for_item(3 * P.asm_li[g], 3 * P.asm_lj[g], [&](int key) { c[key + 1]++; });
      for (int j = P.sfirst[s]; j < P.sfirst[s + 1]; j++)
        for_item(3 * P.dg_loc[j], 3 * P.dg_loc[j], [&](int key) { c[key + 1]++; });
      for (long long k = 0; k + 1 < nk; k++) c[k + 1] += c[k];
      fitems[s + 1] = c[nk - 1];
    }
  });
  lap("tile count");
  // front blocks of at_items in the order of the fronts' tile tasks (level order)
  std::vector<long long> fbase(ns, -1);   // (-1: a front this rank does not assemble)
  {
    long long pos = 0;
    for (size_t q = 0; q < P.ea_tasks.size(); q++) {
      const int s = P.ea_tasks[q].x;
      if (P.ea_tasks[q].y == 0) {   // the front's first tile (0, 0)
        fbase[s] = pos;
        pos += fitems[s + 1];
      }
    }
    resize_room(P.at_items, pos);
  }
  parallel_chunks(ns, 8 * nth, [&](int, int s0, int s1) {
    std::vector<int> fill;   // (reused across the chunk's fronts)
    for (int s = s0; s < s1; s++) {
      if (fbase[s] < 0) continue;
      fill.assign(fcnt.begin() + kbase[s], fcnt.begin() + kbase[s + 1] - 1);
      int* out = P.at_items.data() + fbase[s];
      for (int g = fg[s]; g < fg[s + 1]; g++)
        for_item(3 * P.asm_li[g], 3 * P.asm_lj[g], [&](int key) { out[fill[key]++] = g; });
      for (int j = P.sfirst[s]; j < P.sfirst[s + 1]; j++)
        for_item(3 * P.dg_loc[j], 3 * P.dg_loc[j], [&](int key) { out[fill[key]++] = ~j; });
    }
  });
  lap("tile items");
  resize_room(P.at_iptr, P.ea_tasks.size());
  parallel_chunks((int)P.ea_tasks.size(), nth, [&](int, int q0, int q1) {
    for (int q = q0; q < q1; q++) {
      const int4 t = P.ea_tasks[q];
      const int ti = t.y >> 16, tj = t.y & 0xffff, key = ti * (ti + 1) / 2 + tj;
      const int* c = fcnt.data() + kbase[t.x];
      P.at_iptr[q] = make_int2((int)(fbase[t.x] + c[key]), c[key + 1] - c[key]);
    }
  });
  lap("tile ptrs");
  // a fused tile has no assembly task: it must hold no H entry
  for (size_t q = 0; q < P.syrk_gather.size(); q++) {
    if (P.syrk_gather[q].x < 0) continue;
    const int4 t = P.syrk_tasks[q];
    const int ti = (t.y & kRowMask) >> 6, tj = t.z >> 6, key = ti * (ti + 1) / 2 + tj;
    const int* c = fcnt.data() + kbase[t.x];
    if (c[key + 1] != c[key]) P.schedule_error = true;
  }
  // (the levels' k_assemble_tile bytes: on first use, level_at_bytes)
  for (CholLevel& lv : P.levels) lv.at_bytes = -1.0;
}

// Does the plan's factor structure hold every block of the pattern (old pose
// indices)?  Block (r, c) with new indices i < j must have row j in the front of
// column i (its own poses or its below rows).
// Is block (a, b) (old pose indices < P.n) inside the plan's factor structure?
static bool covered(const CholPlan& P, int a, int b) {
  int i = P.iperm[a], j = P.iperm[b];
  if (i == j) return true;
  if (i > j) std::swap(i, j);
  const int s = P.dg_front[i];
  if (j < P.sfirst[s + 1]) return true;
  const int* b0 = P.rows.data() + P.rptr[s] + (P.sfirst[s + 1] - P.sfirst[s]);
  const int* b1 = P.rows.data() + P.rptr[s + 1];
  return std::binary_search(b0, b1, j);
}

bool chol_covers(const CholPlan& P, const std::vector<int2>& pairs) {
  for (const int2& e : pairs)
    if (e.x >= P.n || e.y >= P.n || !covered(P, e.x, e.y)) return false;
  return true;
}

// Incremental symbolic update for appended poses (the live re-solve,
// graph.cpp:180-200): poses P.n .. n-1 are eliminated last, as extra pivot
// columns of the root front (the last supernode), so no existing row moves.
// A new pose v coupled to an old pose a fills L(v, .) along the elimination
// tree path from a's front to the root: every front on it gains row v at the
// end of its row list (old rows keep their local indices, so the children's
// extend-add maps stay valid; v's own map entry points at the parent's new last
// rows); a root other than the last supernode reached this way becomes its
// child.  Only the fronts on these paths change size.  The schedules and
// assembly lists are then rebuilt from the fronts (chol_schedule).
// new_pairs: every factor added since the plan (old pose indices); factors
// between old poses must lie in the existing structure.  Returns false (plan
// untouched) when the update does not apply: a partitioned plan, an old-old
// factor outside the fill, a tail past max_tail poses since the last full
// analysis, or a factor past max_growth x the analysed one's flops.
bool chol_append(CholPlan& P, int n, const std::vector<int>& row_ptr, const std::vector<int>& slot_col,
                 const std::vector<int2>& new_pairs, int max_tail, double max_growth) {
  const int n0 = P.n, ns = P.ns;
  if (n <= n0 || ns == 0 || P.part_size > 1 || P.parent[ns - 1] != -1 || n - P.n_analyzed > max_tail ||
      P.flops > max_growth * P.flops_analyzed)
    return false;
  for (const int2& e : new_pairs)
    if (e.x < n0 && e.y < n0 && !covered(P, e.x, e.y)) return false;
  const int T = ns - 1;
  // 1. the fill paths: (front, new pose) in increasing pose order per front
  std::vector<int> stamp(ns, -1), added(ns, 0), reparent;
  std::vector<int2> adds;
  for (int v = n0; v < n; v++)
    for (int q = row_ptr[v]; q < row_ptr[v + 1]; q++) {
      const int a = slot_col[q];
      if (a >= n0) continue;
      int s = P.dg_front[P.iperm[a]];
      while (s != T && stamp[s] != v) {
        stamp[s] = v;
        adds.push_back(make_int2(s, v));
        added[s]++;
        if (P.parent[s] < 0) {
          reparent.push_back(s);
          break;
        }
        s = P.parent[s];
      }
    }
  // the growth limit on the plan after this append (the fronts on the fill
  // paths gain 3 rows per new pose, the root its new poses), before anything
  // of the plan is changed
  {
    auto pf = [](double m, double w) {   // size_fronts' flops of one front, closed form
      // sum_{k<w} 1 + r + r (r + 1), r = m - 1 - k
      const double s1 = w * (m - 1) - w * (w - 1) / 2;                       // sum r
      auto sq = [](double a) { return a * (a + 1) * (2 * a + 1) / 6; };      // sum_{r=0..a} r^2
      return w + 2 * s1 + (sq(m - 1) - sq(m - 1 - w));
    };
    double est = P.flops;
    for (int s = 0; s < ns; s++)
      if (added[s]) est += pf(P.m[s] + 3.0 * added[s], P.w[s]) - pf(P.m[s], P.w[s]);
    const double wt = 3.0 * (n - P.sfirst[T]);
    est += pf(wt, wt) - pf(P.m[T], P.w[T]);
    if (est > max_growth * P.flops_analyzed) return false;
  }
  // 2. row lists: old segment, then the new rows; the root front's own poses extended
  std::vector<int> rptr(ns + 1, 0);
  for (int s = 0; s < ns; s++) rptr[s + 1] = rptr[s] + (P.rptr[s + 1] - P.rptr[s]) + added[s] + (s == T ? n - n0 : 0);
  std::vector<int> rows(rptr[ns]);
  std::vector<int> fillp(ns);
  for (int s = 0; s < ns; s++) {
    std::copy(P.rows.begin() + P.rptr[s], P.rows.begin() + P.rptr[s + 1], rows.begin() + rptr[s]);
    fillp[s] = rptr[s] + (P.rptr[s + 1] - P.rptr[s]);
  }
  for (int v = n0; v < n; v++) rows[fillp[T]++] = v;
  std::stable_sort(adds.begin(), adds.end(), [](const int2& x, const int2& y) { return x.x < y.x; });
  for (const int2& t : adds) rows[fillp[t.x]++] = t.y;
  // 3. extend-add maps: old entries kept, the new rows' local index in the parent
  for (int s : reparent) P.parent[s] = T;
  std::vector<int> ea_ptr(ns + 1, 0);
  for (int s = 0; s < ns; s++) ea_ptr[s + 1] = ea_ptr[s] + (P.ea_ptr[s + 1] - P.ea_ptr[s]) + added[s];
  std::vector<int> ea_rel(ea_ptr[ns]);
  P.sfirst[ns] = n;
  for (int s = 0; s < ns; s++) {
    const int old = P.ea_ptr[s + 1] - P.ea_ptr[s];
    std::copy(P.ea_rel.begin() + P.ea_ptr[s], P.ea_rel.begin() + P.ea_ptr[s + 1], ea_rel.begin() + ea_ptr[s]);
    if (!added[s]) continue;
    const int p = P.parent[s];
    const int* b0 = rows.data() + rptr[p];
    const int* b1 = rows.data() + rptr[p + 1];
    const int* nr = rows.data() + rptr[s + 1] - added[s];
    for (int t = 0; t < added[s]; t++) {
      const int v = nr[t];
      // in the root front v is an own pose; elsewhere one of the parent's new rows
      const int li = p == T ? v - P.sfirst[T] : (int)(std::lower_bound(b1 - added[p], b1, v) - b0);
      ea_rel[ea_ptr[s] + old + t] = li;
    }
  }
  // 4. the rest of the plan's per-front / per-pose arrays
  P.rows.swap(rows);
  P.rptr.swap(rptr);
  P.ea_rel.swap(ea_rel);
  P.ea_ptr.swap(ea_ptr);
  for (int s = 0; s < ns; s++) P.m[s] += 3 * added[s];
  P.w[T] = 3 * (n - P.sfirst[T]);
  P.m[T] = P.w[T];
  P.perm.resize(n);
  P.iperm.resize(n);
  P.dg_front.resize(n);
  P.dg_loc.resize(n);
  for (int v = n0; v < n; v++) {
    P.perm[v] = P.iperm[v] = v;
    P.dg_front[v] = T;
    P.dg_loc[v] = v - P.sfirst[T];
  }
  if (!reparent.empty()) {
    P.cptr.assign(ns + 1, 0);
    for (int s = 0; s < ns; s++)
      if (P.parent[s] >= 0) P.cptr[P.parent[s] + 1]++;
    for (int s = 0; s < ns; s++) P.cptr[s + 1] += P.cptr[s];
    P.children.assign(P.cptr[ns], 0);
    std::vector<int> f(P.cptr.begin(), P.cptr.end() - 1);
    for (int s = 0; s < ns; s++)
      if (P.parent[s] >= 0) P.children[f[P.parent[s]]++] = s;
    P.height.assign(ns, 0);
    for (int s = 0; s < ns; s++)
      if (P.parent[s] >= 0) P.height[P.parent[s]] = std::max(P.height[P.parent[s]], P.height[s] + 1);
  }
  P.n = n;
  size_fronts(P);
  // the assembly targets: spliced (the columns of the new factors and poses rebuilt)
  P.asm_dirty.clear();
  for (const int2& e : new_pairs) P.asm_dirty.push_back(std::min(P.iperm[e.x], P.iperm[e.y]));
  for (int v = n0; v < n; v++) P.asm_dirty.push_back(v);
  P.asm_splice = !getenv("PGO_NO_ASM_SPLICE");
  chol_schedule(P, row_ptr, slot_col);
  return true;
}

bool chol_covers(const CholPlan& P, int n, const std::vector<int>& row_ptr, const std::vector<int>& slot_col) {
  if (n != P.n) return false;
  for (int r = 0; r < n; r++)
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      int i = P.iperm[r], j = P.iperm[slot_col[k]];
      if (i == j) continue;
      if (i > j) std::swap(i, j);
      const int s = P.dg_front[i];
      if (j < P.sfirst[s + 1]) continue;
      const int* b0 = P.rows.data() + P.rptr[s] + (P.sfirst[s + 1] - P.sfirst[s]);
      const int* b1 = P.rows.data() + P.rptr[s + 1];
      if (!std::binary_search(b0, b1, j)) return false;
    }
  return true;
}

}  // namespace pgo

namespace pgo {

// Subtree partition of the supernodal tree over `size` ranks (the partitioned
// multi-GPU factorisation): starting from the tree roots, the heaviest
// candidate subtree (by factorisation flops) is split -- its root joins the
// replicated "top" and its children become candidates -- until every
// candidate holds at most 1/(2 size) of the candidates' flops (or cannot be
// split); the candidates are then dealt to ranks largest first, each to the
// least-loaded rank.  owner[s] = rank of front s's subtree, -1 for top fronts.
// Deterministic: every rank computes the same partition from the same plan.
std::vector<int> partition_subtrees(const CholPlan& P, int size, std::vector<double>* rank_flops,
                                    double* top_flops) {
  const int ns = P.ns;
  std::vector<double> f(ns, 0.0), sub(ns, 0.0);
  for (int s = 0; s < ns; s++) {
    for (int k = 0; k < P.w[s]; k++) {
      const double r = P.m[s] - k - 1;
      f[s] += 1 + r + r * (r + 1);
    }
    sub[s] += f[s];
    if (P.parent[s] >= 0) sub[P.parent[s]] += sub[s];   // children precede parents (postorder)
  }
  std::vector<int> owner(ns, -1), cand;
  for (int s = 0; s < ns; s++)
    if (P.parent[s] < 0) cand.push_back(s);
  if (size > 1) {
    for (;;) {
      double tot = 0;
      int best = -1;
      for (int c : cand) {
        tot += sub[c];
        if (best < 0 || sub[c] > sub[best]) best = c;
      }
      if (best < 0 || sub[best] <= tot / (2.0 * size) || P.cptr[best] == P.cptr[best + 1]) break;
      cand.erase(std::find(cand.begin(), cand.end(), best));
      for (int q = P.cptr[best]; q < P.cptr[best + 1]; q++) cand.push_back(P.children[q]);
    }
  }
  std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return sub[a] > sub[b]; });
  std::vector<double> load(size, 0.0);
  std::vector<int> root_rank(ns, -1);
  for (int c : cand) {
    const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    load[r] += sub[c];
    root_rank[c] = r;
  }
  for (int s = ns - 1; s >= 0; s--) {   // parents before children: inherit the subtree's rank
    if (root_rank[s] >= 0) owner[s] = root_rank[s];
    else if (P.parent[s] >= 0 && owner[P.parent[s]] >= 0) owner[s] = owner[P.parent[s]];
  }
  if (rank_flops) *rank_flops = load;
  if (top_flops) {
    *top_flops = 0;
    for (int s = 0; s < ns; s++)
      if (owner[s] < 0) *top_flops += f[s];
  }
  return owner;
}

}  // namespace pgo
