// Plan digest and branch counters (pgo_plan_digest.h).
#include "pgo_plan_digest.h"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace pgo {

const char* const kDigestSectionNames[kDigestSections] = {"fronts", "partition", "levels", "factor",
                                                          "solve",  "assembly",  "selinv"};

const char* const kBranchCounterNames[kBranchCounters] = {
    "bigtile", "inline", "apart", "lag2", "prep", "far", "fused_pairs", "fused_empty", "fused_multipass", "clipped",
    "two_wave", "wg32", "wg64", "wg96", "wg128", "xfirst", "xstep", "xtail", "dropped", "appended"};

namespace {

struct Fnv {
  uint64_t h = 14695981039346656037ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  }
  // a number, by its bytes (a double: its bit pattern)
  template <class T>
  void num(T v) {
    static_assert(std::is_arithmetic<T>::value, "numbers only");
    bytes(&v, sizeof v);
  }
  // ints, long longs, doubles, int2, int4: no padding inside or between
  template <class T>
  void vec(const std::vector<T>& v) {
    num((uint64_t)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
  template <class... T>
  void nums(T... v) {
    (num(v), ...);
  }
  void step(const SolveStep& s) { nums(s.off, s.cnt); }
};

void hash_level(Fnv& f, const CholLevel& lv) {
  f.num((uint64_t)lv.small.size());
  for (const SmallClass& c : lv.small) f.nums(c.off, c.cnt, c.mmax, c.wave, c.flops);
  f.num((uint64_t)lv.panels.size());
  for (const PanelStep& p : lv.panels)
    f.nums(p.kb, p.potrf_off, p.potrf_cnt, p.col_off, p.fcol_cnt, p.col_cnt, p.prep_cnt, p.sdiag_off, p.sdiag_cnt,
           p.syrk_off, p.syrk_cnt, p.syrk_tile, p.syrk_inline, p.syrk_flops, p.plain_flops, p.first_flops, p.step_flops,
           p.plain_lag, p.xfirst, p.xstep, p.far_cnt, p.far_p0, p.far_np, p.far_flops, p.gather_bytes, p.diag_flops,
           p.colupd_flops, p.trsm_flops);
  f.vec(lv.ea_off);
  f.vec(lv.ea_cnt);
  f.nums(lv.front_off, lv.front_cnt, lv.small_maxm, lv.maxm, lv.maxblk);
  f.num((uint64_t)lv.bwd.size());
  for (const SolveStep& s : lv.bwd) f.step(s);
  f.step(lv.bwd_part);
  f.step(lv.bwdc);
  f.nums(lv.xtail, lv.bwd_part_flops, lv.vec_bytes, lv.bwd_part_bytes, lv.bwd_init_bytes, lv.bwd_chain_bytes);
  f.vec(lv.far_pieces);
  f.vec(lv.far_piece_flops);
}

}  // namespace

void plan_digest(const CholPlan& P, uint64_t out[kDigestSections]) {
  Fnv f[kDigestSections];
  {
    Fnv& a = f[kDigestFronts];
    a.nums(P.ordering, P.n, P.ns, P.n_analyzed, P.flops_analyzed, P.nslots);
    a.vec(P.perm), a.vec(P.iperm), a.vec(P.sfirst), a.vec(P.m), a.vec(P.w), a.vec(P.foff), a.vec(P.toff), a.vec(P.voff);
    a.vec(P.rptr), a.vec(P.rows), a.vec(P.parent), a.vec(P.height), a.vec(P.cptr), a.vec(P.children);
    a.vec(P.ea_rel), a.vec(P.ea_ptr);
    a.nums(P.flops, P.nnzl, P.ftotal, P.ttotal, P.vtotal);
  }
  {
    Fnv& a = f[kDigestPartition];
    a.nums(P.part_size, P.part_rank, P.split);
    a.vec(P.owner), a.vec(P.subtree_cnt), a.vec(P.xroot), a.vec(P.xroot_rank), a.vec(P.xroot_off);
    a.vec(P.xsize), a.vec(P.xsol_size), a.nums(P.xmax, P.xsol_max), a.vec(P.xsol_ranges);
    a.vec(P.cown_off), a.vec(P.cown);
    a.num((uint64_t)P.xchg.size());
    for (const XExchange& x : P.xchg) a.nums(x.off, x.cnt), a.vec(x.size);
    a.vec(P.xp_tasks), a.vec(P.xp_loff), a.vec(P.xp_lstride), a.num(P.xp_rslot);
  }
  {
    Fnv& a = f[kDigestLevels];
    a.num((unsigned char)P.schedule_error);
    a.num((uint64_t)P.levels.size());
    for (const CholLevel& lv : P.levels) hash_level(a, lv);
  }
  {
    Fnv& a = f[kDigestFactor];
    a.vec(P.small_list), a.vec(P.level_fronts), a.vec(P.potrf_list);
    a.vec(P.sdiag_tasks), a.vec(P.col_tasks), a.vec(P.syrk_tasks), a.vec(P.syrk_gather);
    a.nums(P.fused_tiles, P.fused_with_pairs, P.fused_multipass, P.fused_edge, P.syrk_flops);
  }
  {
    Fnv& a = f[kDigestSolve];
    a.vec(P.bwd_tasks), a.vec(P.bwd_pref), a.vec(P.bwdc_tasks), a.vec(P.bwd_part_tasks), a.num(P.npart);
  }
  {
    Fnv& a = f[kDigestAssembly];
    a.vec(P.ea_tasks), a.vec(P.ea_pairs), a.vec(P.at_iptr), a.vec(P.at_items);
    a.vec(P.asm_front), a.vec(P.asm_li), a.vec(P.asm_lj), a.vec(P.asm_ptr), a.vec(P.asm_src);
    a.nums((unsigned char)P.asm_bound, (unsigned char)P.asm_splice), a.vec(P.asm_dirty);
    a.vec(P.dg_front), a.vec(P.dg_loc);
  }
  {
    Fnv& a = f[kDigestSelinv];
    const SelPlan& Q = P.sel;
    a.num((uint64_t)Q.levels.size());
    for (const SelLevel& sl : Q.levels) {
      a.nums(sl.small_off, sl.small_cnt, sl.gat_off, sl.gat_cnt, (uint64_t)sl.steps.size());
      for (const SelStep& st : sl.steps) a.nums(st.b, st.tile_off, st.tile_cnt, st.diag_off, st.diag_cnt);
    }
    a.vec(Q.gather), a.vec(Q.tiles), a.vec(Q.diag), a.vec(Q.goff);
    a.nums(Q.gmax, Q.pmax, Q.launches);
  }
  for (int s = 0; s < kDigestSections; s++) out[s] = f[s].h;
}

void plan_branch_counters(const CholPlan& P, long long out[kBranchCounters]) {
  std::fill(out, out + kBranchCounters, 0LL);
  for (const CholLevel& lv : P.levels) {
    bool wave_lo = false, wave_hi = false;
    for (const SmallClass& c : lv.small) {
      if (c.wave > 0) (c.mmax <= 64 ? wave_lo : wave_hi) = true;
      else out[kBrWg32 + std::min(3, std::max(0, (c.mmax - 1) / 32))]++;
    }
    out[kBrTwoWaveLevels] += wave_lo && wave_hi;
    for (const PanelStep& ps : lv.panels) {
      out[kBrBigTile] += ps.syrk_tile == kBigTile;
      out[kBrInline] += ps.syrk_cnt > 0 && ps.syrk_inline;
      out[kBrApart] += ps.syrk_cnt > 0 && !ps.syrk_inline;
      out[kBrLag2] += ps.plain_lag == 2;
      out[kBrPrep] += ps.prep_cnt > 0;
      out[kBrXfirst] += ps.xfirst >= 0;
      out[kBrXstep] += ps.xstep >= 0;
    }
    out[kBrFarPieces] += (long long)lv.far_pieces.size();
    out[kBrXtail] += lv.xtail >= 0;
  }
  out[kBrFusedPairs] = P.fused_with_pairs;
  out[kBrFusedEmpty] = P.fused_tiles - P.fused_with_pairs;
  out[kBrFusedMultipass] = P.fused_multipass;
  for (const int4& t : P.syrk_tasks) out[kBrClipped] += (t.y >> kClipShift) != 0;
  // heights up to each phase's tallest front with no front of this rank
  for (int phase = 0; phase < 2; phase++) {
    std::vector<char> seen;
    for (int s = 0; s < P.ns && s < (int)P.owner.size(); s++)
      if (phase == 0 ? P.owner[s] == P.part_rank : P.owner[s] < 0) {
        if ((int)seen.size() <= P.height[s]) seen.resize(P.height[s] + 1, 0);
        seen[P.height[s]] = 1;
      }
    out[kBrDroppedLevels] += std::count(seen.begin(), seen.end(), 0);
  }
  out[kBrAppended] = P.n - P.n_analyzed;
}

}  // namespace pgo
