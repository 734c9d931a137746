// Digest of a Cholesky plan (pgo_chol.h CholPlan): one 64-bit FNV-1a hash per
// section of the plan's host side, so that "the same plan" is an equality of a
// few numbers and a mismatch names its place -- a reordered task list or a
// changed flops figure shows, which the counts of pgo_debug_plan cannot.  And
// the branch counters: how often a plan took each branch of the scheduler
// (what a set of digest cases has to reach).  Host only, reads the plan only.
#pragma once
#include <cstdint>

#include "pgo_chol.h"

namespace pgo {

enum {
  kDigestFronts = 0,   // fronts and storage: ordering, supernodes, offsets, row lists, tree, extend-add maps, totals
  kDigestPartition,    // partition and exchange layout: owners, split, xroot / xsol, column owners, exchanges
  kDigestLevels,       // level records: CholLevel, SmallClass, PanelStep, SolveStep field by field (no at_bytes)
  kDigestFactor,       // factor task lists: small / level / potrf lists, sdiag / col / syrk tasks, gather, fused counts
  kDigestSolve,        // solve task lists: bwd, bwd_pref, bwdc, bwd_part, npart
  kDigestAssembly,     // assembly: ea_tasks, ea_pairs, at_iptr, at_items, asm_*, dg_*
  kDigestSelinv,       // selected inversion: SelPlan levels, steps, lists (no serial: a process-wide counter)
  kDigestSections
};
extern const char* const kDigestSectionNames[kDigestSections];

// Vectors hash as length then contents (never capacity), doubles by bit
// pattern, structs field by field (no padding bytes).
void plan_digest(const CholPlan& P, uint64_t out[kDigestSections]);

enum {
  kBrBigTile = 0,      // steps with syrk_tile == kBigTile
  kBrInline,           // steps whose plain tiles ride in k_step
  kBrApart,            // ... go to a launch of their own
  kBrLag2,             // plain_lag == 2
  kBrPrep,             // prep_cnt > 0
  kBrFarPieces,
  kBrFusedPairs,       // fused tiles with child rectangles
  kBrFusedEmpty,       // ... without
  kBrFusedMultipass,
  kBrClipped,          // narrow / clipped Schur tiles
  kBrTwoWaveLevels,    // levels with wavefront classes of m <= 64 and of m > 64
  kBrWg32, kBrWg64, kBrWg96, kBrWg128,   // workgroup classes by size bucket
  kBrXfirst, kBrXstep, kBrXtail,         // exchanges
  kBrDroppedLevels,    // heights without a front of this rank, dropped from its levels
  kBrAppended,         // poses added by chol_append since the last full analysis
  kBranchCounters
};
extern const char* const kBranchCounterNames[kBranchCounters];
void plan_branch_counters(const CholPlan& P, long long out[kBranchCounters]);

}  // namespace pgo
