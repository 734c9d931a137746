// The optimiser's control: GTSAM's Levenberg-Marquardt policy (the lambda
// sequence of a round, tryLambda's accept / stop / guard rules, decreaseLambda /
// increaseLambda, checkConvergence, the counters and the stop reason), the
// lambda-lane expectation rule and the Gauss-Newton bookkeeping, as pure host
// arithmetic on scalars.  pgo_optimize owns the device and the ranks and asks
// this module what to try and what the outcomes mean; host_selftest.cpp drives
// it against a sequential transcription of GTSAM's loop.  No HIP types.
#pragma once

#include <vector>

#include "pgo.h"

namespace pgo {

// One lambda try as the device reports it (and as the ranks exchange it: four
// doubles per try).  solved: 1 factorised and solved, 0 a non-positive pivot,
// -1 no try made (past the upper bound, or a lane that sat out the round).
struct TryOutcome {
  double solved, err, xhx, gx;   // err: the error at the candidate; delta'H delta; g'delta
};
static_assert(sizeof(TryOutcome) == 4 * sizeof(double), "the exchanged layout: 4 doubles per try");
constexpr TryOutcome kNoTry = {-1.0, 0.0, 0.0, 0.0};

constexpr int kLmTraceCols = 7;   // the oracle's trace columns (pgo_get_trace appends the wall ms)

struct LmWalk {
  int winner = -1;     // the accepted try of the round (rank winner / L, lane winner % L), -1: none
  bool done = false;   // the linearisation's tries are over
};

class LmControl {
 public:
  // adapt_mode: PGO_LANES_ADAPT (0 every round runs all lanes, 1 the expectation
  // rule, 2 the previous linearisation's count, 3 the rule, all lanes first)
  LmControl(const pgo_params& p, double initial_error, int adapt_mode);

  // the optimiser has anything to do (error_tol not met at entry, max_iterations > 0)
  bool start() const;
  void begin_linearization();
  // The lambdas of a round of T tries from the current lambda and factor:
  // lam_k[k] = lam_k[k - 1] * fac_k[k - 1], valid[k] while below the upper bound.
  void plan_round(int T);
  // Lanes a rank runs this round (of L): one when the factorisation is profiled,
  // else sized to the tries the linearisation is expected to need.
  int round_lanes(int L, bool profiled, bool exchange) const;
  // The round's T outcomes walked in GTSAM's order (tryLambda per try) up to the
  // first try not made; one trace row per walked try.  lin_err: the linearised
  // error GTSAM's guard compares the model decrease with (the error itself
  // unless a robust loss reweights).
  LmWalk walk(const TryOutcome* outs, double lin_err);
  // The plain step of a Gauss-Newton linearisation; false: the solve failed.
  bool gn_step(const TryOutcome& o);
  // After a linearisation's tries: true when another linearisation follows.
  bool next_linearization();
  // status and stop_reason of the finished optimisation
  void finish();

  double lam, factor, err;
  int iters = 0, inner = 0, linearizations = 0;
  int status = PGO_OK, stop_reason = PGO_STOP_CONVERGED;
  int last_outcome = PGO_STOP_CONVERGED;   // how the last linearisation's tries ended
  int prev_walked = 0;                     // tries the previous linearisation walked (0: none yet)
  int walked = 0;                          // tries of this linearisation walked so far
  std::vector<double> lam_k, fac_k;        // the round's plan
  std::vector<char> valid;
  std::vector<double> trace;               // kLmTraceCols per walked try / GN step

 private:
  bool converged(double cur, double nw) const;   // NonlinearOptimizer.cpp checkConvergence
  void trace_row(double it, double lam_t, double solved, double lin_change, double new_e, double fid, double acc);
  pgo_params p_;
  int adapt_mode_;
  double cur_err_ = 0.0;   // the error this linearisation started from
};

// Recorded tries per linearisation: {solved, error at the candidate, model
// decrease}, those of linearisation i at [lin_ptr[i], lin_ptr[i + 1]).
struct LmScript {
  std::vector<int> lin_ptr;
  std::vector<double> tries;     // 3 per try
  std::vector<double> lin_err;   // per linearisation; empty: the error (no robust loss)
};

struct LmReplay {
  std::vector<int> winners;       // (rank, lane) of every accepted try
  std::vector<int> winner_base;   // tries its linearisation had walked before the accepting round
  int rounds = 0;
  bool exhausted = false;     // the control asked for a linearisation the script does not hold
};

// The control driven as pgo_optimize drives it, over P ranks of L lanes, on
// recorded tries instead of a device.  A try past the recorded ones of its
// linearisation is speculative: it returns a poison outcome that would be
// accepted if it were ever walked.  profile_every > 0: every such
// factorisation runs alone (one lane, the others sit the round out).
LmControl lm_replay(const pgo_params& p, double initial_error, int adapt_mode, int P, int L, int profile_every,
                    const LmScript& script, LmReplay* out);

}  // namespace pgo
