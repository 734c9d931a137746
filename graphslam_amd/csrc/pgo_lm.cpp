// The optimiser's control (pgo_lm.h): host arithmetic only.
#include "pgo_lm.h"

#include <algorithm>
#include <cassert>
#include <cmath>

namespace pgo {

LmControl::LmControl(const pgo_params& p, double initial_error, int adapt_mode)
    : lam(p.lambda_initial), factor(p.lambda_factor), err(initial_error), p_(p), adapt_mode_(adapt_mode) {}

bool LmControl::start() const { return !(err <= p_.error_tol) && iters < p_.max_iterations; }

void LmControl::begin_linearization() {
  cur_err_ = err;
  linearizations++;
  walked = 0;
}

bool LmControl::converged(double cur, double nw) const {
  if (nw <= p_.error_tol) return true;
  const double absd = cur - nw;
  const double reld = absd / cur;
  return (p_.relative_error_tol != 0.0 && reld <= p_.relative_error_tol) || absd <= p_.absolute_error_tol;
}

void LmControl::trace_row(double it, double lam_t, double solved, double lin_change, double new_e, double fid,
                          double acc) {
  const double row[kLmTraceCols] = {it, lam_t, solved, lin_change, new_e, fid, acc};
  trace.insert(trace.end(), row, row + kLmTraceCols);
}

// GTSAM tries lam_0 = lam, lam_{k+1} = lam_k * f_k (f_k doubling when the
// factor is not fixed) until one is accepted, the cost change is negligible, or
// lam_{k+1} reaches the upper bound.
void LmControl::plan_round(int T) {
  lam_k.resize(T);
  fac_k.resize(T);
  valid.resize(T);
  lam_k[0] = lam;
  fac_k[0] = factor;
  valid[0] = 1;
  for (int k = 1; k < T; k++) {
    lam_k[k] = lam_k[k - 1] * fac_k[k - 1];
    fac_k[k] = p_.use_fixed_lambda_factor ? fac_k[k - 1] : 2.0 * fac_k[k - 1];
    valid[k] = valid[k - 1] && lam_k[k] < p_.lambda_upper_bound;
  }
}

// Lanes sized to the tries expected, so the round that should reach the
// accepted try runs only the lanes up to it (a one-lane round is cheaper than
// a batched one); all lanes again if that try fails.  The expectation follows
// GTSAM's lambda dynamics: after a first-try acceptance lambda keeps falling
// and the next linearisation is expected to accept at once (1 try); after an
// acceptance that needed k >= 2 tries the next linearisation starts one decade
// below the accepted lambda, which just failed, so 2 tries are expected
// rather than k (C3: 13 rounds either way, two of them 2-lane instead of
// 3-lane).  The first linearisation of an optimize() expects 1: GTSAM starts
// at lambda = 1e-5, a nearly undamped step, which from odometry-initialised
// or warm-started values is accepted.  The tries and their order are
// unchanged (mode 0: every round runs all lanes; 2: the previous
// linearisation's count, all lanes first; 3: this rule, all lanes first).
// Ranks that exchange outcomes run every lane: the round is one parallel try.
int LmControl::round_lanes(int L, bool profiled, bool exchange) const {
  int Lr = profiled ? 1 : L;   // a profiled factorisation (lane 0, eager, timed launches) runs alone
  const int expect = adapt_mode_ == 2    ? prev_walked
                     : prev_walked == 0 ? (adapt_mode_ == 3 ? 0 : 1)
                                        : std::min(prev_walked, 2);
  if (adapt_mode_ != 0 && !exchange && expect > walked) Lr = std::min(Lr, expect - walked);
  return Lr;
}

// Try k of a round ran on rank k / L, lane k % L; the outcomes are walked in
// sequence order with GTSAM's rules, so the accepted step is the sequential one.
LmWalk LmControl::walk(const TryOutcome* outs, double lin_err) {
  const int T = (int)lam_k.size();
  // a lane that sat out a profiled round: its tries count as not made, the
  // walk stops there and the next round resumes from it
  for (int k = 0; k < T; k++)
    if (outs[k].solved == -1.0) {
      for (int j = k; j < T; j++) valid[j] = 0;
      break;
    }
  LmWalk r;
  for (int k = 0; k < T && valid[k]; k++) {
    const TryOutcome& o = outs[k];
    double fidelity = 0.0, lin_change = NAN, try_e = INFINITY;
    bool success = false, stop = false;
    if (o.solved == 1.0) {
      lin_change = -(o.gx + 0.5 * o.xhx);
      if (lin_change >= 0) {
        try_e = o.err;
        const double cost_change = err - try_e;
        if (lin_change > 2.220446049250313e-16 * lin_err) {
          fidelity = cost_change / lin_change;
          success = fidelity > p_.min_model_fidelity;
        }
        if (std::fabs(cost_change) < p_.relative_error_tol * err) stop = true;
      }
    }
    trace_row(iters, lam_k[k], o.solved, lin_change, try_e, fidelity, success ? 1.0 : 0.0);
    walked++;
    // (a rejection below advances lam and factor by the plan's own operations)
    assert(lam == lam_k[k] && factor == fac_k[k]);
    if (success) last_outcome = PGO_STOP_CONVERGED;
    else if (stop) last_outcome = PGO_STOP_SMALL_CHANGE;
    if (success) {  // decreaseLambda
      if (p_.use_fixed_lambda_factor) {
        lam /= p_.lambda_factor;
      } else {
        const double q = 2.0 * fidelity - 1.0;
        lam *= std::max(1.0 / 3.0, 1.0 - q * q * q);
        factor *= 2.0;
      }
      lam = std::max(p_.lambda_lower_bound, lam);
      err = try_e;
      iters++;
      inner++;
      r.winner = k;
      r.done = true;
      break;
    }
    if (stop) {
      r.done = true;
      break;
    }
    lam *= factor;  // increaseLambda
    inner++;
    if (!p_.use_fixed_lambda_factor) factor *= 2.0;
    if (lam >= p_.lambda_upper_bound) {
      last_outcome = PGO_STOP_LAMBDA_BOUND;
      r.done = true;
      break;
    }
  }
  if (r.done) prev_walked = walked;
  return r;
}

bool LmControl::gn_step(const TryOutcome& o) {
  if (o.solved == 0.0) {
    status = PGO_E_INDETERMINANT;
    return false;
  }
  err = o.err;
  iters++;
  inner++;
  trace_row(iters, 0.0, 1.0, NAN, err, 0.0, 1.0);
  return true;
}

bool LmControl::next_linearization() {
  if (status != PGO_OK) return false;
  if (p_.max_outer > 0 && linearizations >= p_.max_outer) {
    last_outcome = PGO_STOP_MAX_OUTER;
    return false;
  }
  return iters < p_.max_iterations && !converged(cur_err_, err) && std::isfinite(cur_err_);
}

void LmControl::finish() {
  if (status == PGO_OK && iters >= p_.max_iterations && p_.max_iterations > 0) status = PGO_W_MAXITER;
  stop_reason = status < 0 ? PGO_STOP_ERROR
                : (status == PGO_W_MAXITER && last_outcome != PGO_STOP_MAX_OUTER ? PGO_STOP_MAX_ITER : last_outcome);
}

LmControl lm_replay(const pgo_params& p, double initial_error, int adapt_mode, int P, int L, int profile_every,
                    const LmScript& script, LmReplay* out) {
  LmControl c(p, initial_error, adapt_mode);
  LmReplay rep;
  const int n_lin = (int)script.lin_ptr.size() - 1;
  const bool exchange = P > 1;
  const int T = P * L;
  long long factorizations = 0;
  // try t of linearisation i, solved at the error `err`: recorded, or the poison
  auto outcome = [&](int i, int t) {
    if (script.lin_ptr[i] + t >= script.lin_ptr[i + 1]) return TryOutcome{1.0, -1e300, 0.0, -1e300};
    const double* s = &script.tries[3 * (size_t)(script.lin_ptr[i] + t)];
    return TryOutcome{s[0], s[1], -0.0, -s[2]};   // -(gx + 0.5 * -0) is the recorded model decrease, bit for bit (a zero's sign too)
  };
  if (c.start()) {
    for (int i = 0;; i++) {
      if (i >= n_lin) {
        rep.exhausted = true;
        break;
      }
      c.begin_linearization();
      if (p.algorithm == PGO_ALG_GN) {
        factorizations++;
        if (!c.gn_step(outcome(i, 0))) break;
      } else {
        const double lin_err = script.lin_err.empty() ? c.err : script.lin_err[i];
        for (;;) {
          const int base = c.walked;
          c.plan_round(T);
          const bool prof_next = profile_every > 0 && (factorizations % profile_every) == 0;
          const int Lr = c.round_lanes(L, prof_next, exchange);
          std::vector<TryOutcome> outs(T, kNoTry);
          for (int me = 0; me < P; me++) {
            int nb = 0;   // the rank's valid tries (a prefix of its lanes)
            while (nb < Lr && c.valid[me * L + nb]) nb++;
            for (int l = 0; l < nb; l++) outs[me * L + l] = outcome(i, base + me * L + l);
          }
          factorizations++;   // (rank 0 always has a try)
          rep.rounds++;
          const LmWalk w = c.walk(outs.data(), lin_err);
          if (w.winner >= 0) {
            rep.winner_base.push_back(base);
            rep.winners.push_back(w.winner / L);
            rep.winners.push_back(w.winner % L);
          }
          if (w.done) break;
        }
      }
      if (!c.next_linearization()) break;
    }
  }
  c.finish();
  if (out) *out = rep;
  return c;
}

}  // namespace pgo

extern "C" int pgo_debug_lm_replay(const pgo_params* params, double initial_error, int ranks, int lanes,
                                   int adapt_mode, int n_lin, const int* lin_ptr, const double* tries,
                                   const double* lin_err, double* trace, int trace_cap, double* out, int out_cap) {
  if (!params || ranks < 1 || lanes < 1 || lanes > 8 || n_lin < 0 || (n_lin && (!lin_ptr || !tries)) ||
      (trace_cap > 0 && !trace) || out_cap < 11 || !out)
    return PGO_E_ARG;
  pgo::LmScript s;
  s.lin_ptr.assign(1, 0);
  for (int i = 0; i < n_lin; i++) {
    if (lin_ptr[i + 1] < lin_ptr[i] || lin_ptr[0] != 0) return PGO_E_ARG;
    s.lin_ptr.push_back(lin_ptr[i + 1]);
  }
  s.tries.assign(tries, tries + 3 * (size_t)s.lin_ptr.back());
  if (lin_err) s.lin_err.assign(lin_err, lin_err + n_lin);
  pgo::LmReplay rep;
  const pgo::LmControl c =
      pgo::lm_replay(*params, initial_error, adapt_mode, ranks, lanes, params->profile_every, s, &rep);
  const double head[11] = {(double)c.iters, (double)c.inner,     (double)c.linearizations, (double)c.status,
                           (double)c.stop_reason, c.lam,         c.factor,                 c.err,
                           (double)rep.rounds,    rep.exhausted ? 1.0 : 0.0, (double)(rep.winners.size() / 2)};
  std::copy(head, head + 11, out);
  for (size_t q = 0; q < rep.winners.size() && 11 + (int)q < out_cap; q++) out[11 + q] = rep.winners[q];
  const int rows = (int)(c.trace.size() / pgo::kLmTraceCols);
  if (trace_cap > 0 && rows > 0)
    std::copy(c.trace.begin(), c.trace.begin() + (size_t)pgo::kLmTraceCols * std::min(rows, trace_cap), trace);
  return rows;
}
