// pgo_gnc.h: the GNC outer loop's control and the host-only entries that drive
// it and the weight formulas without a device.
#include "pgo_gnc.h"

#include <cmath>
#include <cstddef>

namespace pgo {

bool gnc_params_ok(const pgo_gnc_params& p) {
  if (p.loss != PGO_GNC_GM && p.loss != PGO_GNC_TLS) return false;
  if (!(std::isfinite(p.barc_sq) && p.barc_sq > 0.0)) return false;
  if (!(std::isfinite(p.mu_step) && p.mu_step > 1.0)) return false;
  if (p.max_iterations < 0) return false;
  if (!(std::isfinite(p.relative_cost_tol) && p.relative_cost_tol >= 0.0)) return false;
  if (!(std::isfinite(p.weights_tol) && p.weights_tol >= 0.0)) return false;
  return true;
}

bool GncControl::start(double cost0, double rmax_sq) {
  prev_cost = cost0;
  outer = 0;
  const double c2 = p.barc_sq;
  if (p.loss == PGO_GNC_GM) {
    mu = std::fmax(1.0, 2.0 * rmax_sq / c2);
  } else {
    mu = c2 / (2.0 * rmax_sq - c2);
    if (!(mu > 0.0) || !std::isfinite(mu)) {   // every candidate inside the threshold (or no finite r^2)
      mu = NAN;
      stop_reason = PGO_GNC_STOP_ALL_INLIERS;
      return false;
    }
  }
  mu_initial = mu;
  if (p.max_iterations == 0) {
    stop_reason = PGO_GNC_STOP_MAX_ITER;
    return false;
  }
  return true;
}

bool GncControl::step(double cost, double nonbinary) {
  outer++;
  const bool mu_done = p.loss == PGO_GNC_GM ? std::fabs(mu - 1.0) < 1e-3 : !(nonbinary > 0.0);
  if (mu_done) {
    stop_reason = PGO_GNC_STOP_MU;
    return false;
  }
  if (std::fabs(cost - prev_cost) / std::fmax(prev_cost, 1e-7) < p.relative_cost_tol) {
    stop_reason = PGO_GNC_STOP_COST;
    return false;
  }
  if (outer >= p.max_iterations) {
    stop_reason = PGO_GNC_STOP_MAX_ITER;
    return false;
  }
  mu = p.loss == PGO_GNC_GM ? std::fmax(1.0, mu / p.mu_step) : mu * p.mu_step;
  prev_cost = cost;
  return true;
}

}  // namespace pgo

extern "C" {

void pgo_gnc_default_params(pgo_gnc_params* p) {
  if (!p) return;
  p->loss = PGO_GNC_GM;
  p->barc_sq = 11.344866730144373;   // chi2inv(0.99, 3)
  p->mu_step = 1.4;
  p->max_iterations = 100;
  p->relative_cost_tol = 1e-5;
  p->weights_tol = 1e-4;
  p->keep_weights = 1;
}

int pgo_debug_gnc_weight(int loss, double mu, double barc_sq, size_t n, const double* r2, double* w) {
  if ((loss != PGO_GNC_GM && loss != PGO_GNC_TLS) || (n && (!r2 || !w))) return PGO_E_ARG;
  for (size_t i = 0; i < n; i++) w[i] = pgo::gnc_weight(loss, mu, barc_sq, r2[i]);
  return PGO_OK;
}

int pgo_debug_gnc_control(const pgo_gnc_params* params, double initial_error, int rows, const double* rmax_sq,
                          const double* cost, const double* nonbinary, double* mu_out, int* stop_out) {
  (void)initial_error;   // (the error before row 0: reported by the driver, no rule reads it)
  if (!params || rows < 1 || !rmax_sq || !cost || !nonbinary || !mu_out || !stop_out) return PGO_E_ARG;
  if (!pgo::gnc_params_ok(*params)) return PGO_E_ARG;
  pgo::GncControl ctl(*params);
  mu_out[0] = NAN;
  *stop_out = -1;   // the control asked for a row past the recorded ones
  if (!ctl.start(cost[0], rmax_sq[0])) {
    *stop_out = ctl.stop_reason;
    return 1;
  }
  for (int r = 1; r < rows; r++) {
    mu_out[r] = ctl.mu;
    if (!ctl.step(cost[r], nonbinary[r])) {
      *stop_out = ctl.stop_reason;
      return r + 1;
    }
  }
  return rows;
}

}  // extern "C"
