// Graduated non-convexity (pgo_optimize_gnc): the weight of a candidate factor
// as a function of its r^2 = e'Omega e under the surrogate of the current mu,
// and the outer loop's control -- the initial mu, the mu schedule, the stop
// rules -- as pure host arithmetic on scalars.  pgo_optimize_gnc owns the device
// and the inner solves and asks this module what comes next; gnc_selftest.cpp
// and pgo_debug_gnc_control / pgo_debug_gnc_weight drive it without a device.
// The weight formulas are host + device inlines: the sweep kernel
// (pgo_gnc.hip) runs the code the host tests pin.  No HIP types.
#pragma once

#include <math.h>

#include "pgo.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PGO_GNC_HD __host__ __device__
#else
#define PGO_GNC_HD
#endif

namespace pgo {

// TLS: the weight is 1 up to lo and 0 from up on, lo = mu / (mu + 1) c^2,
// up = (mu + 1) / mu c^2.
PGO_GNC_HD inline double gnc_tls_lo(double mu, double c2) { return mu / (mu + 1.0) * c2; }
PGO_GNC_HD inline double gnc_tls_up(double mu, double c2) { return (mu + 1.0) / mu * c2; }

// GM:  w = (mu c^2 / (r^2 + mu c^2))^2
// TLS: w = 1 (r^2 <= lo), 0 (r^2 >= up), else sqrt(c^2 mu (mu + 1) / r^2) - mu
PGO_GNC_HD inline double gnc_weight(int loss, double mu, double c2, double r2) {
  if (loss == PGO_GNC_GM) {
    const double a = mu * c2;
    const double t = a / (r2 + a);
    return t * t;
  }
  if (r2 <= gnc_tls_lo(mu, c2)) return 1.0;
  if (r2 >= gnc_tls_up(mu, c2)) return 0.0;
  return sqrt(c2 * mu * (mu + 1.0) / r2) - mu;
}

// a weight that is neither 0 nor 1 to within tol
PGO_GNC_HD inline bool gnc_nonbinary(double w, double tol) { return w > tol && w < 1.0 - tol; }

// unknown loss, barc_sq <= 0, mu_step <= 1, max_iterations < 0, a negative or
// non-finite tolerance (or a non-finite barc_sq / mu_step)
bool gnc_params_ok(const pgo_gnc_params& p);

class GncControl {
 public:
  explicit GncControl(const pgo_gnc_params& p) : p(p) {}

  // After row 0 (the plain inner solve, cost0 its final error) and the sweep at
  // its result (rmax_sq over the candidates): the initial mu.  False: nothing
  // to iterate (stop_reason set: ALL_INLIERS, or MAX_ITER with max_iterations 0).
  bool start(double cost0, double rmax_sq);
  // After the inner solve of outer iteration `outer + 1` at `mu`: its cost and
  // the non-binary weights the sweep that wrote the weights counted.  True:
  // another iteration follows at the new mu; false: stop_reason says why.
  bool step(double cost, double nonbinary);

  pgo_gnc_params p;
  double mu = NAN, mu_initial = NAN, prev_cost = 0.0;
  int outer = 0;                          // finished outer iterations
  int stop_reason = PGO_GNC_STOP_MAX_ITER;
};

}  // namespace pgo
