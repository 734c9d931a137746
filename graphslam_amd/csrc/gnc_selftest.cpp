// Stand-alone host self-test of the GNC control and weight formulas
// (pgo_gnc.h / pgo_gnc.cpp): no device, no handle.  Built with ASan + UBSan by
// `make asan-gnc` and run by tests/test_gnc_host.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pgo_gnc.h"

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      failures++;                                                  \
    }                                                              \
  } while (0)

int main() {
  pgo_gnc_params p;
  pgo_gnc_default_params(&p);
  CHECK(p.loss == PGO_GNC_GM && p.barc_sq == 11.344866730144373 && p.mu_step == 1.4 && p.max_iterations == 100);
  CHECK(p.relative_cost_tol == 1e-5 && p.weights_tol == 1e-4 && p.keep_weights == 1);
  CHECK(pgo::gnc_params_ok(p));
  {   // every rejected parameter
    pgo_gnc_params q = p;
    q.loss = 2; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.loss = -1; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.barc_sq = 0.0; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.barc_sq = NAN; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.mu_step = 1.0; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.mu_step = INFINITY; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.max_iterations = -1; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.relative_cost_tol = -1e-9; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.weights_tol = NAN; CHECK(!pgo::gnc_params_ok(q)); q = p;
    q.max_iterations = 0; CHECK(pgo::gnc_params_ok(q));
  }
  const double c2 = p.barc_sq;
  const double mu100 = 2.0 * (50.0 * c2) / c2;   // GM's initial mu for rmax_sq = 50 c^2 (100 up to rounding)
  // weights: GM is 1 at r^2 = 0, 1/4 at r^2 = mu c^2, decreasing, 0 far out
  for (double mu : {1e-6, 1.0, 1.4, 1e6}) {
    CHECK(pgo::gnc_weight(PGO_GNC_GM, mu, c2, 0.0) == 1.0);
    CHECK(std::fabs(pgo::gnc_weight(PGO_GNC_GM, mu, c2, mu * c2) - 0.25) < 1e-15);
    CHECK(pgo::gnc_weight(PGO_GNC_GM, mu, c2, 1e300) == 0.0);
    double prev = 1.0;
    for (int i = 1; i < 200; i++) {
      const double w = pgo::gnc_weight(PGO_GNC_GM, mu, c2, mu * c2 * i * 0.1);
      CHECK(w <= prev && w > 0.0);
      prev = w;
    }
    // TLS: exactly 1 up to lo, exactly 0 from up on, inside [0, 1] and continuous between
    const double lo = pgo::gnc_tls_lo(mu, c2), up = pgo::gnc_tls_up(mu, c2);
    CHECK(lo < c2 && c2 < up);
    CHECK(pgo::gnc_weight(PGO_GNC_TLS, mu, c2, 0.0) == 1.0);
    CHECK(pgo::gnc_weight(PGO_GNC_TLS, mu, c2, lo) == 1.0);
    CHECK(pgo::gnc_weight(PGO_GNC_TLS, mu, c2, up) == 0.0);
    CHECK(pgo::gnc_weight(PGO_GNC_TLS, mu, c2, 1e300) == 0.0);
    const double wl = pgo::gnc_weight(PGO_GNC_TLS, mu, c2, std::nextafter(lo, up));
    const double wu = pgo::gnc_weight(PGO_GNC_TLS, mu, c2, std::nextafter(up, lo));
    CHECK(std::fabs(wl - 1.0) <= 1e-9 * (1.0 + mu) && std::fabs(wu) <= 1e-9 * (1.0 + mu));
    const double wc = pgo::gnc_weight(PGO_GNC_TLS, mu, c2, c2);   // at r^2 = c^2: sqrt(mu (mu + 1)) - mu
    CHECK(std::fabs(wc - (std::sqrt(mu * (mu + 1.0)) - mu)) <= 1e-9 * (1.0 + mu));
  }
  CHECK(pgo::gnc_nonbinary(0.5, 1e-4) && !pgo::gnc_nonbinary(1e-4, 1e-4) && !pgo::gnc_nonbinary(1.0 - 1e-4, 1e-4));
  CHECK(!pgo::gnc_nonbinary(0.0, 0.0) && !pgo::gnc_nonbinary(1.0, 0.0) && pgo::gnc_nonbinary(1e-300, 0.0));

  {   // GM schedule: mu0 = 2 rmax / c^2, divided by mu_step down to exactly 1, then STOP_MU
    pgo::GncControl ctl(p);
    CHECK(ctl.start(100.0, 50.0 * c2));
    CHECK(ctl.mu == mu100 && ctl.mu_initial == mu100 && std::fabs(mu100 - 100.0) < 1e-12);
    double cost = 100.0;
    int rows = 0;
    double last = ctl.mu;
    while (true) {
      cost *= 0.9;   // (a 10 % change: the cost rule stays quiet)
      rows++;
      last = ctl.mu;
      if (!ctl.step(cost, 0.0)) break;
      CHECK(ctl.mu == std::fmax(1.0, last / 1.4));
    }
    CHECK(ctl.stop_reason == PGO_GNC_STOP_MU && last == 1.0 && ctl.outer == rows);
    CHECK(rows == 15);   // 100 / 1.4^13 = 1.26, / 1.4 -> max(1, 0.9) = 1: the 15th solve runs at mu 1
  }
  {   // GM with every residual small: mu0 = 1, one iteration
    pgo::GncControl ctl(p);
    CHECK(ctl.start(1.0, 0.1));
    CHECK(ctl.mu == 1.0);
    CHECK(!ctl.step(0.5, 0.0) && ctl.stop_reason == PGO_GNC_STOP_MU && ctl.outer == 1);
  }
  {   // cost rule, and prev_cost 0 guarded by 1e-7
    pgo::GncControl ctl(p);
    CHECK(ctl.start(10.0, 50.0 * c2));
    CHECK(ctl.step(9.0, 0.0));
    CHECK(!ctl.step(9.0 * (1.0 - 0.9e-5), 0.0) && ctl.stop_reason == PGO_GNC_STOP_COST && ctl.outer == 2);
    pgo::GncControl z(p);
    CHECK(z.start(0.0, 50.0 * c2));
    CHECK(!z.step(1e-13, 0.0) && z.stop_reason == PGO_GNC_STOP_COST);
  }
  {   // max_iterations, 0 included
    pgo_gnc_params q = p;
    q.max_iterations = 2;
    pgo::GncControl ctl(q);
    CHECK(ctl.start(10.0, 50.0 * c2));
    CHECK(ctl.step(9.0, 0.0));
    CHECK(!ctl.step(8.0, 0.0) && ctl.stop_reason == PGO_GNC_STOP_MAX_ITER && ctl.outer == 2);
    q.max_iterations = 0;
    pgo::GncControl none(q);
    CHECK(!none.start(10.0, 50.0 * c2) && none.stop_reason == PGO_GNC_STOP_MAX_ITER && none.mu_initial == mu100);
  }
  {   // TLS: mu0 = c^2 / (2 rmax - c^2), multiplied; the degenerate starts
    pgo_gnc_params q = p;
    q.loss = PGO_GNC_TLS;
    pgo::GncControl ctl(q);
    CHECK(ctl.start(10.0, 3.0 * c2));
    CHECK(ctl.mu == c2 / (2.0 * (3.0 * c2) - c2));
    const double m0 = ctl.mu;
    CHECK(ctl.step(9.0, 3.0));
    CHECK(ctl.mu == m0 * 1.4);
    CHECK(!ctl.step(8.0, 0.0) && ctl.stop_reason == PGO_GNC_STOP_MU);
    for (double rmax : {0.0, 0.25 * c2, 0.5 * c2, (double)NAN, (double)INFINITY}) {
      pgo::GncControl a(q);
      const bool go = a.start(10.0, rmax);
      if (std::isinf(rmax)) CHECK(!go && a.stop_reason == PGO_GNC_STOP_ALL_INLIERS);   // mu = 0: not positive
      else CHECK(!go && a.stop_reason == PGO_GNC_STOP_ALL_INLIERS && std::isnan(a.mu_initial));
    }
  }
  {   // the recorded-rows entry agrees with the class
    const double rmax[4] = {50.0 * c2, 0, 0, 0}, cost[4] = {10.0, 9.0, 8.0, 8.0}, nb[4] = {0, 0, 0, 0};
    double mu[4];
    int stop = 99;
    CHECK(pgo_debug_gnc_control(&p, 20.0, 4, rmax, cost, nb, mu, &stop) == 4);
    CHECK(stop == PGO_GNC_STOP_COST && std::isnan(mu[0]) && mu[1] == mu100 && mu[2] == mu100 / 1.4);
    CHECK(pgo_debug_gnc_control(&p, 20.0, 2, rmax, cost, nb, mu, &stop) == 2 && stop == -1);
    CHECK(pgo_debug_gnc_control(&p, 20.0, 0, rmax, cost, nb, mu, &stop) == PGO_E_ARG);
    std::vector<double> r2 = {0.0, 1.0, c2, 1e300}, w(4);
    CHECK(pgo_debug_gnc_weight(PGO_GNC_TLS, 1.0, c2, r2.size(), r2.data(), w.data()) == PGO_OK);
    CHECK(w[0] == 1.0 && w[1] == 1.0 && w[3] == 0.0 && w[2] > 0.0 && w[2] < 1.0);
    CHECK(pgo_debug_gnc_weight(7, 1.0, c2, r2.size(), r2.data(), w.data()) == PGO_E_ARG);
  }
  if (failures) {
    std::printf("gnc selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("gnc selftest ok\n");
  return 0;
}
