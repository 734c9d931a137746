// Device helpers shared by the kernel files (pgo_kernels.hip, pgo_gnc.hip): the
// Pose2 rotation normalisation, the fixed-order reductions and the between
// factor's residual.  Everything is a forced inline: a kernel that uses them
// compiles to what it did when they were defined beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pgo_device.h"

namespace pgo {

// ------------------------------------------------------------ Pose2 helpers
// GTSAM Rot2::normalize: rescale only when |c^2+s^2-1| > 1e-10.
__device__ __forceinline__ void rot_normalize(double& c, double& s) {
  const double scale = c * c + s * s;
  if (fabs(scale - 1.0) > 1e-10) {
    const double f = 1.0 / sqrt(scale);   // pow(scale, -0.5) up to rounding; taken only off the unit circle
    c *= f;
    s *= f;
  }
}

// ------------------------------------------------------------ reductions
template <int G>
__device__ __forceinline__ double sg_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;  // bit-identical in every lane of the sub-group
}

__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = sg_sum<64>(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kThreads / 64; i++) s += lds[i];
  __syncthreads();
  return s;
}

// Sum of nb block partials; every block obtains the bit-identical value.
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nb, double* lds) {
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) v += part[i];
  return block_sum(v, lds);
}

// ------------------------------------------------------------ between factor
// Residual of between factor (p1, p2, z) and the terms of J1 (J2 = I), as in
// k_linearize.
struct BetweenLin {
  double e0, e1, e2, hc, hs, dt1, dt2;
};

__device__ __forceinline__ BetweenLin between_lin(const double4 p1, const double4 p2, const double4 z) {
  BetweenLin b;
  double hc = p1.z * p2.z + p1.w * p2.w, hs = -p1.w * p2.z + p1.z * p2.w;
  rot_normalize(hc, hs);
  const double dx = p2.x - p1.x, dy = p2.y - p1.y;
  const double hx = p1.z * dx + p1.w * dy, hy = -p1.w * dx + p1.z * dy;
  double ec = z.z * hc + z.w * hs, es = -z.w * hc + z.z * hs;
  rot_normalize(ec, es);
  const double tx = hx - z.x, ty = hy - z.y;
  b.e0 = z.z * tx + z.w * ty;
  b.e1 = -z.w * tx + z.z * ty;
  b.e2 = atan2(es, ec);
  b.hc = hc;
  b.hs = hs;
  b.dt1 = -p2.w * dx + p2.z * dy;
  b.dt2 = -p2.z * dx - p2.w * dy;
  return b;
}

}  // namespace pgo
