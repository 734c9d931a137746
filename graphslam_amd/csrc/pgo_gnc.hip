// The weights sweep of graduated non-convexity (pgo_optimize_gnc, gfx950).
//
// One thread per device factor with a grid stride.  A candidate's r^2 =
// e'Omega e comes from between_lin and the unscaled Omega exactly as in
// k_error_robust; its weight under the surrogate of the current mu
// (gnc_weight, pgo_gnc.h: the code the host tests pin) goes into d.ek when
// `write` is set, where the robust linearisation and error kernels read it
// as a fixed weight (kLossFixed).  Every other factor's ek stays as it is.
//
// Five values are reduced in the project's two-stage fixed order: xor
// butterflies inside a wave, one LDS word per wave, one partial per block
// (d.part slices 0..4), then k_gnc_reduce over the partials.  No atomics;
// results repeat bitwise run to run.  Launched eagerly between the inner
// optimizes, never inside a captured graph.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pgo_device.h"
#include "pgo_gnc.h"
#include "pgo_kernel_common.h"

namespace pgo {

constexpr int kPartGnc = 0;   // slices 0..4: free between optimizes (the PCG and error launches own
                              // them only while they run, stream-ordered before and after the sweep)
constexpr int kGncValues = 5;

__device__ __forceinline__ double block_max(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = lds[0];
#pragma unroll
  for (int i = 1; i < kThreads / 64; i++) s = fmax(s, lds[i]);
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kThreads) void k_gnc_weights(DevGraph d, const double4* __restrict__ pose,
                                                          const unsigned char* __restrict__ cand, int loss,
                                                          double mu, double c2, double wtol, int write) {
  __shared__ double lds[kThreads / 64];
  double rmax = 0.0, sw = 0.0, nonbin = 0.0, nout = 0.0, ncand = 0.0;
  for (int t = blockIdx.x * kThreads + threadIdx.x; t < d.ne; t += gridDim.x * kThreads) {
    if (!cand[t]) continue;
    const int2 ij = d.eij[t];
    const BetweenLin b = between_lin(pose[ij.x], pose[ij.y], d.ez[t]);
    const double2 oA = d.eom[3 * t], oB = d.eom[3 * t + 1], oC = d.eom[3 * t + 2];
    const double u0 = oA.x * b.e0 + oA.y * b.e1 + oB.x * b.e2;
    const double u1 = oA.y * b.e0 + oB.y * b.e1 + oC.x * b.e2;
    const double u2 = oB.x * b.e0 + oC.x * b.e1 + oC.y * b.e2;
    const double r2 = b.e0 * u0 + b.e1 * u1 + b.e2 * u2;
    const double w = gnc_weight(loss, mu, c2, r2);
    if (write) d.ek[t] = w;
    rmax = fmax(rmax, r2);
    sw += w;
    nonbin += gnc_nonbinary(w, wtol) ? 1.0 : 0.0;
    nout += r2 > c2 ? 1.0 : 0.0;
    ncand += 1.0;
  }
  rmax = block_max(rmax, lds);
  sw = block_sum(sw, lds);
  nonbin = block_sum(nonbin, lds);
  nout = block_sum(nout, lds);
  ncand = block_sum(ncand, lds);
  if (threadIdx.x == 0) {
    d.part[(kPartGnc + 0) * kMaxBlocks + blockIdx.x] = rmax;
    d.part[(kPartGnc + 1) * kMaxBlocks + blockIdx.x] = sw;
    d.part[(kPartGnc + 2) * kMaxBlocks + blockIdx.x] = nonbin;
    d.part[(kPartGnc + 3) * kMaxBlocks + blockIdx.x] = nout;
    d.part[(kPartGnc + 4) * kMaxBlocks + blockIdx.x] = ncand;
  }
}

// Single block: out[0] the max of slice 0's nb partials, out[1..4] the sums of
// slices 1..4 (k_reduce's order; the counts are whole numbers below 2^53, exact).
__global__ __launch_bounds__(kThreads) void k_gnc_reduce(const double* __restrict__ part, int nb,
                                                         double* __restrict__ out) {
  __shared__ double lds[kThreads / 64];
  double m = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) m = fmax(m, part[(size_t)kPartGnc * kMaxBlocks + i]);
  m = block_max(m, lds);
  if (threadIdx.x == 0) out[0] = m;
  for (int v = 1; v < kGncValues; v++) {
    const double s = sum_partials(part + (size_t)(kPartGnc + v) * kMaxBlocks, nb, lds);
    if (threadIdx.x == 0) out[v] = s;
  }
}

hipError_t launch_gnc_weights(const DevGraph& d, const double4* pose, const unsigned char* cand, int loss,
                              double mu, double c2, double wtol, int write, double* out5) {
  if (!cand || !pose || !out5 || !d.part || (write && !d.ek)) return hipErrorInvalidValue;
  const int nb = grid_for(d.ne);
  k_gnc_weights<<<nb, kThreads, 0, d.stream>>>(d, pose, cand, loss, mu, c2, wtol, write);
  k_gnc_reduce<<<1, kThreads, 0, d.stream>>>(d.part, nb, out5);
  return hipGetLastError();
}

}  // namespace pgo
