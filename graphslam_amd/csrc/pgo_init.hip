// HIP kernels of the two-stage linear initialisation (pgo_initialize_linear,
// gfx950): the assembly of the two linear systems and the write-back of their
// solutions.  DESIGN.md, "Linear initialisation".
//
// Both systems have one block per between factor and per vertex, like H, so
// each is written into the Cholesky-mode linearisation's layout -- D (6 per
// row), the owner slot's record V[9 e + q], the right-hand side in d.g -- and
// the plan, the tile assembly, the factorisation and the solve run unchanged:
//   stage 1 (orientations): scalar system in the theta slot, the (x, y) slots
//     an identity:  off-diagonal diag(0, 0, -w_e), diagonal diag(1, 1, sum w);
//   stage 2 (positions): 2x2 system in the (x, y) slots, the theta slot an
//     identity:  off-diagonal [[-M, 0], [0, 0]], diagonal [[sum M, 0], [0, 1]].
// Both off-diagonal blocks are symmetric: the owner block's orientation
// (eside) does not matter.  Robust losses are ignored.
//
// The sweeps are k_linearize's: one sub-group of G lanes per vertex row, one
// lane per slot, fixed-order sub-group sums, lane 0 adds the row's priors; no
// atomics, bitwise reproducible run to run.
#include <hip/hip_ext.h>
#include <math.h>

#include "pgo_device.h"

namespace pgo {

namespace {

template <int G>
__device__ __forceinline__ double sg_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

// GTSAM Rot2::normalize (as pgo_kernels.hip)
__device__ __forceinline__ void rot_normalize(double& c, double& s) {
  const double scale = c * c + s * s;
  if (fabs(scale - 1.0) > 1e-10) {
    const double f = 1.0 / sqrt(scale);
    c *= f;
    s *= f;
  }
}

// information of theta with the translation marginalised out:
// o22 - (o02, o12) Omega_tt^-1 (o02, o12)'
__device__ __forceinline__ double theta_information(double o00, double o01, double o02, double o11, double o12,
                                                    double o22) {
  const double det = o00 * o11 - o01 * o01;
  return o22 - (o11 * o02 * o02 - 2.0 * o01 * o02 * o12 + o00 * o12 * o12) / det;
}

}  // namespace

// Stage 1: sum_e w_e (theta_j - theta_i - tgt_e)^2 + sum_q w_q (theta_v - ptgt_q)^2
// with tgt_e = delta_e + 2 pi k_e (device factor order) and ptgt_q = theta_q +
// 2 pi k_q (device prior order) from the host's spanning tree.  Reads no pose.
template <int G>
__global__ __launch_bounds__(kThreads) void k_init_orient(DevGraph d, const double* __restrict__ tgt,
                                                         const double* __restrict__ ptgt) {
  const int lane = threadIdx.x & (G - 1);
  const int nsg = gridDim.x * (kThreads / G);
  for (int row = (blockIdx.x * kThreads + threadIdx.x) / G; row < d.n; row += nsg) {
    double a = 0, b = 0;
    const int beg = d.row_ptr[row], end = d.row_ptr[row + 1];
    for (int k = beg + lane; k < end; k += G) {
      const int se = d.slot_edge[k], e = se >> 2;
      const double2 oA = d.eom[3 * e], oB = d.eom[3 * e + 1], oC = d.eom[3 * e + 2];
      const double w = theta_information(oA.x, oA.y, oB.x, oB.y, oC.x, oC.y);
      const double t = w * tgt[e];
      if (se & 2) {   // the owner slot: the factor's record
        double* v = d.V + 9 * (size_t)e;
        v[0] = 0; v[1] = 0; v[2] = 0; v[3] = 0; v[4] = 0; v[5] = 0; v[6] = 0; v[7] = 0; v[8] = -w;
      }
      a += w;
      b += (se & 1) ? t : -t;   // row ej: + w tgt; row ei: - w tgt
    }
    if (lane == 0) {
      for (int q = d.prior_ptr[row]; q < d.prior_ptr[row + 1]; q++) {
        const double2 oA = d.pom[3 * q], oB = d.pom[3 * q + 1], oC = d.pom[3 * q + 2];
        const double w = theta_information(oA.x, oA.y, oB.x, oB.y, oC.x, oC.y);
        a += w;
        b += w * ptgt[q];
      }
    }
    a = sg_sum<G>(a);
    b = sg_sum<G>(b);
    if (lane == 0) {
      double* D = d.D + 6 * (size_t)row;
      D[0] = 1.0; D[1] = 0.0; D[2] = 0.0; D[3] = 1.0; D[4] = 0.0; D[5] = a;
      double* g = d.g + 3 * (size_t)row;
      g[0] = 0.0; g[1] = 0.0; g[2] = b;
    }
  }
}

// Stage 2: the graph's Gaussian error over the positions with every rotation
// held at pose's (c, s) -- the only part of pose it reads.  Per factor (i, j, z):
//   A = R_z' R_i',  c = R_z' t_z,  e_th = the factor's angle residual,
//   M = A' Omega_tt A,  r = A' (Omega_tt c - Omega_tth e_th);
//   H_ii += M, H_jj += M, H_ij = -M, b_j += r, b_i -= r.
// Per prior (v, p_q):  M_q = R_v Omega_tt R_v',  H_vv += M_q,
//   b_v += M_q p_q - R_v Omega_tth e_th.
// The unknowns are the absolute positions.
template <int G>
__global__ __launch_bounds__(kThreads) void k_init_trans(DevGraph d, const double4* __restrict__ pose) {
  const int lane = threadIdx.x & (G - 1);
  const int nsg = gridDim.x * (kThreads / G);
  for (int row = (blockIdx.x * kThreads + threadIdx.x) / G; row < d.n; row += nsg) {
    double a00 = 0, a01 = 0, a11 = 0, g0 = 0, g1 = 0;
    const int beg = d.row_ptr[row], end = d.row_ptr[row + 1];
#pragma unroll 1
    for (int k = beg + lane; k < end; k += G) {
      const int se = d.slot_edge[k], e = se >> 2;
      const int2 ij = d.eij[e];
      const double4 p1 = pose[ij.x], p2 = pose[ij.y], z = d.ez[e];
      const double2 oA = d.eom[3 * e], oB = d.eom[3 * e + 1], oC = d.eom[3 * e + 2];
      const double o00 = oA.x, o01 = oA.y, o02 = oB.x, o11 = oB.y, o12 = oC.x;
      // e_th as k_error forms it: theta of z^-1 (R_i' R_j)
      double hc = p1.z * p2.z + p1.w * p2.w, hs = -p1.w * p2.z + p1.z * p2.w;
      rot_normalize(hc, hs);
      double ec = z.z * hc + z.w * hs, es = -z.w * hc + z.z * hs;
      rot_normalize(ec, es);
      const double eth = atan2(es, ec);
      // A = R_z' R_i' = [[ca, sa], [-sa, ca]]
      const double ca = p1.z * z.z - p1.w * z.w, sa = p1.w * z.z + p1.z * z.w;
      // B = Omega_tt A, M = A' B (symmetric: one off-diagonal value for both)
      const double b00 = o00 * ca - o01 * sa, b01 = o00 * sa + o01 * ca;
      const double b10 = o01 * ca - o11 * sa, b11 = o01 * sa + o11 * ca;
      const double m00 = ca * b00 - sa * b10, m01 = ca * b01 - sa * b11, m11 = sa * b01 + ca * b11;
      const double cx = z.z * z.x + z.w * z.y, cy = -z.w * z.x + z.z * z.y;
      const double u0 = o00 * cx + o01 * cy - o02 * eth, u1 = o01 * cx + o11 * cy - o12 * eth;
      const double r0 = ca * u0 - sa * u1, r1 = sa * u0 + ca * u1;
      if (se & 2) {   // the owner slot: the factor's record
        double* v = d.V + 9 * (size_t)e;
        v[0] = -m00; v[1] = -m01; v[2] = 0; v[3] = -m01; v[4] = -m11; v[5] = 0; v[6] = 0; v[7] = 0; v[8] = 0;
      }
      a00 += m00; a01 += m01; a11 += m11;
      if (se & 1) { g0 += r0; g1 += r1; }   // row ej
      else { g0 -= r0; g1 -= r1; }          // row ei
    }
    if (lane == 0) {
      for (int q = d.prior_ptr[row]; q < d.prior_ptr[row + 1]; q++) {
        const double4 x = pose[row], pz = d.pz[q];
        const double2 oA = d.pom[3 * q], oB = d.pom[3 * q + 1], oC = d.pom[3 * q + 2];
        const double o00 = oA.x, o01 = oA.y, o02 = oB.x, o11 = oB.y, o12 = oC.x;
        double c = x.z * pz.z + x.w * pz.w, s = -x.w * pz.z + x.z * pz.w;
        rot_normalize(c, s);
        const double eth = -atan2(s, c);   // PriorFactor: e = -Local(x, prior)
        // T = Omega_tt R_v', M_q = R_v T
        const double t00 = o00 * x.z - o01 * x.w, t01 = o00 * x.w + o01 * x.z;
        const double t10 = o01 * x.z - o11 * x.w, t11 = o01 * x.w + o11 * x.z;
        const double m00 = x.z * t00 - x.w * t10, m01 = x.z * t01 - x.w * t11, m11 = x.w * t01 + x.z * t11;
        const double v0 = o02 * eth, v1 = o12 * eth;
        a00 += m00; a01 += m01; a11 += m11;
        g0 += m00 * pz.x + m01 * pz.y - (x.z * v0 - x.w * v1);
        g1 += m01 * pz.x + m11 * pz.y - (x.w * v0 + x.z * v1);
      }
    }
    a00 = sg_sum<G>(a00); a01 = sg_sum<G>(a01); a11 = sg_sum<G>(a11);
    g0 = sg_sum<G>(g0); g1 = sg_sum<G>(g1);
    if (lane == 0) {
      double* D = d.D + 6 * (size_t)row;
      D[0] = a00; D[1] = a01; D[2] = 0.0; D[3] = a11; D[4] = 0.0; D[5] = 1.0;
      double* g = d.g + 3 * (size_t)row;
      g[0] = g0; g[1] = g1; g[2] = 0.0;
    }
  }
}

// theta-hat (the theta slot of stage 1's solution, not wrapped) -> Rot2(c, s)
__global__ __launch_bounds__(kThreads) void k_init_write_orient(int n, const double* __restrict__ x,
                                                               double4* __restrict__ out) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    double s, c;
    sincos(x[3 * (size_t)i + 2], &s, &c);
    out[i] = make_double4(0.0, 0.0, c, s);
  }
}

// p-hat (the x, y slots of stage 2's solution) beside the orientations already in out
__global__ __launch_bounds__(kThreads) void k_init_write_trans(int n, const double* __restrict__ x,
                                                              double4* __restrict__ out) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    out[i].x = x[3 * (size_t)i];
    out[i].y = x[3 * (size_t)i + 1];
  }
}

// ------------------------------------------------------------ launchers
#define PGO_INIT_DISPATCH_G(KERNEL, ...)                                         \
  switch (d.G) {                                                                 \
    case 4: KERNEL<4><<<grid, kThreads, 0, d.stream>>>(__VA_ARGS__); break;      \
    case 8: KERNEL<8><<<grid, kThreads, 0, d.stream>>>(__VA_ARGS__); break;      \
    case 16: KERNEL<16><<<grid, kThreads, 0, d.stream>>>(__VA_ARGS__); break;    \
    default: KERNEL<32><<<grid, kThreads, 0, d.stream>>>(__VA_ARGS__); break;    \
  }

hipError_t launch_init_orient(const DevGraph& d, const double* tgt, const double* ptgt) {
  if (d.n == 0) return hipSuccess;
  const dim3 grid((unsigned)grid_rows(d));
  PGO_INIT_DISPATCH_G(k_init_orient, d, tgt, ptgt);
  return hipGetLastError();
}

hipError_t launch_init_trans(const DevGraph& d, const double4* pose) {
  if (d.n == 0) return hipSuccess;
  const dim3 grid((unsigned)grid_rows(d));
  PGO_INIT_DISPATCH_G(k_init_trans, d, pose);
  return hipGetLastError();
}

hipError_t launch_init_write_orient(const DevGraph& d, const double* x, double4* out) {
  if (d.n == 0) return hipSuccess;
  k_init_write_orient<<<grid_for(d.n), kThreads, 0, d.stream>>>(d.n, x, out);
  return hipGetLastError();
}

hipError_t launch_init_write_trans(const DevGraph& d, const double* x, double4* out) {
  if (d.n == 0) return hipSuccess;
  k_init_write_trans<<<grid_for(d.n), kThreads, 0, d.stream>>>(d.n, x, out);
  return hipGetLastError();
}

}  // namespace pgo
