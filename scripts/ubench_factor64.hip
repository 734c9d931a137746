// Microbenchmark of the diagonal tile's factor + inverse on the panel chain
// (diag_factor_invert: 16-column blocks, wave 0's 16x16 blocks by diag16_fs):
// one workgroup, an SPD tile, clock64 stamps (PGO_DIAG_CLOCKS).  Checks
// X A X^T = I for live sizes 64, 37, 8 and 1.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include scripts/ubench_factor64.hip -o graphslam_amd/build/ubench_factor64
#define PGO_DIAG_CLOCKS 1
#include "../graphslam_amd/csrc/pgo_chol.hip"

#include <cstdio>
#include <vector>
#include <cmath>
#include <algorithm>

using namespace pgo;

__global__ __launch_bounds__(256) void u_factor(const double* A, double* out, int reps, int nbl, double* LX = nullptr) {
  __shared__ __attribute__((aligned(16))) double T[64 * 65], W[64 * 65], bc[64];
  for (int rep = 0; rep < reps; rep++) {
    for (int i = threadIdx.x; i < 64 * 65; i += 256) {
      const int r = i % 65, cc = i / 65;
      T[i] = r < 64 ? ((r < nbl && cc < nbl) ? A[r + 64 * cc] : (r == cc ? 1.0 : 0.0)) : 0.0;
      W[i] = 0.0;
    }
    __syncthreads();
    const int bad = diag_factor_invert(T, W, bc, nbl) ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) out[0] += W[63 + 63 * 65] + bad;
    if (threadIdx.x == 0 && bad) out[1] += bad;
  }
  if (LX)
    for (int i = threadIdx.x; i < 4096; i += 256) LX[i] = W[(i & 63) + (i >> 6) * 65];
}

static double check(const std::vector<double>& A, const double* X, int n) {
  std::vector<double> XA(4096, 0.0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      double s = 0;
      for (int k = 0; k <= i; k++) s += X[i + 64 * k] * A[k + 64 * j];
      XA[i + 64 * j] = s;
    }
  double e1 = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      double s = 0;
      for (int k = 0; k <= j; k++) s += XA[i + 64 * k] * X[j + 64 * k];
      e1 = std::max(e1, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  double up = 0;
  for (int i = 0; i < 64; i++)
    for (int j = i + 1; j < 64; j++) up = std::max(up, std::fabs(X[i + 64 * j]));
  printf("  max |X A X^T - I| %.3g  max |X upper| %.3g\n", e1, up);
  return e1;
}

int main() {
  std::vector<double> A(64 * 64);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) * (1.0 / 16777216.0) - 0.5; };
  std::vector<double> B(64 * 64);
  for (auto& v : B) v = rnd();
  for (int i = 0; i < 64; i++)   // A = B B^T + 2 I + a Hilbert-like part
    for (int j = 0; j < 64; j++) {
      double t = 0;
      for (int k = 0; k < 64; k++) t += B[i + 64 * k] * B[j + 64 * k];
      A[i + 64 * j] = t + (i == j ? 2.0 : 0.0) + 1.0 / (1.0 + i + j);
    }
  double *dA, *dO, *dLX;
  hipMalloc(&dA, sizeof(double) * 4096);
  hipMalloc(&dO, 2 * sizeof(double));
  hipMalloc(&dLX, sizeof(double) * 4096);
  hipMemcpy(dA, A.data(), sizeof(double) * 4096, hipMemcpyHostToDevice);
  int fail = 0;
  for (int nbl : {64, 37, 8, 1}) {
    std::vector<double> X(4096);
    hipMemset(dO, 0, 2 * sizeof(double));
    u_factor<<<1, 256>>>(dA, dO, 1, nbl, dLX);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
    double o[2];
    hipMemcpy(o, dO, 2 * sizeof(double), hipMemcpyDeviceToHost);
    hipMemcpy(X.data(), dLX, sizeof(double) * 4096, hipMemcpyDeviceToHost);
    printf("nbl %d bad %.0f\n", nbl, o[1]);
    if (check(A, X.data(), nbl) > 1e-9 || o[1] != 0) fail = 1;
  }
  u_factor<<<1, 256>>>(dA, dO, 3, 64);
  hipDeviceSynchronize();
  long long clk[32];
  hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_diag_clk), sizeof(clk));
  printf("total %lld cycles\n", clk[12] - clk[0]);
  long long prev = clk[0];
  for (int J = 0; J < 4; J++) {   // A: wave 0's diagonal block (+ the update before it), B: the panel / inverse-row products
    const long long b = J < 3 ? clk[2 + 3 * J] : clk[12];
    printf("  J%d A %lld  B %lld\n", J, clk[1 + 3 * J] - prev, b - clk[1 + 3 * J]);
    prev = b;
  }
  printf("  diag16_fs (J3, fenced): chol8 %lld, fwd+store %lld, A22/Y+load %lld, chol8 %lld, fwd+store %lld\n",
         clk[21] - clk[20], clk[22] - clk[21], clk[23] - clk[22], clk[24] - clk[23], clk[25] - clk[24]);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0);
  u_factor<<<1, 256>>>(dA, dO, 100, 64);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  printf("per factor+inverse (incl. LDS load): %.2f us\n", 1e3 * ms / 100);
  printf(fail ? "FAIL\n" : "PASS\n");
  return fail;
}
