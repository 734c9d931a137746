// Phase breakdown of diag16_fs (the 16x16 diagonal block of the 64x64
// factor + inverse): one wave, the block in LDS, the fenced clock stamps the
// function carries under PGO_DIAG_CLOCKS (s_waitcnt + sched_barrier around
// s_memtime, so no instruction moves across a stamp).  Stamps serialise the
// phases: the total is an upper bound of the unstamped time.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include scripts/ubench_diag16.hip -o graphslam_amd/build/ubench_diag16
#define PGO_DIAG_CLOCKS 1
#include "../graphslam_amd/csrc/pgo_chol.hip"

#include <cstdio>

using namespace pgo;

__global__ __launch_bounds__(64) void u_d16(const double* A, double* out, long long* clk) {
  __shared__ double T[16 * 65], W[16 * 65], sc[64];
  long long t0 = 0, t1 = 0;
  for (int rep = 0; rep < 4; rep++) {
    for (int i = threadIdx.x; i < 16 * 65; i += 64) {
      T[i] = (i % 65) < 16 ? A[(i % 65) + 16 * (i / 65)] : 0.0;
      W[i] = 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    t0 = clock64();
    const bool bad = diag16_fs(T, W, sc);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    t1 = clock64();
    if (threadIdx.x == 0) out[0] += T[15 + 15 * 65] + W[15 + 15 * 65] + bad;
  }
  if (threadIdx.x == 0) clk[0] = t1 - t0;
}

int main() {
  double h[256];
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++) h[i + 16 * j] = (i == j ? 40.0 : 0.0) + 1.0 / (1.0 + i + j);
  double *dA, *dO;
  long long* dc;
  hipMalloc(&dA, sizeof(h));
  hipMalloc(&dO, 64 * sizeof(double));
  hipMalloc(&dc, sizeof(long long));
  hipMemset(dO, 0, 64 * sizeof(double));
  hipMemcpy(dA, h, sizeof(h), hipMemcpyHostToDevice);
  u_d16<<<1, 64>>>(dA, dO, dc);
  long long total = 0, c[32];
  hipMemcpy(&total, dc, sizeof(total), hipMemcpyDeviceToHost);
  hipMemcpyFromSymbol(c, HIP_SYMBOL(g_diag_clk), sizeof(c));
  const char* nm[] = {"chol8 A11", "fwd8 (X11, L21) + store", "A22 -= L21 L21', Y, load A22", "chol8 A22",
                      "fwd8 (X22, X21) + store"};
  printf("diag16_fs stamped total: %lld cycles\n", total);
  for (int q = 0; q < 5; q++) printf("  %-30s %6lld\n", nm[q], c[21 + q] - c[20 + q]);
  return 0;
}
