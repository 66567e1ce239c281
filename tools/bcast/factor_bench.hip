// Micro-benchmark (diagnostic, not part of the product): the tick's dense 26 x 26 right-looking Cholesky (tsidb_tick.hpp: tick_chol)
//   form a  float64 broadcasts as v_readlane pairs in groups of four (the product before the DPP form, and its float32 form)
//   form b  row_dup (v_permlane16_swap) once per pivot + v_fmac_f64_dpp row_newbcast (tsidb_common.hpp: bcast_fnma)
// One env per wavefront, two wavefronts per SIMD, 20 KB of LDS per workgroup - the residency k_tick runs at.  Both forms
// factor the same SPD matrices; the factors (lanes < 26, all 26 registers, and 1 / L[k][k]) are compared bit for bit.
// Prints the shader cycles per factorisation (s_memtime around the repetition loop, mean over the wavefronts) and the
// launch's time per factorisation from HIP events at full residency.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -disable-machine-licm -ffp-contract=on -I tsid_control_amd/csrc \
//         -o tools/bcast/factor_bench tools/bcast/factor_bench.hip          (tools/bcast/run.sh builds and runs it)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsidb_tick.hpp"
using namespace tsidb;

constexpr int REPS = 64, NMAT = 256, LDA = NV + 1; // (odd LDS row stride: the row loads are conflict-free)

template <bool DPPB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k(const double *Ag, double *Lg, double *rdg, long long *cyc, int *bad) {
  extern __shared__ double lds[]; // 20 KB requested at launch; NV * LDA doubles used
  const int lane = threadIdx.x, e = blockIdx.x;
  const double *A = Ag + (size_t)(e % NMAT) * NV * NV;
  if (lane < NV)
    for (int j = 0; j < NV; j++) lds[lane * LDA + j] = A[lane * NV + j];
  __syncthreads();
  double a[NV], rdv = 0;
  int notspd = 0, ln = lane;
  const long long t0 = clock64();
  for (int rep = 0; rep < REPS; rep++) {
#pragma unroll
    for (int j = 0; j < NV; j++) a[j] = lane < NV ? lds[lane * LDA + j] : 0.0;
    rdv = 0;
    tick_chol<double, DPPB>(a, rdv, notspd, ln);
#pragma unroll
    for (int j = 0; j < NV; j++) asm volatile("" : "+v"(a[j])); // (the factor is "used" every repetition)
  }
  const long long t1 = clock64();
  if (lane == 0) { cyc[e] = t1 - t0; bad[e] = notspd; }
  if (lane < NV) {
    for (int j = 0; j < NV; j++) Lg[((size_t)e * NV + lane) * NV + j] = a[j];
    rdg[(size_t)e * NV + lane] = rdv;
  }
}

#define CHECK(x) do { hipError_t err_ = (x); if (err_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(err_)); return 2; } } while (0)

int main() {
  const int n = 8192;
  std::vector<double> A((size_t)NMAT * NV * NV);
  srand(1);
  for (int e = 0; e < NMAT; e++) { // A = G G^T + diag: SPD, dense
    double G[NV][NV];
    for (int i = 0; i < NV; i++) for (int j = 0; j < NV; j++) G[i][j] = j <= i ? ((rand() % 2001) - 1000) * 3e-4 : 0.0;
    for (int i = 0; i < NV; i++) G[i][i] = 1.0 + (rand() % 1000) * 1e-3;
    for (int i = 0; i < NV; i++) for (int j = 0; j < NV; j++) {
      double s = 0;
      for (int c = 0; c < NV; c++) s += G[i][c] * G[j][c];
      A[((size_t)e * NV + i) * NV + j] = s;
    }
  }
  double *dA, *dL[2], *drd[2];
  long long *dcyc;
  int *dbad;
  const size_t nL = (size_t)n * NV * NV, nr = (size_t)n * NV;
  CHECK(hipMalloc(&dA, A.size() * 8));
  for (int f = 0; f < 2; f++) { CHECK(hipMalloc(&dL[f], nL * 8)); CHECK(hipMalloc(&drd[f], nr * 8)); }
  CHECK(hipMalloc(&dcyc, n * sizeof(long long)));
  CHECK(hipMalloc(&dbad, n * sizeof(int)));
  CHECK(hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  std::vector<long long> cyc(n);
  std::vector<int> bad(n);
  int rc = 0;
  for (int ne : {256, 2048, 4096, 8192}) { // one wavefront per SIMD at most (latency) up to full residency, several rounds of it
    double ms[2] = {0, 0}, cy[2] = {0, 0};
    for (int it = 0; it < 4; it++) { // (the first round warms up; the forms alternate)
      for (int f = 0; f < 2; f++) {
        CHECK(hipEventRecord(e0));
        if (f == 0) hipLaunchKernelGGL(k<false>, dim3(ne), dim3(64), 20480, 0, dA, dL[0], drd[0], dcyc, dbad);
        else hipLaunchKernelGGL(k<true>, dim3(ne), dim3(64), 20480, 0, dA, dL[1], drd[1], dcyc, dbad);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        CHECK(hipMemcpy(cyc.data(), dcyc, ne * sizeof(long long), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(bad.data(), dbad, ne * sizeof(int), hipMemcpyDeviceToHost));
        double s = 0;
        for (int e = 0; e < ne; e++) { s += (double)cyc[e]; if (bad[e]) rc = 1; }
        if (it == 0 || t < ms[f]) { ms[f] = t; cy[f] = s / ne / REPS; }
      }
    }
    printf("envs %5d: cycles per factorisation  a (v_readlane) %8.1f   b (DPP row_newbcast) %8.1f   b / a %.3f |  ns per factorisation per env  a %7.2f  b %7.2f  b / a %.3f\n",
           ne, cy[0], cy[1], cy[1] / cy[0], ms[0] * 1e6 / ((double)ne * REPS), ms[1] * 1e6 / ((double)ne * REPS), ms[1] / ms[0]);
  }
  if (rc) printf("a matrix was reported not positive definite\n");
  std::vector<double> L0(nL), L1(nL), r0(nr), r1(nr);
  CHECK(hipMemcpy(L0.data(), dL[0], nL * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(L1.data(), dL[1], nL * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(r0.data(), drd[0], nr * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(r1.data(), drd[1], nr * 8, hipMemcpyDeviceToHost));
  size_t nd = 0, nonzero = 0;
  for (size_t i = 0; i < nL; i++) { nd += memcmp(&L0[i], &L1[i], 8) != 0; nonzero += L0[i] != 0.0; }
  for (size_t i = 0; i < nr; i++) nd += memcmp(&r0[i], &r1[i], 8) != 0;
  printf("factors of %d envs (%d distinct matrices): %zu of %zu values differ bitwise (%zu non-zero)\n", n, NMAT, nd, nL + nr, nonzero);
  return rc || nd != 0 || nonzero == 0;
}
