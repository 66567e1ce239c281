// tsidb_unit.hip - test-only harness: one small __global__ wrapper per device primitive of tsidb_common.hpp, tsidb_tick.hpp
// and tsidb_sim.hpp, so that the suite can run each of them alone (tests/test_gpu_unit_*.py through tests/unit_testlib.py).
//
// What this layer covers, and what it does not: the primitives are __forceinline__, so every wrapper here is its own
// compilation of the primitive's SOURCE in the wrapper's context - its semantics, its constants, its branch thresholds and
// the hazard handling its inline asm brings along.  It is NOT the product's machine code: k_tick / k_sim inline the same
// source into other surroundings, with another register allocation and schedule.  The product's code is pinned by the
// end-to-end parity and bit tests; this file pins the building blocks at inputs those tests never reach.
//
// Conventions: one wavefront of 64 lanes per block.  Wave-level wrappers take n blocks and arrays of n * 64 elements per
// operand (register arrays: n * 64 * K, element k of lane l of block b at (b * 64 + l) * K + k); element-wise wrappers take n
// elements.  Every entry point takes device pointers, a count and a stream, launches at most one kernel and returns
// hipGetLastError(); n <= 0 or a null pointer launches nothing and returns hipErrorInvalidValue.  No allocation, no
// synchronisation, no output: the tests own the memory.  None of the product's kernels is instantiated here.
#include "tsidb_tick.hpp"
#include "tsidb_sim.hpp"

using namespace tsidb;

#define TSIDBU_API extern "C" __attribute__((visibility("default")))
#define TSIDBU_CHECK(n, ...)                                                     \
  do {                                                                           \
    const void *ptrs_[] = {__VA_ARGS__};                                         \
    if ((n) <= 0) return (int)hipErrorInvalidValue;                              \
    for (const void *p_ : ptrs_)                                                 \
      if (!p_) return (int)hipErrorInvalidValue;                                 \
  } while (0)
#define TSIDBU_WAVES(kernel, n, stream, ...)                                     \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(n), dim3(WAVE), 0, stream, __VA_ARGS__);     \
    return (int)hipGetLastError();                                               \
  } while (0)
#define TSIDBU_ELEMS(kernel, n, stream, ...)                                     \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(((n) + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, __VA_ARGS__); \
    return (int)hipGetLastError();                                               \
  } while (0)

namespace {

// ------------------------------------------------------------------ dimensions
constexpr int NFNMA_FIXED = 12; // masks every build has; the robot's own follow
constexpr unsigned chol_mask(int k) { return ((1u << NV) - 1u) & ~((2u << k) - 1u); }
constexpr unsigned FNMA_FIXED[NFNMA_FIXED] = {
    1u << 0, 1u << 15, 1u << 16, 1u << 25,            // one bit
    (1u << 15) | (1u << 16), 0x00030003u, 0x00818181u, // bits on both sides of lane 16
    chol_mask(0), chol_mask(7), chol_mask(8), chol_mask(NV - 2), // tick_chol's masks (more than eight bits: the recursive path)
    0x0000ff00u};
constexpr int NFNMA = NFNMA_FIXED + NV; // + MJ_DOFANC[k] & ((1 << k) - 1), k = 0 .. NV - 1
constexpr unsigned fnma_mask(int i) { return i < NFNMA_FIXED ? FNMA_FIXED[i] : (MJ_DOFANC[i - NFNMA_FIXED] & ((1u << (i - NFNMA_FIXED)) - 1u)); }
// bcast_fnma2: chains of 1, 4, 5 and 9 terms on either parity (even lanes feed s0, odd lanes s1), mixed, and the robot's
constexpr int NFNMA2_FIXED = 11;
constexpr unsigned FNMA2_FIXED[NFNMA2_FIXED] = {
    0x00000001u, 0x00000002u,             // 1 term, even / odd
    0x00010111u, 0x00020222u,             // 4 terms (across lane 16): one full group
    0x00010511u, 0x00020a22u,             // 5 terms: a second group on that chain
    0x00015555u, 0x0002aaaau,             // 9 terms: three groups
    0x0003ffffu & ((1u << NV) - 1u),      // 9 + 9
    0x00010000u, 0x00830421u & ((1u << NV) - 1u)};
constexpr int NFNMA2 = NFNMA2_FIXED + NV;
constexpr unsigned fnma2_mask(int i) { return i < NFNMA2_FIXED ? FNMA2_FIXED[i] : (MJ_DOFANC[i - NFNMA2_FIXED] & ((1u << (i - NFNMA2_FIXED)) - 1u)); }

// ------------------------------------------------------------------ wave reductions
template <typename T> __global__ void k_wave_sum(const T *in, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = wave_sum(in[i]);
}
template <typename T> __global__ void k_wave_sum3(const T *a, const T *b, const T *c, T *oa, T *ob, T *oc) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  T x = a[i], y = b[i], z = c[i];
  wave_sum3(x, y, z);
  oa[i] = x; ob[i] = y; oc[i] = z;
}
__global__ void k_wave_sum_int(const int *in, int *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = wave_sum_int(in[i]);
}
template <typename T> __global__ void k_wave_min(const T *in, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = wave_min(in[i]);
}
template <typename T> __global__ void k_wave_argmin(const T *v, const int *idx, T *ov, int *oi) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  T x = v[i];
  int j = idx[i];
  wave_argmin(x, j);
  ov[i] = x; oi[i] = j;
}
template <typename T> __global__ void k_subtree_sum32(const T *v, const int *last, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = subtree_sum32(v[i], last[i] & 63);
}
template <typename T> __global__ void k_bperm(const T *v, const int *src, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = bperm(v[i], src[i] & 63);
}
template <typename T> __global__ void k_bcast(const T *v, const int *src, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = bcast(v[i], src[i] & 63);
}
template <typename T> __global__ void k_lane63(const T *v, T *out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  out[i] = lane63(v[i]);
}
// out[(b * 64 + s) * 64 + lane] = what `lane` reads from source lane s
template <typename T> __global__ void k_rdlane(const T *v, T *out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const T x = v[b * WAVE + lane];
#pragma unroll
  for (int s = 0; s < WAVE; s++) out[(b * WAVE + s) * WAVE + lane] = rdlane(x, s);
}
template <typename T> __global__ void k_rdlane_dyn(const T *v, const int *order, T *out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const T x = v[b * WAVE + lane];
  for (int s = 0; s < WAVE; s++) {
    const int src = order[b * WAVE + s] & 63; // run-time, the same on every lane
    out[(b * WAVE + s) * WAVE + lane] = rdlane_dyn(x, src);
  }
}
__global__ void k_env_of_block(int *out, int n) {
  const int b = blockIdx.x * WAVE + threadIdx.x;
  if (b < n) out[b] = env_of_block(b, n);
}

// ------------------------------------------------------------------ row_dup / bcast_fnma / bcast_fnma2
// VAR 0: x comes straight from its load; VAR 1: x is the product of a VALU multiply in the statement right before row_dup, and
// the row-replicated copies are multiplied once more right before the FMA group (the DPP source's producer is then the VALU
// instruction in front of the asm statement: the case its wait states are there for).  sc[0] and sc[1] are powers of two in
// the tests, so the expected operand x * sc[0] * sc[1] is exact.
template <int VAR> __device__ __forceinline__ RowDup make_dup(const double *x, const double *sc, int i) {
  if constexpr (VAR == 0) return row_dup(x[i]);
  else {
    const double s0 = sc[0], s1 = sc[1];
    const double xv = x[i] * s0;
    RowDup d = row_dup(xv);
    d.lo *= s1; d.hi *= s1;
    return d;
  }
}
template <int VAR> __global__ void k_row_dup(const double *x, const double *sc, double *lo, double *hi) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  const RowDup d = make_dup<VAR>(x, sc, i);
  lo[i] = d.lo; hi[i] = d.hi;
}
template <unsigned MASK, int VAR> __global__ void k_fnma(const double *x, const double *sc, const double *m, const double *a_in, double *a_out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  double a[32];
#pragma unroll
  for (int j = 0; j < 32; j++) a[j] = a_in[i * 32 + j];
  const double mv = m[i];
  const RowDup d = make_dup<VAR>(x, sc, i);
  bcast_fnma<MASK>(a, d, mv);
#pragma unroll
  for (int j = 0; j < 32; j++) a_out[i * 32 + j] = a[j];
}
template <unsigned MASK, int VAR> __global__ void k_fnma2(const double *x, const double *sc, const double *m_in, const double *s_in, double *s_out) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  double m[32];
#pragma unroll
  for (int j = 0; j < 32; j++) m[j] = m_in[i * 32 + j];
  double s0 = s_in[2 * i], s1 = s_in[2 * i + 1];
  const RowDup d = make_dup<VAR>(x, sc, i);
  bcast_fnma2<MASK>(s0, s1, d, m);
  s_out[2 * i] = s0; s_out[2 * i + 1] = s1;
}
typedef void (*fnma_kernel_t)(const double *, const double *, const double *, const double *, double *);
template <int I> struct FnmaTab {
  static fnma_kernel_t get(int idx, int var) {
    if (idx == I) return var ? k_fnma<fnma_mask(I), 1> : k_fnma<fnma_mask(I), 0>;
    if constexpr (I + 1 < NFNMA) return FnmaTab<I + 1>::get(idx, var);
    else return nullptr;
  }
};
template <int I> struct Fnma2Tab {
  static fnma_kernel_t get(int idx, int var) {
    if (idx == I) return var ? k_fnma2<fnma2_mask(I), 1> : k_fnma2<fnma2_mask(I), 0>;
    if constexpr (I + 1 < NFNMA2) return Fnma2Tab<I + 1>::get(idx, var);
    else return nullptr;
  }
};

// ------------------------------------------------------------------ scalar maths, small geometry (one element per lane)
template <typename T> __global__ void k_rsqrt(const T *x, T *y, int n) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) y[i] = rsqrt_t(x[i]);
}
template <typename T> __global__ void k_rcp(const T *x, T *y, int n) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) y[i] = rcp_t(x[i]);
}
template <typename T> __global__ void k_sincos(const T *x, T *s, T *c, int n) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) { T sv, cv; sincos_t(x[i], sv, cv); s[i] = sv; c[i] = cv; }
}
template <typename T> __global__ void k_log6(const T *R, const T *p, T *out, int n) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) {
    T Rl[9], pl[3], o[6];
#pragma unroll
    for (int k = 0; k < 9; k++) Rl[k] = R[i * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) pl[k] = p[i * 3 + k];
    log6(Rl, pl, o);
#pragma unroll
    for (int k = 0; k < 6; k++) out[i * 6 + k] = o[k];
  }
}
template <typename T> __global__ void k_quat_to_R(const T *q, T *R, int n) { // q = x, y, z, w
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) {
    T Rl[9];
    quat_to_R(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3], Rl);
#pragma unroll
    for (int k = 0; k < 9; k++) R[i * 9 + k] = Rl[k];
  }
}
template <typename T> __global__ void k_mat_to_quat(const T *R, T *q, int n) { // q = w, x, y, z
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) {
    T Rl[9], ql[4];
#pragma unroll
    for (int k = 0; k < 9; k++) Rl[k] = R[i * 9 + k];
    mat_to_quat(Rl, ql);
#pragma unroll
    for (int k = 0; k < 4; k++) q[4 * i + k] = ql[k];
  }
}
template <typename T> __global__ void k_make_frame(const T *nrm, T *t1, T *t2, int n) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) {
    T nl[3], a[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; k++) nl[k] = nrm[3 * i + k];
    make_frame(nl, a, b);
#pragma unroll
    for (int k = 0; k < 3; k++) { t1[3 * i + k] = a[k]; t2[3 * i + k] = b[k]; }
  }
}
template <typename T> __global__ void k_tri_closest(const T *tri, T *d2, T *q, int n) { // tri = a, b, c
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) {
    T t[9], ql[3];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = tri[9 * i + k];
    d2[i] = origin_tri_closest(t, t + 3, t + 6, ql);
#pragma unroll
    for (int k = 0; k < 3; k++) q[3 * i + k] = ql[k];
  }
}
template <typename T> __global__ void k_terrain_h(const T *terr, const T *xy, T *h, int n) { // one 20-entry table for all
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i < n) h[i] = terrain_h(terr, xy[2 * i], xy[2 * i + 1]);
}

// ------------------------------------------------------------------ factorisations (lane i = row i; A is [n][NV][NV])
template <typename T> __device__ __forceinline__ void load_rows(const T *A, int b, int lane, T (&a)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; j++) a[j] = lane < NV ? A[(b * NV + lane) * NV + j] : T(0);
}
template <typename T> __device__ __forceinline__ void store_rows(T *U, int b, int lane, const T (&a)[NV]) { // [n][64][NV]
#pragma unroll
  for (int j = 0; j < NV; j++) U[(b * WAVE + lane) * NV + j] = a[j];
}
template <typename T, bool DPPB> __global__ void k_tick_chol(const T *A, T *L, T *rdv_out, int *notspd_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  T a[NV], rdv = 0;
  load_rows(A, b, lane, a);
  int notspd = 0, ln = lane;
  tick_chol<T, DPPB>(a, rdv, notspd, ln);
  store_rows(L, b, lane, a);
  rdv_out[b * WAVE + lane] = rdv;
  notspd_out[b * WAVE + lane] = notspd;
}
template <typename T, bool DENSE> __global__ void k_chol26_solve(const T *A, const T *rhs, T *U, T *x, int *spd_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  T a[NV];
  load_rows(A, b, lane, a);
  bool spd = false;
  T xv;
  if constexpr (DENSE) xv = chol26_dense<T>(a, rhs[b * WAVE + lane], lane, spd);
  else xv = chol26_solve<T, false>(a, rhs[b * WAVE + lane], lane, spd);
  store_rows(U, b, lane, a);
  x[b * WAVE + lane] = xv;
  spd_out[b * WAVE + lane] = spd ? 1 : 0;
}
// chol26_factor, then chol26_subst with the factor parked in LDS at row stride LDM, as k_sim's Newton loop does
template <typename T> __global__ void k_chol26_factor_subst(const T *A, const T *rhs, T *U, T *rdv_out, T *x, int *spd_out) {
  __shared__ T H[NV * LDM];
  const int b = blockIdx.x, lane = threadIdx.x;
  T a[NV], rdv;
  load_rows(A, b, lane, a);
  bool spd = false;
  chol26_factor<T>(a, rdv, lane, spd);
  if (lane < NV) {
#pragma unroll
    for (int j = 0; j < NV; j++) H[lane * LDM + j] = a[j];
    H[lane * LDM + NV] = rdv;
  }
  __syncthreads();
  const T xv = chol26_subst<T>(a, H, rdv, rhs[b * WAVE + lane], lane);
  store_rows(U, b, lane, a);
  rdv_out[b * WAVE + lane] = rdv;
  x[b * WAVE + lane] = xv;
  spd_out[b * WAVE + lane] = spd ? 1 : 0;
}
// m rank-1 changes in sequence on the factor U (rows [n][NV][NV]), rdv [n][64]: xs [n][m][64], sigma [n][m], chain [n][m];
// stops at the first one the routine refuses; done[b * 64 + lane] = how many were applied
template <typename T>
__global__ void k_chol26_rank1(const T *Uin, const T *rdv_in, const T *xs, const T *sigma, const unsigned long long *chain, int m, T *U,
                               T *rdv_out, int *done) {
  const int b = blockIdx.x, lane = threadIdx.x;
  T a[NV];
  load_rows(Uin, b, lane, a);
  T rdv = rdv_in[b * WAVE + lane];
  int cnt = 0;
  for (int r = 0; r < m; r++) {
    const unsigned long long ch = chain[b * m + r];
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(ch & 0xffffffffull)), hi = __builtin_amdgcn_readfirstlane((unsigned)(ch >> 32));
    const T sg = sigma[b * m + r];
    if (!chol26_rank1<T>(a, rdv, xs[(b * m + r) * WAVE + lane], sg, ((unsigned long long)hi << 32) | lo, lane)) break;
    cnt++;
  }
  store_rows(U, b, lane, a);
  rdv_out[b * WAVE + lane] = rdv;
  done[b * WAVE + lane] = cnt;
}

} // namespace

// ================================================================== exports
// NV, the number of bcast_fnma / bcast_fnma2 masks compiled in, LDM; the MJ_DOFANC table; the mask lists
TSIDBU_API int tsidbu_dims(int *dims4, unsigned *dofanc32, unsigned *fnma_masks64, unsigned *fnma2_masks64) {
  if (!dims4 || !dofanc32 || !fnma_masks64 || !fnma2_masks64) return (int)hipErrorInvalidValue;
  dims4[0] = NV; dims4[1] = NFNMA; dims4[2] = NFNMA2; dims4[3] = LDM;
  for (int k = 0; k < 32; k++) dofanc32[k] = k < NV ? MJ_DOFANC[k] : 0u;
  for (int k = 0; k < 64; k++) fnma_masks64[k] = k < NFNMA ? fnma_mask(k) : 0u;
  for (int k = 0; k < 64; k++) fnma2_masks64[k] = k < NFNMA2 ? fnma2_mask(k) : 0u;
  return 0;
}

#define TSIDBU_UNARY(name, kernel, T)                                                         \
  TSIDBU_API int name(const T *in, T *out, int n, hipStream_t st) {                           \
    TSIDBU_CHECK(n, in, out);                                                                 \
    TSIDBU_WAVES(kernel, n, st, in, out);                                                     \
  }
TSIDBU_UNARY(tsidbu_wave_sum_f32, k_wave_sum<float>, float)
TSIDBU_UNARY(tsidbu_wave_sum_f64, k_wave_sum<double>, double)
TSIDBU_UNARY(tsidbu_wave_sum_int, k_wave_sum_int, int)
TSIDBU_UNARY(tsidbu_wave_min_f32, k_wave_min<float>, float)
TSIDBU_UNARY(tsidbu_wave_min_f64, k_wave_min<double>, double)
TSIDBU_UNARY(tsidbu_wave_min_i32, k_wave_min<int>, int)
TSIDBU_UNARY(tsidbu_lane63_f32, k_lane63<float>, float)
TSIDBU_UNARY(tsidbu_lane63_f64, k_lane63<double>, double)
TSIDBU_UNARY(tsidbu_lane63_i32, k_lane63<int>, int)
TSIDBU_UNARY(tsidbu_rdlane_f32, k_rdlane<float>, float)   // out: n * 64 * 64
TSIDBU_UNARY(tsidbu_rdlane_f64, k_rdlane<double>, double)
#undef TSIDBU_UNARY

#define TSIDBU_SUM3(name, T)                                                                                   \
  TSIDBU_API int name(const T *a, const T *b, const T *c, T *oa, T *ob, T *oc, int n, hipStream_t st) {        \
    TSIDBU_CHECK(n, a, b, c, oa, ob, oc);                                                                      \
    TSIDBU_WAVES(k_wave_sum3<T>, n, st, a, b, c, oa, ob, oc);                                                  \
  }
TSIDBU_SUM3(tsidbu_wave_sum3_f32, float)
TSIDBU_SUM3(tsidbu_wave_sum3_f64, double)
#undef TSIDBU_SUM3

#define TSIDBU_ARGMIN(name, T)                                                                \
  TSIDBU_API int name(const T *v, const int *idx, T *ov, int *oi, int n, hipStream_t st) {    \
    TSIDBU_CHECK(n, v, idx, ov, oi);                                                          \
    TSIDBU_WAVES(k_wave_argmin<T>, n, st, v, idx, ov, oi);                                    \
  }
TSIDBU_ARGMIN(tsidbu_wave_argmin_f32, float)
TSIDBU_ARGMIN(tsidbu_wave_argmin_f64, double)
#undef TSIDBU_ARGMIN

#define TSIDBU_VIDX(name, kernel, T)                                                          \
  TSIDBU_API int name(const T *v, const int *idx, T *out, int n, hipStream_t st) {            \
    TSIDBU_CHECK(n, v, idx, out);                                                             \
    TSIDBU_WAVES(kernel, n, st, v, idx, out);                                                 \
  }
TSIDBU_VIDX(tsidbu_subtree_sum32_f32, k_subtree_sum32<float>, float)
TSIDBU_VIDX(tsidbu_subtree_sum32_f64, k_subtree_sum32<double>, double)
TSIDBU_VIDX(tsidbu_bperm_f32, k_bperm<float>, float)
TSIDBU_VIDX(tsidbu_bperm_f64, k_bperm<double>, double)
TSIDBU_VIDX(tsidbu_bcast_f32, k_bcast<float>, float)
TSIDBU_VIDX(tsidbu_bcast_f64, k_bcast<double>, double)
TSIDBU_VIDX(tsidbu_rdlane_dyn_f32, k_rdlane_dyn<float>, float)   // idx: n * 64 source lanes, out: n * 64 * 64
TSIDBU_VIDX(tsidbu_rdlane_dyn_f64, k_rdlane_dyn<double>, double)
#undef TSIDBU_VIDX

TSIDBU_API int tsidbu_env_of_block(int *out, int n, hipStream_t st) {
  TSIDBU_CHECK(n, out);
  TSIDBU_ELEMS(k_env_of_block, n, st, out, n);
}

TSIDBU_API int tsidbu_row_dup(int var, const double *x, const double *sc, double *lo, double *hi, int n, hipStream_t st) {
  TSIDBU_CHECK(n, x, sc, lo, hi);
  if (var != 0 && var != 1) return (int)hipErrorInvalidValue;
  if (var) TSIDBU_WAVES(k_row_dup<1>, n, st, x, sc, lo, hi);
  TSIDBU_WAVES(k_row_dup<0>, n, st, x, sc, lo, hi);
}
// a_in / a_out: n * 64 * 32 (lane's accumulators a[0..31]); m: n * 64
TSIDBU_API int tsidbu_bcast_fnma(int mask_index, int var, const double *x, const double *sc, const double *m, const double *a_in, double *a_out,
                                 int n, hipStream_t st) {
  TSIDBU_CHECK(n, x, sc, m, a_in, a_out);
  if ((var != 0 && var != 1) || mask_index < 0 || mask_index >= NFNMA) return (int)hipErrorInvalidValue;
  const fnma_kernel_t k = FnmaTab<0>::get(mask_index, var);
  TSIDBU_WAVES(k, n, st, x, sc, m, a_in, a_out);
}
// m_in: n * 64 * 32 (lane's multipliers m[0..31]); s_in / s_out: n * 64 * 2 (s0, s1)
TSIDBU_API int tsidbu_bcast_fnma2(int mask_index, int var, const double *x, const double *sc, const double *m_in, const double *s_in,
                                  double *s_out, int n, hipStream_t st) {
  TSIDBU_CHECK(n, x, sc, m_in, s_in, s_out);
  if ((var != 0 && var != 1) || mask_index < 0 || mask_index >= NFNMA2) return (int)hipErrorInvalidValue;
  const fnma_kernel_t k = Fnma2Tab<0>::get(mask_index, var);
  TSIDBU_WAVES(k, n, st, x, sc, m_in, s_in, s_out);
}

#define TSIDBU_MAP1(name, kernel, T)                                                          \
  TSIDBU_API int name(const T *x, T *y, int n, hipStream_t st) {                              \
    TSIDBU_CHECK(n, x, y);                                                                    \
    TSIDBU_ELEMS(kernel, n, st, x, y, n);                                                     \
  }
#define TSIDBU_MAP2(name, kernel, T)                                                          \
  TSIDBU_API int name(const T *x, T *y, T *z, int n, hipStream_t st) {                        \
    TSIDBU_CHECK(n, x, y, z);                                                                 \
    TSIDBU_ELEMS(kernel, n, st, x, y, z, n);                                                  \
  }
TSIDBU_MAP1(tsidbu_rsqrt_f32, k_rsqrt<float>, float)
TSIDBU_MAP1(tsidbu_rsqrt_f64, k_rsqrt<double>, double)
TSIDBU_MAP1(tsidbu_rcp_f32, k_rcp<float>, float)
TSIDBU_MAP1(tsidbu_rcp_f64, k_rcp<double>, double)
TSIDBU_MAP2(tsidbu_sincos_f64, k_sincos<double>, double)
TSIDBU_MAP1(tsidbu_quat_to_R_f32, k_quat_to_R<float>, float)
TSIDBU_MAP1(tsidbu_quat_to_R_f64, k_quat_to_R<double>, double)
TSIDBU_MAP1(tsidbu_mat_to_quat_f32, k_mat_to_quat<float>, float)
TSIDBU_MAP1(tsidbu_mat_to_quat_f64, k_mat_to_quat<double>, double)
TSIDBU_MAP2(tsidbu_make_frame_f32, k_make_frame<float>, float)
TSIDBU_MAP2(tsidbu_make_frame_f64, k_make_frame<double>, double)
TSIDBU_MAP2(tsidbu_tri_closest_f32, k_tri_closest<float>, float)
TSIDBU_MAP2(tsidbu_tri_closest_f64, k_tri_closest<double>, double)
TSIDBU_MAP2(tsidbu_log6_f32, k_log6<float>, float)      // R: n * 9, p: n * 3, out: n * 6
TSIDBU_MAP2(tsidbu_log6_f64, k_log6<double>, double)
TSIDBU_MAP2(tsidbu_terrain_h_f32, k_terrain_h<float>, float) // terr: 20, xy: n * 2, h: n
TSIDBU_MAP2(tsidbu_terrain_h_f64, k_terrain_h<double>, double)
#undef TSIDBU_MAP1
#undef TSIDBU_MAP2

#define TSIDBU_TICK_CHOL(name, T, DPPB)                                                                     \
  TSIDBU_API int name(const T *A, T *L, T *rdv, int *notspd, int n, hipStream_t st) {                       \
    TSIDBU_CHECK(n, A, L, rdv, notspd);                                                                     \
    TSIDBU_WAVES((k_tick_chol<T, DPPB>), n, st, A, L, rdv, notspd);                                         \
  }
TSIDBU_TICK_CHOL(tsidbu_tick_chol_f64_dpp, double, true)
TSIDBU_TICK_CHOL(tsidbu_tick_chol_f64, double, false)
TSIDBU_TICK_CHOL(tsidbu_tick_chol_f32, float, false)
#undef TSIDBU_TICK_CHOL

#define TSIDBU_SOLVE(name, T, DENSE)                                                                        \
  TSIDBU_API int name(const T *A, const T *rhs, T *U, T *x, int *spd, int n, hipStream_t st) {              \
    TSIDBU_CHECK(n, A, rhs, U, x, spd);                                                                     \
    TSIDBU_WAVES((k_chol26_solve<T, DENSE>), n, st, A, rhs, U, x, spd);                                     \
  }
TSIDBU_SOLVE(tsidbu_chol26_solve_f32, float, false)
TSIDBU_SOLVE(tsidbu_chol26_solve_f64, double, false)
TSIDBU_SOLVE(tsidbu_chol26_dense_f32, float, true)
TSIDBU_SOLVE(tsidbu_chol26_dense_f64, double, true)
#undef TSIDBU_SOLVE

#define TSIDBU_FACTOR(name, T)                                                                              \
  TSIDBU_API int name(const T *A, const T *rhs, T *U, T *rdv, T *x, int *spd, int n, hipStream_t st) {      \
    TSIDBU_CHECK(n, A, rhs, U, rdv, x, spd);                                                                \
    TSIDBU_WAVES(k_chol26_factor_subst<T>, n, st, A, rhs, U, rdv, x, spd);                                  \
  }
TSIDBU_FACTOR(tsidbu_chol26_factor_subst_f32, float)
TSIDBU_FACTOR(tsidbu_chol26_factor_subst_f64, double)
#undef TSIDBU_FACTOR

#define TSIDBU_RANK1(name, T)                                                                                                  \
  TSIDBU_API int name(const T *Uin, const T *rdv_in, const T *xs, const T *sigma, const unsigned long long *chain, int m, T *U, \
                      T *rdv, int *done, int n, hipStream_t st) {                                                              \
    TSIDBU_CHECK(n, Uin, rdv_in, xs, sigma, chain, U, rdv, done);                                                              \
    if (m <= 0) return (int)hipErrorInvalidValue;                                                                              \
    TSIDBU_WAVES(k_chol26_rank1<T>, n, st, Uin, rdv_in, xs, sigma, chain, m, U, rdv, done);                                    \
  }
TSIDBU_RANK1(tsidbu_chol26_rank1_f32, float)
TSIDBU_RANK1(tsidbu_chol26_rank1_f64, double)
#undef TSIDBU_RANK1
