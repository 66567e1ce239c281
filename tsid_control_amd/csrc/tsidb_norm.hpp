// tsidb_norm.hpp - running statistics of the policy's input rows (include/tsidb.h tsidb_policy_norm_update): rsl_rl's
// EmpiricalNormalization per network, on the very values k_policy_actor loads - x = (double)(float)block[e][c] - and the
// float32 affine map (shift, scale) the actor applies.  No reference counterpart (the reference has no policy).
//
// k_policy_norm_partial: a workgroup of 256 lanes per (tile of 16 columns, segment of NORM_SEG rows, network).  Lane (cl, rl) =
// (tid & 15, tid >> 4) holds column tile * 16 + cl of the rows seg * NORM_SEG + 16 j + rl, j = 0 .. NORM_SEG / 16 - 1, in
// registers: the 16 lanes of one rl read 16 consecutive columns of one row.  Two passes over the registers: the lane's sum in the
// order of j, the 16 lanes' sums added in the order of rl by the lane rl = 0 -> the segment's mean; then the centred squares the
// same way -> M2.  (mean, M2) go to the segment's slice of the workspace; its n follows from N.
// k_policy_norm_merge: one workgroup per network, one lane per column: the slices merged IN SEGMENT ORDER by Chan's formula,
// the running update, and the affine pair.  count is read by every lane before a barrier and written by lane 0 behind it.
// Float64 throughout, no atomics, every sum in one order that depends on N and NORM_SEG alone: no bit depends on the grid or the
// device, two calls on the same state write the same bits.
#pragma once
#include "tsidb_actor.hpp"

namespace tsidb {

constexpr int NORM_SEG = 256;                  // TSIDB_POL_NORM_SEG_ROWS
constexpr int NORM_PER_LANE = NORM_SEG / 16;   // rows a lane holds
constexpr int NORM_MERGE_LANES = ACT_MAXW;     // one lane per column of the widest input row

// one network's side of an update, by value in the launch
struct NormNet {
  int n_blocks, K;                             // K = 0: no such network in this call
  const void *blk[ACT_MAXB];
  int blk_ld[ACT_MAXB], blk_cols[ACT_MAXB];
  double *part;                                // [nseg, 2, K] the segments' (mean, M2)
  double *stats;                               // [2, K] running mean, running variance
  long long *count;                            // [1]
  float *affine;                               // [2, K] shift, scale
  double eps;
  long long until;                             // 0 = none
};

struct NormArgs {
  NormNet net[2];
  int n, nseg, first;                          // first: the network of blockIdx.z = 0 / blockIdx.y = 0 of the merge
};

// sums red[0 .. 15][cl] in the order of rl; called by the lanes rl = 0 behind a barrier
__device__ __forceinline__ double norm_column_sum(const double (*red)[16], int cl) {
  double s = red[0][cl];
#pragma unroll
  for (int r = 1; r < 16; r++) s += red[r][cl];
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) void k_policy_norm_partial(NormArgs a) {
  __shared__ double red[16][16];
  __shared__ double mean_s[16];
  const NormNet &net = a.net[blockIdx.z + a.first];
  const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
  const int col = blockIdx.x * 16 + cl, seg = blockIdx.y;
  if ((int)blockIdx.x * 16 >= net.K) return;   // (the other network is wider: block-uniform, ahead of every barrier)
  // the column's block
  const T *src = nullptr;
  int ld = 0;
  if (col < net.K) {
    int off = 0;
    for (int bi = 0; bi < net.n_blocks; bi++) {
      const int cols = net.blk_cols[bi];
      if (col >= off && col < off + cols) { src = (const T *)net.blk[bi] + (col - off); ld = net.blk_ld[bi]; }
      off += cols;
    }
  }
  const int e0 = seg * NORM_SEG + rl;
  const int nrows = a.n - seg * NORM_SEG < NORM_SEG ? a.n - seg * NORM_SEG : NORM_SEG;   // >= 1: nseg = ceil(n / NORM_SEG)
  double x[NORM_PER_LANE];
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < NORM_PER_LANE; j++) {
    const int e = e0 + 16 * j;
    x[j] = 0.0;
    if (src && e < a.n) x[j] = (double)(float)src[(size_t)e * ld];   // (rows at or beyond N are never read)
    s += x[j];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0) mean_s[cl] = norm_column_sum(red, cl) / (double)nrows;
  __syncthreads();
  const double m = mean_s[cl];
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < NORM_PER_LANE; j++) {
    const double d = x[j] - m;
    if (e0 + 16 * j < a.n) q += d * d;
  }
  red[rl][cl] = q;
  __syncthreads();
  if (rl == 0 && col < net.K) {
    double *out = net.part + (size_t)seg * 2 * net.K;
    out[col] = m;
    out[net.K + col] = norm_column_sum(red, cl);
  }
}

__global__ __launch_bounds__(NORM_MERGE_LANES) void k_policy_norm_merge(NormArgs a) {
  const NormNet &net = a.net[blockIdx.y + a.first];
  const long long count = net.count[0];
  __syncthreads();                             // every lane has read count before lane 0 writes it
  if (net.until > 0 && count >= net.until) return;
  const int c = threadIdx.x;
  const double nb = (double)a.n;
  if (c == 0) net.count[0] = count + (long long)a.n;
  if (c >= net.K) return;
  // Chan's merge of the segments, in their order
  double na = 0.0, mean_b = 0.0, m2 = 0.0;
  for (int seg = 0; seg < a.nseg; seg++) {
    const double *p = net.part + (size_t)seg * 2 * net.K;
    const int rows = a.n - seg * NORM_SEG < NORM_SEG ? a.n - seg * NORM_SEG : NORM_SEG;
    const double ns = (double)rows, nab = na + ns;
    const double d = p[c] - mean_b;
    const double t = d * (ns / nab);
    mean_b = mean_b + t;
    m2 = m2 + p[net.K + c] + d * t * na;
    na = nab;
  }
  const double var_b = m2 / nb;
  // rsl_rl's EmpiricalNormalization.update
  const double rate = nb / (double)(count + (long long)a.n);
  const double mean = net.stats[c], var = net.stats[net.K + c];
  const double delta = mean_b - mean;
  const double mean1 = mean + rate * delta;
  const double var1 = var + rate * (var_b - var + delta * (mean_b - mean1));
  net.stats[c] = mean1;
  net.stats[net.K + c] = var1;
  net.affine[c] = (float)mean1;
  net.affine[net.K + c] = (float)(1.0 / (sqrt(var1) + net.eps));
}

} // namespace tsidb
