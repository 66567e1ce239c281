// tsidb_optim.hpp - the step's side of a PPO iteration (include/tsidb.h tsidb_policy_opt_step): the gradient norm and its clip
// factor, the exact Gaussian KL of the learner's last minibatch with rsl_rl's adaptive step size, and torch.optim.Adam's
// single-tensor step on every weight, bias and log_std, in place.  No reference counterpart (the reference has no policy).
//
// Three launches, no atomics, no counters, every sum in one fixed order: two calls from the same state give the same bits.
//
// k_policy_opt_partial: a workgroup of OPT_LANES lanes per chunk of OPT_CHUNK gradient elements and, behind the chunks, per
// segment of LRN_SEG minibatch rows of the KL.  Lane t of a chunk loads the elements 4 t .. 4 t + 3 of its piece as one float4
// (scalar loads at a ragged tail or where a pointer is not 16-byte aligned: the same elements, the same order), squares and
// adds them in float64; lane t of a segment forms the KL of the rows t and t + OPT_LANES.  The lanes' sums are halved through
// LDS, slot[t] += slot[t + s], and slot 0 goes to the workgroup's place in the workspace.
// k_policy_opt_scalars: one workgroup.  The chunk sums, staged through LDS, are added in chunk order by one lane, the segments'
// sums likewise; that lane forms norm, coef, kl, the new lr, the bias corrections and the skip flag, writes lr, step and stats,
// and leaves what the step needs (coef, lr / bc1, sqrt(bc2), skip) in the workspace.
// k_policy_opt_apply: the first launch's chunk grid again: four elements of g, p, m, v per lane, the Adam step, p, m, v stored.
// A skipped step returns before it loads anything.  The pieces - up to 17 ragged tensors - are a table by value in the launch.
#pragma once
#include "tsidb_learner.hpp"

namespace tsidb {

constexpr int OPT_CHUNK = TSIDB_POL_OPT_CHUNK;
constexpr int OPT_LANES = TSIDB_POL_OPT_LANES;
constexpr int OPT_MAXPIECES = 4 * ACT_MAXL + 1;      // weight and bias of every layer of two networks, log_std
static_assert(OPT_CHUNK == 4 * OPT_LANES, "a lane holds four elements of a chunk");
static_assert(LRN_SEG == 2 * OPT_LANES, "a lane holds two rows of a KL segment");

struct OptPiece {
  float *p;                                          // the parameter, written in place
  const float *g;                                    // its gradient, read only
  float *m;                                          // its exp_avg inside moments; exp_avg_sq is m + P
  int n, chunk0;                                     // elements; the piece's first chunk
  int vec;                                           // p, g, m and m + P are 16-byte aligned
};

struct OptScalars {                                  // k_policy_opt_scalars -> k_policy_opt_apply; norm, kl: for the caller
  double norm, kl;                                   // as formed, before stats' float32 cast
  float coef, step_size, bc2_sqrt;
  int skip;
};

struct OptArgs {
  OptPiece piece[OPT_MAXPIECES];
  int npieces, nchunks, nseg;                        // nseg = 0: no schedule
  size_t P;
  const float *mu, *mean, *log_std, *log_std_old;    // the KL's inputs
  const int *index;
  int rows, M;
  double b1, b2, max_norm, desired_kl;
  float omb1, b2f, omb2, epsf;                       // (float)(1 - b1), (float)b2, (float)(1 - b2), (float)eps
  float lr_min, lr_max;
  int skip_nonfinite;
  float *lr;
  long long *step;
  float *stats;
  double *part;                                      // [nchunks] chunk sums, then [nseg, 2] (kl sum, rows used)
  OptScalars *sc;
};

// the piece a chunk belongs to (block-uniform)
__device__ __forceinline__ int opt_piece_of(const OptArgs &a, int chunk) {
  int k = 0;
  while (k + 1 < a.npieces && a.piece[k + 1].chunk0 <= chunk) k++;
  return k;
}

// slot[t] += slot[t + s], s = OPT_LANES / 2 .. 1, of two values at once; the result is in red[.][0] behind the last barrier
__device__ __forceinline__ void opt_halve(double (*red)[OPT_LANES], int tid, double x, double y) {
  red[0][tid] = x;
  red[1][tid] = y;
  __syncthreads();
  for (int s = OPT_LANES / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(OPT_LANES) void k_policy_opt_partial(OptArgs a) {
  __shared__ double red[2][OPT_LANES];
  __shared__ double kc[3][NA];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b < a.nchunks) {
    const OptPiece &pc = a.piece[opt_piece_of(a, b)];
    const int e = (b - pc.chunk0) * OPT_CHUNK + 4 * tid;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (pc.vec && e + 3 < pc.n) {
      const float4 q = *reinterpret_cast<const float4 *>(pc.g + e);
      g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) if (e + i < pc.n) g[i] = pc.g[e + i];
    }
    const double d0 = g[0], d1 = g[1], d2 = g[2], d3 = g[3];
    const double s = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    opt_halve(red, tid, s, 0.0);
    if (tid == 0) a.part[b] = red[0][0];
    return;
  }
  // ---- a segment of the KL
  const int seg = b - a.nchunks;
  if (tid < NA) {
    const double s = (double)a.log_std[tid], so = (double)a.log_std_old[tid];
    kc[0][tid] = s - so;
    kc[1][tid] = exp(2.0 * so);
    kc[2][tid] = 2.0 * exp(2.0 * s);
  }
  __syncthreads();
  double sum = 0.0, used = 0.0;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int m = seg * LRN_SEG + tid + r * OPT_LANES;
    if (m >= a.M) continue;
    const int j = a.index[m];
    if (j < 0 || j >= a.rows) continue;
    const float *mo = a.mean + (size_t)j * NA, *mn = a.mu + (size_t)m * NA;
    double k = 0.0;
    for (int c = 0; c < NA; c++) {
      const double d = (double)mo[c] - (double)mn[c];
      const double q = (kc[1][c] + d * d) / kc[2][c];
      k += (kc[0][c] + q) - 0.5;
    }
    sum += k;
    used += 1.0;
  }
  opt_halve(red, tid, sum, used);
  if (tid == 0) {
    a.part[a.nchunks + 2 * seg] = red[0][0];
    a.part[a.nchunks + 2 * seg + 1] = red[1][0];
  }
}

__global__ __launch_bounds__(OPT_LANES) void k_policy_opt_scalars(OptArgs a) {
  __shared__ double buf[OPT_CHUNK];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int base = 0; base < a.nchunks; base += OPT_CHUNK) {
    const int n = a.nchunks - base < OPT_CHUNK ? a.nchunks - base : OPT_CHUNK;
    for (int i = tid; i < n; i += OPT_LANES) buf[i] = a.part[base + i];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < n; i++) total += buf[i];
    __syncthreads();
  }
  if (tid != 0) return;
  const bool sched = a.nseg > 0;
  double kl = 0.0, used = 0.0;
  for (int seg = 0; seg < a.nseg; seg++) {
    kl += a.part[a.nchunks + 2 * seg];
    used += a.part[a.nchunks + 2 * seg + 1];
  }
  if (sched) kl = kl / (double)a.M;
  const double norm = sqrt(total);
  double coef = 1.0;
  if (a.max_norm > 0.0) {
    const double x = a.max_norm / (norm + 1e-6);
    coef = x > 1.0 ? 1.0 : x;                        // (a NaN stays a NaN, as torch's clamp leaves it)
  }
  const float lr0 = a.lr[0];
  const long long step0 = a.step[0];
  const bool skip = a.skip_nonfinite && (!isfinite(norm) || (sched && !isfinite(kl)));
  float lr = lr0;
  long long t = step0;
  OptScalars sc = {norm, kl, (float)coef, 0.f, 1.f, skip ? 1 : 0};
  if (!skip) {
    if (sched) {
      if (kl > 2.0 * a.desired_kl) lr = fmaxf(a.lr_min, lr0 / 1.5f);
      else if (kl > 0.0 && kl < a.desired_kl / 2.0) lr = fminf(a.lr_max, lr0 * 1.5f);
    }
    t = step0 + 1;
    const double bc1 = 1.0 - pow(a.b1, (double)t), bc2 = 1.0 - pow(a.b2, (double)t);
    sc.step_size = (float)((double)lr / bc1);
    sc.bc2_sqrt = (float)sqrt(bc2);
    a.lr[0] = lr;
    a.step[0] = t;
  }
  *a.sc = sc;
  a.stats[0] = (float)norm;
  a.stats[1] = (float)coef;
  a.stats[2] = (float)kl;
  a.stats[3] = lr;
  a.stats[4] = (float)t;
  a.stats[5] = skip ? 1.f : 0.f;
  a.stats[6] = (float)used;
  a.stats[7] = lr > lr0 ? 1.f : lr < lr0 ? -1.f : 0.f;
}

// torch.optim.Adam's single-tensor arithmetic on one element, every product and sum rounded on its own as torch's kernels do
__device__ __forceinline__ void opt_adam(const OptArgs &a, const OptScalars &sc, float grad, float &p, float &m, float &v) {
  const float g = sc.coef * grad;
  const float dm = (g - m) * a.omb1;
  m = m + dm;
  const float vb = a.b2f * v, gg = (a.omb2 * g) * g;
  v = vb + gg;
  const float denom = sqrtf(v) / sc.bc2_sqrt + a.epsf;
  const float q = sc.step_size * (m / denom);
  p = p - q;
}

__global__ __launch_bounds__(OPT_LANES) void k_policy_opt_apply(OptArgs a) {
  const OptScalars sc = *a.sc;
  if (sc.skip) return;
  const int tid = threadIdx.x, b = blockIdx.x;
  const OptPiece &pc = a.piece[opt_piece_of(a, b)];
  const int e = (b - pc.chunk0) * OPT_CHUNK + 4 * tid;
  float *vv = pc.m + a.P;
  if (pc.vec && e + 3 < pc.n) {
    const float4 g = *reinterpret_cast<const float4 *>(pc.g + e);
    float4 p = *reinterpret_cast<const float4 *>(pc.p + e);
    float4 m = *reinterpret_cast<const float4 *>(pc.m + e);
    float4 v = *reinterpret_cast<const float4 *>(vv + e);
    opt_adam(a, sc, g.x, p.x, m.x, v.x);
    opt_adam(a, sc, g.y, p.y, m.y, v.y);
    opt_adam(a, sc, g.z, p.z, m.z, v.z);
    opt_adam(a, sc, g.w, p.w, m.w, v.w);
    *reinterpret_cast<float4 *>(pc.p + e) = p;
    *reinterpret_cast<float4 *>(pc.m + e) = m;
    *reinterpret_cast<float4 *>(vv + e) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (e + i >= pc.n) break;
      float p = pc.p[e + i], m = pc.m[e + i], v = vv[e + i];
      opt_adam(a, sc, pc.g[e + i], p, m, v);
      pc.p[e + i] = p; pc.m[e + i] = m; vv[e + i] = v;
    }
  }
}

} // namespace tsidb
