// tsidb_learner.hpp - the update's side of a PPO iteration (include/tsidb.h tsidb_policy_learn): the clipped surrogate, the
// clipped value loss and the entropy of one minibatch of stored rollout rows, and the gradient of every weight, bias and of
// log_std.  The optimiser stays the caller's.  No reference counterpart (the reference's only controller is TSID, main.py:113-129).
//
// Three launches, no atomics, every sum in one fixed order: two calls on the same inputs give the same bits.
//
// k_policy_learn_rows: k_policy_actor's tile - four wavefronts per 16 minibatch rows and per network (blockIdx.y: actor, critic).
// The rows index[m] of the stored float32 inputs are gathered into LDS, act_layers (tsidb_actor.hpp) runs the forward pass the
// actor ran, each layer's rows H_l go to the workspace; the epilogue evaluates the loss of each row and G_last = dloss / d(output);
// then backward-data, layer by layer, G_{l-1} = (G_l W_l) * act'(H_{l-1}), between the same two LDS images, each G_l to the
// workspace.  Fragments of v_mfma_f32_16x16x4_f32 for G_l W_l (i = lane & 15, g = lane >> 4):
//   A[row i][k g]   = G_l[row i of the tile][n0 + g]                         (LDS)
//   B[k g][col i]   = W_l[n0 + g][k0 + i]: 16 contiguous floats per g        (global, in place)
//   D[row 4 g + r][col i] = G_{l-1}[row 4 g + r][k0 + i]
// A row past M, or whose index is outside [0, rows), is gathered as zeros and gets G_last = 0: it adds nothing anywhere.
//
// k_policy_learn_wgrad: one wavefront per (job, output tile, group of 4 input tiles, row segment), the batch as the k dimension:
//   A[row i][k g] = G_l[m0 + g][n0 + i],  B[k g][col i] = H_{l-1}[m0 + g][k0 + i],  D = dW_l[n0 + 4 g + r][k0 + i]
// H_{-1} is the gathered input, and column fan-in of H is a constant 1: its column of dW is db.  The per-row loss pieces are one
// more job (G = a column of ones): their column sums are dlog_std and the stats.  Rows are cut into segments of
// TSIDB_POL_LEARN_SEG_ROWS, a constant that depends on nothing, each segment's result goes to its own slice of the workspace.
//
// k_policy_learn_reduce: one thread per gradient element adds the segments' slices in segment order and overwrites .grad.
//
// The imitation variant (tsidb_policy_learn_imit): k_policy_learn_rows_imit and k_policy_learn_reduce_imit are the IMIT = true
// instantiations of the two bodies below, k_policy_learn_wgrad is shared.  The rows kernel adds the label's term to G_last = dmu,
// scales the surrogate's dlogp, zeroes the surrogate pieces of a row the policy did not act on, and writes LRN_NI more per-row
// pieces behind the six; the row-piece job of the weight gradient sums them with the others, in the same fixed order.  The
// IMIT = false instantiations are the kernels as they were: same names, same arguments, same code.
//
// The symmetry variant (tsidb_policy_learn_sym): k_policy_learn_rows_sym and k_policy_learn_reduce_sym are the SYM = true
// instantiations.  A workgroup runs its tile twice: pass 0 is the plain one, pass 1 gathers the same stored rows through the
// network's signed permutation (x'[c] = sign[c] x[perm[c]]), runs the forward pass again and writes every per-row array at rows
// Mp + m0 + r - the originals keep rows [0, Mp) of arrays of 2 Mp rows, the mirrors take [Mp, 2 Mp), the weight gradient runs
// over 2 Mp rows.  Pass 0 leaves mu of its 16 rows in a 16 x NA LDS image: S_a mu is the constant target of pass 1's mirror term.
// LRN_NS more per-row pieces sit behind the six.  The SYM = false instantiations are the kernels as they were.
#pragma once
#include <type_traits>
#include "tsidb_actor.hpp"

namespace tsidb {

constexpr int LRN_SEG = TSIDB_POL_LEARN_SEG_ROWS;
constexpr int LRN_KGROUP = 4;              // input tiles per wavefront of the weight gradient: they share the A fragment
constexpr int LRN_NR = NA + 6;             // per-row pieces: dlogp (z_a^2 - 1) [NA], then the LRN_R_* columns
enum { LRN_R_LPI = 0, LRN_R_LV, LRN_R_KL, LRN_R_CLIPPED, LRN_R_USED, LRN_R_BAD };
constexpr int LRN_NI = 4;                  // the imitation variant's pieces, behind the six: w l_m, w, w > 0, surrogate skipped
enum { LRN_I_LIM = 0, LRN_I_WSUM, LRN_I_WPOS, LRN_I_SKIPPED };
constexpr int LRN_NS = 2;                  // the symmetry variant's pieces, behind the six: |mu(x') - S_a mu(x)|^2, mirrored row used
enum { LRN_S_LSYM = 0, LRN_S_USED };
constexpr int LRN_MAXJOBS = 2 * ACT_MAXL + 1;

struct LearnNet {
  ActorNet net;                            // as the forward pass takes it (the block fields unused)
  const float *in;                         // [rows, K] the stored input rows
  size_t x, h[ACT_MAXL], g[ACT_MAXL];      // workspace offsets in floats: gathered rows [Mp, K], H_l and G_l [Mp, width_l]
};

struct LearnArgs {
  LearnNet net[2];                         // actor, critic (net[1].net.n_layers = 0: none)
  int M, rows, LD, value_clip;
  const int *index;
  const float *action, *logp, *value, *advantage, *returns, *adv_stats, *log_std;
  float clip, value_coef;
  float *ws;
  size_t r;                                // workspace offset of the per-row pieces [Mp, LRN_NR]
};

// tsidb_policy_learn_imit's additions to the rows kernel; target is read only where coef > 0 or the row's weight is not 0
struct LearnImit {
  const float *target, *weight;            // [rows, NA], [rows] (NULL: 1)
  const int *skip;                         // [rows] (NULL: none)
  float coef, surrogate_coef;
  int huber;
};

// tsidb_policy_learn_sym's additions to the rows kernel.  A perm entry outside its row reads as a 0 column.
struct LearnSym {
  const int *perm[2];                      // actor input [K_actor], critic input [K_critic] (NULL without a critic)
  const float *sign[2];
  const int *aperm;                        // action [NA]
  const float *asign;
  int augment, Mp;                         // Mp: the first workspace row of the mirrors
  float coef;                              // the mirror term's weight
};

__device__ __forceinline__ float act_prime(int kind, float y) {   // the activation's derivative from its output
  if (kind == ACT_ELU) return y > 0.f ? 1.f : y + 1.f;
  if (kind == ACT_TANH) return 1.f - y * y;
  return y > 0.f ? 1.f : 0.f;
}

template <bool IMIT, bool SYM = false>
__device__ __forceinline__ void policy_learn_rows_body(const LearnArgs &a, const LearnImit &im, [[maybe_unused]] const LearnSym &sy = LearnSym{}) {
  static_assert(!(IMIT && SYM), "the symmetry variant has no imitation term");
  constexpr int NR = IMIT ? LRN_NR + LRN_NI : SYM ? LRN_NR + LRN_NS : LRN_NR;   // the stride of the per-row pieces
  extern __shared__ float lrn_lds[];
  __shared__ int lrn_row[ACT_TILE];        // the stored row of each tile row, -1 = none
  [[maybe_unused]] float *lrn_mu = nullptr;   // SYM: mu of pass 0 [ACT_TILE, NA]
  if constexpr (SYM) {
    __shared__ float lrn_mu_image[ACT_TILE * NA];
    lrn_mu = lrn_mu_image;
  }
  const int which = blockIdx.y;
  const LearnNet &ln = a.net[which];
  const ActorNet &net = ln.net;
  const int LD = a.LD, tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * ACT_TILE;
  float *X[2] = {lrn_lds, lrn_lds + ACT_TILE * LD};
  float *ws = a.ws;

  if (tid < ACT_TILE) {
    int j = -1;
    if (m0 + tid < a.M) {
      j = a.index[m0 + tid];
      if (j < 0 || j >= a.rows) j = -1;
    }
    lrn_row[tid] = j;
  }
  __syncthreads();

  // one pass over the tile; mir (a compile-time constant): the tile's mirror image, at workspace rows Mp + m0 ..
  auto run_pass = [&](auto mirrored) {
  constexpr bool mir = decltype(mirrored)::value;
  [[maybe_unused]] const bool surr = !mir || sy.augment;   // the pass carries the surrogate and the value loss
  const int w0 = mir ? sy.Mp + m0 : m0;    // the tile's first workspace row

  if constexpr (mir) {
    if (!surr && which == 1) {             // no mirrored rows for the critic: exact zeros where the weight gradient reads
      float *R = ws + a.r;
      for (int idx = tid; idx < ACT_TILE * net.K; idx += WAVE * ACT_WAVES) ws[ln.x + (size_t)w0 * net.K + idx] = 0.f;
      for (int L = 0; L < net.n_layers; L++) {
        const int width = net.width[L];
        for (int idx = tid; idx < ACT_TILE * width; idx += WAVE * ACT_WAVES) {
          ws[ln.h[L] + (size_t)w0 * width + idx] = 0.f;
          ws[ln.g[L] + (size_t)w0 * width + idx] = 0.f;
        }
      }
      if (tid < ACT_TILE) R[(size_t)(w0 + tid) * NR + NA + LRN_R_LV] = 0.f;
      return;                              // (block-uniform)
    }
  }

  // ---- the input rows, gathered; a row without a stored row and the columns up to the next multiple of 4 are 0
  for (int idx = tid; idx < ACT_TILE * net.K; idx += WAVE * ACT_WAVES) {
    const int r = idx / net.K, c = idx - r * net.K, j = lrn_row[r];
    float v;
    if constexpr (!mir) {
      v = j >= 0 ? ln.in[(size_t)j * net.K + c] : 0.f;
    } else {
      const int src = sy.perm[which][c];
      v = j >= 0 && src >= 0 && src < net.K ? sy.sign[which][c] * ln.in[(size_t)j * net.K + src] : 0.f;
    }
    X[0][r * LD + c] = v;
    ws[ln.x + (size_t)(w0 + r) * net.K + c] = v;
  }
  if (tid < ACT_TILE * 4) {
    const int r = tid >> 2, c = net.K + (tid & 3);
    if (c < ((net.K + 3) & ~3)) X[0][r * LD + c] = 0.f;
  }
  __syncthreads();

  // ---- forward: the actor's layers, each layer's rows to the workspace
  act_layers(net, X, LD, i, g, wave, [&](int L, const float *H, int width) {
    for (int idx = tid; idx < ACT_TILE * width; idx += WAVE * ACT_WAVES) {
      const int r = idx / width, c = idx - r * width;
      ws[ln.h[L] + (size_t)(w0 + r) * width + c] = H[r * LD + c];
    }
  });

  // ---- the loss of each row and G_last, into the image the last layer did not write
  const int last = net.n_layers - 1;
  const float *Y = X[net.n_layers & 1];
  float *G = X[(net.n_layers + 1) & 1];
  const float invM = 1.f / (float)(SYM && sy.augment ? 2 * a.M : a.M);
  float *R = ws + a.r;
  if (which == 1) {
    if (tid < ACT_TILE) {
      const int j = lrn_row[tid];
      float lv = 0.f, dv = 0.f;
      if (j >= 0) {
        const float v = Y[tid * LD], old = a.value[j], ret = a.returns[j];
        const float e1 = v - ret, l1 = e1 * e1;
        float raw = 2.f * e1;
        lv = l1;
        if (a.value_clip) {
          const float d = v - old, dc = fminf(fmaxf(d, -a.clip), a.clip);
          const float e2 = (old + dc) - ret, l2 = e2 * e2;
          const float ins = fabsf(d) <= a.clip ? 1.f : 0.f;
          if (l1 < l2) { raw = 2.f * e2 * ins; lv = l2; }
          else if (l1 == l2) raw = e1 + e2 * ins;
        }
        dv = raw * a.value_coef * invM;
      }
      R[(size_t)(w0 + tid) * NR + NA + LRN_R_LV] = lv;
      G[tid * LD] = dv;
      G[tid * LD + 1] = G[tid * LD + 2] = G[tid * LD + 3] = 0.f;
      ws[ln.g[last] + (size_t)(w0 + tid)] = dv;
    }
  } else {
    float *DL = G + LD - 1;                // dlogp of row r at G[r * LD + LD - 1]: past every column a layer uses
    for (int idx = tid; idx < ACT_TILE * NA; idx += WAVE * ACT_WAVES) {
      const int r = idx / NA, c = idx - r * NA, j = lrn_row[r];
      if constexpr (!mir) {
        G[r * LD + c] = j >= 0 ? (a.action[(size_t)j * NA + c] - Y[r * LD + c]) / expf(a.log_std[c]) : 0.f;   // z
        if constexpr (SYM) lrn_mu[r * NA + c] = Y[r * LD + c];
      } else {                             // z of the mirrored action; 0 where the pass has no surrogate
        const int src = sy.aperm[c];
        const float act = j >= 0 && src >= 0 && src < NA ? sy.asign[c] * a.action[(size_t)j * NA + src] : 0.f;
        G[r * LD + c] = j >= 0 && surr ? (act - Y[r * LD + c]) / expf(a.log_std[c]) : 0.f;
      }
    }
    __syncthreads();
    if (tid < ACT_TILE) {
      const int j = lrn_row[tid];
      float piece[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dlogp = 0.f;
      [[maybe_unused]] float ipiece[LRN_NI] = {0.f, 0.f, 0.f, 0.f};
      [[maybe_unused]] float spiece[LRN_NS] = {0.f, 0.f};
      if constexpr (mir) {
        if (j >= 0) {                      // the mirror term's row: |mu(x') - S_a mu(x)|^2, S_a mu(x) from pass 0's image
          float ls = 0.f;
          for (int c = 0; c < NA; c++) {
            const int src = sy.aperm[c];
            const float t = src >= 0 && src < NA ? sy.asign[c] * lrn_mu[tid * NA + src] : 0.f;
            const float d = Y[tid * LD + c] - t;
            ls += d * d;
          }
          spiece[LRN_S_LSYM] = ls;
          spiece[LRN_S_USED] = 1.f;
        }
      }
      if (j >= 0 && surr) {
        float s = 0.f;
        for (int c = 0; c < NA; c++) {
          const float z = G[tid * LD + c];
          s += 0.5f * z * z + a.log_std[c];
        }
        const float logp = -s - (float)(0.5 * NA * 1.8378770664093453);   // ln 2 pi; the actor's own expression
        const float old = a.logp[j];
        const float ratio = expf(logp - old);
        float adv = a.advantage[j];
        if (a.adv_stats) adv = (adv - a.adv_stats[0]) * a.adv_stats[1];
        const float lo = 1.f - a.clip, hi = 1.f + a.clip;
        const float t1 = -adv * ratio, t2 = -adv * fminf(fmaxf(ratio, lo), hi);
        const bool inside = ratio >= lo && ratio <= hi;
        const float dr = inside || t1 > t2 ? -adv * invM : 0.f;
        dlogp = ratio * dr;
        piece[LRN_R_LPI] = fmaxf(t1, t2);
        piece[LRN_R_KL] = old - logp;
        piece[LRN_R_CLIPPED] = inside ? 0.f : 1.f;
        piece[LRN_R_USED] = 1.f;
        if constexpr (IMIT) {
          dlogp = dlogp * im.surrogate_coef;
          if (im.skip && im.skip[j] != 0) {  // the env executed another action than the stored one: no surrogate for the row
            dlogp = 0.f;
            piece[LRN_R_LPI] = piece[LRN_R_KL] = piece[LRN_R_CLIPPED] = 0.f;
            ipiece[LRN_I_SKIPPED] = 1.f;
          }
          const float w = im.weight ? im.weight[j] : 1.f;
          ipiece[LRN_I_WSUM] = w;
          ipiece[LRN_I_WPOS] = w > 0.f ? 1.f : 0.f;
          if (im.target && w != 0.f) {       // a select, not a product: the label behind a zero weight is not read
            float li = 0.f;
            for (int c = 0; c < NA; c++) {
              const float d = Y[tid * LD + c] - im.target[(size_t)j * NA + c], ad = fabsf(d);
              li += im.huber ? (ad <= 1.f ? 0.5f * d * d : ad - 0.5f) : d * d;
            }
            ipiece[LRN_I_LIM] = w * (li / (float)NA);
          }
        }
      } else if (j < 0 && !mir && m0 + tid < a.M) {   // (a bad index is counted once, by pass 0)
        piece[LRN_R_BAD] = 1.f;
      }
      DL[tid * LD] = dlogp;
      float *Rr = R + (size_t)(w0 + tid) * NR + NA;
      for (int c = 0; c < 6; c++)
        if (c != LRN_R_LV || a.net[1].net.n_layers == 0) Rr[c] = piece[c];   // (LV is the critic's workgroup's; 0 without one)
      if constexpr (IMIT)
        for (int c = 0; c < LRN_NI; c++) Rr[6 + c] = ipiece[c];
      if constexpr (SYM)
        for (int c = 0; c < LRN_NS; c++) Rr[6 + c] = spiece[c];
    }
    __syncthreads();
    for (int idx = tid; idx < ACT_TILE * NA; idx += WAVE * ACT_WAVES) {
      const int r = idx / NA, c = idx - r * NA;
      const float z = G[r * LD + c], dlogp = DL[r * LD];
      float dmu = dlogp * z / expf(a.log_std[c]);
      if constexpr (IMIT) {                  // the label's term: on the mean alone, log_std gets nothing from it
        const int j = lrn_row[r];
        if (j >= 0 && im.coef > 0.f) {
          const float w = im.weight ? im.weight[j] : 1.f;
          if (w != 0.f) {
            const float d = Y[r * LD + c] - im.target[(size_t)j * NA + c];
            const float gd = im.huber ? fminf(fmaxf(d, -1.f), 1.f) : 2.f * d;
            const float gi = im.coef * invM / (float)NA * w * gd;
            dmu = dmu + gi;
          }
        }
      }
      if constexpr (mir) {                   // the mirror term: on the mean of the mirrored row alone, its target a constant
        if (sy.coef > 0.f && lrn_row[r] >= 0) {
          const int src = sy.aperm[c];
          const float t = src >= 0 && src < NA ? sy.asign[c] * lrn_mu[r * NA + src] : 0.f;
          const float d = Y[r * LD + c] - t;
          const float gs = sy.coef * (2.f / (float)(a.M * NA)) * d;
          dmu = dmu + gs;
        }
      }
      G[r * LD + c] = dmu;
      ws[ln.g[last] + (size_t)(w0 + r) * NA + c] = dmu;
      R[(size_t)(w0 + r) * NR + c] = dlogp * (z * z - 1.f);
    }
    if (tid < ACT_TILE * 4) {
      const int r = tid >> 2, c = NA + (tid & 3);
      if (c < ((NA + 3) & ~3)) G[r * LD + c] = 0.f;
    }
  }
  __syncthreads();

  // ---- backward-data: G_{l-1} = (G_l W_l) * act'(H_{l-1}), the images alternating as in the forward pass
  for (int L = last; L >= 1; L--) {
    const float *A = X[L & 1], *W = net.W[L];          // (G_last sits in X[(n_layers + 1) & 1] = X[last & 1]: G_l where the layer's input was)
    float *D = X[(L + 1) & 1];
    const int Nn = net.width[L], Kk = net.width[L - 1], ktiles = (Kk + 15) >> 4;
    const float *Hprev = ws + ln.h[L - 1];
    float *Gprev = ws + ln.g[L - 1];
    for (int base = 0; base < ktiles; base += ACT_WAVES * ACT_NACC) {
      act_f32x4 acc[ACT_NACC];
      int kcol[ACT_NACC];
#pragma unroll
      for (int j = 0; j < ACT_NACC; j++) {
        acc[j] = act_f32x4{0.f, 0.f, 0.f, 0.f};
        kcol[j] = (base + wave + ACT_WAVES * j) * 16 + i;
      }
      for (int n0 = 0; n0 < Nn; n0 += 4) {
        const int n = n0 + g;
        const float av = A[i * LD + n];                // (n < round_up(Nn, 4): the pad columns hold 0)
#pragma unroll
        for (int j = 0; j < ACT_NACC; j++) {
          if (base + wave + ACT_WAVES * j < ktiles) {  // wave-uniform
            const float bv = n < Nn && kcol[j] < Kk ? W[(size_t)n * Kk + kcol[j]] : 0.f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ACT_NACC; j++) {
        if (base + wave + ACT_WAVES * j < ktiles) {
          const int k = kcol[j];
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r;
            float y = 0.f;
            if (k < Kk) {
              y = acc[j][r] * act_prime(net.activation, Hprev[(size_t)(w0 + row) * Kk + k]);
              Gprev[(size_t)(w0 + row) * Kk + k] = y;
            }
            D[row * LD + k] = y;                       // (k < round_up(Kk, 16) <= LD: the pad columns get 0)
          }
        }
      }
    }
    __syncthreads();
  }
  };                                       // run_pass
  run_pass(std::false_type{});
  if constexpr (SYM) run_pass(std::true_type{});
}

__global__ __launch_bounds__(WAVE * ACT_WAVES) void k_policy_learn_rows(LearnArgs a) { policy_learn_rows_body<false>(a, LearnImit{}); }
__global__ __launch_bounds__(WAVE * ACT_WAVES) void k_policy_learn_rows_imit(LearnArgs a, LearnImit im) { policy_learn_rows_body<true>(a, im); }
__global__ __launch_bounds__(WAVE * ACT_WAVES) void k_policy_learn_rows_sym(LearnArgs a, LearnSym sy) { policy_learn_rows_body<false, true>(a, LearnImit{}, sy); }

// ---------------------------------------------------------------------------- the weight gradients, segment by segment
struct WgradJob {
  size_t g, h, p;        // workspace offsets: G [Mp, gw] (unused with ones), H [Mp, hw], the job's slice of a segment's partial [gw, hw + 1]
  int gw, hw, ones;      // ones: G is a single column of 1
  int nkg, blk0;         // groups of input tiles; the job's first blockIdx.x
};

struct WgradArgs {
  WgradJob job[LRN_MAXJOBS];
  int njobs, Mp;
  float *ws;
  size_t part, total;    // workspace offset of the partials [nseg, total]
};

__global__ __launch_bounds__(WAVE) void k_policy_learn_wgrad(WgradArgs a) {
  int ji = 0;
  while (ji + 1 < a.njobs && (int)blockIdx.x >= a.job[ji + 1].blk0) ji++;
  const WgradJob &job = a.job[ji];
  const int t = blockIdx.x - job.blk0, nt = t / job.nkg, kg = t - nt * job.nkg;
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const int seg = blockIdx.y, mb = seg * LRN_SEG, me = min(a.Mp, mb + LRN_SEG);
  const int gw = job.gw, hw = job.hw, kext = hw + 1, n = nt * 16 + i;
  const float *G = a.ws + job.g, *H = a.ws + job.h;
  act_f32x4 acc[LRN_KGROUP];
  int kcol[LRN_KGROUP];
#pragma unroll
  for (int j = 0; j < LRN_KGROUP; j++) {
    acc[j] = act_f32x4{0.f, 0.f, 0.f, 0.f};
    kcol[j] = (kg * LRN_KGROUP + j) * 16 + i;
  }
  for (int mm = mb; mm < me; mm += 4) {                // (Mp is a multiple of 16: whole groups of 4 rows)
    const size_t m = mm + g;
    const float av = n < gw ? (job.ones ? 1.f : G[m * gw + n]) : 0.f;
#pragma unroll
    for (int j = 0; j < LRN_KGROUP; j++) {
      if ((kg * LRN_KGROUP + j) * 16 < kext) {         // wave-uniform
        const int k = kcol[j];
        const float bv = k < hw ? H[m * hw + k] : (k == hw ? 1.f : 0.f);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
  }
  float *P = a.ws + a.part + (size_t)seg * a.total + job.p;
#pragma unroll
  for (int j = 0; j < LRN_KGROUP; j++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int nn = nt * 16 + 4 * g + r, k = kcol[j];
      if (nn < gw && k < kext) P[(size_t)nn * kext + k] = acc[j][r];
    }
  }
}

// ---------------------------------------------------------------------------- the segments added up, in segment order
struct ReducePiece {
  size_t p;              // the layer's offset in a segment's partial, [width, kext]
  int width, kext;
  float *dW, *db;        // [width, kext - 1], [width] (NULL: no bias)
};

struct ReduceArgs {
  ReducePiece piece[2 * ACT_MAXL];
  int npieces, nseg, M;
  const float *ws;
  size_t part, total, rp;   // rp: offset of the row pieces' sums [LRN_NR + 1] in a segment's partial = the layers' elements in all
  const float *log_std;
  float *log_std_grad, *stats;
  float value_coef, entropy_coef;
};

// tsidb_policy_learn_imit's additions to the reduction: the coefficients of the full loss and where the four sums go
struct ReduceImit {
  float coef, surrogate_coef;
  float *stats;          // [TSIDB_POL_IMIT_NSTATS]
};

// tsidb_policy_learn_sym's additions to the reduction; ReduceArgs.M is then the rows the means are over (2 M with augment)
struct ReduceSym {
  float coef;
  int M;                 // the minibatch's rows: L_sym = sum / (M NA)
  float *stats;          // [TSIDB_POL_SYM_NSTATS]
};

template <bool IMIT, bool SYM = false>
__device__ __forceinline__ void policy_learn_reduce_body(const ReduceArgs &a, const ReduceImit &im, [[maybe_unused]] const ReduceSym &sy = ReduceSym{}) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float *P = a.ws + a.part;
  auto total_of = [&](size_t off) {
    float s = 0.f;
    for (int seg = 0; seg < a.nseg; seg++) s += P[(size_t)seg * a.total + off];
    return s;
  };
  if (e < a.rp) {
    int pi = 0;
    while (pi + 1 < a.npieces && e >= a.piece[pi + 1].p) pi++;
    const ReducePiece &pc = a.piece[pi];
    const size_t o = e - pc.p;
    const int n = (int)(o / pc.kext), k = (int)(o - (size_t)n * pc.kext);
    const float s = total_of(e);
    if (k < pc.kext - 1) pc.dW[(size_t)n * (pc.kext - 1) + k] = s;
    else if (pc.db) pc.db[n] = s;
  } else if (e < a.rp + NA) {
    const int c = (int)(e - a.rp);
    a.log_std_grad[c] = total_of(e) - a.entropy_coef;
  } else if (e == a.rp + NA) {
    const float invM = 1.f / (float)a.M;
    float ent = 0.f;
    for (int c = 0; c < NA; c++) ent += a.log_std[c] + (float)(0.5 + 0.5 * 1.8378770664093453);
    const float lpi = total_of(a.rp + NA + LRN_R_LPI) * invM, lv = total_of(a.rp + NA + LRN_R_LV) * invM;
    a.stats[0] = lpi;
    a.stats[1] = lv;
    a.stats[2] = ent;
    a.stats[3] = total_of(a.rp + NA + LRN_R_KL) * invM;
    a.stats[4] = total_of(a.rp + NA + LRN_R_CLIPPED) * invM;
    if constexpr (SYM) {
      const float lsym = total_of(a.rp + NA + 6 + LRN_S_LSYM) / (float)(sy.M * NA);
      float loss = lpi + a.value_coef * lv - a.entropy_coef * ent;
      if (sy.coef > 0.f) {
        const float t = sy.coef * lsym;
        loss = loss + t;
      }
      a.stats[5] = loss;
      sy.stats[0] = lsym;
    } else if constexpr (!IMIT) {
      a.stats[5] = lpi + a.value_coef * lv - a.entropy_coef * ent;
    } else {
      const float lim = total_of(a.rp + NA + 6 + LRN_I_LIM) * invM;
      const float spi = im.surrogate_coef * lpi;          // (statements of their own: a coefficient of 1 and one of 0 leave
      float loss = spi + a.value_coef * lv - a.entropy_coef * ent;   //  the expression above, bit for bit)
      if (im.coef > 0.f) {
        const float t = im.coef * lim;
        loss = loss + t;
      }
      a.stats[5] = loss;
      im.stats[0] = lim;
    }
    a.stats[6] = total_of(a.rp + NA + LRN_R_USED);
    a.stats[7] = total_of(a.rp + NA + LRN_R_BAD);
  } else if (IMIT && e < a.rp + NA + LRN_NI) {   // the three other sums, a thread each: a segment-ordered sum is a serial chain of loads
    const int k = (int)(e - (a.rp + NA));        // 1 .. LRN_NI - 1
    im.stats[k] = total_of(a.rp + NA + 6 + k);
  } else if (SYM && e == a.rp + NA + 1) {        // the mirrored rows used
    sy.stats[1] = total_of(a.rp + NA + 6 + LRN_S_USED);
  }
}

__global__ __launch_bounds__(256) void k_policy_learn_reduce(ReduceArgs a) { policy_learn_reduce_body<false>(a, ReduceImit{}); }
__global__ __launch_bounds__(256) void k_policy_learn_reduce_imit(ReduceArgs a, ReduceImit im) { policy_learn_reduce_body<true>(a, im); }
__global__ __launch_bounds__(256) void k_policy_learn_reduce_sym(ReduceArgs a, ReduceSym sy) { policy_learn_reduce_body<false, true>(a, ReduceImit{}, sy); }

} // namespace tsidb
