// tsidb_actor.hpp - the policy's side of a rollout (include/tsidb.h tsidb_policy_actor / tsidb_policy_gae): a dense actor and
// an optional critic evaluated on the env's own rows, the Gaussian sample and its log-probability, and the advantage recursion
// over a recorded rollout.  No reference counterpart: the reference's only controller is TSID (main.py:113-129).
//
// k_policy_actor: a workgroup of four wavefronts per tile of ACT_TILE = 16 envs and per network (blockIdx.y: actor, critic).
// The input row is assembled from up to four column blocks of the env's buffers (cast to float32 on load) into LDS, the layers
// run on v_mfma_f32_16x16x4_f32 with the activations passing between two LDS images, the epilogue samples.  Weights and biases
// are read in place, in nn.Linear's layout, at every launch: nothing is packed or cached, so an optimiser step on the tensors
// behind the pointers is seen by the next launch.
//
// Fragment layout of v_mfma_f32_16x16x4_f32, D[16 x 16] += A[16 x 4] B[4 x 16] (i = lane & 15, g = lane >> 4):
//   A: one float per lane, A[row i][k g]      = activation of env i of the tile, input k0 + g        (LDS, row stride LD)
//   B: one float per lane, B[k g][col i]      = weight[out n0 + i][in k0 + g]                         (global, in place)
//   D: four floats per lane, D[row 4 g + r][col i], r = 0 .. 3 = env 4 g + r of the tile, output n0 + i
// K and N are padded to the tile with zeros in registers (B) and LDS (A): k >= fan-in and n >= width load 0, never memory.
// LD = 4 mod 32 floats: the 64 A addresses i * LD + k0 + g fall into 64 different (bank, half) slots - 4 i + g mod 64 are all
// different - so the read takes the two passes 64 lanes need and no more; the D store of one register (row 4 g + r, col i:
// 16 g + 4 r + i mod 64 over the lanes) likewise.
//
// The sample: eps = sqrt(-2 ln(1 - U1)) cos(2 pi U2) with U1, U2 the hash draws of streams 21 and 22, column = actuator, env =
// env + env_offset, counter = episode * 2^32 + ep_len (the observation noise's), formed in float64 and cast to float32 once.
// Two calls on the same (env, episode, ep_len) draw the same noise: the sample belongs to the observation, not to the call.
#pragma once
#include "tsidb_common.hpp"
#include "tsidb_policy.hpp"

namespace tsidb {

constexpr int ACT_TILE = 16;        // envs per workgroup
constexpr int ACT_WAVES = 4;        // wavefronts per workgroup
constexpr int ACT_NACC = 4;         // independent accumulators per wavefront: 4 N-tiles share one A fragment
constexpr int ACT_MAXW = 512;       // TSIDB_POL_NET_MAXWIDTH
constexpr int ACT_MAXL = 4;         // TSIDB_POL_NET_MAXLAYERS
constexpr int ACT_MAXB = 4;         // TSIDB_POL_NET_MAXBLOCKS
enum { ACT_ELU = 0, ACT_TANH = 1, ACT_RELU = 2 };
enum { ACT_S_U1 = 21, ACT_S_U2 = 22 };

typedef float act_f32x4 __attribute__((ext_vector_type(4)));

// one network, by value in the launch
struct ActorNet {
  int n_layers, n_blocks, activation, K;   // K = the input columns in total
  int width[ACT_MAXL];
  const float *W[ACT_MAXL], *b[ACT_MAXL];  // [width, fan-in] row-major, [width] (NULL = no bias)
  const void *blk[ACT_MAXB];               // column blocks of the input row, the path's type
  int blk_ld[ACT_MAXB], blk_cols[ACT_MAXB];
  float *input;                            // [N, K] the assembled rows, or NULL
};

struct ActorArgs {
  ActorNet net[2];                         // actor, critic (net[1].n_layers = 0: none)
  int n, LD, sample, first;                // first: the network of blockIdx.y = 0 (1 = a critic-only call)
  void *action;                            // [N, NA] the path's type
  float *action32, *mean, *logp, *value;
  const float *log_std;
  const int *episode, *ep_len;
  unsigned long long seed, env_offset;
};

// LDS row stride in floats for a network pair whose widest row (input or layer) is w: w rounded up to 32, + 4
__host__ __device__ inline int act_ld(int w) { return ((w + 31) / 32) * 32 + 4; }
__host__ __device__ inline size_t act_lds_bytes(int ld) { return (size_t)2 * ACT_TILE * ld * sizeof(float); }

__device__ __forceinline__ float act_fn(int kind, float x) {
  if (kind == ACT_ELU) return x > 0.f ? x : expm1f(x);
  if (kind == ACT_TANH) return tanhf(x);
  return x > 0.f ? x : 0.f;
}

// The layers of one network on the tile's 16 rows: X[0] holds the input rows (pad columns 0), layer L reads X[L & 1] and writes
// X[(L + 1) & 1]; after_layer(L, image, width) runs behind each layer's barrier (k_policy_actor: nothing; k_policy_learn_rows
// stores the rows).  One copy, so that the learner's forward pass is the actor's bit for bit: same k order, same zero padding.
template <typename Hook>
__device__ __forceinline__ void act_layers(const ActorNet &net, float *const X[2], int LD, int i, int g, int wave, Hook &&after_layer) {
  int Kin = net.K;
  for (int L = 0; L < net.n_layers; L++) {
    const float *A = X[L & 1], *W = net.W[L], *bias = net.b[L];
    float *D = X[(L + 1) & 1];
    const int Nout = net.width[L], ntiles = (Nout + 15) >> 4;
    const bool hidden = L + 1 < net.n_layers;
    for (int base = 0; base < ntiles; base += ACT_WAVES * ACT_NACC) {
      act_f32x4 acc[ACT_NACC];
      const float *wrow[ACT_NACC];
      bool live[ACT_NACC];
#pragma unroll
      for (int j = 0; j < ACT_NACC; j++) {
        const int n = (base + wave + ACT_WAVES * j) * 16 + i;
        acc[j] = act_f32x4{0.f, 0.f, 0.f, 0.f};
        live[j] = n < Nout;                          // (a column past the width: B = 0, nothing is loaded)
        wrow[j] = W + (size_t)(live[j] ? n : 0) * Kin;
      }
      for (int k0 = 0; k0 < Kin; k0 += 4) {
        const int k = k0 + g;
        const float av = A[i * LD + k];              // (k < round_up(Kin, 4): the pad columns hold 0)
#pragma unroll
        for (int j = 0; j < ACT_NACC; j++) {
          if (base + wave + ACT_WAVES * j < ntiles) {   // wave-uniform
            const float bv = live[j] && k < Kin ? wrow[j][k] : 0.f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ACT_NACC; j++) {
        const int nt = base + wave + ACT_WAVES * j;
        if (nt < ntiles) {
          const int n = nt * 16 + i;
          const float bn = live[j] && bias ? bias[n] : 0.f;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            float y = 0.f;
            if (live[j]) {
              y = acc[j][r] + bn;
              if (hidden) y = act_fn(net.activation, y);
            }
            D[(4 * g + r) * LD + n] = y;             // (n < round_up(Nout, 16) <= LD: the pad columns get 0)
          }
        }
      }
    }
    Kin = Nout;
    __syncthreads();
    after_layer(L, D, Nout);
  }
}

// the input normalisation of a launch (k_policy_actor_norm): per network the float32 pair affine [2, K] = shift, scale that
// tsidb_policy_norm_update keeps (tsidb_norm.hpp; NULL = this network's rows stay raw) and the clamp (0 = none)
struct ActorNorm {
  const float *affine[2];
  float clip[2];
};

// NORM = false is k_policy_actor as it was before there was a normaliser, instruction for instruction: `nm` is not touched
template <typename T, bool NORM>
__device__ __forceinline__ void policy_actor_body(const ActorArgs &a, const ActorNorm *nm) {
  extern __shared__ float act_lds[];
  const int which = blockIdx.y + a.first;
  const ActorNet &net = a.net[which];
  const int LD = a.LD, tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform, and said so to the compiler: the tile tests become scalar branches
  const int e0 = blockIdx.x * ACT_TILE;
  float *X[2] = {act_lds, act_lds + ACT_TILE * LD};

  // ---- the input rows: block by block, cast on load; rows past the batch and the columns up to the next multiple of 4 are 0
  int off = 0;
  for (int bi = 0; bi < net.n_blocks; bi++) {
    const T *src = (const T *)net.blk[bi];
    const int cols = net.blk_cols[bi], ld = net.blk_ld[bi];
    for (int idx = tid; idx < ACT_TILE * cols; idx += WAVE * ACT_WAVES) {
      const int r = idx / cols, c = idx - r * cols, e = e0 + r;
      float v = 0.f;
      if (e < a.n) {
        v = (float)src[(size_t)e * ld + c];
        if constexpr (NORM) {
          const float *aff = nm->affine[which];
          if (aff) {                                 // one float32 subtraction, one float32 product: nothing to contract
            const float clip = nm->clip[which];
            v = (v - aff[off + c]) * aff[net.K + off + c];
            if (clip > 0.f) v = fminf(fmaxf(v, -clip), clip);
          }
        }
        if (net.input) net.input[(size_t)e * net.K + off + c] = v;
      }
      X[0][r * LD + off + c] = v;
    }
    off += cols;
  }
  if (tid < ACT_TILE * 4) {
    const int r = tid >> 2, c = net.K + (tid & 3);
    if (c < ((net.K + 3) & ~3)) X[0][r * LD + c] = 0.f;
  }
  __syncthreads();

  // ---- the layers
  act_layers(net, X, LD, i, g, wave, [](int, const float *, int) {});

  // ---- the epilogue, from the LDS image of the last layer
  const float *Y = X[net.n_layers & 1];
  float *E = X[(net.n_layers + 1) & 1];              // (free by now: eps of the tile)
  if (which == 1) {
    if (tid < ACT_TILE && e0 + tid < a.n && a.value) a.value[e0 + tid] = Y[tid * LD];
    return;
  }
  for (int idx = tid; idx < ACT_TILE * NA; idx += WAVE * ACT_WAVES) {
    const int r = idx / NA, c = idx - r * NA, e = e0 + r;
    if (e >= a.n) continue;
    const float mu = Y[r * LD + c];
    float eps = 0.f, act = mu;
    if (a.sample) {
      const unsigned long long ge = a.env_offset + (unsigned long long)e;
      const unsigned long long ctr = ((unsigned long long)(unsigned)a.episode[e] << 32) | (unsigned long long)(unsigned)a.ep_len[e];
      const double u1 = pol_draw(a.seed, ACT_S_U1, c, ge, ctr), u2 = pol_draw(a.seed, ACT_S_U2, c, ge, ctr);
      eps = (float)(sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2));
      act = mu + expf(a.log_std[c]) * eps;
    }
    E[r * LD + c] = eps;
    const size_t o = (size_t)e * NA + c;
    if (a.mean) a.mean[o] = mu;
    if (a.action32) a.action32[o] = act;
    if (a.action) ((T *)a.action)[o] = (T)act;
  }
  if (!a.logp) return;
  __syncthreads();
  if (tid < ACT_TILE && e0 + tid < a.n) {
    float s = 0.f;
    for (int c = 0; c < NA; c++) {
      const float eps = E[tid * LD + c];
      s += 0.5f * eps * eps + (a.log_std ? a.log_std[c] : 0.f);
    }
    a.logp[e0 + tid] = -s - (float)(0.5 * NA * 1.8378770664093453);   // ln 2 pi
  }
}

template <typename T>
__global__ __launch_bounds__(WAVE * ACT_WAVES) void k_policy_actor(ActorArgs a) {
  policy_actor_body<T, false>(a, nullptr);
}

// the same launch with the input rows normalised on load: what goes to LDS and to net.input is (x - shift) * scale, clamped
template <typename T>
__global__ __launch_bounds__(WAVE * ACT_WAVES) void k_policy_actor_norm(ActorArgs a, ActorNorm nm) {
  policy_actor_body<T, true>(a, &nm);
}

// ---------------------------------------------------------------------------- generalised advantage estimation
// one lane per env, backwards over the T recorded steps; every access is [t, env]: coalesced across the lanes
template <typename T>
__global__ __launch_bounds__(256) void k_policy_gae(int n, int steps, const T *__restrict__ reward, const T *__restrict__ done,
                                                    const int *__restrict__ timeout, const float *__restrict__ value, float gamma, float lam,
                                                    float *advantage, float *returns) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float adv = 0.f, vnext = value[(size_t)steps * n + e];
  for (int t = steps - 1; t >= 0; t--) {
    const size_t o = (size_t)t * n + e;
    const float v = value[o], nd = 1.f - (float)done[o];
    const float r = (float)reward[o] + gamma * v * (float)timeout[o];
    const float delta = r + gamma * vnext * nd - v;
    adv = delta + gamma * lam * nd * adv;
    advantage[o] = adv;
    returns[o] = adv + v;
    vnext = v;
  }
}

} // namespace tsidb
