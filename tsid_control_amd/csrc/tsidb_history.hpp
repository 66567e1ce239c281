// tsidb_history.hpp - the observation history of the policy environment (include/tsidb.h tsidb_policy_obs_history): the last
// `frames` selections of the env's observation tensors, stacked per env as one row the actor takes as an input block.  No
// reference counterpart: the reference's only controller is TSID on the full state (main.py:113-129).
//
// Layout [N, frames * K], frame-major, oldest frame first: frame h of env e is row[h K .. (h + 1) K), K = the sum of the
// sources' widths.  A ring would store one frame per step instead of moving frames - 1, but its reader would need the frames
// in time order from a fixed address (k_policy_actor's blocks, a captured graph): the shift is in place.
//
// Shape, as the other policy kernels: one wavefront per env, four envs per workgroup, lanes striding over the columns of a
// frame - every load and store of a wavefront is one run of consecutive elements of one frame.  A lane owns (env, column c):
// it walks h upwards and only ever touches row[h K + c], so no lane reads what another writes - no LDS, no barrier, no atomic.
// The rows start wherever frames * K puts them (K = 71 float32: 4-byte aligned), so the accesses are one element per lane.
#pragma once
#include "tsidb_policy.hpp"

namespace tsidb {

constexpr int POL_OBSH_MAXSRC = 4;      // TSIDB_POL_OBSH_MAXSRC
constexpr int POL_OBSH_MAXFRAMES = 32;  // TSIDB_POL_OBSH_MAXFRAMES
constexpr int POL_OBSH_MAXCOLS = 4096;  // TSIDB_POL_OBSH_MAXCOLS: frames * K
constexpr int POL_OBSH_CHUNK = 8;       // frames a lane loads before it stores them

// tsidb_policy_obs_history in the path's arithmetic type, passed by value; K = the sum of src_cols
template <typename T>
struct PolicyObsHistory {
  T *history;
  int frames, n_src, K;
  const T *src[POL_OBSH_MAXSRC];
  int src_ld[POL_OBSH_MAXSRC], src_cols[POL_OBSH_MAXSRC];
};

// after k_reset and the observation kernels.  An env whose done flag is set: every frame = the current selection.  Any other
// env, with push: frame[h] = frame[h + 1], the newest = the current selection; without push: untouched.  The shift loads
// POL_OBSH_CHUNK frames into registers before it stores them one frame down - a load-store loop would wait for every store,
// which the compiler must assume aliases the next load.  Chunk j + 1 loads frames above everything chunk j stored.
// The loop over the sources is unrolled so that the by-value arrays are indexed by constants (no scratch copy of them).
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_obs_history(int n, PolicyObsHistory<T> a, const T *__restrict__ done_rows,
                                                                                  int rows_ld, int push) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  const bool fill = !(done_rows[E * rows_ld + NROW - 1] == T(0));
  if (!fill && !push) return;
  const int K = a.K, last = a.frames - 1;
  T *row = a.history + E * (size_t)(a.frames * K);
  int off = 0;
#pragma unroll
  for (int s = 0; s < POL_OBSH_MAXSRC; s++) {
    if (s < a.n_src) {
      const T *x = a.src[s] + E * (size_t)a.src_ld[s];
      for (int c = lane; c < a.src_cols[s]; c += WAVE) {
        T *col = row + off + c;
        const T now = x[c];
        if (fill) {
          for (int h = 0; h < last; h++) col[h * K] = now;
        } else {
          for (int h0 = 0; h0 < last; h0 += POL_OBSH_CHUNK) {
            T r[POL_OBSH_CHUNK];
#pragma unroll
            for (int j = 0; j < POL_OBSH_CHUNK; j++) r[j] = h0 + j < last ? col[(h0 + j + 1) * K] : T(0);
#pragma unroll
            for (int j = 0; j < POL_OBSH_CHUNK; j++)
              if (h0 + j < last) col[(h0 + j) * K] = r[j];
          }
        }
        col[last * K] = now;
      }
      off += a.src_cols[s];
    }
  }
}

} // namespace tsidb
