// tsidb_api.hip - kernels and the C-ABI of libtsidb.so (include/tsidb.h).  gfx950 only.
#include "../../include/tsidb.h"
#include "tsidb_common.hpp"
#include "tsidb_sim.hpp"
#include "tsidb_tick.hpp"
#include "tsidb_policy.hpp"
#include "tsidb_history.hpp"
#include "tsidb_actor.hpp"
#include "tsidb_learner.hpp"
#include "tsidb_norm.hpp"
#include "tsidb_optim.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace tsidb;

// ============================================================================ kernels
// walking reference update (Walk_Planner.py:23-31 samples -> WalkController.py:189-253): 16 lanes per env (r = 0..15).  Runs
// either as its own kernel (k_walk, tsidb_walk_update) or in the prologue of k_tick (tsidb_tick_walk: one launch less on
// the tick stream, which is what bounds small batches).
template <typename T>
struct WalkArgs {
  const T *coef; const int *side; const int *nsteps; const T *rest; const T *com; int K;
  T t_now; const T *t_off; T Tstep, t_start, omega, z0, dz;
  const T *frames; T *foot_ref; T *contact_ref; uint8_t *cact; T *com_ref;
  const int *ncon; const int *con; int *latch; unsigned long long fgeoms0, fgeoms1; T td_frac; const double *t_dev;
};
template <typename T>
__device__ __forceinline__ void walk_update_env(const WalkArgs<T> &wa, int e, int r) {
  const T *coef = wa.coef, *rest = wa.rest, *com = wa.com, *t_off = wa.t_off, *frames = wa.frames;
  const int *side = wa.side, *nsteps = wa.nsteps, *ncon = wa.ncon, *con = wa.con;
  int *latch = wa.latch;
  T *foot_ref = wa.foot_ref, *contact_ref = wa.contact_ref, *com_ref = wa.com_ref;
  uint8_t *cact = wa.cact;
  const int K = wa.K;
  const T t_now = wa.t_now, Tstep = wa.Tstep, t_start = wa.t_start, omega = wa.omega, z0 = wa.z0, dz = wa.dz, td_frac = wa.td_frac;
  const unsigned long long fgeoms0 = wa.fgeoms0, fgeoms1 = wa.fgeoms1;
  const double *t_dev = wa.t_dev;
  // 16 lanes per env: every lane evaluates the (cheap) polynomials, each writes its share of the rows, so
  // the table reads hit one line per env and the reference rows are written as contiguous runs
  const size_t E = (size_t)e;
  // per-env start delay (de-phased schedules): the env's own clock starts at t_off[e]
  T t = t_dev ? (T)t_dev[0] : t_now; // device clock (always float64: a float32 clock advanced by dt per tick drifts by
                                     // ~one dt over a few thousand ticks): a captured graph replays with the time it finds there
  if (t_off) { t -= t_off[e]; t = t > 0 ? t : T(0); }
  // timeline: [0, t_start) both feet down; step k in [t_start + k T, t_start + (k+1) T); then the final stand
  const int k = t < t_start ? -1 : (int)floor((t - t_start) / Tstep);
  const T s = k < 0 ? t : (t - t_start) - k * Tstep;
  const int ns = nsteps[e];
  const bool walking = k >= 0 && k < ns;
  const int kk = k < 0 ? 0 : k;
  const int kc = kk < (ns > 0 ? ns - 1 : 0) ? kk : (ns > 0 ? ns - 1 : 0);
  const int sd = side[E * K + kc];
  const int kr = kk < ns ? kk : ns;
  // contact-timing feedback (closed loop): if the sim reported the swing foot on the floor in the last part of its
  // swing, the step's touch-down is taken now - the foot counts as a stance foot for the rest of step k (latched per
  // env), so the contact is added at the placement the foot really has
  bool early = false;
  if (latch) {
    const int lk = latch[e];
    early = walking && lk == k;
    if (walking && !early && s > td_frac * Tstep) {
      const unsigned long long fg = sd == 0 ? fgeoms0 : fgeoms1; // the collision geoms of the swing foot's body
      const int nc = ncon[e];
      for (int c = 0; c < nc; c++) {
        const int cp = con[E * MAXCON + c];
        if (((fg >> (cp >> 16)) & 1ull) && !(cp & 0x8000)) early = true;
      }
    }
  }
  const bool act[2] = {cact[E * 2] != 0, cact[E * 2 + 1] != 0}; // read by every lane before lane 0 rewrites them
  const T *c = coef + (E * K + kc) * 16;
  const T pw[4] = {T(1), s, s * s, s * s * s}, d1[4] = {T(0), T(1), 2 * s, 3 * s * s}, d2[4] = {T(0), T(0), T(2), 6 * s};
  T pos[4], vel[4], acc[4];
#pragma unroll
  for (int a = 0; a < 4; a++) {
    pos[a] = vel[a] = acc[a] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { pos[a] += c[4 * a + i] * pw[i]; vel[a] += c[4 * a + i] * d1[i]; acc[a] += c[4 * a + i] * d2[i]; }
  }
#pragma unroll
  for (int f = 0; f < 2; f++) {
    const bool swing = walking && sd == f && !early;
    const T *rs = rest + ((E * (K + 1) + kr) * 2 + f) * 4;
    const T x = swing ? pos[0] : rs[0], y = swing ? pos[1] : rs[1], z = swing ? pos[2] : rs[3], yaw = swing ? pos[3] : rs[2];
    const T cy = cos(yaw), sy = sin(yaw);
    const bool active = act[f];
    const T *fr = frames + E * 24 + 12 * f; // R row-major, p
    T *fo = foot_ref + E * 48 + 24 * f;
    // element i of the tsid SE3 sample (p, R column-major, v6, a6) / of the current placement as an SE3 vector
    auto smp_at = [&](int i) -> T {
      if (i < 3) return i == 0 ? x : (i == 1 ? y : z);
      if (i < 12) {
        const int q = i - 3;
        return q == 0 ? cy : q == 1 ? sy : q == 3 ? -sy : q == 4 ? cy : q == 8 ? T(1) : T(0);
      }
      if (!swing) return T(0);
      const int q = i - 12, a = q < 6 ? q : q - 6;
      const T *src = q < 6 ? vel : acc;
      return a < 3 ? (a == 0 ? src[0] : a == 1 ? src[1] : src[2]) : (a == 5 ? src[3] : T(0));
    };
    auto cur_at = [&](int i) -> T { return i < 3 ? fr[9 + i] : fr[((i - 3) % 3) * 3 + (i - 3) / 3]; };
    if (!swing && !active && r < 12) contact_ref[E * 24 + 12 * f + r] = cur_at(r); // add_contact at the current placement
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int i = r + 16 * h;
      if (i < 24) fo[i] = (swing && active) ? (i < 12 ? cur_at(i) : T(0)) // remove_contact: the foot task restarts here
                                            : smp_at(i);
    }
    if (r == 0) {
      if (!swing && !active) cact[E * 2 + f] = 1;
      if (swing && active) cact[E * 2 + f] = 0;
    }
  }
  if (latch && r == 0 && early) latch[e] = k; // (every lane of the env read the old value above: same wavefront)
  // CoM reference: LIPM segment (zmp, d, c) of the current phase in the plane, quintic descent in height
  if (r < 9) {
    const int ph = k + 1 < ns + 1 ? k + 1 : ns + 1;
    const T sc = (k >= 0 && ph > ns) ? (t - t_start) - ns * Tstep : s;
    const int a = r % 3, d = r / 3; // axis, derivative order
    T val;
    if (a < 2) {
      const T ep = exp(omega * sc), em = exp(-omega * sc);
      const T *sg = com + ((E * (K + 2) + ph) * 2 + a) * 3;
      const T u = T(0.5) * sg[1] * ep + sg[2] * em;
      val = d == 0 ? sg[0] + u : d == 1 ? omega * (T(0.5) * sg[1] * ep - sg[2] * em) : omega * omega * u;
    } else {
      const T q = t_start > 0 ? (t < t_start ? t / t_start : T(1)) : T(1);
      const T sz = q * q * q * (10 - 15 * q + 6 * q * q);
      const T dsz = t_start > 0 ? 30 * q * q * (1 - q) * (1 - q) / t_start : T(0);
      const T ddsz = t_start > 0 ? 60 * q * (1 - q) * (1 - 2 * q) / (t_start * t_start) : T(0);
      val = d == 0 ? z0 - dz * sz : d == 1 ? -dz * dsz : -dz * ddsz;
    }
    com_ref[E * 9 + 3 * d + a] = val;
  }
}

// One launch, three bodies: the tick is compiled for every contact configuration (NS = 2, 1, 0 feet in
// contact: 50 / 38 / 26 variables, every loop bound a compile-time constant) and each workgroup branches
// to the body of its env.  Three separate kernels (tried first) allocate registers a little better, but
// a variant with nothing to do still queues 4096 workgroups that each need the full LDS allocation, and
// in one stream it holds the working variant back behind whatever else occupies the GPU (the sim of
// the previous step): 11.0 M -> 12.9 M env-steps/s from merging them.
// COP: the variant with the CoP force task rows (legacy/biped.py:79-80) compiled in; the reference's
// ctrl/WalkController.py stack (w_cop = 0) runs the variant without them.
#define TSIDB_WPE 2 // wavefronts per SIMD the float64 kernels are register-allocated for (LDS allows 2: DESIGN.md section 5)
template <typename T, bool COP>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(TSIDB_WPE))) void k_tick(const DevModel<T> *__restrict__ mp, int n, T *q, T *v, const T *com_ref,
                                                  const T *posture_ref, const T *foot_ref, const T *contact_ref,
                                                  const uint8_t *cact, const T *cop_frames, T *tau, T *dv, T *f,
                                                  int *status, T *obs, int obs_ld, T *frames, int *info, const T *qpos_sim,
                                                  const T *qvel_sim, const T *cop_ref, WalkArgs<T> wa, T *q_snap, T *v_snap, int fast_eq) {
  __shared__ TickLds<T> L;
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= n) return;
  const int e = env_of_block(blockIdx.x, n);
  const size_t E = (size_t)e;
  if (wa.coef) { // this tick's walking reference update first (tsidb_tick_walk): it rewrites the references read below
    if (lane < 16) walk_update_env<T>(wa, e, lane);
    __syncthreads();
  }
  const int ns = (cact[E * 2] != 0) + (cact[E * 2 + 1] != 0);
  {
    // a non-finite state or reference never enters the solver: the env is flagged HQP_STATUS_ERROR (4) and
    // left untouched (the dual active-set loop's exit tests are comparisons, which NaN makes meaningless)
    const T *qs = qpos_sim ? qpos_sim + E * NQ : q + E * NQ, *vs = qvel_sim ? qvel_sim + E * NV : v + E * NV;
    T chk = 0;
    if (lane < NQ) chk += fabs(qs[lane]);
    if (lane < NV) chk += fabs(vs[lane]);
    if (lane < 9) chk += fabs(com_ref[E * 9 + lane]);
    if (lane < NA) chk += fabs(posture_ref[E * NA + lane]);
    if (lane < 48) chk += fabs(foot_ref[E * 48 + lane]);
    if (lane < 24) chk += fabs(contact_ref[E * 24 + lane]);
    if (__ballot(!(chk <= Eps<T>::inf))) {
      // nothing of an earlier tick is handed on either: tau = dv = f = 0, as after a failed solve (in the closed loop
      // the env's motors go limp instead of being driven by stale torques)
      if (lane < NA) tau[E * NA + lane] = 0;
      if (lane < NV) dv[E * NV + lane] = 0;
      if (lane < 24) f[E * 24 + lane] = 0;
      if (lane == 0) {
        status[e] = 4;
        if (info) { info[E * 4] = 0; info[E * 4 + 1] = 0; }
        if (obs && obs_ld >= NROW) { obs[E * obs_ld + NOBS] = 0; obs[E * obs_ld + NOBS + 1] = 1; }
      }
      if (q_snap && lane < NQ) q_snap[E * NQ + lane] = q[E * NQ + lane]; // (the snapshot is the state as it stands)
      if (v_snap && lane < NV) v_snap[E * NV + lane] = v[E * NV + lane];
      return;
    }
  }
#ifdef TSIDB_ONLY_NS // (diagnostic builds: one body, to read its resource usage alone)
  if (ns != TSIDB_ONLY_NS) return;
#endif
  if (ns == 2) {
    tsid_tick_env<T, 2, COP>(*mp, L, lane, q + E * NQ, v + E * NV, com_ref + E * 9, posture_ref + E * NA, foot_ref + E * 48,
                         contact_ref + E * 24, cact + E * 2, cop_frames ? cop_frames + E * 24 : nullptr, tau + E * NA,
                         dv + E * NV, f + E * 24, status + e, obs ? obs + E * obs_ld : nullptr, (obs && obs_ld >= NROW) ? obs + E * obs_ld + NOBS : nullptr, info ? info + E * 4 : nullptr,
                         qpos_sim ? qpos_sim + E * NQ : nullptr, qvel_sim ? qvel_sim + E * NV : nullptr, cop_ref ? cop_ref + E * 3 : nullptr, fast_eq != 0);
  } else if (ns == 1) {
    tsid_tick_env<T, 1, COP>(*mp, L, lane, q + E * NQ, v + E * NV, com_ref + E * 9, posture_ref + E * NA, foot_ref + E * 48,
                         contact_ref + E * 24, cact + E * 2, cop_frames ? cop_frames + E * 24 : nullptr, tau + E * NA,
                         dv + E * NV, f + E * 24, status + e, obs ? obs + E * obs_ld : nullptr, (obs && obs_ld >= NROW) ? obs + E * obs_ld + NOBS : nullptr, info ? info + E * 4 : nullptr,
                         qpos_sim ? qpos_sim + E * NQ : nullptr, qvel_sim ? qvel_sim + E * NV : nullptr, cop_ref ? cop_ref + E * 3 : nullptr, fast_eq != 0);
  } else {
    tsid_tick_env<T, 0, COP>(*mp, L, lane, q + E * NQ, v + E * NV, com_ref + E * 9, posture_ref + E * NA, foot_ref + E * 48,
                         contact_ref + E * 24, cact + E * 2, cop_frames ? cop_frames + E * 24 : nullptr, tau + E * NA,
                         dv + E * NV, f + E * 24, status + e, obs ? obs + E * obs_ld : nullptr, (obs && obs_ld >= NROW) ? obs + E * obs_ld + NOBS : nullptr, info ? info + E * 4 : nullptr,
                         qpos_sim ? qpos_sim + E * NQ : nullptr, qvel_sim ? qvel_sim + E * NV : nullptr, cop_ref ? cop_ref + E * 3 : nullptr, fast_eq != 0);
  }
  if (frames && lane < 24) frames[E * 24 + lane] = L.oMf[lane / 12][lane % 12];
  // a second copy of the TSID state this tick ends on (what q / v hold now): the sim stage of the pipelined step reads it
  // from there while the next tick already overwrites q / v (two copy kernels per step otherwise)
  if (q_snap && lane < NQ) q_snap[E * NQ + lane] = L.qs[lane];
  if (v_snap && lane < NV) v_snap[E * NV + lane] = L.vs[lane];
}

// NW = wavefronts per env: 1 when the batch fills the GPU, 2 for small batches (tsidb_sim.hpp: sim_step_env).
// B consecutive sim steps per launch (tsidb_sim_batch; the pipelined open-loop step hands over a batch of TSID state snapshots):
// envs do not interact, so each workgroup simply steps its env B times - no launch gaps between the steps, which at small
// batches were 10 % of a step.  B = 1 is the plain tsidb_sim.
// (the snapshots of a batch are slots of one [K, N, NQ] / [K, N, NV] ring: two base pointers and the slot numbers packed four
//  bits each - sixteen separate pointers were 32 SGPRs live across the whole step body)
template <typename T> struct SimRing { const T *q, *v; unsigned long long slots; };
// WPE = wavefronts per SIMD the kernel is register-allocated for.  float64 needs 256 registers for its matrix rows: two.
// float32 (10.6 KB of LDS per env: 15 workgroups per CU by LDS) has a second build for THREE (168 VGPRs, 65 spilled): alone
// that kernel is 5 % slower, but the third slot per SIMD lets the tick kernel of the next step (146 VGPRs) run beside it -
// pipelined 18.9 -> 23.6 M env-steps/s at 4096 walkers, 21.3 -> 24.9 M at 16 384; below ~3000 envs, where a step is one
// wavefront's latency, and in the closed loop (tick and sim back to back) the spills cost 2-9 %, so launch_sim picks it for
// open-loop steps of 3072 envs and more (profiles/r04_f32_wpe3.txt, r04_f32_wpe3_sizes.txt).  Same arithmetic: bit-identical.
// XF = the step reads the external wrenches xfrc (tsidb_set_xfrc); launch_sim selects it only while a buffer is registered,
// so the kernels without it are unchanged (xfrc is then not read).
// RO = the step writes the readouts ro (tsidb_set_sim_readouts; the last step of a batch leaves its values); likewise selected
// only while a buffer is registered (ro, the last argument, is then not read).
// SE = the step writes the site sensors to ro.sens (tsidb_set_sensors), [N, nsite, NSENS]; likewise selected only while a buffer
// is registered, and built together with RO = true only (unregistered readouts are NULL pointers there and store nothing).
// CT = the step takes its actuation from ctrl (tsidb_set_ctrl), [N, NA], in the mode ctrl_mode; likewise selected only while a
// buffer is registered (ctrl and ctrl_mode, the last arguments, are then not read).  Built in two forms: alone, and with RO = true
// and SE = true (registered readouts or sensors beside ctrl select that one: unregistered readouts are NULL pointers, and without
// registered sensors the model's site count is zero and no lane writes a row).
template <typename T, int NW, bool MULTI, int WPE = TSIDB_WPE, bool XF = false, bool RO = false, bool SE = false, bool CT = false>
__global__ __launch_bounds__(WAVE * NW) __attribute__((amdgpu_waves_per_eu(WPE))) void k_sim(const DevModel<T> *__restrict__ mp, int n, int B, SimRing<T> ring, T *qpos, T *qvel,
                                              T *qacc_ws, const T *env_params, const T *terrain, const T *xfrc, const T *motor_tau, T *qacc, int *ncon,
                                              int *con, int *info, SimOut<T> ro, const T *ctrl, int ctrl_mode) {
  __shared__ SimLds<T> L;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  if ((int)blockIdx.x >= n) return;
  const int e = env_of_block(blockIdx.x, n);
  const size_t E = (size_t)e;
  for (int b = 0; b < (MULTI ? B : 1); b++) { // (MULTI = false: one step, no loop in the code at all)
    // (the model pointer is laundered per step: otherwise every load of a model constant in the 1200-line step body is
    //  loop-invariant, gets hoisted in front of the loop and stays live across the whole step - the kernel, at its register
    //  limit already, then spilled a hundred values to scratch and ran 20 % slower)
    const DevModel<T> *mq = mp;
    if constexpr (MULTI) {
      asm volatile("" : "+s"(mq), "+s"(qpos), "+s"(qvel), "+s"(qacc_ws), "+s"(env_params), "+s"(terrain), "+s"(motor_tau) : : "memory");
      asm volatile("" : "+s"(qacc), "+s"(ncon), "+s"(con), "+s"(info) : : "memory");
      if constexpr (XF) asm volatile("" : "+s"(xfrc) : : "memory");
      if constexpr (RO) asm volatile("" : "+s"(ro.con_force), "+s"(ro.con_frame), "+s"(ro.con_pos), "+s"(ro.act_force), "+s"(ro.foot_grf) : : "memory");
      if constexpr (SE) asm volatile("" : "+s"(ro.sens) : : "memory");
      if constexpr (CT) asm volatile("" : "+s"(ctrl) : : "memory");
    }
    SimOut<T> roe{}; // (the env's rows)
    if constexpr (RO) {
      roe.con_force = ro.con_force ? ro.con_force + E * MAXCON * 6 : nullptr;
      roe.con_frame = ro.con_frame ? ro.con_frame + E * MAXCON * 9 : nullptr;
      roe.con_pos = ro.con_pos ? ro.con_pos + E * MAXCON * 4 : nullptr;
      roe.act_force = ro.act_force ? ro.act_force + E * NA : nullptr;
      roe.foot_grf = ro.foot_grf ? ro.foot_grf + E * 12 : nullptr;
      roe.foot_body[0] = ro.foot_body[0]; roe.foot_body[1] = ro.foot_body[1];
    }
    if constexpr (SE) roe.sens = ro.sens + E * NSENS * mq->nsite;
    const size_t slot = (size_t)((ring.slots >> (4 * b)) & 15ull);
    const T *q_tsid = ring.q ? ring.q + slot * (size_t)n * NQ : nullptr, *v_tsid = ring.v ? ring.v + slot * (size_t)n * NV : nullptr;
    bool skip;
    SimIn<T> in{};
    {
      // non-finite sim state / targets, or a sim state that has diverged (sum of |qpos| + |qvel| beyond SIM_STATE_BOUND:
      // the reference's own loop gets there, its teleported sim accumulates velocity until the contact forces explode -
      // and products of such values overflow to inf / NaN inside the step): skip the step, failure bit 4 in info[3]
      // (the values loaded here are the ones the step stages: sim_step_env takes them, it does not read the rows again)
      T chk = 0, big = 0;
      if (lane < NQ) { in.qpos = qpos[E * NQ + lane]; if (q_tsid) in.qt = q_tsid[E * NQ + lane]; }
      if (lane < NV) { in.qvel = qvel[E * NV + lane]; if (v_tsid) in.vt = v_tsid[E * NV + lane]; }
      if (lane < NQ) { big += fabs(in.qpos); chk += q_tsid ? fabs(in.qt) : T(0); }
      if (lane < NV) { big += fabs(in.qvel); chk += fabs(qacc_ws[E * NV + lane]) + (v_tsid ? fabs(in.vt) : T(0)); }
      if (lane < NA && motor_tau) chk += fabs(motor_tau[E * NA + lane]);
      if constexpr (XF) for (int i = lane; i < NB * 6; i += WAVE) chk += fabs(xfrc[E * NB * 6 + i]); // (external wrenches)
      if constexpr (CT) { if (lane < NA) chk += fabs(ctrl[E * NA + lane]); } // (direct actuator control)
      big = wave_sum(big);
      skip = __ballot(!(chk <= Eps<T>::inf)) || !(big <= T(SIM_STATE_BOUND));
      if (skip && wv == 0) {
        if (lane == 0) {
          if (info) { info[E * 4 + 2] = 0; info[E * 4 + 3] = 4; }
          if (ncon) ncon[e] = 0;
        }
        if (con && lane < MAXCON) con[E * MAXCON + lane] = -1;
        if constexpr (RO) sim_readouts_zero(roe, lane);
        if constexpr (SE) sim_sensors_zero(*mq, roe.sens, lane);
      }
    }
    if (!skip)
      sim_step_env<T, NW, XF, RO, SE, CT>(*mq, L, lane, wv, in, q_tsid ? q_tsid + E * NQ : nullptr, v_tsid ? v_tsid + E * NV : nullptr, qpos + E * NQ, qvel + E * NV, qacc_ws + E * NV,
                          env_params ? env_params + E * 8 : nullptr, terrain ? terrain + E * 20 : nullptr, XF ? xfrc + E * NB * 6 : nullptr,
                          motor_tau ? motor_tau + E * NA : nullptr, qacc ? qacc + E * NV : nullptr, ncon ? ncon + e : nullptr, con ? con + E * MAXCON : nullptr,
                          info ? info + E * 4 : nullptr, roe, CT ? ctrl + E * NA : nullptr, ctrl_mode);
    if constexpr (MULTI) __syncthreads(); // both wavefronts; the step's state is written before the next step reads it
  }
}

template <typename T>
__global__ __launch_bounds__(WAVE) void k_rbd(const DevModel<T> *__restrict__ mp, int n, const T *q, const T *v, T *M, T *hb,
                                              T *Jcom, T *Jf, T *oMf, T *com) {
  __shared__ TickLds<T> L;
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= n) return;
  const int e = env_of_block(blockIdx.x, n);
  const size_t E = (size_t)e;
  if (lane < NQ) L.qs[lane] = q[E * NQ + lane];
  if (lane < NV) L.vs[lane] = v[E * NV + lane];
  __syncthreads();
  rbd_terms<T>(*mp, L, lane);
  for (int i = lane; i < NV * NV; i += WAVE) M[E * NV * NV + i] = L.Dyn[(i / NV) * LDD + i % NV];
  if (lane < NV) hb[E * NV + lane] = L.h[lane];
  for (int i = lane; i < 3 * NV; i += WAVE) Jcom[E * 3 * NV + i] = L.k.Jcom[(i / NV) * LDF + i % NV];
  for (int i = lane; i < 12 * NV; i += WAVE) Jf[E * 12 * NV + i] = L.k.Jf[(i / NV) * LDF + i % NV];
  if (lane < 24) oMf[E * 24 + lane] = L.oMf[lane / 12][lane % 12];
  if (lane < 3) com[E * 3 + lane] = L.com[lane];
}

// reset: standing state + references (WalkController.py:22-26,72-79,81,122,151-152,164-165; main.py:57-64)
// done_rows (may be NULL): the [N, rows_ld] rows k_tick writes - only envs whose done flag (column NOBS + 1) is set are reset
// (episode lifecycle on the device: no host round trip between `done` and the restart).  posture_bias (may be NULL, [NA]):
// added to the captured posture reference (a walking workload's bent-knee posture).  frames (may be NULL): receives the
// sole placements, as the host facade copies them after a reset.
template <typename T>
__global__ __launch_bounds__(WAVE) void k_reset(const DevModel<T> *__restrict__ mp, int n, const int *env_ids, int n_ids, T *q,
                                                T *v, T *qpos, T *qvel, T *qacc_ws, T *com_ref, T *posture_ref,
                                                T *foot_ref, T *contact_ref, uint8_t *cact, T *cop_frames, T *cop_ref,
                                                const T *done_rows, int rows_ld, const T *posture_bias, T *frames, T *xfrc, T *ctrl) {
  __shared__ TickLds<T> L;
  const DevModel<T> &m = *mp;
  const int lane = threadIdx.x;
  int e = blockIdx.x;
  if (env_ids) {
    if (e >= n_ids) return;
    e = env_ids[e];
  }
  if (e < 0 || e >= n) return;
  const size_t E = (size_t)e;
  if (done_rows && !(done_rows[E * rows_ld + NOBS + 1] != T(0))) return;
  if (lane < NQ) L.qs[lane] = m.q0[lane];
  if (lane < NV) L.vs[lane] = 0;
  __syncthreads();
  rbd_terms<T>(m, L, lane);
  const T zlf = L.oMf[0][11];
  __syncthreads();
  if (lane == 0) L.qs[2] -= zlf; // WalkController.py:74
  __syncthreads();
  rbd_terms<T>(m, L, lane);
  if (lane < NQ) q[E * NQ + lane] = L.qs[lane];
  if (lane < NV) { v[E * NV + lane] = 0; qvel[E * NV + lane] = 0; qacc_ws[E * NV + lane] = 0; }
  if (lane < NQ) {
    T val = L.qs[lane]; // main.py:64: raw copy (quirks F6a/F6b); joints are all zero in "standing"
    if (m.params[P_QUIRKS] == 0 || m.params[P_CLOSED_LOOP] != 0) {
      if (lane == 3) val = L.qs[6];
      else if (lane > 3 && lane < 7) val = L.qs[lane - 1];
      else if (lane >= 7) val = L.qs[m.mj_ctrl_qidx[lane - 7]];
    }
    qpos[E * NQ + lane] = val;
  }
  if (lane < 24) {
    const int f = lane / 12, i = lane % 12;
    // SE3ToVector layout: p(3), R column-major(9)
    T val = i < 3 ? L.oMf[f][9 + i] : L.oMf[f][3 * ((i - 3) % 3) + (i - 3) / 3];
    contact_ref[E * 24 + lane] = val;
    cop_frames[E * 24 + lane] = L.oMf[f][i];
    if (frames) frames[E * 24 + lane] = L.oMf[f][i];
  }
  if (lane < 48) {
    const int i = lane % 24;
    // foot tasks never get a reference in the reference (quirk F6c): identity placement
    foot_ref[E * 48 + lane] = (i == 3 || i == 7 || i == 11) ? T(1) : T(0);
  }
  if (lane < 9) com_ref[E * 9 + lane] = lane < 3 ? L.com[lane] : T(0);
  if (lane < NA) posture_ref[E * NA + lane] = L.qs[7 + lane] + (posture_bias ? posture_bias[lane] : T(0));
  if (lane < 2) cact[E * 2 + lane] = 1;
  // CoP task reference: between the soles, on the floor
  if (cop_ref && lane < 3) cop_ref[E * 3 + lane] = lane < 2 ? T(0.5) * (L.oMf[0][9 + lane] + L.oMf[1][9 + lane]) : T(0);
  // external wrenches (tsidb_set_xfrc) end with the episode, as mj_resetData clears xfrc_applied
  if (xfrc) for (int i = lane; i < NB * 6; i += WAVE) xfrc[E * NB * 6 + i] = 0;
  // direct actuator control (tsidb_set_ctrl) likewise: mj_resetData clears ctrl
  if (ctrl && lane < NA) ctrl[E * NA + lane] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_walk(int n, WalkArgs<T> wa) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = gid >> 4, r = gid & 15;
  if (e >= n) return;
  walk_update_env<T>(wa, e, r);
}

// ---------------------------------------------------------------------------- episode plan on the device
// One thread per env: everything a walking episode needs from a path - footsteps (ctrl/Footstep_Planner.py:92-125: a step
// every step_length of accumulated path length at pos + t L/2 +- n W/2, yaw along the tangent, closing steps :114-123),
// swing polynomials from footstep k to k + 2 (ctrl/Walk_Planner.py:23-31, ctrl/Foot_Trajectory.py:5-27: x, y, yaw linear,
// z the parabola / cubic through the knots), rest placements, and the CoM plan: DCM end points backwards from the final
// stand, then one LIPM segment (ctrl/LIPM.py:34-49 in closed form) per phase - the tables WalkSchedule.__init__ builds on
// the host, so that a reset with a new path never leaves the GPU.  Arithmetic in float64 whatever the path's type.
__device__ __forceinline__ void plan_poly(int nk, const double *x, const double *f, double *c) { // Newton's divided differences
  double d1[3] = {0, 0, 0}, d2[2] = {0, 0}, d3 = 0;
  for (int i = 0; i + 1 < nk; i++) d1[i] = (f[i + 1] - f[i]) / (x[i + 1] - x[i]);
  for (int i = 0; i + 2 < nk; i++) d2[i] = (d1[i + 1] - d1[i]) / (x[i + 2] - x[i]);
  if (nk == 4) d3 = (d2[1] - d2[0]) / (x[3] - x[0]);
  const double x1 = nk > 2 ? x[1] : 0.0, x2 = nk > 3 ? x[2] : 0.0;
  c[0] = f[0];
  c[1] = d1[0] - d2[0] * x1 + d3 * x1 * x2;
  c[2] = d2[0] - d3 * (x1 + x2);
  c[3] = d3;
}
struct PlanParams { double v[16]; };
template <typename T>
__global__ __launch_bounds__(64) void k_plan(int n, const int *env_ids, int n_ids, const T *done_rows, int rows_ld, PlanParams PP,
                                             const T *cop_frames, const T *com_ref, const double *path, const int *npts, int P,
                                             const double *scale, int *episode, int bump, int K, double *steps, T *coef, int *side,
                                             int *nsteps, T *rest, T *com, int *flags, T *t_offset, int *latch, double t_now,
                                             const double *t_dev) {
  const double *pp = PP.v;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (env_ids) {
    if (e >= n_ids) return;
    e = env_ids[e];
  }
  if (e < 0 || e >= n) return;
  const size_t E = (size_t)e;
  if (done_rows && !(done_rows[E * rows_ld + NOBS + 1] != T(0))) return;
  const double L = pp[0], Tst = pp[3], rise_ratio = pp[4], t_start = pp[5], foot_press = pp[7], ds = pp[8];
  const T *fr = cop_frames + E * 24;
  const double lf[2] = {(double)fr[9], (double)fr[10]}, rf[2] = {(double)fr[21], (double)fr[22]};
  const double com0[3] = {(double)com_ref[E * 9], (double)com_ref[E * 9 + 1], (double)com_ref[E * 9 + 2]};
  const double heading = atan2(-(lf[0] - rf[0]), lf[1] - rf[1]);
  const double ch = cos(heading), sh = sin(heading), mid[2] = {0.5 * (lf[0] + rf[0]), 0.5 * (lf[1] + rf[1])};
  double *st = steps + E * (K + 2) * 4; // x, y, yaw, side per footstep
  int nst = 0, cut = 0;
  auto put = [&](double x, double y, double yaw, int sd) { st[4 * nst] = x; st[4 * nst + 1] = y; st[4 * nst + 2] = yaw; st[4 * nst + 3] = sd; nst++; };
  auto add_step = [&](double dx, double dy, int sd, const double *pos) {
    if (nst >= K + 2) { cut = 1; return; }
    const double nrm = sqrt(dx * dx + dy * dy), tx = dx / nrm, ty = dy / nrm, sign = sd == 0 ? 1.0 : -1.0;
    put(pos[0] + tx * (pp[0] / 2) + (-ty) * (pp[1] / 2 * sign), pos[1] + ty * (pp[0] / 2) + tx * (pp[1] / 2 * sign), atan2(dy, dx), sd);
  };
  put(lf[0], lf[1], heading, 0);
  put(rf[0], rf[1], heading, 1);
  int sd = 1;
  double travelled = 0, dx = 0, dy = 0, prev[2] = {0, 0}, a[2] = {0, 0}, sc = 1.0;
  if (!path) {
    if (episode && bump) episode[e] += 1;
    if (scale) sc = scale[e];
    else if (episode) sc = pp[13] + (pp[14] - pp[13]) * ((double)(plan_hash((unsigned long long)pp[15], (unsigned long long)e, (unsigned long long)episode[e]) >> 11) * (1.0 / 9007199254740992.0));
  }
  int nv = path ? npts[e] : (int)pp[12];
  if (path && nv > P) nv = P; // (never read past the env's row of the path table)
  double ux = 0, uy = 0, uth = 0;
  for (int i = 0; i < nv; i++) {
    double b[2];
    if (path) { b[0] = path[(E * P + i) * 2]; b[1] = path[(E * P + i) * 2 + 1]; }
    else {
      ux += pp[9] * pp[11] * cos(uth); uy += pp[9] * pp[11] * sin(uth); uth += pp[10] * pp[11];
      const double px = ux * sc, py = uy * sc;
      b[0] = (ch * px - sh * py) + mid[0]; b[1] = (sh * px + ch * py) + mid[1];
    }
    if (i == 0) { prev[0] = a[0] = b[0]; prev[1] = a[1] = b[1]; continue; }
    const double seg = sqrt((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]));
    int mres = ds > 0 && seg / ds < 4096.0 ? (int)ceil(seg / ds) : (ds > 0 ? 4096 : 1);
    if (ds > 0 && !(seg / ds < 4096.0)) cut |= 4; // a piece of more than 4096 resample intervals (or a non-finite vertex): resampled coarser, flag bit 4
    if (mres < 1) mres = 1;
    for (int j = 1; j <= mres; j++) {
      const double qf = (double)j / mres, p[2] = {a[0] + (b[0] - a[0]) * qf, a[1] + (b[1] - a[1]) * qf};
      const double ddx = p[0] - prev[0], ddy = p[1] - prev[1];
      if (ddx != 0 || ddy != 0) { dx = ddx; dy = ddy; } // (a repeated vertex keeps the direction of the piece before it)
      travelled += hypot(ddx, ddy);
      if (travelled >= L) { sd = !sd; add_step(dx, dy, sd, prev); travelled = 0; }
      prev[0] = p[0]; prev[1] = p[1];
    }
    a[0] = b[0]; a[1] = b[1];
  }
  // a path without a direction (fewer than two distinct vertices; the reference's planner raises on it) plans no step: the env
  // stands, flag bit 1
  // the LIPM needs a positive CoM height above the feet after the descent (plan() before a reset, or com_drop >= that height,
  // would put NaN into every table): such an env plans no step and stands, flag bit 8
  const bool no_height = !(com0[2] - pp[6] > 1e-3);
  const bool degenerate = !(dx != 0 || dy != 0) || no_height;
  if (no_height) nst = 2;
  if (!degenerate) {
    sd = !sd;
    add_step(dx, dy, sd, prev);
    if (travelled > 0) { sd = !sd; add_step(dx, dy, sd, prev); }
  }
  const int ns = nst - 2;
  nsteps[e] = ns;
  if (flags) flags[e] = cut | (degenerate ? 2 : 0) | (no_height ? 8 : 0);
  for (int k = nst; k < K + 2; k++) st[4 * k] = st[4 * k + 1] = st[4 * k + 2] = st[4 * k + 3] = 0;
  // swing polynomials and rest placements; yaw relative to the initial heading
  double cur[2][4];
  for (int s2 = 0; s2 < 2; s2++) {
    const int f = (int)st[4 * s2 + 3];
    cur[f][0] = st[4 * s2]; cur[f][1] = st[4 * s2 + 1]; cur[f][2] = st[4 * s2 + 2] - heading; cur[f][3] = 0;
  }
  for (int k = 0; k <= K; k++) {
    T *ro = rest + (E * (K + 1) + k) * 8;
    for (int i = 0; i < 8; i++) ro[i] = (T)cur[i / 4][i % 4];
    if (k >= K) break;
    double c[16];
    for (int i = 0; i < 16; i++) c[i] = 0;
    int sw = 0;
    if (k < ns) {
      sw = (int)st[4 * k + 3];
      const double nxt[4] = {st[4 * (k + 2)], st[4 * (k + 2) + 1], st[4 * (k + 2) + 2] - heading, -foot_press};
      const double x2[2] = {0, Tst};
      double f2[2];
      f2[0] = cur[sw][0]; f2[1] = nxt[0]; plan_poly(2, x2, f2, c + 0);
      f2[0] = cur[sw][1]; f2[1] = nxt[1]; plan_poly(2, x2, f2, c + 4);
      f2[0] = cur[sw][2]; f2[1] = nxt[2]; plan_poly(2, x2, f2, c + 12);
      if (rise_ratio != 0.5) {
        const double rise = Tst * rise_ratio, x4[4] = {0, rise, Tst - rise, Tst}, f4[4] = {cur[sw][3], cur[sw][3] + pp[2], nxt[3] + pp[2], nxt[3]};
        plan_poly(4, x4, f4, c + 8);
      } else {
        const double x3[3] = {0, Tst * rise_ratio, Tst}, f3[3] = {cur[sw][3], cur[sw][3] + pp[2], nxt[3]};
        plan_poly(3, x3, f3, c + 8);
      }
      for (int i = 0; i < 4; i++) cur[sw][i] = nxt[i];
    }
    T *co = coef + (E * K + k) * 16;
    for (int i = 0; i < 16; i++) co[i] = (T)c[i];
    side[E * K + k] = sw;
  }
  // CoM plan: DCM end points backwards (kept in the table's d slot), then forwards one LIPM segment per phase
  const double w = sqrt(9.80665 / (no_height ? 1e-3 : com0[2] - pp[6])), ewT = exp(-w * Tst);
  T *cm = com + E * (K + 2) * 6;
  double fin[2] = {com0[0], com0[1]}, xi[2];
  if (ns > 0) { fin[0] = 0.5 * (st[4 * ns] + st[4 * (ns + 1)]); fin[1] = 0.5 * (st[4 * ns + 1] + st[4 * (ns + 1) + 1]); }
  xi[0] = fin[0]; xi[1] = fin[1];
  for (int k = ns - 1; k >= 0; k--) // xi_k waits in the d slot of phase k + 1 for the forward pass (rounded to T there)
    for (int ax = 0; ax < 2; ax++) { const double z = st[4 * (k + 1) + ax]; xi[ax] = z + (xi[ax] - z) * ewT; cm[((k + 1) * 2 + ax) * 3 + 1] = (T)xi[ax]; }
  double x[2] = {com0[0], com0[1]};
  const double ep0 = exp(w * t_start), em0 = exp(-w * t_start), epT = exp(w * Tst), emT = exp(-w * Tst);
  for (int ax = 0; ax < 2; ax++) {
    const double x0k = ns > 0 ? (sizeof(T) == 8 ? (double)cm[(1 * 2 + ax) * 3 + 1] : xi[ax]) : fin[ax];
    const double z = (x0k - x[ax] * ep0) / (1.0 - ep0), d = x[ax] - z, c2 = (x[ax] - z) - 0.5 * d;
    cm[ax * 3] = (T)z; cm[ax * 3 + 1] = (T)d; cm[ax * 3 + 2] = (T)c2;
    x[ax] = z + (0.5 * d * ep0 + c2 * em0);
  }
  auto xi_at = [&](int k0, int ax) { // float32 tables cannot park a float64 DCM end point: run the recursion again from the end
    double vv = fin[ax];
    for (int k = ns - 1; k >= k0; k--) { const double z = st[4 * (k + 1) + ax]; vv = z + (vv - z) * ewT; }
    return vv;
  };
  for (int k = 0; k < ns; k++)
    for (int ax = 0; ax < 2; ax++) {
      T *sg = cm + ((k + 1) * 2 + ax) * 3;
      const double z = st[4 * (k + 1) + ax], d = (sizeof(T) == 8 ? (double)sg[1] : xi_at(k, ax)) - z, c2 = (x[ax] - z) - 0.5 * d;
      sg[0] = (T)z; sg[1] = (T)d; sg[2] = (T)c2;
      x[ax] = z + (0.5 * d * epT + c2 * emT);
    }
  for (int k = ns + 1; k < K + 2; k++)
    for (int ax = 0; ax < 2; ax++) { T *sg = cm + (k * 2 + ax) * 3; sg[0] = (T)fin[ax]; sg[1] = 0; sg[2] = (T)(x[ax] - fin[ax]); }
  // the env's clock restarts: its timeline runs on t - t_offset
  if (t_offset) t_offset[e] = (T)(t_dev ? t_dev[0] : t_now);
  if (latch) latch[e] = -1;
}

// ============================================================================ host side
namespace {

struct Sect {
  char name[24];
  uint32_t dtype, count;
  uint64_t offset;
};

struct Blob {
  std::vector<uint8_t> raw;
  // every section must lie inside the blob (a truncated or corrupt file must not make the host read past it)
  void validate() const {
    const size_t nb = raw.size();
    if (nb < 16) throw std::string("model blob: truncated header");
    uint32_t n;
    memcpy(&n, raw.data() + 8, 4);
    if (n > 4096 || 16 + (size_t)n * sizeof(Sect) > nb) throw std::string("model blob: bad section table");
    const Sect *s = (const Sect *)(raw.data() + 16);
    for (uint32_t i = 0; i < n; i++) {
      const size_t esz = s[i].dtype == 0 ? 8 : 4;
      if (s[i].dtype > 1 || (s[i].offset & 7) || s[i].offset > nb || (size_t)s[i].count * esz > nb - s[i].offset)
        throw std::string("model blob: bad section ") + std::string(s[i].name, strnlen(s[i].name, 24));
    }
  }
  const Sect *find(const char *name) const {
    uint32_t n;
    memcpy(&n, raw.data() + 8, 4);
    const Sect *s = (const Sect *)(raw.data() + 16);
    for (uint32_t i = 0; i < n; i++)
      if (strncmp(s[i].name, name, 24) == 0) return &s[i];
    return nullptr;
  }
  const double *f64(const char *name, uint32_t cnt) const {
    const Sect *s = find(name);
    if (!s || s->dtype != 0 || (cnt && s->count != cnt)) throw std::string("model blob: bad section ") + name;
    return (const double *)(raw.data() + s->offset);
  }
  const int *i32(const char *name, uint32_t cnt) const {
    const Sect *s = find(name);
    if (!s || s->dtype != 1 || (cnt && s->count != cnt)) throw std::string("model blob: bad section ") + name;
    return (const int *)(raw.data() + s->offset);
  }
  uint32_t count(const char *name) const {
    const Sect *s = find(name);
    return s ? s->count : 0;
  }
};

void quat_wxyz_to_R_host(const double *q, double *R) {
  double w = q[0], x = q[1], y = q[2], z = q[3], n = 1.0 / std::sqrt(w * w + x * x + y * y + z * z);
  w *= n; x *= n; y *= n; z *= n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

template <int N>
void tree_tables(const int *parent, int n, int *depth, int *nchild, int (*child)[MAXCHILD], unsigned *anc, int *maxdepth,
                 int *last, int (*up)[N]) {
  // subtree sums are taken as differences of a prefix scan over the lanes, which needs the numbering to be
  // a depth-first pre-order (every subtree a contiguous index range j..last[j]); both pinocchio's joint
  // order and MuJoCo's body order are
  if (n > 32) throw std::string("model blob: more than 32 tree nodes");
  for (int j = 0; j < n; j++) last[j] = j;
  for (int j = n - 1; j > 0; j--) {
    if (parent[j] < 0 || parent[j] >= j) throw std::string("model blob: tree nodes are not numbered parent-first");
    if (last[j] > last[parent[j]]) last[parent[j]] = last[j];
  }
  for (int j = 0; j < n; j++) { // every index in (j, last[j]] must descend from j
    for (int i = j + 1; i <= last[j]; i++) {
      int a = i;
      while (a > j) a = parent[a];
      if (a != j) throw std::string("model blob: tree numbering is not a depth-first pre-order");
    }
  }
  *maxdepth = 0;
  for (int j = 0; j < n; j++) {
    nchild[j] = 0;
    depth[j] = parent[j] < 0 ? 0 : depth[parent[j]] + 1;
    anc[j] = (parent[j] < 0 ? 0u : anc[parent[j]]) | (1u << j);
    if (depth[j] > *maxdepth) *maxdepth = depth[j];
  }
  for (int j = 0; j < n; j++)
    if (parent[j] >= 0) {
      int p = parent[j];
      if (nchild[p] >= MAXCHILD) throw std::string("model blob: too many children per body");
      child[p][nchild[p]++] = j;
    }
  // ancestors 1, 2, 4 levels up for the pointer-jumping forward pass (three rounds cover depth <= 7)
  if (*maxdepth > 7) throw std::string("model blob: kinematic tree deeper than 7 levels");
  for (int j = 0; j < n; j++) up[0][j] = parent[j];
  for (int r = 1; r < 3; r++)
    for (int j = 0; j < n; j++) up[r][j] = up[r - 1][j] < 0 ? -1 : up[r - 1][up[r - 1][j]];
}

// chain[j] = j and its ancestors other than the root, deepest first, -1 padded (tree depth <= 7, checked by tree_tables)
static void chain_table(const int *parent, int n, int (*chain)[8]) {
  for (int j = 0; j < n; j++) {
    int k = 0;
    for (int i = 0; i < 8; i++) chain[j][i] = -1;
    for (int a = j; a > 0 && k < 8; a = parent[a]) chain[j][k++] = a;
  }
}

} // namespace

static_assert(MAXSITE == TSIDB_MAXSITE && NSENS == TSIDB_NSENS, "include/tsidb.h and the kernels agree on the sensor rows");
static_assert((int)CTRL_POSITION == TSIDB_CTRL_POSITION && (int)CTRL_MOTOR == TSIDB_CTRL_MOTOR && (int)CTRL_RESIDUAL == TSIDB_CTRL_RESIDUAL,
              "include/tsidb.h and the kernels agree on the ctrl modes");
static_assert(POL_NT == TSIDB_POL_NT && POL_HIST == TSIDB_POL_HIST && POL_NPRIV == TSIDB_POL_NPRIV && (NA != 20 || POL_NOBS == TSIDB_POL_NOBS),
              "include/tsidb.h and the kernels agree on the policy environment's rows");
static_assert(NORM_SEG == TSIDB_POL_NORM_SEG_ROWS && NORM_SEG % 16 == 0, "include/tsidb.h and the kernels agree on the normaliser's segments");
static_assert(POL_MAXSCAN == TSIDB_POL_MAXSCAN, "include/tsidb.h and the kernels agree on the height scan's size");
static_assert(POL_TEACH_NT == TSIDB_POL_TEACH_NT && (NA != 20 || POL_TEACH_NOBS == TSIDB_POL_TEACH_NOBS),
              "include/tsidb.h and the kernels agree on the teacher's rows");

// Batches up to this many envs default to two wavefronts per env in k_sim and to CU-split streams (tsidb_stream_create):
// measured, DESIGN.md section 5 "Streams"
constexpr int SMALL_BATCH_ENVS = 512;

struct tsidb_ctx {
  int device = 0, dtype = 0, num_envs = 0;
  int sim_waves = 1; // wavefronts per env in k_sim (tsidb_set_option)
  std::vector<hipStream_t> used_streams; // streams this handle has launched model-reading kernels on (tsidb_set_params waits for them)
  bool streams_overflow = false;         // more streams than the table holds: tsidb_set_params waits for the whole device
  void note_stream(hipStream_t s) {
    for (hipStream_t x : used_streams) if (x == s) return;
    if (used_streams.size() < 32) used_streams.push_back(s);
    else streams_overflow = true;
  }
  int qp_fast_eq = 1; // the tick tries the equality-constrained optimum by a PP x PP Cholesky before the QR (TSIDB_OPT_QP_FAST_EQ)
  unsigned lds_pad = 0; // diagnostic: unused dynamic LDS per workgroup of k_tick / k_sim (occupancy experiments)
  int cu_split = -1;    // tsidb_stream_create: tick and sim streams on disjoint halves of the CUs (-1 = up to SMALL_BATCH_ENVS)
  bool cu_split_on() const { return cu_split == 1 || (cu_split < 0 && num_envs <= SMALL_BATCH_ENVS); }
  Blob blob;
  std::vector<double> params;
  void *d_model = nullptr, *d_hull = nullptr, *d_box = nullptr;
  int *d_eadr = nullptr, *d_edge = nullptr;
  const void *com_ref = nullptr, *posture_ref = nullptr, *foot_ref = nullptr, *contact_ref = nullptr, *cop_frames = nullptr;
  const uint8_t *contact_active = nullptr;
  const void *env_params = nullptr, *terrain = nullptr, *cop_ref = nullptr, *posture_bias = nullptr;
  void *xfrc = nullptr; // [N, NB, 6] external body wrenches (tsidb_set_xfrc); k_reset zeroes the reset envs' rows
  void *ctrl = nullptr; // [N, NA] direct actuator control (tsidb_set_ctrl) in the mode ctrl_mode; k_reset zeroes the reset envs' rows
  int ctrl_mode = TSIDB_CTRL_OFF;
  void *ro[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // sim readouts (tsidb_set_sim_readouts): con_force, con_frame, con_pos,
                                                                // act_force, foot_grf
  bool has_readouts() const { return ro[0] || ro[1] || ro[2] || ro[3] || ro[4]; }
  int foot_body[2] = {-1, -1}; // sim bodies that carry the left / right sole frame
  // site sensors (tsidb_set_sensors): the site table as given (orientation as a row-major rotation) and the output buffer
  int n_sites = 0, site_body[TSIDB_MAXSITE] = {};
  double site_pos[TSIDB_MAXSITE][3] = {}, site_R[TSIDB_MAXSITE][9] = {};
  void *sens = nullptr; // [N, n_sites, TSIDB_NSENS]
  unsigned long long foot_geoms[2] = {0, 0}; // bit g: collision geom g is on that body
  // the policy environment (tsidb_policy_config): its parameter vector, the action scale and default pose, the body mask
  bool pol_set = false;
  double pol[TSIDB_POL_NPARAMS] = {}, pol_scale[NA] = {}, pol_def[NA] = {};
  unsigned pol_mask = 0;
  double pol_dr[TSIDB_POL_DR_NPARAMS] = {}; // tsidb_policy_randomize's vector; all 0 = every group off
  bool ter_set = false;                      // tsidb_policy_terrain_config: per-episode terrain and dynamics, the height scan
  double pol_ter[TSIDB_POL_TER_NPARAMS] = {};
  bool teach_set = false;                    // tsidb_policy_teacher_config: the two sigmas and the teacher terms' weights
  double teach[TSIDB_POL_TEACH_NPARAMS] = {};
  bool ep_set = false;                       // tsidb_policy_episode_config: episode statistics, the terrain curriculum
  double pol_ep[TSIDB_POL_EPP_NPARAMS] = {};
  std::vector<const void *> big_lds;         // the kernels whose dynamic LDS limit has been raised above 64 KB (allow_dynamic_lds)
  std::string err;
};

#define HIP_OK(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) throw std::string(#call " failed: ") + hipGetErrorString(e_); \
  } while (0)

// The one branch on the arithmetic type: fn(T()) with T = double for TSIDB_F64, float otherwise
template <typename F>
static auto with_dtype(int dtype, F &&fn) {
  if (dtype == TSIDB_F64) return fn(double());
  return fn(float());
}

template <typename T>
static void build_model(tsidb_ctx *h, DevModel<T> &m) {
  const Blob &b = h->blob;
  memset(&m, 0, sizeof m);
  // ---- TSID side
  memcpy(m.pin_parent, b.i32("pin_parent", NJ), sizeof m.pin_parent);
  tree_tables(m.pin_parent, NJ, m.pin_depth, m.pin_nchild, m.pin_child, m.pin_anc, &m.pin_maxdepth, m.pin_last, m.pin_up);
  chain_table(m.pin_parent, NJ, m.pin_chain);
  const double *pl = b.f64("pin_place", NJ * 12), *in = b.f64("pin_inertia", NJ * 10);
  double mass = 0;
  for (int j = 0; j < NJ; j++) {
    for (int i = 0; i < 12; i++) m.pin_place[j][i] = (T)pl[12 * j + i];
    for (int i = 0; i < 10; i++) m.pin_inertia[j][i] = (T)in[10 * j + i];
    mass += in[10 * j];
  }
  m.mass = (T)mass;
  memcpy(m.frame_parent, b.i32("pin_frame_parent", 2), sizeof m.frame_parent);
  for (int f = 0; f < 2; f++) { // k_tick's Hessian assembly leaves out the frame Jacobians' structural zeros by TSID_FRAME_DOFS
    if (m.frame_parent[f] < 0 || m.frame_parent[f] >= NJ) throw std::string("model blob: contact frame's parent joint out of range");
    unsigned dofs = 0x3Fu;
    for (int j = 1; j < NJ; j++)
      if ((m.pin_anc[m.frame_parent[f]] >> j) & 1u) dofs |= 1u << (5 + j);
    if (dofs != TSID_FRAME_DOFS[f])
      throw std::string("model blob's contact-frame joint chains differ from the topology this library was compiled for "
                        "(regenerate csrc/tsidb_topology.hpp with model_compiler.py and rebuild)");
  }
  const double *fp = b.f64("pin_frame_place", 24), *q0 = b.f64("pin_q0", NQ);
  for (int i = 0; i < 24; i++) m.frame_place[i / 12][i % 12] = (T)fp[i];
  for (int i = 0; i < NQ; i++) m.q0[i] = (T)q0[i];
  // ---- parameters and the constant QP blocks derived from them
  const double *P = h->params.data();
  for (int i = 0; i < P_COUNT; i++) m.params[i] = (T)P[i];
  double Tg[6][12] = {{0}};
  for (int i = 0; i < 4; i++) {
    const double *p = P + P_CPOINTS + 3 * i;
    for (int k = 0; k < 3; k++) Tg[k][3 * i + k] = 1.0;
    Tg[3][3 * i + 1] = -p[2]; Tg[3][3 * i + 2] = p[1];
    Tg[4][3 * i + 0] = p[2];  Tg[4][3 * i + 2] = -p[0];
    Tg[5][3 * i + 0] = -p[1]; Tg[5][3 * i + 1] = p[0];
  }
  for (int i = 0; i < 6; i++) for (int c = 0; c < 12; c++) m.Tgen[i][c] = (T)Tg[i][c];
  { // friction pyramid (Contact6d::updateForceInequalityConstraints)
    const double *n = P + P_NORMAL, mu = P[P_MU];
    auto cr = [](const double *a, const double *c, double *o) {
      o[0] = a[1] * c[2] - a[2] * c[1]; o[1] = a[2] * c[0] - a[0] * c[2]; o[2] = a[0] * c[1] - a[1] * c[0];
    };
    double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}, t1[3], t2[3];
    cr(n, ex, t1);
    if (std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]) < 1e-5) cr(n, ey, t1);
    cr(n, t1, t2);
    double n1 = std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]), n2 = std::sqrt(t2[0] * t2[0] + t2[1] * t2[1] + t2[2] * t2[2]);
    for (int i = 0; i < 3; i++) { t1[i] /= n1; t2[i] /= n2; }
    for (int i = 0; i < 4; i++)
      for (int k = 0; k < 3; k++) {
        m.Bcone[4 * i + 0][3 * i + k] = (T)(-t1[k] - mu * n[k]);
        m.Bcone[4 * i + 1][3 * i + k] = (T)(t1[k] - mu * n[k]);
        m.Bcone[4 * i + 2][3 * i + k] = (T)(-t2[k] - mu * n[k]);
        m.Bcone[4 * i + 3][3 * i + k] = (T)(t2[k] - mu * n[k]);
        m.Bcone[16][3 * i + k] = (T)n[k];
      }
    for (int i = 0; i < 16; i++) { m.cone_lb[i] = (T)-1e10; m.cone_ub[i] = 0; }
    for (int k = 0; k < 3; k++) { m.cop_t[0][k] = (T)t1[k]; m.cop_t[1][k] = (T)t2[k]; }
    m.cone_lb[16] = (T)P[P_FMIN];
    m.cone_ub[16] = (T)P[P_FMAX];
  }
  { // force-regularisation Hessian block: w (W T)^T (W T) + reg I, its Cholesky factor inverse-transposed
    const double wreg[6] = {1, 1, 1e-3, 2, 2, 2};
    double Hf[12][12] = {{0}}, Lf[12][12] = {{0}}, X[12][12] = {{0}};
    for (int a = 0; a < 12; a++)
      for (int c = 0; c < 12; c++) {
        double s = 0;
        for (int i = 0; i < 6; i++) s += wreg[i] * Tg[i][a] * wreg[i] * Tg[i][c];
        Hf[a][c] = P[P_W_FORCEREF] * s + (a == c ? P[P_HESS_REG] : 0.0);
      }
    double tr = 0;
    for (int a = 0; a < 12; a++) tr += Hf[a][a];
    for (int j = 0; j < 12; j++) {
      double s = Hf[j][j];
      for (int k = 0; k < j; k++) s -= Lf[j][k] * Lf[j][k];
      if (!(s > 0)) throw std::string("force-regularisation block is not positive definite");
      Lf[j][j] = std::sqrt(s);
      for (int i = j + 1; i < 12; i++) {
        double t = Hf[i][j];
        for (int k = 0; k < j; k++) t -= Lf[i][k] * Lf[j][k];
        Lf[i][j] = t / Lf[j][j];
      }
    }
    for (int c = 0; c < 12; c++) // X = L^-1 by forward substitution
      for (int i = 0; i < 12; i++) {
        double s = i == c ? 1.0 : 0.0;
        for (int k = 0; k < i; k++) s -= Lf[i][k] * X[k][c];
        X[i][c] = s / Lf[i][i];
      }
    double trJ = 0;
    for (int a = 0; a < 12; a++) {
      for (int c = 0; c < 12; c++) m.Jf0[a][c] = (T)X[c][a]; // L^-T
      trJ += X[a][a];
    }
    m.Hf_trace = (T)tr;
    m.Jf0_trace = (T)trJ;
  }
  // ---- sim side (absent in a TSID-only build)
  if constexpr (!TOPO_HAS_SIM) return;
  memcpy(m.mj_parent, b.i32("mj_parent", NB), sizeof m.mj_parent);
  for (int j = 0; j < NB; j++)
    if (m.mj_parent[j] != TOPO_PARENT[j])
      throw std::string("model blob's sim tree differs from the topology this library was compiled for "
                        "(regenerate csrc/tsidb_topology.hpp with model_compiler.py and rebuild)");
  tree_tables(m.mj_parent, NB, m.mj_depth, m.mj_nchild, m.mj_child, m.mj_anc, &m.mj_maxdepth, m.mj_last, m.mj_up);
  chain_table(m.mj_parent, NB, m.mj_chain);
  const double *mp = b.f64("mj_pos", NB * 3), *mq = b.f64("mj_quat", NB * 4), *mi = b.f64("mj_inertia", NB * 10);
  for (int j = 0; j < NB; j++) {
    double R[9];
    quat_wxyz_to_R_host(mq + 4 * j, R);
    for (int i = 0; i < 9; i++) m.mj_R[j][i] = (T)R[i];
    for (int i = 0; i < 3; i++) m.mj_pos[j][i] = (T)mp[3 * j + i];
    for (int i = 0; i < 10; i++) m.mj_inertia[j][i] = (T)mi[10 * j + i];
  }
  const double *arm = b.f64("mj_armature", NV), *fl = b.f64("mj_frictionloss", NV), *iw = b.f64("mj_dof_invw0", NV);
  const double *bw = b.f64("mj_body_invw0", NB * 2), *M0 = b.f64("mj_dof_M0", NV);
  double mean = 0;
  for (int i = 0; i < NV; i++) {
    m.mj_armature[i] = (T)arm[i]; m.mj_frictionloss[i] = (T)(fl[i] * P[P_SIM_FLOSS_SCALE]); m.mj_dof_invw0[i] = (T)iw[i];
    mean += M0[i];
  }
  m.meaninertia = (T)(mean / NV);
  for (int i = 0; i < NB * 2; i++) m.mj_body_invw0[i / 2][i % 2] = (T)bw[i];
  memcpy(m.mj_act_dof, b.i32("mj_act_dof", NA), sizeof m.mj_act_dof);
  memcpy(m.mj_ctrl_qidx, b.i32("mj_ctrl_qidx", NA), sizeof m.mj_ctrl_qidx);
  for (int a2 = 0; a2 < NA; a2++) m.tsid2sim[m.mj_ctrl_qidx[a2] - 7] = a2;
  const double *kp = b.f64("mj_act_kp", NA), *kv = b.f64("mj_act_kv", NA);
  for (int i = 0; i < NA; i++) { m.mj_act_kp[i] = (T)kp[i]; m.mj_act_kv[i] = (T)kv[i]; }
  memcpy(m.hull_adr, b.i32("mj_hull_adr", NG + 1), sizeof m.hull_adr);
  memcpy(m.geom_body, b.i32("mj_geom_body", NG), sizeof m.geom_body);
  for (int g = 0; g < NG; g++)
    if (m.geom_body[g] < 0 || m.geom_body[g] >= NB || (g > 0 && m.geom_body[g] < m.geom_body[g - 1]))
      throw std::string("model blob: geoms must be listed in body order");
  const double *rb = b.f64("mj_rbound", NG * 4), *op = b.f64("mj_opt", 7), *ct = b.f64("mj_contact", 12);
  for (int i = 0; i < NG * 4; i++) m.rbound[i / 4][i % 4] = (T)rb[i];
  if ((int)ct[8] != CONDIM) throw std::string("model blob: contact dimension differs from this library's");
  const double *dmp = b.f64("mj_damping", NV), *ar = b.f64("mj_act_range", NA * 4);
  bool anyd = false;
  for (int i = 0; i < NV; i++) { m.mj_damping[i] = (T)dmp[i]; anyd |= dmp[i] != 0.0; }
  if (anyd != EULERDAMP) throw std::string("model blob: joint damping differs from what this library was built for");
  for (int i = 0; i < NA * 4; i++) {
    const double lim = sizeof(T) == 8 ? 1e300 : 1e30;
    m.act_range[i / 4][i % 4] = (T)(ar[i] > lim ? lim : (ar[i] < -lim ? -lim : ar[i]));
  }
  for (int i = 0; i < 7; i++) m.opt[i] = (T)op[i];
  m.opt[0] = (T)P[P_DT];                         // main.py:52 mj_model.opt.timestep = conf.dt
  m.opt[6] = sizeof(T) == 8 ? (T)1e-9 : (T)2e-6; // support-vertex tie tolerance
  for (int i = 0; i < 12; i++) m.contact[i] = (T)ct[i];
  const uint32_t nvert = h->blob.count("mj_hull_vert") / 3;
  m.hull_x = (const T *)h->d_hull;
  m.hull_y = m.hull_x + nvert;
  m.hull_z = m.hull_y + nvert;
  {
    const uint32_t np2 = b.count("mj_pairs");
    if (np2 % 2 || np2 / 2 > MAXPAIR) throw std::string("model blob: too many candidate body pairs");
    const int *pp = b.i32("mj_pairs", 0);
    m.npair = (int)(np2 / 2);
    for (int k = 0; k < m.npair; k++) {
      if (pp[2 * k] < 0 || pp[2 * k] >= NG || pp[2 * k + 1] < 0 || pp[2 * k + 1] >= NG) throw std::string("model blob: bad geom pair");
      // (geoms and bodies fit a byte each: NB <= NG <= 64; geom_body was range-checked above)
      m.pair_pk[k] = (unsigned)pp[2 * k] | (unsigned)pp[2 * k + 1] << 8 | (unsigned)m.geom_body[pp[2 * k]] << 16 | (unsigned)m.geom_body[pp[2 * k + 1]] << 24;
    }
    const double *hc = b.f64("mj_hull_center", NG * 3), *hb = b.f64("mj_hull_box", NG * 6);
    for (int i = 0; i < NG * 3; i++) m.hcen[i / 3][i % 3] = (T)hc[i];
    for (int i = 0; i < NG * 6; i++) m.hbox[i / 6][i % 6] = (T)hb[i];
    if (sizeof(T) == 4) for (int j = 0; j < NG; j++) for (int i = 3; i < 6; i++) m.hbox[j][i] = m.hbox[j][i] * (T)1.00001 + (T)1e-7;
  }
  memcpy(m.chunk_adr, b.i32("mj_chunk_adr", NG + 1), sizeof m.chunk_adr);
  m.chunk_box = (const T *)h->d_box;
  m.hull_eadr = h->d_eadr;
  m.hull_edge = h->d_edge;
  m.nsite = h->n_sites;
  for (int s = 0; s < h->n_sites; s++) {
    m.site_body[s] = h->site_body[s];
    for (int i = 0; i < 3; i++) m.site_pos[s][i] = (T)h->site_pos[s][i];
    for (int i = 0; i < 9; i++) m.site_R[s][i] = (T)h->site_R[s][i];
  }
}

// The kernels index the hull arrays with addresses taken from the blob and pack (geom << 16 | vertex) with bit 15 as
// the robot<->robot flag: check every address table against the section it indexes before anything is uploaded
// (Blob::validate only knows section bounds).
static void validate_geometry(const Blob &b) {
  if constexpr (!TOPO_HAS_SIM) return;
  const int *ha = b.i32("mj_hull_adr", NG + 1), *ca = b.i32("mj_chunk_adr", NG + 1);
  const int64_t nvert = b.count("mj_hull_vert") / 3, nchunk = b.count("mj_chunk_box") / 6, nedge = b.count("mj_hull_edge");
  if (b.count("mj_hull_vert") % 3 || b.count("mj_chunk_box") % 6) throw std::string("model blob: hull vertex / chunk box sections are not whole records");
  if (ha[0] != 0 || ha[NG] != nvert || ca[0] != 0 || ca[NG] != nchunk) throw std::string("model blob: hull / chunk address tables do not span their sections");
  for (int g = 0; g < NG; g++) {
    const int64_t nv = (int64_t)ha[g + 1] - ha[g], nc = (int64_t)ca[g + 1] - ca[g];
    if (nv < 1 || nc < 1) throw std::string("model blob: hull or chunk addresses are not increasing");
    if (nv >= 0x8000) throw std::string("model blob: a hull has 32768 or more vertices (contact ids keep the vertex in 15 bits)");
    if (nc > WAVE || nc * WAVE < nv) throw std::string("model blob: a hull's chunks do not cover it (at most 64 chunks of 64 vertices)");
  }
  if ((int64_t)b.count("mj_hull_eadr") != nvert + 1) throw std::string("model blob: hull graph address table has the wrong length");
  const int *ea = b.i32("mj_hull_eadr", 0), *ed = b.i32("mj_hull_edge", 0);
  if (ea[0] != 0 || ea[nvert] > nedge) throw std::string("model blob: hull graph addresses exceed the edge list");
  for (int g = 0; g < NG; g++)
    for (int v = ha[g]; v < ha[g + 1]; v++) {
      if (ea[v + 1] < ea[v]) throw std::string("model blob: hull graph addresses are not increasing");
      for (int e = ea[v]; e < ea[v + 1]; e++)
        if (ed[e] < 0 || ed[e] >= ha[g + 1] - ha[g]) throw std::string("model blob: hull graph edge leaves its hull");
    }
}

template <typename T>
static void upload_model(tsidb_ctx *h) {
  const Blob &b = h->blob;
  if (!h->d_model && !TOPO_HAS_SIM) HIP_OK(hipMalloc(&h->d_model, sizeof(DevModel<T>)));
  if (!h->d_hull && TOPO_HAS_SIM) {
    const uint32_t nvert3 = b.count("mj_hull_vert"), nedge = b.count("mj_hull_edge"), neadr = b.count("mj_hull_eadr");
    const double *hv = b.f64("mj_hull_vert", 0);
    std::vector<T> hvt(nvert3);
    for (uint32_t i = 0; i < nvert3; i++) hvt[(i % 3) * (nvert3 / 3) + i / 3] = (T)hv[i]; // AoS -> SoA
    HIP_OK(hipMalloc(&h->d_hull, nvert3 * sizeof(T)));
    HIP_OK(hipMemcpy(h->d_hull, hvt.data(), nvert3 * sizeof(T), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void **)&h->d_eadr, neadr * sizeof(int)));
    HIP_OK(hipMemcpy(h->d_eadr, b.i32("mj_hull_eadr", 0), neadr * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void **)&h->d_edge, nedge * sizeof(int)));
    HIP_OK(hipMemcpy(h->d_edge, b.i32("mj_hull_edge", 0), nedge * sizeof(int), hipMemcpyHostToDevice));
    const uint32_t nbox6 = b.count("mj_chunk_box");
    const double *bx = b.f64("mj_chunk_box", 0);
    std::vector<T> bxt(nbox6);
    for (uint32_t i = 0; i < nbox6; i++) bxt[i] = (T)bx[i];
    // boxes must bound the vertices AFTER conversion to T: widen the half extents by one rounding step
    if (sizeof(T) == 4) for (uint32_t i = 0; i < nbox6; i++) if (i % 6 >= 3) bxt[i] = bxt[i] * (T)1.00001 + (T)1e-7;
    HIP_OK(hipMalloc(&h->d_box, nbox6 * sizeof(T)));
    HIP_OK(hipMemcpy(h->d_box, bxt.data(), nbox6 * sizeof(T), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&h->d_model, sizeof(DevModel<T>)));
  }
  static thread_local DevModel<T> m;
  build_model<T>(h, m);
  HIP_OK(hipMemcpy(h->d_model, &m, sizeof m, hipMemcpyHostToDevice));
}

#define GUARD_BEGIN                      \
  if (!h) return -1;                     \
  try {                                  \
    HIP_OK(hipSetDevice(h->device));
#define GUARD_END                        \
  }                                      \
  catch (const std::string &s) {         \
    h->err = s;                          \
    return 1;                            \
  }                                      \
  return 0;

// A library built without the sim stage refuses what needs it: true, with the message in h->err for the caller to return or
// throw, if `wanted`.  `who` names the entry point ("tsidb_x: ").
static bool lacks_sim(tsidb_ctx *h, bool wanted, const char *who, const char *advice = "") {
  if (TOPO_HAS_SIM || !wanted) return false;
  h->err = std::string(who) + "this library was built without the sim stage" + advice;
  return true;
}

// Kernels in flight (the pipelined sim stage runs on a side stream) read the model constants: wait for the streams THIS handle
// has launched on before the constants are replaced - not for the whole device (other handles, the caller's own work and
// collectives keep running).  A stream the caller has destroyed since has nothing in flight: its error is dropped.  A handle
// that has launched on more streams than it keeps track of waits for the whole device instead.
static void wait_for_own_streams(tsidb_ctx *h) {
  if (h->streams_overflow) HIP_OK(hipDeviceSynchronize());
  else
    for (hipStream_t st : h->used_streams)
      if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
}

extern "C" int tsidb_set_env_params(tsidb_handle h, const void *env_params, const void *terrain) {
  if (!h) return -1;
  h->env_params = env_params; // NULL restores the nominal model
  h->terrain = terrain;       // NULL = no terrain steps
  return 0;
}

extern "C" int tsidb_set_xfrc(tsidb_handle h, void *xfrc) {
  if (!h) return -1;
  if (lacks_sim(h, xfrc != nullptr, "tsidb_set_xfrc: ")) return 1;
  h->xfrc = xfrc; // NULL = no external wrenches
  return 0;
}

extern "C" int tsidb_set_ctrl(tsidb_handle h, void *ctrl, int mode) {
  GUARD_BEGIN
  if (mode != TSIDB_CTRL_OFF && mode != TSIDB_CTRL_POSITION && mode != TSIDB_CTRL_MOTOR && mode != TSIDB_CTRL_RESIDUAL)
    throw std::string("tsidb_set_ctrl: unknown mode (TSIDB_CTRL_OFF, _POSITION, _MOTOR or _RESIDUAL)");
  if ((ctrl == nullptr) != (mode == TSIDB_CTRL_OFF)) throw std::string("tsidb_set_ctrl: a buffer needs a mode other than TSIDB_CTRL_OFF, and TSIDB_CTRL_OFF a NULL buffer");
  if (lacks_sim(h, ctrl != nullptr, "tsidb_set_ctrl: ")) throw h->err;
  wait_for_own_streams(h); // (a sim stage in flight was launched with the old buffer and mode)
  h->ctrl = ctrl;
  h->ctrl_mode = mode;
  GUARD_END
}

extern "C" int tsidb_set_sim_readouts(tsidb_handle h, void *con_force, void *con_frame, void *con_pos, void *act_force, void *foot_grf) {
  if (!h) return -1;
  void *const p[5] = {con_force, con_frame, con_pos, act_force, foot_grf};
  if (lacks_sim(h, con_force || con_frame || con_pos || act_force || foot_grf, "tsidb_set_sim_readouts: ")) return 1;
  for (int i = 0; i < 5; i++) h->ro[i] = p[i]; // all NULL = no readouts
  return 0;
}

static void need_refs(tsidb_ctx *h) {
  if (!h->com_ref) throw std::string("reference buffers not registered (call tsidb_set_refs first)");
  if (h->params[P_W_COP] != 0.0 && !h->cop_ref) throw std::string("w_cop != 0 needs a CoP reference (tsidb_set_cop_ref)");
}

// tsidb_walk_args (include/tsidb.h) -> the kernel's argument block, with the registered reference buffers
template <typename T>
static WalkArgs<T> walk_args(tsidb_ctx *h, const tsidb_walk_args *a) {
  if (!a->coef || !a->side || !a->nsteps || !a->rest || !a->com || !a->frames || a->K <= 0) throw std::string("walking reference update: null table or K <= 0");
  if (!(a->step_duration > 0) || !(a->omega > 0) || a->t_start < 0) throw std::string("walking reference update: bad timing");
  if (a->td_latch && (!a->ncon || !a->con_pairs)) throw std::string("walking reference update: touch-down feedback needs ncon and con_pairs");
  WalkArgs<T> w;
  w.coef = (const T *)a->coef; w.side = a->side; w.nsteps = a->nsteps; w.rest = (const T *)a->rest; w.com = (const T *)a->com; w.K = a->K;
  w.t_now = (T)a->t; w.t_off = (const T *)a->t_offset; w.Tstep = (T)a->step_duration; w.t_start = (T)a->t_start; w.omega = (T)a->omega;
  w.z0 = (T)a->com_z0; w.dz = (T)a->com_drop; w.frames = (const T *)a->frames; w.foot_ref = (T *)h->foot_ref; w.contact_ref = (T *)h->contact_ref;
  w.cact = (uint8_t *)h->contact_active; w.com_ref = (T *)h->com_ref; w.ncon = a->ncon; w.con = a->con_pairs; w.latch = a->td_latch;
  w.fgeoms0 = h->foot_geoms[0]; w.fgeoms1 = h->foot_geoms[1]; w.td_frac = (T)a->td_fraction; w.t_dev = a->t_device;
  return w;
}

// k_tick instantiation: the CoP force task rows are compiled in only while w_cop != 0
template <typename T>
static auto tick_kernel(const tsidb_ctx *h) {
  return h->params[P_W_COP] != 0.0 ? k_tick<T, true> : k_tick<T, false>;
}

// walk: the walking reference update runs in the tick's prologue (tsidb_tick_walk); q_snap / v_snap: copies of the state it ends on
static void launch_tick(tsidb_ctx *h, void *q, void *v, void *tau, void *dv, void *f, int32_t *status, void *obs, int obs_ld,
                        void *frames, int32_t *info, hipStream_t s, const void *qpos_sim = nullptr, const void *qvel_sim = nullptr,
                        const tsidb_walk_args *walk = nullptr, void *q_snap = nullptr, void *v_snap = nullptr) {
  with_dtype(h->dtype, [&](auto t) {
    using T = decltype(t);
    const WalkArgs<T> wa = walk ? walk_args<T>(h, walk) : WalkArgs<T>{}; // (coef == NULL: no walking update)
    if (obs && obs_ld < NOBS) throw std::string("obs row stride must be at least TSIDB_NOBS");
    h->note_stream(s);
    hipLaunchKernelGGL(tick_kernel<T>(h), dim3(h->num_envs), dim3(WAVE), h->lds_pad, s, (const DevModel<T> *)h->d_model, h->num_envs,
                       (T *)q, (T *)v, (const T *)h->com_ref, (const T *)h->posture_ref, (const T *)h->foot_ref,
                       (const T *)h->contact_ref, h->contact_active, (const T *)h->cop_frames, (T *)tau, (T *)dv, (T *)f,
                       status, (T *)obs, obs_ld, (T *)frames, info, (const T *)qpos_sim, (const T *)qvel_sim, (const T *)h->cop_ref, wa,
                       (T *)q_snap, (T *)v_snap, h->qp_fast_eq);
  });
  HIP_OK(hipGetLastError());
}

// k_sim instantiation for a launch of B steps, with workgroups of WAVE * h->sim_waves lanes and lds_pad bytes of dynamic LDS.
// Two wavefronts per env (collision beside the unconstrained dynamics, bit-identical) shorten the step only while every
// wavefront has a SIMD to itself: 2 N sim wavefronts + N of the tick running beside them on 1024 SIMDs, or 2 N on the
// 512 SIMDs of the sim stream's half when the streams are CU-split (<= 512 envs) - the library picks NW = 2 up to 512
// envs (tsidb_create; k_sim 5-9 % shorter; at 448 / 512 envs it pays since round 4's shorter tick made the sim the longer
// stream there: 7.8 -> 8.0 M env-steps/s).  Beyond that it loses, and the round-4 traces show how
// (profiles/r04_trace_pipeline_*.txt, DESIGN.md section 5 "Streams"): at 1024 envs the 2048 wavefronts of a sim batch
// take every wave slot of the GPU (2 per SIMD) for the whole batch, and the tick launched beside it "runs" 338-526 us
// instead of 58 waiting for a slot; at 512 envs on half the CUs the two wavefronts of an env share SIMDs with their
// neighbours', the sim becomes the slower stream (up to 95 us per step) and the tick stream stalls on the snapshot ring.
// (a registered xfrc buffer selects the XF = true instantiations, registered readouts the RO = true ones; the float32 build for
//  three wavefronts per SIMD has neither, nor sensors, nor ctrl: the default build, bit-identical to it, runs instead; it is also
//  never picked with lds_pad != 0)
template <typename T>
static auto sim_kernel(const tsidb_ctx *h, int B, bool motor_tau) {
  if constexpr (sizeof(T) == 4)
    if (B == 1 && h->sim_waves == 1 && !motor_tau && h->num_envs >= 3072 && !h->lds_pad && !h->xfrc && !h->has_readouts() && !h->sens && !h->ctrl)
      return k_sim<float, 1, false, 3, false, false>;
  // (registered sensors select the SE = true instantiations, which exist with RO = true only: the nearest superset)
  // (a registered ctrl buffer selects the CT = true instantiations: without readouts and sensors, or - the nearest superset while
  //  either is registered - with both)
#define TSIDB_SIM_RO(NW, MULTI, XF) {k_sim<T, NW, MULTI, TSIDB_WPE, XF, false>, k_sim<T, NW, MULTI, TSIDB_WPE, XF, true>, k_sim<T, NW, MULTI, TSIDB_WPE, XF, true, true>, \
                                     k_sim<T, NW, MULTI, TSIDB_WPE, XF, false, false, true>, k_sim<T, NW, MULTI, TSIDB_WPE, XF, true, true, true>}
  const decltype(&k_sim<T, 1, false>) pick[2][2][2][5] = { // [sim_waves == 2][B > 1][xfrc registered][readouts / sensors / ctrl / ctrl + readouts or sensors registered]
      {{TSIDB_SIM_RO(1, false, false), TSIDB_SIM_RO(1, false, true)}, {TSIDB_SIM_RO(1, true, false), TSIDB_SIM_RO(1, true, true)}},
      {{TSIDB_SIM_RO(2, false, false), TSIDB_SIM_RO(2, false, true)}, {TSIDB_SIM_RO(2, true, false), TSIDB_SIM_RO(2, true, true)}}};
#undef TSIDB_SIM_RO
  return pick[h->sim_waves == 2][B > 1][h->xfrc != nullptr][h->ctrl ? (h->sens || h->has_readouts() ? 4 : 3) : h->sens ? 2 : h->has_readouts()];
}

// B sim steps in one launch, step b driven by slot slots[b] of the [K, N, NQ] / [K, N, NV] rings q_ring / v_ring (slot 0 if NULL)
static void launch_sim(tsidb_ctx *h, int B, const void *q_ring, const void *v_ring, const int32_t *slots, void *qpos, void *qvel, void *qacc_ws,
                       void *qacc, int32_t *ncon, int32_t *con, int32_t *info, hipStream_t s, const void *motor_tau = nullptr) {
  if (lacks_sim(h, true, "")) throw h->err;
  if (B < 1 || B > TSIDB_MAX_SIM_BATCH) throw std::string("sim batch must be 1 .. TSIDB_MAX_SIM_BATCH steps");
  h->note_stream(s);
  unsigned long long slot_bits = 0;
  for (int b = 0; b < B; b++) {
    const int sl = slots ? slots[b] : 0;
    if (sl < 0 || sl > 15) throw std::string("sim batch: slot numbers must be 0 .. 15");
    slot_bits |= (unsigned long long)sl << (4 * b);
  }
  with_dtype(h->dtype, [&](auto t) {
    using T = decltype(t);
    if constexpr (TOPO_HAS_SIM) // (a TSID-only build instantiates no k_sim)
      hipLaunchKernelGGL(sim_kernel<T>(h, B, motor_tau != nullptr), dim3(h->num_envs), dim3(WAVE * h->sim_waves), h->lds_pad, s,
                         (const DevModel<T> *)h->d_model, h->num_envs, B, SimRing<T>{(const T *)q_ring, (const T *)v_ring, slot_bits},
                         (T *)qpos, (T *)qvel, (T *)qacc_ws, (const T *)h->env_params, (const T *)h->terrain, (const T *)h->xfrc,
                         (const T *)motor_tau, (T *)qacc, ncon, con, info,
                         SimOut<T>{(T *)h->ro[0], (T *)h->ro[1], (T *)h->ro[2], (T *)h->ro[3], (T *)h->ro[4], {h->foot_body[0], h->foot_body[1]}, (T *)h->sens},
                         (const T *)h->ctrl, h->ctrl_mode);
  });
  HIP_OK(hipGetLastError());
}

static void launch_reset(tsidb_ctx *h, const int32_t *env_ids, int n_ids, void *q, void *v, void *qpos, void *qvel, void *qacc_ws,
                         const void *done_rows, int rows_ld, void *frames, hipStream_t s) {
  const int grid = env_ids ? n_ids : h->num_envs;
  if (grid <= 0) return;
  h->note_stream(s);
  with_dtype(h->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_reset<T>, dim3(grid), dim3(WAVE), 0, s, (const DevModel<T> *)h->d_model, h->num_envs, env_ids, n_ids, (T *)q,
                       (T *)v, (T *)qpos, (T *)qvel, (T *)qacc_ws, (T *)h->com_ref, (T *)h->posture_ref, (T *)h->foot_ref,
                       (T *)h->contact_ref, (uint8_t *)h->contact_active, (T *)h->cop_frames, (T *)h->cop_ref, (const T *)done_rows,
                       rows_ld, (const T *)h->posture_bias, (T *)frames, (T *)h->xfrc, (T *)h->ctrl);
  });
  HIP_OK(hipGetLastError());
}

// ---- the policy environment (tsidb_policy.hpp)
template <typename T>
static PolicyCfg<T> policy_cfg(const tsidb_ctx *h) {
  const double *p = h->pol;
  PolicyCfg<T> c;
  c.clip = (T)p[TSIDB_POL_P_CLIP]; c.alpha = (T)p[TSIDB_POL_P_ALPHA]; c.sigma = (T)p[TSIDB_POL_P_SIGMA]; c.h_target = (T)p[TSIDB_POL_P_H_TARGET];
  c.t_air = (T)p[TSIDB_POL_P_T_AIR]; c.deadband = (T)p[TSIDB_POL_P_DEADBAND]; c.air_dt = (T)(p[TSIDB_POL_P_DECIMATION] * h->params[P_DT]);
  c.done_height = (T)h->params[P_DONE_HEIGHT]; c.done_tilt = (T)h->params[P_DONE_TILT];
  for (int k = 0; k < POL_NT; k++) c.w[k] = (T)p[TSIDB_POL_P_WEIGHTS + k];
  for (int a = 0; a < NA; a++) { c.scale[a] = (T)h->pol_scale[a]; c.def[a] = (T)h->pol_def[a]; }
  for (int i = 0; i < 3; i++) { c.cmd_lo[i] = p[TSIDB_POL_P_CMD_LO + i]; c.cmd_hi[i] = p[TSIDB_POL_P_CMD_HI + i]; }
  c.seed = (unsigned long long)p[TSIDB_POL_P_SEED]; c.foot_geoms[0] = h->foot_geoms[0]; c.foot_geoms[1] = h->foot_geoms[1];
  c.term_mask = h->pol_mask; c.max_steps = (int)p[TSIDB_POL_P_MAX_EPISODE_STEPS]; c.position_mode = h->ctrl_mode == TSIDB_CTRL_POSITION;
  return c;
}

// what every tsidb_policy_* launch needs first; returns the buffers in the path's type
template <typename T>
static PolicyBufs<T> policy_bufs(tsidb_ctx *h, const tsidb_policy_bufs *b, const char *who) {
  if (lacks_sim(h, true, who)) throw h->err;
  if (!h->ctrl) throw std::string(who) + "no ctrl buffer registered (call tsidb_set_ctrl first)";
  if (!h->pol_set) throw std::string(who) + "not configured (call tsidb_policy_config first)";
  if (!b || !b->act_hist || !b->last_action || !b->prev_action || !b->command || !b->air_time || !b->ep_len || !b->episode || !b->terms || !b->timeout)
    throw std::string(who) + "null buffer in tsidb_policy_bufs";
  if (b->obs && b->obs_ld < POL_NOBS + POL_NPRIV) throw std::string(who) + "obs row stride must be at least TSIDB_POL_NOBS + TSIDB_POL_NPRIV";
  return PolicyBufs<T>{(T *)b->act_hist, (T *)b->last_action, (T *)b->prev_action, (T *)b->command, (T *)b->air_time, b->ep_len, b->episode,
                       b->delay, (T *)b->terms, b->timeout, (T *)b->obs, b->obs_ld};
}

static PolicyDR policy_dr(const tsidb_ctx *h) {
  const double *p = h->pol_dr;
  PolicyDR d;
  d.seed = (unsigned long long)p[TSIDB_POL_DR_SEED]; d.env_offset = (unsigned long long)p[TSIDB_POL_DR_ENV_OFFSET];
  d.reset_joint_pos = p[TSIDB_POL_DR_RESET_JOINT_POS]; d.reset_joint_vel = p[TSIDB_POL_DR_RESET_JOINT_VEL];
  for (int i = 0; i < 3; i++) { d.reset_lin[i] = p[TSIDB_POL_DR_RESET_BASE_LIN_VEL + i]; d.reset_ang[i] = p[TSIDB_POL_DR_RESET_BASE_ANG_VEL + i]; }
  d.reset_yaw = p[TSIDB_POL_DR_RESET_YAW]; d.reset_xy = p[TSIDB_POL_DR_RESET_XY]; d.reset_lift = p[TSIDB_POL_DR_RESET_LIFT];
  d.noise_ang_vel = p[TSIDB_POL_DR_NOISE_ANG_VEL]; d.noise_gravity = p[TSIDB_POL_DR_NOISE_GRAVITY];
  d.noise_joint_pos = p[TSIDB_POL_DR_NOISE_JOINT_POS]; d.noise_joint_vel = p[TSIDB_POL_DR_NOISE_JOINT_VEL];
  d.force_lo = p[TSIDB_POL_DR_PUSH_FORCE_LO]; d.force_hi = p[TSIDB_POL_DR_PUSH_FORCE_HI]; d.zero_prob = p[TSIDB_POL_DR_COMMAND_ZERO_PROB];
  d.push_interval = (int)p[TSIDB_POL_DR_PUSH_INTERVAL]; d.push_duration = (int)p[TSIDB_POL_DR_PUSH_DURATION];
  d.command_interval = (int)p[TSIDB_POL_DR_COMMAND_INTERVAL];
  return d;
}
// which groups of the randomisation are on: a launch whose group is entirely off is not made
static bool dr_any(const tsidb_ctx *h, int first, int last) {
  for (int i = first; i <= last; i++) if (h->pol_dr[i] != 0) return true;
  return false;
}
static bool dr_push_on(const tsidb_ctx *h) { return h->pol_dr[TSIDB_POL_DR_PUSH_INTERVAL] >= 1 && h->pol_dr[TSIDB_POL_DR_PUSH_DURATION] >= 1; }
static bool dr_reset_on(const tsidb_ctx *h) { return dr_any(h, TSIDB_POL_DR_RESET_JOINT_POS, TSIDB_POL_DR_RESET_LIFT); }
static bool dr_obs_on(const tsidb_ctx *h) {
  return dr_any(h, TSIDB_POL_DR_NOISE_ANG_VEL, TSIDB_POL_DR_NOISE_JOINT_VEL) || dr_any(h, TSIDB_POL_DR_COMMAND_INTERVAL, TSIDB_POL_DR_COMMAND_ZERO_PROB) ||
         h->pol_dr[TSIDB_POL_DR_ENV_OFFSET] != 0;
}

static PolicyTer policy_ter(const tsidb_ctx *h) {
  const double *p = h->pol_ter;
  PolicyTer d;
  d.seed = (unsigned long long)p[TSIDB_POL_TER_SEED]; d.env_offset = (unsigned long long)p[TSIDB_POL_TER_ENV_OFFSET];
  d.mass_lo = p[TSIDB_POL_TER_MASS_LO]; d.mass_hi = p[TSIDB_POL_TER_MASS_HI]; d.fric_lo = p[TSIDB_POL_TER_FRICTION_LO]; d.fric_hi = p[TSIDB_POL_TER_FRICTION_HI];
  d.tilt_max = p[TSIDB_POL_TER_TILT_MAX]; d.height_lo = p[TSIDB_POL_TER_STEP_HEIGHT_LO]; d.height_hi = p[TSIDB_POL_TER_STEP_HEIGHT_HI];
  d.length_lo = p[TSIDB_POL_TER_STEP_LENGTH_LO]; d.length_hi = p[TSIDB_POL_TER_STEP_LENGTH_HI]; d.step_prob = p[TSIDB_POL_TER_STEP_PROB];
  d.flat_cells = (int)p[TSIDB_POL_TER_FLAT_CELLS]; d.num_levels = (int)p[TSIDB_POL_TER_NUM_LEVELS];
  d.nx = (int)p[TSIDB_POL_TER_SCAN_NX]; d.ny = (int)p[TSIDB_POL_TER_SCAN_NY];
  d.x0 = p[TSIDB_POL_TER_SCAN_X0]; d.x1 = p[TSIDB_POL_TER_SCAN_X1]; d.y0 = p[TSIDB_POL_TER_SCAN_Y0]; d.y1 = p[TSIDB_POL_TER_SCAN_Y1];
  d.clip_lo = p[TSIDB_POL_TER_SCAN_CLIP_LO]; d.clip_hi = p[TSIDB_POL_TER_SCAN_CLIP_HI]; d.noise = p[TSIDB_POL_TER_SCAN_NOISE];
  return d;
}

// what both teacher launches need on top of policy_bufs: the teacher's configuration and the registered references
template <typename T>
static PolicyRefs<T> policy_teacher_refs(const tsidb_ctx *h, const char *who) {
  if (!h->teach_set) throw std::string(who) + "not configured (call tsidb_policy_teacher_config first)";
  if (!h->com_ref || !h->foot_ref || !h->contact_active) throw std::string(who) + "reference buffers not registered (call tsidb_set_refs first)";
  return PolicyRefs<T>{(const T *)h->com_ref, (const T *)h->foot_ref, h->contact_active};
}

static PolicyTeach policy_teach(const tsidb_ctx *h) {
  PolicyTeach tc;
  tc.sigma_com = h->teach[TSIDB_POL_TEACH_SIGMA_COM]; tc.sigma_foot = h->teach[TSIDB_POL_TEACH_SIGMA_FOOT];
  for (int k = 0; k < POL_TEACH_NT; k++) tc.w[k] = h->teach[TSIDB_POL_TEACH_WEIGHTS + k];
  tc.w_termination = h->pol[TSIDB_POL_P_WEIGHTS + POL_T_TERMINATION]; tc.clip = h->pol[TSIDB_POL_P_CLIP];
  for (int a = 0; a < NA; a++) { tc.scale[a] = h->pol_scale[a]; tc.def[a] = h->pol_def[a]; }
  tc.ctrl_mode = h->ctrl_mode;
  return tc;
}

// what both episode launches need on top of policy_bufs: the configuration and the required buffers
template <typename T>
static PolicyEpisode<T> policy_episode(const tsidb_ctx *h, const tsidb_policy_episode *ep, const char *who) {
  if (!h->ep_set) throw std::string(who) + "not configured (call tsidb_policy_episode_config first)";
  if (!ep || !ep->run || !ep->start_xy || !ep->last || !ep->sum) throw std::string(who) + "null buffer in tsidb_policy_episode (run, start_xy, last, sum)";
  return PolicyEpisode<T>{ep->run, ep->start_xy, ep->last, ep->sum, ep->level, (const T *)ep->teacher_terms};
}

// the controller's rows a launch reads (or, the teacher, writes): `what` says which for the message
static void need_rows(const char *who, const void *rows, int ld, const char *what = "tsidb_reset_done read (done flag in column TSIDB_NOBS + 1)") {
  if (!rows || ld < NROW) throw std::string(who) + "needs the [N, >= TSIDB_NROW] rows " + what;
}

// true if every p[i], i in slots, is a whole number in [0, bound)
static bool whole_below(const double *p, std::initializer_list<int> slots, double bound = INFINITY) {
  for (int i : slots) if (!(p[i] >= 0 && p[i] == std::floor(p[i]) && p[i] < bound)) return false;
  return true;
}

// The frame of every entry that launches on the caller's stream: the guard, then body(launch) with the entry's checks.
// launch(kernel, grid, block, lds, args...) notes the stream and puts the kernel on it; a body that returns without calling it
// launches nothing.
template <typename Body>
static int stream_call(tsidb_ctx *h, void *stream, Body body) {
  GUARD_BEGIN
  hipStream_t s = (hipStream_t)stream;
  body([&](auto kernel, dim3 grid, dim3 block, size_t lds, auto... args) {
    h->note_stream(s);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  });
  HIP_OK(hipGetLastError());
  GUARD_END
}

// The frame of every tsidb_policy_* launch over the envs: stream_call's, the path's type T, then body(T(), launch) with
// launch(kernel, args...) on the policy grid and block
template <typename Body>
static int policy_call(tsidb_ctx *h, void *stream, Body body) {
  return stream_call(h, stream, [&](auto launch) {
    with_dtype(h->dtype, [&](auto t) {
      body(t, [&](auto kernel, auto... args) {
        launch(kernel, dim3((h->num_envs + POL_ENVS_PER_BLOCK - 1) / POL_ENVS_PER_BLOCK), dim3(WAVE * POL_ENVS_PER_BLOCK), 0, args...);
      });
    });
  });
}

// ... with what policy_bufs checks first: body(T(), b, launch)
template <typename Body>
static int policy_call(tsidb_ctx *h, const tsidb_policy_bufs *bufs, const char *who, void *stream, Body body) {
  return policy_call(h, stream, [&](auto t, auto launch) { body(t, policy_bufs<decltype(t)>(h, bufs, who), launch); });
}

// The frame of a tsidb_policy_*_config entry: the guard; a library without the sim stage refuses; `params` is N finite numbers
// (`needs`: the message if not; optional: NULL, 0 switches the slice off and stores zeros; negative: the message for a number
// below 0, where none may be); checks(p) with the entry's own; then, behind the handle's kernels in flight, p goes to the
// handle's member dest and its member set (if any) says whether the slice is on.
template <size_t N, typename Checks>
static int store_params(tsidb_ctx *h, const char *who, const double *params, int n, const char *needs, double (tsidb_ctx::*dest)[N],
                        bool tsidb_ctx::*set, bool optional, const char *negative, Checks checks) {
  GUARD_BEGIN
  if (lacks_sim(h, true, who)) throw h->err;
  double p[N] = {};
  const bool on = !optional || params || n;
  if (on) {
    if (!params || n != (int)N) throw std::string(who) + needs;
    for (int i = 0; i < n; i++) {
      if (!std::isfinite(params[i])) throw std::string(who) + "non-finite parameter";
      if (negative && params[i] < 0) throw std::string(who) + negative;
      p[i] = params[i];
    }
    checks(p);
  }
  wait_for_own_streams(h); // (kernels in flight were launched with the old values)
  memcpy(h->*dest, p, sizeof p);
  if (set) h->*set = on;
  GUARD_END
}

extern "C" {

int tsidb_policy_config(tsidb_handle h, const double *pol_params, int n_params, const double *scale, const double *default_pos,
                        uint32_t term_body_mask) {
  const char *who = "tsidb_policy_config: ";
  // (without scale or default_pos the parameters count as missing: one message for the three)
  const int rc = store_params(h, who, scale && default_pos ? pol_params : nullptr, n_params, "needs TSIDB_POL_NPARAMS parameters, scale [NA] and default_pos [NA]",
                              &tsidb_ctx::pol, &tsidb_ctx::pol_set, false, nullptr, [&](const double *p) {
    for (int a = 0; a < NA; a++) if (!std::isfinite(scale[a]) || !std::isfinite(default_pos[a])) throw std::string(who) + "non-finite scale or default position";
    if (p[TSIDB_POL_P_CLIP] < 0) throw std::string(who) + "clip must be >= 0";
    if (!(p[TSIDB_POL_P_ALPHA] > 0 && p[TSIDB_POL_P_ALPHA] <= 1)) throw std::string(who) + "alpha must be in (0, 1]";
    if (!(p[TSIDB_POL_P_SIGMA] > 0)) throw std::string(who) + "sigma must be positive";
    if (p[TSIDB_POL_P_DECIMATION] < 1 || p[TSIDB_POL_P_MAX_EPISODE_STEPS] < 0 || p[TSIDB_POL_P_MAX_EPISODE_STEPS] > 2147483647.0 || p[TSIDB_POL_P_SEED] < 0)
      throw std::string(who) + "decimation must be >= 1, max_episode_steps 0 .. 2^31 - 1, seed >= 0";
    for (int i = 0; i < 3; i++) if (p[TSIDB_POL_P_CMD_LO + i] > p[TSIDB_POL_P_CMD_HI + i]) throw std::string(who) + "command range: lo > hi";
    if (NB < 32 && (term_body_mask >> NB)) throw std::string(who) + "term_body_mask names a body the robot does not have";
  });
  if (rc) return rc;
  memcpy(h->pol_scale, scale, sizeof h->pol_scale);
  memcpy(h->pol_def, default_pos, sizeof h->pol_def);
  h->pol_mask = term_body_mask;
  return 0;
}

int tsidb_policy_act(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *action, void *stream) {
  return policy_call(h, bufs, "tsidb_policy_act: ", stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    if (!action) throw std::string("tsidb_policy_act: null action");
    launch(k_policy_act<T>, h->num_envs, policy_cfg<T>(h), b, (const T *)action, (T *)h->ctrl);
  });
}

int tsidb_policy_reward(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *qpos, const void *qvel, const int32_t *ncon,
                        const int32_t *con_pairs, const int32_t *info, void *reward, void *done, int row_ld, void *stream) {
  return policy_call(h, bufs, "tsidb_policy_reward: ", stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    if (!qpos || !qvel || !ncon || !con_pairs || !info || !reward || !done || row_ld < 1) throw std::string("tsidb_policy_reward: null buffer or row stride < 1");
    launch(k_policy_reward<T>, (const DevModel<T> *)h->d_model, h->num_envs, policy_cfg<T>(h), b, (const T *)qpos, (const T *)qvel, ncon, con_pairs,
           info, (const T *)h->ro[3], (T *)reward, (T *)done, row_ld);
  });
}

int tsidb_policy_obs(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld, const void *qpos,
                     const void *qvel, const int32_t *ncon, const int32_t *con_pairs, void *stream) {
  const char *who = "tsidb_policy_obs: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    need_rows(who, done_rows, rows_ld);
    if (!qpos || !qvel || !ncon || !con_pairs) throw std::string(who) + "null buffer";
    launch(dr_obs_on(h) ? &k_policy_obs<T, true> : &k_policy_obs<T, false>,   // (off: the unrandomised kernel, bit for bit)
           (const DevModel<T> *)h->d_model, h->num_envs, policy_cfg<T>(h), b, (const T *)done_rows, rows_ld, (const T *)qpos, (const T *)qvel, ncon,
           con_pairs, (T *)h->ctrl, policy_dr(h));
  });
}

int tsidb_policy_randomize(tsidb_handle h, const double *dr_params, int n_params) {
  const char *who = "tsidb_policy_randomize: ";
  return store_params(h, who, dr_params, n_params, "needs TSIDB_POL_DR_NPARAMS parameters (or NULL, 0: everything off)", &tsidb_ctx::pol_dr, nullptr, true,
                      "negative parameter (amplitudes, forces, intervals, seed, offset and probability are all >= 0)", [&](const double *p) {
    if (!whole_below(p, {TSIDB_POL_DR_SEED, TSIDB_POL_DR_ENV_OFFSET, TSIDB_POL_DR_PUSH_INTERVAL, TSIDB_POL_DR_PUSH_DURATION, TSIDB_POL_DR_COMMAND_INTERVAL}))
      throw std::string(who) + "seed, env_offset and the intervals must be whole numbers";
    if (!whole_below(p, {TSIDB_POL_DR_SEED}, 4294967296.0)) throw std::string(who) + "seed must be below 2^32";
    if (!whole_below(p, {TSIDB_POL_DR_ENV_OFFSET, TSIDB_POL_DR_PUSH_INTERVAL, TSIDB_POL_DR_COMMAND_INTERVAL}, 2147483648.0))
      throw std::string(who) + "env_offset and the intervals must be below 2^31";
    if (p[TSIDB_POL_DR_PUSH_DURATION] > p[TSIDB_POL_DR_PUSH_INTERVAL]) throw std::string(who) + "push_duration > push_interval";
    if (p[TSIDB_POL_DR_PUSH_FORCE_LO] > p[TSIDB_POL_DR_PUSH_FORCE_HI]) throw std::string(who) + "push_force_lo > push_force_hi";
    if (p[TSIDB_POL_DR_COMMAND_ZERO_PROB] > 1) throw std::string(who) + "command_zero_prob must be in [0, 1]";
  });
}

int tsidb_policy_perturb(tsidb_handle h, const tsidb_policy_bufs *bufs, void *stream) {
  return policy_call(h, bufs, "tsidb_policy_perturb: ", stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    if (!dr_push_on(h)) return;
    if (!h->xfrc) throw std::string("tsidb_policy_perturb: no xfrc buffer registered (call tsidb_set_xfrc first)");
    launch(k_policy_perturb<T>, h->num_envs, b, policy_dr(h), (T *)h->xfrc);
  });
}

int tsidb_policy_reset_noise(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld, void *qpos, void *qvel,
                             void *stream) {
  const char *who = "tsidb_policy_reset_noise: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    need_rows(who, done_rows, rows_ld);
    if (!qpos || !qvel) throw std::string(who) + "null buffer";
    if (!dr_reset_on(h)) return;
    launch(k_policy_reset_noise<T>, (const DevModel<T> *)h->d_model, h->num_envs, b, policy_dr(h), (const T *)done_rows, rows_ld, (T *)qpos, (T *)qvel);
  });
}

int tsidb_policy_terrain_config(tsidb_handle h, const double *ter_params, int n_params) {
  const char *who = "tsidb_policy_terrain_config: ";
  return store_params(h, who, ter_params, n_params, "needs TSIDB_POL_TER_NPARAMS parameters (or NULL, 0: everything off)", &tsidb_ctx::pol_ter,
                      &tsidb_ctx::ter_set, true, nullptr, [&](const double *p) {
    if (!whole_below(p, {TSIDB_POL_TER_SEED, TSIDB_POL_TER_ENV_OFFSET, TSIDB_POL_TER_FLAT_CELLS, TSIDB_POL_TER_NUM_LEVELS, TSIDB_POL_TER_SCAN_NX, TSIDB_POL_TER_SCAN_NY}))
      throw std::string(who) + "seed, env_offset, flat_cells, num_levels, scan_nx and scan_ny must be whole numbers >= 0";
    if (!whole_below(p, {TSIDB_POL_TER_SEED}, 4294967296.0)) throw std::string(who) + "seed must be below 2^32";
    if (!whole_below(p, {TSIDB_POL_TER_ENV_OFFSET}, 2147483648.0)) throw std::string(who) + "env_offset must be below 2^31";
    for (int i : {(int)TSIDB_POL_TER_MASS_LO, (int)TSIDB_POL_TER_FRICTION_LO, (int)TSIDB_POL_TER_STEP_HEIGHT_LO, (int)TSIDB_POL_TER_STEP_LENGTH_LO})
      if (p[i] > p[i + 1]) throw std::string(who) + "range: lo > hi (mass, friction, step_height, step_length)";
    if (!(p[TSIDB_POL_TER_MASS_LO] > 0) || !(p[TSIDB_POL_TER_FRICTION_LO] > 0)) throw std::string(who) + "mass and friction must be positive";
    if (p[TSIDB_POL_TER_TILT_MAX] < 0 || !(p[TSIDB_POL_TER_TILT_MAX] < 0.7853981633974483)) throw std::string(who) + "tilt_max must be in [0, pi/4)";
    if (p[TSIDB_POL_TER_STEP_HEIGHT_LO] < 0) throw std::string(who) + "step heights must be >= 0";
    if (!(p[TSIDB_POL_TER_STEP_LENGTH_LO] > 0)) throw std::string(who) + "step lengths must be positive";
    if (p[TSIDB_POL_TER_STEP_PROB] < 0 || p[TSIDB_POL_TER_STEP_PROB] > 1) throw std::string(who) + "step_prob must be in [0, 1]";
    if (p[TSIDB_POL_TER_FLAT_CELLS] > 7) throw std::string(who) + "flat_cells must be 0 .. 7";
    if (p[TSIDB_POL_TER_NUM_LEVELS] < 1 || p[TSIDB_POL_TER_NUM_LEVELS] >= 2147483648.0) throw std::string(who) + "num_levels must be 1 .. 2^31 - 1";
    const double nx = p[TSIDB_POL_TER_SCAN_NX], ny = p[TSIDB_POL_TER_SCAN_NY];
    if (nx > TSIDB_POL_MAXSCAN || ny > TSIDB_POL_MAXSCAN || nx * ny > TSIDB_POL_MAXSCAN) throw std::string(who) + "scan_nx * scan_ny must be at most TSIDB_POL_MAXSCAN";
    if ((nx == 0) != (ny == 0)) throw std::string(who) + "scan_nx and scan_ny must both be 0 (no scan) or both positive";
    if (p[TSIDB_POL_TER_SCAN_CLIP_LO] > p[TSIDB_POL_TER_SCAN_CLIP_HI]) throw std::string(who) + "scan clip_lo > clip_hi";
    if (p[TSIDB_POL_TER_SCAN_NOISE] < 0) throw std::string(who) + "scan_noise must be >= 0";
  });
}

int tsidb_policy_terrain_reset(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *done_rows, int rows_ld, const void *qpos,
                               const int32_t *level, void *stream) {
  const char *who = "tsidb_policy_terrain_reset: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    if (!h->ter_set) throw std::string(who) + "not configured (call tsidb_policy_terrain_config first)";
    if (!h->env_params || !h->terrain) throw std::string(who) + "needs both the env_params and the terrain table registered (call tsidb_set_env_params first)";
    need_rows(who, done_rows, rows_ld);
    if (!qpos) throw std::string(who) + "null buffer";
    // (the tables are the caller's device buffers, registered read-only for the sim: this launch is their one writer)
    launch(k_policy_terrain_reset<T>, h->num_envs, b, policy_ter(h), (const T *)done_rows, rows_ld, (const T *)qpos, level,
           (T *)const_cast<void *>(h->env_params), (T *)const_cast<void *>(h->terrain));
  });
}

int tsidb_policy_height_scan(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *qpos, void *scan, int scan_ld, void *stream) {
  const char *who = "tsidb_policy_height_scan: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    const PolicyTer d = policy_ter(h);
    if (d.nx * d.ny == 0) return;   // (also before tsidb_policy_terrain_config)
    if (!qpos || !scan) throw std::string(who) + "null buffer";
    if (scan_ld < d.nx * d.ny) throw std::string(who) + "scan row stride must be at least scan_nx * scan_ny";
    launch(k_policy_height_scan<T>, h->num_envs, b, d, (const T *)qpos, (const T *)h->env_params, (const T *)h->terrain, (T *)scan, scan_ld);
  });
}

int tsidb_policy_teacher_config(tsidb_handle h, const double *teach_params, int n_params) {
  const char *who = "tsidb_policy_teacher_config: ";
  return store_params(h, who, teach_params, n_params, "needs TSIDB_POL_TEACH_NPARAMS parameters", &tsidb_ctx::teach, &tsidb_ctx::teach_set, false, nullptr,
                      [&](const double *p) {
    if (!(p[TSIDB_POL_TEACH_SIGMA_COM] > 0) || !(p[TSIDB_POL_TEACH_SIGMA_FOOT] > 0)) throw std::string(who) + "sigma_com and sigma_foot must be positive";
  });
}

int tsidb_policy_teacher(tsidb_handle h, const tsidb_policy_bufs *bufs, void *rows, int rows_ld, const void *q, const void *tau,
                         const int32_t *status, const int32_t *ncon, const int32_t *con_pairs, void *teacher_terms, void *teacher_action,
                         void *stream) {
  const char *who = "tsidb_policy_teacher: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    const PolicyRefs<T> r = policy_teacher_refs<T>(h, who);
    need_rows(who, rows, rows_ld, "of the last tick (reward and done in columns TSIDB_NOBS, TSIDB_NOBS + 1)");
    if (!q || !tau || !status || !ncon || !con_pairs || !teacher_terms || !teacher_action) throw std::string(who) + "null buffer";
    launch(k_policy_teacher<T>, (const DevModel<T> *)h->d_model, h->num_envs, policy_cfg<T>(h), policy_teach(h), b, r, (T *)rows, rows_ld, (const T *)q,
           (const T *)tau, status, ncon, con_pairs, (const T *)h->ctrl, (T *)teacher_terms, (T *)teacher_action);
  });
}

int tsidb_policy_teacher_obs(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *rows, int rows_ld, const void *qpos, const void *tau,
                             void *teacher_obs, int obs_ld, void *stream) {
  const char *who = "tsidb_policy_teacher_obs: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &, auto launch) {
    using T = decltype(t);
    const PolicyRefs<T> r = policy_teacher_refs<T>(h, who);
    need_rows(who, rows, rows_ld);
    if (!qpos || !tau || !teacher_obs) throw std::string(who) + "null buffer";
    if (obs_ld < POL_TEACH_NOBS) throw std::string(who) + "teacher_obs row stride must be at least 14 + NA";
    launch(k_policy_teacher_obs<T>, (const DevModel<T> *)h->d_model, h->num_envs, r, (const T *)rows, rows_ld, (const T *)qpos, (const T *)tau,
           (T *)teacher_obs, obs_ld);
  });
}

int tsidb_policy_teacher_mix(tsidb_handle h, const tsidb_policy_bufs *bufs, const void *teacher_action, void *action, float *label,
                             float *weight, int32_t *executed, const float *beta, uint64_t seed, uint64_t env_offset, void *stream) {
  const char *who = "tsidb_policy_teacher_mix: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    if (!teacher_action || !label || !weight || !executed) throw std::string(who) + "null buffer (teacher_action, label, weight, executed)";
    if (seed >= (1ull << 32) || env_offset >= (1ull << 31)) throw std::string(who) + "seed must be below 2^32 and env_offset below 2^31";
    launch(k_policy_teacher_mix<T>, h->num_envs, b, (const T *)teacher_action, (T *)action, label, weight, executed, beta,
           (unsigned long long)seed, (unsigned long long)env_offset);
  });
}

int tsidb_policy_episode_config(tsidb_handle h, const double *ep_params, int n_params) {
  const char *who = "tsidb_policy_episode_config: ";
  return store_params(h, who, ep_params, n_params, "needs TSIDB_POL_EPP_NPARAMS parameters (or NULL, 0: the slice off)", &tsidb_ctx::pol_ep,
                      &tsidb_ctx::ep_set, true, nullptr, [&](const double *p) {
    for (int i : {(int)TSIDB_POL_EPP_CURRICULUM, (int)TSIDB_POL_EPP_RANDOM_TOP})
      if (p[i] != 0 && p[i] != 1) throw std::string(who) + "curriculum and random_top are flags: 0 or 1";
    if (p[TSIDB_POL_EPP_CURRICULUM] == 1 && !(p[TSIDB_POL_EPP_UP_DISTANCE] > 0)) throw std::string(who) + "up_distance must be positive with the curriculum on";
    if (p[TSIDB_POL_EPP_DOWN_FRACTION] < 0) throw std::string(who) + "down_fraction must be >= 0";
  });
}

int tsidb_policy_episode_end(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_episode *ep, const void *qpos, const void *reward,
                             const void *done, int row_ld, void *stream) {
  const char *who = "tsidb_policy_episode_end: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &b, auto launch) {
    using T = decltype(t);
    const PolicyEpisode<T> pe = policy_episode<T>(h, ep, who);
    if (!qpos || !reward || !done || row_ld < 1) throw std::string(who) + "null buffer or row stride < 1";
    PolicyCur c = {};
    c.curriculum = h->pol_ep[TSIDB_POL_EPP_CURRICULUM] == 1;
    c.num_levels = h->ter_set ? (int)h->pol_ter[TSIDB_POL_TER_NUM_LEVELS] : 0;
    if (c.curriculum) {
      if (!h->ter_set) throw std::string(who) + "the curriculum needs a terrain (call tsidb_policy_terrain_config first: num_levels, seed and env_offset are its)";
      if (!(h->pol[TSIDB_POL_P_MAX_EPISODE_STEPS] > 0)) throw std::string(who) + "the curriculum needs max_episode_steps > 0 (the distance a command asks for is over a whole episode)";
      if (!pe.level) throw std::string(who) + "the curriculum needs the level buffer of tsidb_policy_episode";
      c.seed = (unsigned long long)h->pol_ter[TSIDB_POL_TER_SEED]; c.env_offset = (unsigned long long)h->pol_ter[TSIDB_POL_TER_ENV_OFFSET];
      c.up_distance = h->pol_ep[TSIDB_POL_EPP_UP_DISTANCE]; c.down_fraction = h->pol_ep[TSIDB_POL_EPP_DOWN_FRACTION];
      c.random_top = h->pol_ep[TSIDB_POL_EPP_RANDOM_TOP] == 1;
      c.t_episode = h->pol[TSIDB_POL_P_MAX_EPISODE_STEPS] * (h->pol[TSIDB_POL_P_DECIMATION] * h->params[P_DT]);
    }
    launch(k_policy_episode_end<T>, h->num_envs, b, pe, c, (const T *)qpos, (const T *)reward, (const T *)done, row_ld);
  });
}

int tsidb_policy_episode_begin(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_episode *ep, const void *done_rows, int rows_ld,
                               const void *qpos, void *stream) {
  const char *who = "tsidb_policy_episode_begin: ";
  return policy_call(h, bufs, who, stream, [&](auto t, const auto &, auto launch) {
    using T = decltype(t);
    const PolicyEpisode<T> pe = policy_episode<T>(h, ep, who);
    need_rows(who, done_rows, rows_ld);
    if (!qpos) throw std::string(who) + "null buffer";
    launch(k_policy_episode_begin<T>, h->num_envs, pe, (const T *)done_rows, rows_ld, (const T *)qpos);
  });
}

// (no tsidb_policy_bufs: the sources are whatever the caller names)
int tsidb_policy_obs_history(tsidb_handle h, const struct tsidb_policy_obs_history *hist, const void *done_rows, int rows_ld, int push,
                             void *stream) {
  const char *who = "tsidb_policy_obs_history: ";
  return policy_call(h, stream, [&](auto t, auto launch) {
  static_assert(TSIDB_POL_OBSH_MAXSRC == POL_OBSH_MAXSRC && TSIDB_POL_OBSH_MAXFRAMES == POL_OBSH_MAXFRAMES && TSIDB_POL_OBSH_MAXCOLS == POL_OBSH_MAXCOLS);
  if (!hist || !hist->history) throw std::string(who) + "null struct tsidb_policy_obs_history or history buffer";
  if (hist->frames < 1 || hist->frames > POL_OBSH_MAXFRAMES) throw std::string(who) + "frames must be 1 .. TSIDB_POL_OBSH_MAXFRAMES";
  if (hist->n_src < 1 || hist->n_src > POL_OBSH_MAXSRC) throw std::string(who) + "n_src must be 1 .. TSIDB_POL_OBSH_MAXSRC";
  int K = 0;
  for (int s = 0; s < hist->n_src; s++) {
    if (!hist->src[s]) throw std::string(who) + "null source";
    if (hist->src_cols[s] < 1 || hist->src_cols[s] > POL_OBSH_MAXCOLS || hist->src_ld[s] < hist->src_cols[s])
      throw std::string(who) + "a source needs src_cols >= 1 and src_ld >= src_cols";
    K += hist->src_cols[s];
  }
  if (hist->frames * K > POL_OBSH_MAXCOLS) throw std::string(who) + "frames * K exceeds TSIDB_POL_OBSH_MAXCOLS";
  need_rows(who, done_rows, rows_ld);
  if (push != 0 && push != 1) throw std::string(who) + "push is a flag: 0 or 1";
  using T = decltype(t);
  PolicyObsHistory<T> a = {};
  a.history = (T *)hist->history; a.frames = hist->frames; a.n_src = hist->n_src; a.K = K;
  for (int i = 0; i < hist->n_src; i++) { a.src[i] = (const T *)hist->src[i]; a.src_ld[i] = hist->src_ld[i]; a.src_cols[i] = hist->src_cols[i]; }
  launch(k_policy_obs_history<T>, h->num_envs, a, (const T *)done_rows, rows_ld, push);
  });
}

} // extern "C"

// The checks of a tsidb_policy_net, in the order they fire; pre = "<entry>: <actor | critic>: ".  First the counts (whole =
// false: the block count alone, for an entry that reads nothing else of the struct)
static void net_counts(const tsidb_policy_net *p, const std::string &pre, bool whole = true) {
  if (whole && (p->n_layers < 1 || p->n_layers > ACT_MAXL)) throw pre + "n_layers must be 1 .. 4";
  if (p->n_blocks < 1 || p->n_blocks > ACT_MAXB) throw pre + "n_blocks must be 1 .. 4";
  if (whole && p->activation != ACT_ELU && p->activation != ACT_TANH && p->activation != ACT_RELU)
    throw pre + "unknown activation (TSIDB_POL_ACT_ELU, _TANH or _RELU)";
}

// ... then the input blocks, copied to blk, blk_ld and blk_cols; returns K, the columns in total.  blk = NULL: the column
// counts alone (the learner's rows are the batch's: it reads no block pointer or stride)
static int net_blocks(const tsidb_policy_net *p, const std::string &pre, const void **blk, int *blk_ld, int *blk_cols) {
  long total = 0;
  for (int i = 0; i < p->n_blocks; i++) {
    if (blk && !p->block[i]) throw pre + "null input block";
    if (p->block_cols[i] < 1 || p->block_cols[i] > ACT_MAXW) throw pre + "block_cols must be 1 .. 512";
    if (blk && p->block_ld[i] < p->block_cols[i]) throw pre + "block_ld < block_cols";
    if (blk) { blk[i] = p->block[i]; blk_ld[i] = p->block_ld[i]; }
    blk_cols[i] = p->block_cols[i];
    total += p->block_cols[i];
  }
  if (total < 1 || total > ACT_MAXW) throw pre + "the input blocks must hold 1 .. 512 columns in total";
  return (int)total;
}

// ... then the layers, copied to n; last = the width the last layer must have
static void net_layers(const tsidb_policy_net *p, const std::string &pre, int last, const char *last_name, ActorNet &n) {
  n.n_layers = p->n_layers; n.activation = p->activation;
  for (int l = 0; l < p->n_layers; l++) {
    if (p->width[l] < 1 || p->width[l] > ACT_MAXW) throw pre + "width must be 1 .. 512";
    if (!p->weight[l]) throw pre + "null weight";
    n.width[l] = p->width[l]; n.W[l] = p->weight[l]; n.b[l] = p->bias[l];
  }
  if (p->width[p->n_layers - 1] != last) throw pre + "the last width must be " + last_name;
}

// tsidb_policy_net as the kernel takes it, checked; `name` = "actor" / "critic"
static ActorNet actor_net(const tsidb_policy_net *p, const char *who, const char *name, int last, const char *last_name, float *input) {
  const std::string pre = std::string(who) + name + ": ";
  ActorNet n = {};
  net_counts(p, pre);
  n.n_blocks = p->n_blocks; n.input = input;
  n.K = net_blocks(p, pre, n.blk, n.blk_ld, n.blk_cols);
  net_layers(p, pre, last, last_name, n);
  return n;
}

// the widest row, input or layer, of a call's two networks (an absent one has K = 0 and no layers)
static int widest_of(const ActorNet &a, const ActorNet &b) {
  int widest = 0;
  for (const ActorNet *n : {&a, &b}) {
    if (n->K > widest) widest = n->K;
    for (int l = 0; l < n->n_layers; l++) if (n->width[l] > widest) widest = n->width[l];
  }
  return widest;
}

// Dynamic LDS beyond the default 64 KB (rows wider than 480) has to be allowed per kernel: once per handle and kernel
static void allow_dynamic_lds(tsidb_ctx *h, const void *kernel, size_t lds) {
  if (lds <= 65536 || std::find(h->big_lds.begin(), h->big_lds.end(), kernel) != h->big_lds.end()) return;
  HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)act_lds_bytes(act_ld(ACT_MAXW))));
  h->big_lds.push_back(kernel);
}

// tsidb_policy_actor and tsidb_policy_actor_norm: one body; without a normaliser the launch is k_policy_actor's, as ever
static int policy_actor_call(tsidb_handle h, const char *who, const tsidb_policy_bufs *bufs, const tsidb_policy_net *actor,
                             const tsidb_policy_net *critic, const tsidb_policy_norm *actor_norm, const tsidb_policy_norm *critic_norm,
                             const tsidb_policy_actor_out *out, const void *log_std, uint64_t seed, uint64_t env_offset, int flags,
                             void *stream) {
  return stream_call(h, stream, [&](auto launch) {
  if (!actor && !critic) throw std::string(who) + "null actor (only a call with a critic may leave it out)";
  if (!out) throw std::string(who) + "null out";
  ActorArgs a = {};
  if (actor) a.net[0] = actor_net(actor, who, "actor", NA, "NA", out->actor_input);
  if (critic) a.net[1] = actor_net(critic, who, "critic", 1, "1", out->critic_input);
  if (seed >= (1ull << 32) || env_offset >= (1ull << 31)) throw std::string(who) + "seed must be below 2^32 and env_offset below 2^31";
  a.sample = actor ? flags & TSIDB_POL_ACTOR_SAMPLE : 0;
  a.first = actor ? 0 : 1;
  if (a.sample) {
    if (!bufs || !bufs->episode || !bufs->ep_len) throw std::string(who) + "sampling needs bufs (episode, ep_len)";
    if (!log_std) throw std::string(who) + "sampling needs log_std";
    a.episode = bufs->episode; a.ep_len = bufs->ep_len;
  }
  a.n = h->num_envs; a.LD = act_ld(widest_of(a.net[0], a.net[1]));
  a.action = out->action; a.action32 = out->action32; a.mean = out->mean; a.logp = out->logp; a.value = out->value;
  a.log_std = (const float *)log_std; a.seed = seed; a.env_offset = env_offset;
  ActorNorm nm = {};
  const tsidb_policy_norm *norms[2] = {actor_norm, critic_norm};
  for (int y = 0; y < 2; y++) {
    const tsidb_policy_norm *p = norms[y];
    if (!p) continue;
    if (!(y ? critic : actor)) throw std::string(who) + (y ? "critic_norm without a critic" : "actor_norm without an actor");
    if (!(p->clip >= 0.f)) throw std::string(who) + (y ? "critic" : "actor") + "_norm: clip must be >= 0 (0 = none)";
    nm.affine[y] = p->affine; nm.clip[y] = p->clip;
  }
  const bool normed = nm.affine[0] || nm.affine[1];
  const size_t lds = act_lds_bytes(a.LD);
  const dim3 grid((h->num_envs + ACT_TILE - 1) / ACT_TILE, actor && critic ? 2 : 1), block(WAVE * ACT_WAVES);
  with_dtype(h->dtype, [&](auto t) {
    using T = decltype(t);
    allow_dynamic_lds(h, normed ? (const void *)&k_policy_actor_norm<T> : (const void *)&k_policy_actor<T>, lds);
    if (normed) launch(k_policy_actor_norm<T>, grid, block, lds, a, nm);
    else launch(k_policy_actor<T>, grid, block, lds, a);
  });
  });
}

// the block fields of a network as the normaliser's update takes them: actor_net's checks of them, nothing else of the struct
static NormNet norm_net(const tsidb_policy_net *p, const char *who, const char *name) {
  const std::string pre = std::string(who) + name + ": ";
  NormNet n = {};
  net_counts(p, pre, false);
  n.n_blocks = p->n_blocks;
  n.K = net_blocks(p, pre, n.blk, n.blk_ld, n.blk_cols);
  return n;
}

static int norm_segments(int n) { return (n + NORM_SEG - 1) / NORM_SEG; }

extern "C" {

int tsidb_policy_actor(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                       const tsidb_policy_actor_out *out, const void *log_std, uint64_t seed, uint64_t env_offset, int flags,
                       void *stream) {
  return policy_actor_call(h, "tsidb_policy_actor: ", bufs, actor, critic, nullptr, nullptr, out, log_std, seed, env_offset, flags, stream);
}

int tsidb_policy_actor_norm(tsidb_handle h, const tsidb_policy_bufs *bufs, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                            const tsidb_policy_norm *actor_norm, const tsidb_policy_norm *critic_norm,
                            const tsidb_policy_actor_out *out, const void *log_std, uint64_t seed, uint64_t env_offset, int flags,
                            void *stream) {
  return policy_actor_call(h, "tsidb_policy_actor_norm: ", bufs, actor, critic, actor_norm, critic_norm, out, log_std, seed, env_offset,
                           flags, stream);
}

int tsidb_policy_norm_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, size_t *bytes) {
  GUARD_BEGIN
  const char *who = "tsidb_policy_norm_workspace: ";
  if (!actor && !critic) throw std::string(who) + "null actor and critic";
  if (!bytes) throw std::string(who) + "null bytes";
  size_t cols = 0;
  if (actor) cols += norm_net(actor, who, "actor").K;
  if (critic) cols += norm_net(critic, who, "critic").K;
  *bytes = (size_t)norm_segments(h->num_envs) * 2 * cols * sizeof(double);
  GUARD_END
}

int tsidb_policy_norm_update(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                             const tsidb_policy_norm *actor_norm, const tsidb_policy_norm *critic_norm, void *workspace,
                             size_t workspace_bytes, void *stream) {
  const char *who = "tsidb_policy_norm_update: ";
  return stream_call(h, stream, [&](auto launch) {
  if (!actor && !critic) throw std::string(who) + "null actor and critic";
  NormArgs a = {};
  a.n = h->num_envs; a.nseg = norm_segments(h->num_envs); a.first = actor ? 0 : 1;
  size_t need = 0;
  int widest = 0;
  for (int y = 0; y < 2; y++) {
    const tsidb_policy_net *p = y ? critic : actor;
    const tsidb_policy_norm *q = y ? critic_norm : actor_norm;
    const char *name = y ? "critic" : "actor";
    if (!p) continue;
    NormNet &n = a.net[y];
    n = norm_net(p, who, name);
    if (!q || !q->stats || !q->count || !q->affine) throw std::string(who) + name + ": no normaliser (norm, stats, count, affine)";
    if (!(q->eps > 0.0) || !std::isfinite(q->eps)) throw std::string(who) + name + ": eps must be > 0";
    if (q->until < 0) throw std::string(who) + name + ": until must be >= 0 (0 = no limit)";
    n.stats = q->stats; n.count = (long long *)q->count; n.affine = q->affine; n.eps = q->eps; n.until = q->until;
    n.part = (double *)workspace + need / sizeof(double);
    need += (size_t)a.nseg * 2 * n.K * sizeof(double);
    if (n.K > widest) widest = n.K;
  }
  if (!workspace) throw std::string(who) + "null workspace";
  if (workspace_bytes < need) throw std::string(who) + "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed";
  const int nets = actor && critic ? 2 : 1;
  with_dtype(h->dtype, [&](auto t) { launch(k_policy_norm_partial<decltype(t)>, dim3((widest + 15) / 16, a.nseg, nets), dim3(256), 0, a); });
  launch(k_policy_norm_merge, dim3(1, nets), dim3(NORM_MERGE_LANES), 0, a);
  });
}

int tsidb_policy_gae(tsidb_handle h, int T, const void *reward, const void *done, const int32_t *timeout, const float *value,
                     float gamma, float lam, float *advantage, float *returns, void *stream) {
  const char *who = "tsidb_policy_gae: ";
  return stream_call(h, stream, [&](auto launch) {
    if (T < 1) throw std::string(who) + "T must be >= 1";
    if (!reward || !done || !timeout || !value || !advantage || !returns) throw std::string(who) + "null buffer";
    with_dtype(h->dtype, [&](auto t) {
      using F = decltype(t);
      launch(k_policy_gae<F>, dim3((h->num_envs + 255) / 256), dim3(256), 0, h->num_envs, T, (const F *)reward, (const F *)done, timeout, value, gamma,
             lam, advantage, returns);
    });
  });
}

} // extern "C"

// tsidb_policy_net as the learner takes it: the actor's checks apart from the block pointers and strides; the input rows are
// the batch's
static LearnNet learn_net(const tsidb_policy_net *p, const char *who, const char *name, int last, const char *last_name) {
  const std::string pre = std::string(who) + name + ": ";
  LearnNet n = {};
  net_counts(p, pre);
  n.net.K = net_blocks(p, pre, nullptr, nullptr, n.net.blk_cols);
  net_layers(p, pre, last, last_name, n.net);
  return n;
}

// both networks of a training call (no critic: net.n_layers = 0)
static std::array<LearnNet, 2> learn_nets(const tsidb_policy_net *actor, const tsidb_policy_net *critic, const char *who) {
  return {learn_net(actor, who, "actor", NA, "NA"), critic ? learn_net(critic, who, "critic", 1, "1") : LearnNet{}};
}

// The walk over (actor | critic) x layer of a training call's gradient pointers, checked: fn(W, dW, b, db), b and db NULL for a
// layer without bias
template <typename F>
static void each_layer_grad(const char *who, const tsidb_policy_net *actor, const tsidb_policy_net *critic, const tsidb_policy_grads *actor_grads,
                            const tsidb_policy_grads *critic_grads, const LearnNet *nets, F fn) {
  for (int y = 0; y < 2; y++) {
    const tsidb_policy_net *p = y ? critic : actor;
    const tsidb_policy_grads *gr = y ? critic_grads : actor_grads;
    for (int l = 0; l < nets[y].net.n_layers; l++) {
      if (!gr->weight[l]) throw std::string(who) + (y ? "critic" : "actor") + ": null weight gradient";
      if (p->bias[l] && !gr->bias[l]) throw std::string(who) + (y ? "critic" : "actor") + ": null bias gradient where the bias exists";
      fn(p->weight[l], gr->weight[l], p->bias[l], p->bias[l] ? gr->bias[l] : nullptr);
    }
  }
}

// The workspace of a call, in floats: mu [Mp, NA], v [Mp]; per network the gathered rows, the hidden H_l and every G_l; the
// per-row pieces; the segments' partial sums.  Fills the offsets of the three launches where they are given.  nr: the per-row
// pieces of a row, LRN_NR, or LRN_NR + LRN_NI for the imitation variant.
static size_t learn_layout(LearnNet *nets, int M, WgradArgs *w, ReduceArgs *r, size_t *r_off, int nr = LRN_NR) {
  const size_t Mp = (size_t)((M + ACT_TILE - 1) / ACT_TILE) * ACT_TILE;
  const int nseg = (int)((Mp + LRN_SEG - 1) / LRN_SEG);
  size_t off = 0, p = 0;
  int blk = 0, nj = 0, np = 0;
  for (int y = 0; y < 2; y++) {                      // the outputs first, where the caller may look
    const ActorNet &n = nets[y].net;
    if (n.n_layers) nets[y].h[n.n_layers - 1] = off;
    off += Mp * (y == 0 ? NA : 1);
  }
  for (int y = 0; y < 2; y++) {
    LearnNet &ln = nets[y];
    const ActorNet &n = ln.net;
    if (!n.n_layers) continue;
    ln.x = off; off += Mp * n.K;
    for (int l = 0; l + 1 < n.n_layers; l++) { ln.h[l] = off; off += Mp * n.width[l]; }
    for (int l = 0; l < n.n_layers; l++) { ln.g[l] = off; off += Mp * n.width[l]; }
    for (int l = 0; l < n.n_layers; l++) {
      const int fan = l ? n.width[l - 1] : n.K, kext = fan + 1;
      if (w) {
        WgradJob &j = w->job[nj++];
        j.g = ln.g[l]; j.h = l ? ln.h[l - 1] : ln.x; j.p = p; j.gw = n.width[l]; j.hw = fan; j.ones = 0;
        j.nkg = ((kext + 15) / 16 + LRN_KGROUP - 1) / LRN_KGROUP; j.blk0 = blk;
        blk += ((n.width[l] + 15) / 16) * j.nkg;
      }
      if (r) { ReducePiece &pc = r->piece[np++]; pc.p = p; pc.width = n.width[l]; pc.kext = kext; }
      p += (size_t)n.width[l] * kext;
    }
  }
  const size_t rows_off = off;
  off += Mp * nr;
  if (r_off) *r_off = rows_off;
  if (w) {
    WgradJob &j = w->job[nj++];
    j.g = 0; j.h = rows_off; j.p = p; j.gw = 1; j.hw = nr; j.ones = 1;
    j.nkg = ((nr + 1 + 15) / 16 + LRN_KGROUP - 1) / LRN_KGROUP; j.blk0 = blk;
    blk += j.nkg;
    w->njobs = nj; w->Mp = (int)Mp; w->part = off; w->total = p + nr + 1;
  }
  if (r) { r->npieces = np; r->nseg = nseg; r->M = M; r->part = off; r->total = p + nr + 1; r->rp = p; }
  off += (size_t)nseg * (p + nr + 1);
  return off;
}

static int learn_blocks(const WgradArgs &w) {
  const WgradJob &j = w.job[w.njobs - 1];
  return j.blk0 + ((j.gw + 15) / 16) * j.nkg;
}

// The rows of the symmetry variant's per-row arrays: the originals' Mp, then as many for their mirrors
static int learn_sym_rows(int M) { return 2 * ((M + ACT_TILE - 1) / ACT_TILE) * ACT_TILE; }

// tsidb_policy_learn_workspace, tsidb_policy_learn_imit_workspace and tsidb_policy_learn_sym_workspace: one body
static int learn_workspace_call(tsidb_handle h, const char *who, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes,
                                int nr, bool sym = false) {
  GUARD_BEGIN
  if (!actor) throw std::string(who) + "null actor";
  if (!bytes) throw std::string(who) + "null bytes";
  if (M < 1) throw std::string(who) + "M must be >= 1";
  if (sym && M > (1 << 29)) throw std::string(who) + "M is too large";
  auto nets = learn_nets(actor, critic, who);
  *bytes = learn_layout(nets.data(), sym ? learn_sym_rows(M) : M, nullptr, nullptr, nullptr, nr) * sizeof(float);
  GUARD_END
}

// tsidb_policy_learn, tsidb_policy_learn_imit and tsidb_policy_learn_sym: one body; without imit and sym the launches are the
// three kernels' as ever
static int learn_call(tsidb_handle h, const char *who, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                      const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads, const tsidb_policy_grads *critic_grads,
                      const float *log_std, float *log_std_grad, const tsidb_policy_learn_cfg *cfg, const tsidb_policy_imit *imit,
                      float *workspace, size_t workspace_bytes, float *stats, void *stream, const tsidb_policy_symmetry *sym = nullptr) {
  return stream_call(h, stream, [&](auto launch) {
  if (!actor) throw std::string(who) + "null actor";
  if (!batch) throw std::string(who) + "null batch";
  if (!actor_grads) throw std::string(who) + "null actor_grads";
  if (critic && !critic_grads) throw std::string(who) + "null critic_grads";
  if (!cfg) throw std::string(who) + "null cfg";
  if (!log_std || !log_std_grad) throw std::string(who) + "null log_std or log_std_grad";
  if (!stats) throw std::string(who) + "null stats";
  if (!workspace) throw std::string(who) + "null workspace";
  if (!batch->index) throw std::string(who) + "null index";
  if (batch->M < 1) throw std::string(who) + "M must be >= 1";
  if (batch->rows < 1) throw std::string(who) + "rows must be >= 1";
  if (!(cfg->clip > 0.f)) throw std::string(who) + "clip must be > 0";
  if (!batch->actor_input || !batch->action || !batch->logp || !batch->advantage)
    throw std::string(who) + "null stored array (actor_input, action, logp, advantage)";
  if (critic && (!batch->critic_input || !batch->value || !batch->returns))
    throw std::string(who) + "a critic needs critic_input, value and returns";
  if (imit) {
    const float coefs[] = {imit->imitation_coef, imit->surrogate_coef, cfg->value_coef, cfg->entropy_coef};
    for (float c : coefs) if (!(c >= 0.f) || !std::isfinite(c)) throw std::string(who) + "a coefficient is negative or not finite";
    if (imit->imitation_coef > 0.f && !imit->target) throw std::string(who) + "imitation_coef > 0 needs target";
    if (!imit->stats) throw std::string(who) + "null imit stats";
    if (imit->loss != TSIDB_POL_IMIT_MSE && imit->loss != TSIDB_POL_IMIT_HUBER) throw std::string(who) + "unknown loss (TSIDB_POL_IMIT_MSE or _HUBER)";
  }
  if (sym) {
    if (!sym->actor_perm || !sym->actor_sign || !sym->action_perm || !sym->action_sign) throw std::string(who) + "null actor or action table";
    if (critic && (!sym->critic_perm || !sym->critic_sign)) throw std::string(who) + "a critic needs critic_perm and critic_sign";
    if (!(sym->mirror_coef >= 0.f) || !std::isfinite(sym->mirror_coef)) throw std::string(who) + "mirror_coef is negative or not finite";
    if (!sym->stats) throw std::string(who) + "null sym stats";
    if (batch->M > (1 << 29)) throw std::string(who) + "M is too large";
  }
  const int nr = imit ? LRN_NR + LRN_NI : sym ? LRN_NR + LRN_NS : LRN_NR;
  LearnArgs a = {};
  const auto nets = learn_nets(actor, critic, who);
  a.net[0] = nets[0]; a.net[1] = nets[1];
  WgradArgs w = {};
  ReduceArgs r = {};
  const size_t need = learn_layout(a.net, sym ? learn_sym_rows(batch->M) : batch->M, &w, &r, &a.r, nr) * sizeof(float);
  if (workspace_bytes < need) throw std::string(who) + "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed";
  int np = 0;
  each_layer_grad(who, actor, critic, actor_grads, critic_grads, a.net, [&](const float *, float *dW, const float *, float *db) {
    r.piece[np].dW = dW; r.piece[np++].db = db;
  });
  a.net[0].in = batch->actor_input; a.net[1].in = batch->critic_input;
  a.M = batch->M; a.rows = batch->rows; a.LD = act_ld(widest_of(a.net[0].net, a.net[1].net)); a.value_clip = cfg->value_clip;
  a.index = batch->index; a.action = batch->action; a.logp = batch->logp; a.value = batch->value; a.advantage = batch->advantage;
  a.returns = batch->returns; a.adv_stats = batch->adv_stats; a.log_std = log_std;
  a.clip = cfg->clip; a.value_coef = cfg->value_coef; a.ws = workspace;
  w.ws = workspace;
  r.ws = workspace; r.log_std = log_std; r.log_std_grad = log_std_grad; r.stats = stats;
  r.value_coef = cfg->value_coef; r.entropy_coef = cfg->entropy_coef;
  const size_t lds = act_lds_bytes(a.LD);
  allow_dynamic_lds(h, imit ? (const void *)&k_policy_learn_rows_imit : sym ? (const void *)&k_policy_learn_rows_sym : (const void *)&k_policy_learn_rows, lds);
  const int tiles = sym ? w.Mp / (2 * ACT_TILE) : w.Mp / ACT_TILE;     // (sym: a workgroup runs its tile and the tile's mirror)
  const dim3 rows_grid(tiles, critic ? 2 : 1), rows_block(WAVE * ACT_WAVES);
  const dim3 reduce_grid((unsigned)((r.rp + NA + (imit ? LRN_NI : sym ? LRN_NS : 1) + 255) / 256));
  const int augment = sym && sym->augment != 0;
  if (sym) {
    r.M = augment ? 2 * batch->M : batch->M;                           // the rows the means are over
    launch(k_policy_learn_rows_sym, rows_grid, rows_block, lds, a,
           LearnSym{{sym->actor_perm, sym->critic_perm}, {sym->actor_sign, sym->critic_sign}, sym->action_perm, sym->action_sign, augment, w.Mp / 2,
                    sym->mirror_coef});
  } else if (imit) {
    launch(k_policy_learn_rows_imit, rows_grid, rows_block, lds, a,
           LearnImit{imit->target, imit->weight, imit->skip_surrogate, imit->imitation_coef, imit->surrogate_coef, imit->loss == TSIDB_POL_IMIT_HUBER});
  } else {
    launch(k_policy_learn_rows, rows_grid, rows_block, lds, a);
  }
  launch(k_policy_learn_wgrad, dim3(learn_blocks(w), r.nseg), dim3(WAVE), 0, w);
  if (sym) launch(k_policy_learn_reduce_sym, reduce_grid, dim3(256), 0, r, ReduceSym{sym->mirror_coef, batch->M, sym->stats});
  else if (imit) launch(k_policy_learn_reduce_imit, reduce_grid, dim3(256), 0, r, ReduceImit{imit->imitation_coef, imit->surrogate_coef, imit->stats});
  else launch(k_policy_learn_reduce, reduce_grid, dim3(256), 0, r);
  });
}

extern "C" {

int tsidb_policy_learn_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes) {
  return learn_workspace_call(h, "tsidb_policy_learn_workspace: ", actor, critic, M, bytes, LRN_NR);
}

int tsidb_policy_learn_imit_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes) {
  return learn_workspace_call(h, "tsidb_policy_learn_imit_workspace: ", actor, critic, M, bytes, LRN_NR + LRN_NI);
}

int tsidb_policy_learn(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                       const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                       const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                       const tsidb_policy_learn_cfg *cfg, float *workspace, size_t workspace_bytes, float *stats, void *stream) {
  return learn_call(h, "tsidb_policy_learn: ", actor, critic, batch, actor_grads, critic_grads, log_std, log_std_grad, cfg, nullptr, workspace,
                    workspace_bytes, stats, stream);
}

int tsidb_policy_learn_sym_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes) {
  return learn_workspace_call(h, "tsidb_policy_learn_sym_workspace: ", actor, critic, M, bytes, LRN_NR + LRN_NS, true);
}

int tsidb_policy_learn_sym(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                           const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                           const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                           const tsidb_policy_learn_cfg *cfg, const tsidb_policy_symmetry *sym, float *workspace, size_t workspace_bytes,
                           float *stats, void *stream) {
  return learn_call(h, "tsidb_policy_learn_sym: ", actor, critic, batch, actor_grads, critic_grads, log_std, log_std_grad, cfg, nullptr, workspace,
                    workspace_bytes, stats, stream, sym);
}

int tsidb_policy_learn_imit(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                            const tsidb_policy_learn_batch *batch, const tsidb_policy_grads *actor_grads,
                            const tsidb_policy_grads *critic_grads, const float *log_std, float *log_std_grad,
                            const tsidb_policy_learn_cfg *cfg, const tsidb_policy_imit *imit, float *workspace, size_t workspace_bytes,
                            float *stats, void *stream) {
  return learn_call(h, "tsidb_policy_learn_imit: ", actor, critic, batch, actor_grads, critic_grads, log_std, log_std_grad, cfg, imit, workspace,
                    workspace_bytes, stats, stream);
}

} // extern "C"

// The pieces of a step in the header's order - the actor's layers (weight, bias), the critic's, log_std - with their chunks
// counted, and off: where each piece starts among the P elements of all pieces.  The pointers are the call's to fill.
static void opt_layout(const LearnNet *nets, OptArgs &a, size_t *off) {
  size_t P = 0;
  int np = 0, chunks = 0;
  auto add = [&](int n) {
    OptPiece &pc = a.piece[np++];
    pc.n = n; pc.chunk0 = chunks;
    off[np - 1] = P;
    chunks += (n + OPT_CHUNK - 1) / OPT_CHUNK;
    P += (size_t)n;
  };
  for (int y = 0; y < 2; y++) {
    const ActorNet &n = nets[y].net;
    for (int l = 0; l < n.n_layers; l++) {
      add(n.width[l] * (l ? n.width[l - 1] : n.K));
      if (n.b[l]) add(n.width[l]);
    }
  }
  add(NA);
  a.npieces = np; a.nchunks = chunks; a.P = P;
}

static int opt_segments(int M) { return M > 0 ? (M + LRN_SEG - 1) / LRN_SEG : 0; }

static size_t opt_workspace_bytes(int nchunks, int nseg) { return ((size_t)nchunks + 2 * (size_t)nseg) * sizeof(double) + sizeof(OptScalars); }

extern "C" {

int tsidb_policy_opt_workspace(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic, int M, size_t *bytes) {
  GUARD_BEGIN
  const char *who = "tsidb_policy_opt_workspace: ";
  if (!actor) throw std::string(who) + "null actor";
  if (!bytes) throw std::string(who) + "null bytes";
  if (M < 0) throw std::string(who) + "M must be >= 0 (0 = no schedule)";
  OptArgs a = {};
  size_t off[OPT_MAXPIECES];
  opt_layout(learn_nets(actor, critic, who).data(), a, off);
  *bytes = opt_workspace_bytes(a.nchunks, opt_segments(M));
  GUARD_END
}

int tsidb_policy_opt_step(tsidb_handle h, const tsidb_policy_net *actor, const tsidb_policy_net *critic,
                          const tsidb_policy_grads *actor_grads, const tsidb_policy_grads *critic_grads, float *log_std,
                          const float *log_std_grad, const tsidb_policy_opt_cfg *cfg, const tsidb_policy_opt_state *state,
                          const tsidb_policy_opt_kl *kl, void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "tsidb_policy_opt_step: ";
  return stream_call(h, stream, [&](auto launch) {
  if (!actor) throw std::string(who) + "null actor";
  if (!actor_grads) throw std::string(who) + "null actor_grads";
  if (critic && !critic_grads) throw std::string(who) + "null critic_grads";
  if (!cfg) throw std::string(who) + "null cfg";
  if (!state) throw std::string(who) + "null state";
  if (!log_std || !log_std_grad) throw std::string(who) + "null log_std or log_std_grad";
  if (!state->moments || !state->lr || !state->step || !state->stats) throw std::string(who) + "null state pointer (moments, lr, step, stats)";
  if (!workspace) throw std::string(who) + "null workspace";
  if (!(cfg->b1 >= 0.0 && cfg->b1 < 1.0) || !(cfg->b2 >= 0.0 && cfg->b2 < 1.0)) throw std::string(who) + "b1 and b2 must be in [0, 1)";
  if (!(cfg->eps > 0.0) || !std::isfinite(cfg->eps)) throw std::string(who) + "eps must be > 0";
  if (!(cfg->max_norm >= 0.0) || !std::isfinite(cfg->max_norm)) throw std::string(who) + "max_norm must be >= 0 (0 = no clipping)";
  if (!(cfg->desired_kl >= 0.0) || !std::isfinite(cfg->desired_kl)) throw std::string(who) + "desired_kl must be >= 0 (0 = no schedule)";
  if (!(cfg->lr_min > 0.f) || !(cfg->lr_min <= cfg->lr_max) || !std::isfinite(cfg->lr_max)) throw std::string(who) + "lr_min must be > 0 and <= lr_max";
  const bool sched = cfg->desired_kl > 0.0;
  if (sched) {
    if (!kl || !kl->mean || !kl->index || !kl->mu || !state->log_std_old)
      throw std::string(who) + "the schedule needs kl (mean, index, mu) and log_std_old";
    if (kl->M < 1) throw std::string(who) + "M must be >= 1";
    if (kl->rows < 1) throw std::string(who) + "rows must be >= 1";
  }
  const auto nets = learn_nets(actor, critic, who);
  OptArgs a = {};
  size_t off[OPT_MAXPIECES];
  opt_layout(nets.data(), a, off);
  a.nseg = sched ? opt_segments(kl->M) : 0;
  const size_t need = opt_workspace_bytes(a.nchunks, a.nseg);
  if (workspace_bytes < need) throw std::string(who) + "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed";
  int np = 0;
  auto fill = [&](const float *p, const float *g) {
    OptPiece &pc = a.piece[np];
    pc.p = const_cast<float *>(p); pc.g = g;
    pc.m = state->moments + off[np++];
    pc.vec = (((uintptr_t)pc.p | (uintptr_t)pc.g | (uintptr_t)pc.m | (uintptr_t)(pc.m + a.P)) & 15) == 0;
  };
  each_layer_grad(who, actor, critic, actor_grads, critic_grads, nets.data(), [&](const float *W, const float *dW, const float *b, const float *db) {
    fill(W, dW);
    if (b) fill(b, db);
  });
  fill(log_std, log_std_grad);
  if (sched) { a.mu = kl->mu; a.mean = kl->mean; a.index = kl->index; a.rows = kl->rows; a.M = kl->M; a.log_std_old = state->log_std_old; }
  a.log_std = log_std;
  a.b1 = cfg->b1; a.b2 = cfg->b2; a.max_norm = cfg->max_norm; a.desired_kl = cfg->desired_kl;
  a.omb1 = (float)(1.0 - cfg->b1); a.b2f = (float)cfg->b2; a.omb2 = (float)(1.0 - cfg->b2); a.epsf = (float)cfg->eps;
  a.lr_min = cfg->lr_min; a.lr_max = cfg->lr_max; a.skip_nonfinite = cfg->skip_nonfinite != 0;
  a.lr = state->lr; a.step = (long long *)state->step; a.stats = state->stats;
  a.part = (double *)workspace;
  a.sc = (OptScalars *)(a.part + a.nchunks + 2 * a.nseg);
  launch(k_policy_opt_partial, dim3(a.nchunks + a.nseg), dim3(OPT_LANES), 0, a);
  launch(k_policy_opt_scalars, dim3(1), dim3(OPT_LANES), 0, a);
  launch(k_policy_opt_apply, dim3(a.nchunks), dim3(OPT_LANES), 0, a);
  });
}

} // extern "C"

extern "C" {

int tsidb_create(const void *model_blob, size_t nbytes, const double *params, int n_params, int num_envs, int device,
                 int dtype, tsidb_handle *out) {
  if (!out) return -1;
  *out = nullptr;
  tsidb_ctx *h = new tsidb_ctx();
  *out = h; // returned even on failure so that tsidb_last_error can be read; caller destroys it
  try {
    if (!model_blob || nbytes < 16 || memcmp(model_blob, "TSIDBM01", 8) != 0) throw std::string("not a TSIDBM01 model blob");
    if (!params || n_params != P_COUNT) throw std::string("params must hold TSIDB_P_COUNT doubles");
    if (num_envs <= 0) throw std::string("num_envs must be positive");
    if (dtype != TSIDB_F64 && dtype != TSIDB_F32) throw std::string("dtype must be TSIDB_F64 or TSIDB_F32");
    h->device = device; h->dtype = dtype; h->num_envs = num_envs;
    h->sim_waves = num_envs <= SMALL_BATCH_ENVS ? 2 : 1;
    h->blob.raw.assign((const uint8_t *)model_blob, (const uint8_t *)model_blob + nbytes);
    h->blob.validate();
    { // the blob must be for the robot this library was built for
      const int want[9] = {NJ, NQ, NV, NA, NB, TOPO_HAS_SIM, NG, CONDIM, TOPO_EULERDAMP};
      const int *got = h->blob.i32("model_dims", 9);
      for (int i = 0; i < 9; i++)
        if (got[i] != want[i])
          throw std::string("model blob is for another robot than this library (dimensions differ: build the library with "
                            "the blob's topology header, -DTSIDB_TOPOLOGY_HEADER)");
    }
    h->params.assign(params, params + n_params);
    if (lacks_sim(h, h->params[P_SIM_ENABLED] != 0.0, "", ": set sim_enabled = False")) throw h->err;
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw std::string("no such HIP device (this library has no CPU path)");
    HIP_OK(hipSetDevice(device));
    validate_geometry(h->blob);
    with_dtype(dtype, [&](auto t) { upload_model<decltype(t)>(h); });
    if (TOPO_HAS_SIM) { // sim body of each sole frame: frame -> TSID joint -> sim joint (mj_sim2tsid) -> body
      const int *fp = h->blob.i32("pin_frame_parent", 2), *s2t = h->blob.i32("mj_sim2tsid", NA);
      for (int f = 0; f < 2; f++)
        for (int i = 0; i < NA; i++)
          if (s2t[i] == fp[f] - 1) h->foot_body[f] = 1 + i;
      if (h->foot_body[0] < 0 || h->foot_body[1] < 0) throw std::string("model blob: sole frames are not on sim bodies");
      static_assert(NG <= 64, "foot geoms are kept as a 64-bit mask");
      const int *gb = h->blob.i32("mj_geom_body", NG);
      for (int f = 0; f < 2; f++)
        for (int g = 0; g < NG; g++)
          if (gb[g] == h->foot_body[f]) h->foot_geoms[f] |= 1ull << g;
    }
  } catch (const std::string &s) {
    h->err = s;
    return 1;
  }
  return 0;
}

int tsidb_destroy(tsidb_handle h) {
  if (!h) return -1;
  // (a tsidb_create that failed part-way may have allocated some of them: upload_model allocates d_model last)
  for (void *p : {h->d_model, h->d_hull, h->d_box, (void *)h->d_eadr, (void *)h->d_edge})
    if (p) { (void)hipSetDevice(h->device); (void)hipFree(p); }
  delete h;
  return 0;
}

const char *tsidb_last_error(tsidb_handle h) { return h ? h->err.c_str() : "null handle"; }

int tsidb_set_params(tsidb_handle h, const double *params, int n_params) {
  GUARD_BEGIN
  if (!params || n_params != P_COUNT) throw std::string("params must hold TSIDB_P_COUNT doubles");
  h->params.assign(params, params + n_params);
  wait_for_own_streams(h);
  with_dtype(h->dtype, [&](auto t) { upload_model<decltype(t)>(h); });
  GUARD_END
}

int tsidb_set_sensors(tsidb_handle h, int n_sites, const int32_t *site_body, const double *site_pos, const double *site_quat,
                      void *sensordata) {
  GUARD_BEGIN
  if (lacks_sim(h, n_sites || sensordata, "tsidb_set_sensors: ")) throw h->err;
  if (n_sites < 0 || n_sites > TSIDB_MAXSITE) throw std::string("tsidb_set_sensors: n_sites must be 0 .. TSIDB_MAXSITE");
  if ((n_sites == 0) != (sensordata == nullptr)) throw std::string("tsidb_set_sensors: sites without a buffer, or a buffer without sites");
  if (n_sites && (!site_body || !site_pos || !site_quat)) throw std::string("tsidb_set_sensors: null site table");
  double R[TSIDB_MAXSITE][9];
  for (int s = 0; s < n_sites; s++) {
    if (site_body[s] < 0 || site_body[s] >= NB) throw std::string("tsidb_set_sensors: site body out of range");
    double nn = 0;
    for (int i = 0; i < 3; i++) if (!std::isfinite(site_pos[3 * s + i])) throw std::string("tsidb_set_sensors: non-finite site position");
    for (int i = 0; i < 4; i++) {
      if (!std::isfinite(site_quat[4 * s + i])) throw std::string("tsidb_set_sensors: non-finite site quaternion");
      nn += site_quat[4 * s + i] * site_quat[4 * s + i];
    }
    nn = std::sqrt(nn);
    if (!(nn > 0) || !std::isfinite(nn)) throw std::string("tsidb_set_sensors: zero site quaternion");
    const double w = site_quat[4 * s] / nn, x = site_quat[4 * s + 1] / nn, y = site_quat[4 * s + 2] / nn, z = site_quat[4 * s + 3] / nn;
    const double Rs[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                          2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    memcpy(R[s], Rs, sizeof Rs);
  }
  wait_for_own_streams(h); // (the site table is part of the model constants)
  h->n_sites = n_sites;
  for (int s = 0; s < n_sites; s++) {
    h->site_body[s] = site_body[s];
    memcpy(h->site_pos[s], site_pos + 3 * s, sizeof h->site_pos[s]);
    memcpy(h->site_R[s], R[s], sizeof R[s]);
  }
  h->sens = sensordata;
  with_dtype(h->dtype, [&](auto t) { upload_model<decltype(t)>(h); });
  GUARD_END
}

int tsidb_set_refs(tsidb_handle h, const void *com_ref, const void *posture_ref, const void *foot_ref,
                   const void *contact_ref, const uint8_t *contact_active, const void *cop_frames) {
  if (!h) return -1;
  if (!com_ref || !posture_ref || !foot_ref || !contact_ref || !contact_active || !cop_frames) {
    h->err = "tsidb_set_refs: null reference buffer";
    return 1;
  }
  h->com_ref = com_ref; h->posture_ref = posture_ref; h->foot_ref = foot_ref;
  h->contact_ref = contact_ref; h->contact_active = contact_active; h->cop_frames = cop_frames;
  return 0;
}

int tsidb_set_option(tsidb_handle h, int option, int value) {
  if (!h) return -1;
  if (option == TSIDB_OPT_SIM_WAVES && (value == 1 || value == 2)) { h->sim_waves = value; return 0; }
  if (option == TSIDB_OPT_LDS_PAD && value >= 0 && value <= 40960) { h->lds_pad = (unsigned)value; return 0; }
  if (option == TSIDB_OPT_QP_FAST_EQ && (value == 0 || value == 1)) { h->qp_fast_eq = value; return 0; }
  if (option == TSIDB_OPT_CU_SPLIT && value >= -1 && value <= 1) { h->cu_split = value; return 0; }
  h->err = "tsidb_set_option: unknown option or value";
  return 1;
}

int tsidb_get_option(tsidb_handle h, int option, int *value) {
  if (!h) return -1;
  if (!value) { h->err = "tsidb_get_option: null value"; return 1; }
  if (option == TSIDB_OPT_SIM_WAVES) { *value = h->sim_waves; return 0; }
  if (option == TSIDB_OPT_LDS_PAD) { *value = (int)h->lds_pad; return 0; }
  if (option == TSIDB_OPT_QP_FAST_EQ) { *value = h->qp_fast_eq; return 0; }
  if (option == TSIDB_OPT_CU_SPLIT) { *value = h->cu_split_on() ? 1 : 0; return 0; }
  h->err = "tsidb_get_option: unknown option";
  return 1;
}

int tsidb_stream_create(tsidb_handle h, int role, void **stream) {
  GUARD_BEGIN
  if (!stream || (role != TSIDB_STREAM_TICK && role != TSIDB_STREAM_SIM)) throw std::string("tsidb_stream_create: role must be TSIDB_STREAM_TICK or TSIDB_STREAM_SIM");
  hipStream_t s = nullptr;
  if (h->cu_split_on()) {
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, h->device));
    const int ncu = prop.multiProcessorCount, half = ncu / 2;
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int c = role == TSIDB_STREAM_TICK ? 0 : half; c < (role == TSIDB_STREAM_TICK ? half : ncu); c++) mask[(size_t)c / 32] |= 1u << (c % 32);
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
      (void)hipGetLastError(); // CU masking not available here: an ordinary stream, and no further attempts for this handle
      s = nullptr;
      h->cu_split = 0;
    }
  }
  if (!s) HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  GUARD_END
}

int tsidb_stream_destroy(tsidb_handle h, void *stream) {
  GUARD_BEGIN
  if (stream) {
    for (size_t i = 0; i < h->used_streams.size(); i++)
      if (h->used_streams[i] == (hipStream_t)stream) { h->used_streams.erase(h->used_streams.begin() + i); break; }
    HIP_OK(hipStreamDestroy((hipStream_t)stream)); // (hipStreamDestroy lets the stream's pending work finish)
  }
  GUARD_END
}

int tsidb_set_cop_ref(tsidb_handle h, const void *cop_ref) {
  if (!h) return -1;
  h->cop_ref = cop_ref;
  return 0;
}

int tsidb_reset(tsidb_handle h, const int32_t *env_ids, int n_ids, void *q, void *v, void *qpos, void *qvel,
                void *qacc_ws, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!q || !v || !qpos || !qvel || !qacc_ws) throw std::string("tsidb_reset: null state buffer");
  launch_reset(h, env_ids, n_ids, q, v, qpos, qvel, qacc_ws, nullptr, 0, nullptr, (hipStream_t)stream);
  GUARD_END
}

int tsidb_reset_done(tsidb_handle h, const void *rows, int rows_ld, void *q, void *v, void *qpos, void *qvel, void *qacc_ws,
                     void *frames, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!rows || rows_ld < NROW) throw std::string("tsidb_reset_done: needs the [N, >= TSIDB_NROW] rows tsidb_tick writes (done flag in column TSIDB_NOBS + 1)");
  if (!q || !v || !qpos || !qvel || !qacc_ws) throw std::string("tsidb_reset_done: null state buffer");
  launch_reset(h, nullptr, 0, q, v, qpos, qvel, qacc_ws, rows, rows_ld, frames, (hipStream_t)stream);
  GUARD_END
}

int tsidb_set_posture_bias(tsidb_handle h, const void *posture_bias) {
  if (!h) return -1;
  h->posture_bias = posture_bias;
  return 0;
}

int tsidb_walk_plan(tsidb_handle h, const int32_t *env_ids, int n_ids, const void *done_rows, int rows_ld,
                    const double *plan_params, int n_plan_params, const double *path, const int32_t *npts, int P,
                    const double *scale, int32_t *episode, int bump_episode, int K, double *steps, void *coef, int32_t *side,
                    int32_t *nsteps, void *rest, void *com, int32_t *flags, void *t_offset, int32_t *td_latch, double t,
                    const double *t_device, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!plan_params || n_plan_params != TSIDB_PLAN_NPARAMS) throw std::string("tsidb_walk_plan: plan_params must hold TSIDB_PLAN_NPARAMS doubles");
  if (!steps || !coef || !side || !nsteps || !rest || !com || K <= 0) throw std::string("tsidb_walk_plan: null table or K <= 0");
  if (path && (!npts || P < 2)) throw std::string("tsidb_walk_plan: an explicit path needs npts and P >= 2");
  if (!path && !(plan_params[12] >= 2)) throw std::string("tsidb_walk_plan: the unicycle path needs at least two vertices");
  if (!(plan_params[0] > 0) || !(plan_params[3] > 0) || !(plan_params[5] > 0) || !(plan_params[4] > 0 && plan_params[4] < 1))
    throw std::string("tsidb_walk_plan: step_length, step_duration, t_start must be positive and rise_ratio inside (0, 1)");
  if (done_rows && rows_ld < NROW) throw std::string("tsidb_walk_plan: the done mask needs rows of at least TSIDB_NROW values");
  // one thread per env walks its path vertex by vertex: every loop bound that comes from a parameter is checked here
  for (int i = 0; i < TSIDB_PLAN_NPARAMS; i++)
    if (!std::isfinite(plan_params[i])) throw std::string("tsidb_walk_plan: non-finite plan parameter");
  if (!(plan_params[1] > 0) || !(plan_params[2] >= 0) || !(plan_params[6] >= 0))
    throw std::string("tsidb_walk_plan: step_width must be positive, step_height and com_drop non-negative");
  if (plan_params[8] != 0 && !(plan_params[8] >= plan_params[0] / 1000))
    throw std::string("tsidb_walk_plan: resample_ds must be 0 (vertices as given) or at least step_length / 1000");
  if (!path) {
    if (!(plan_params[12] <= 65536)) throw std::string("tsidb_walk_plan: the unicycle path may have at most 65536 vertices");
    if (!scale && !(plan_params[13] > 0 && plan_params[14] >= plan_params[13])) throw std::string("tsidb_walk_plan: scale range must satisfy 0 < lo <= hi");
    if (!(plan_params[11] > 0)) throw std::string("tsidb_walk_plan: the unicycle path's time step must be positive");
  } else if (P > 65536) throw std::string("tsidb_walk_plan: an explicit path may have at most 65536 vertices per env");
  const int cnt = env_ids ? n_ids : h->num_envs;
  if (cnt <= 0) return 0;
  PlanParams PP;
  for (int i = 0; i < 16; i++) PP.v[i] = plan_params[i];
  hipStream_t s = (hipStream_t)stream;
  const int grid = (cnt + 63) / 64;
  with_dtype(h->dtype, [&](auto t_) {
    using T = decltype(t_);
    hipLaunchKernelGGL(k_plan<T>, dim3(grid), dim3(64), 0, s, h->num_envs, env_ids, n_ids, (const T *)done_rows, rows_ld, PP,
                       (const T *)h->cop_frames, (const T *)h->com_ref, path, npts, P, scale, episode, bump_episode, K, steps,
                       (T *)coef, side, nsteps, (T *)rest, (T *)com, flags, (T *)t_offset, td_latch, t, t_device);
  });
  HIP_OK(hipGetLastError());
  GUARD_END
}

int tsidb_tick(tsidb_handle h, void *q, void *v, void *tau, void *dv, void *f, int32_t *status, void *obs, int obs_ld,
               void *frames, int32_t *info, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!q || !v || !tau || !dv || !f || !status) throw std::string("tsidb_tick: null buffer");
  launch_tick(h, q, v, tau, dv, f, status, obs, obs_ld, frames, info, (hipStream_t)stream);
  GUARD_END
}

int tsidb_sim(tsidb_handle h, const void *q_tsid, const void *v_tsid, void *qpos, void *qvel, void *qacc_ws, void *qacc,
              int32_t *ncon, int32_t *con_pairs, int32_t *info, void *stream) {
  GUARD_BEGIN
  if (!qpos || !qvel || !qacc_ws) throw std::string("tsidb_sim: null state buffer");
  launch_sim(h, 1, q_tsid, v_tsid, nullptr, qpos, qvel, qacc_ws, qacc, ncon, con_pairs, info, (hipStream_t)stream);
  GUARD_END
}

int tsidb_sim_batch(tsidb_handle h, int n_steps, const void *q_ring, const void *v_ring, const int32_t *slots, void *qpos, void *qvel,
                    void *qacc_ws, void *qacc, int32_t *ncon, int32_t *con_pairs, int32_t *info, void *stream) {
  GUARD_BEGIN
  if (!qpos || !qvel || !qacc_ws || !q_ring || !slots) throw std::string("tsidb_sim_batch: null buffer");
  launch_sim(h, n_steps, q_ring, v_ring, slots, qpos, qvel, qacc_ws, qacc, ncon, con_pairs, info, (hipStream_t)stream);
  GUARD_END
}

int tsidb_sim_ctrl(tsidb_handle h, int n_steps, void *qpos, void *qvel, void *qacc_ws, void *qacc, int32_t *ncon, int32_t *con_pairs,
                   int32_t *info, void *stream) {
  GUARD_BEGIN
  if (!h->ctrl) throw std::string("tsidb_sim_ctrl: no ctrl buffer registered (call tsidb_set_ctrl first)");
  if (!qpos || !qvel || !qacc_ws) throw std::string("tsidb_sim_ctrl: null state buffer");
  launch_sim(h, n_steps, nullptr, nullptr, nullptr, qpos, qvel, qacc_ws, qacc, ncon, con_pairs, info, (hipStream_t)stream);
  GUARD_END
}

int tsidb_step(tsidb_handle h, void *q, void *v, void *qpos, void *qvel, void *qacc_ws, void *tau, void *dv, void *f,
               int32_t *status, void *obs, int obs_ld, void *frames, int32_t *ncon, int32_t *con_pairs, int32_t *info,
               int n_substeps, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!q || !v || !tau || !dv || !f || !status) throw std::string("tsidb_step: null buffer");
  const bool sim = h->params[P_SIM_ENABLED] != 0.0, closed = h->params[P_CLOSED_LOOP] != 0.0;
  if (sim && (!qpos || !qvel || !qacc_ws)) throw std::string("tsidb_step: null sim state buffer");
  hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < n_substeps; it++) {
    // closed loop: the tick reads the sim state, the sim is driven by tau and keeps its own base pose
    launch_tick(h, q, v, tau, dv, f, status, obs, obs_ld, frames, info, s, closed ? qpos : nullptr, closed ? qvel : nullptr);
    if (sim) launch_sim(h, 1, closed ? nullptr : q, closed ? nullptr : v, nullptr, qpos, qvel, qacc_ws, nullptr, ncon, con_pairs, info, s, closed ? tau : nullptr);
  }
  GUARD_END
}

int tsidb_walk_update(tsidb_handle h, const void *coef, const int32_t *side, const int32_t *nsteps, const void *rest,
                      const void *com, int K, double t, double step_duration, double t_start, double omega, double com_z0,
                      double com_drop, const void *frames, const void *t_offset, const int32_t *ncon, const int32_t *con_pairs,
                      int32_t *td_latch, double td_fraction, const void *t_device, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  const tsidb_walk_args a = {coef, side, nsteps, rest, com, K, t, step_duration, t_start, omega, com_z0, com_drop, frames, t_offset,
                             ncon, con_pairs, td_latch, td_fraction, (const double *)t_device};
  hipStream_t s = (hipStream_t)stream;
  const int grid = (h->num_envs * 16 + 255) / 256;
  with_dtype(h->dtype, [&](auto t) { hipLaunchKernelGGL(k_walk<decltype(t)>, dim3(grid), dim3(256), 0, s, h->num_envs, walk_args<decltype(t)>(h, &a)); });
  HIP_OK(hipGetLastError());
  GUARD_END
}

int tsidb_tick_walk(tsidb_handle h, const tsidb_walk_args *walk, void *q, void *v, void *tau, void *dv, void *f, int32_t *status,
                    void *obs, int obs_ld, void *frames, int32_t *info, void *q_snapshot, void *v_snapshot, void *stream) {
  GUARD_BEGIN
  need_refs(h);
  if (!q || !v || !tau || !dv || !f || !status) throw std::string("tsidb_tick_walk: null buffer");
  launch_tick(h, q, v, tau, dv, f, status, obs, obs_ld, frames, info, (hipStream_t)stream, nullptr, nullptr, walk, q_snapshot, v_snapshot);
  GUARD_END
}

int tsidb_rbd_terms(tsidb_handle h, const void *q, const void *v, void *M, void *hbias, void *Jcom, void *Jf, void *oMf,
                    void *com, void *stream) {
  GUARD_BEGIN
  if (!q || !v || !M || !hbias || !Jcom || !Jf || !oMf || !com) throw std::string("tsidb_rbd_terms: null buffer");
  hipStream_t s = (hipStream_t)stream;
  h->note_stream(s);
  with_dtype(h->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_rbd<T>, dim3(h->num_envs), dim3(WAVE), 0, s, (const DevModel<T> *)h->d_model, h->num_envs, (const T *)q,
                       (const T *)v, (T *)M, (T *)hbias, (T *)Jcom, (T *)Jf, (T *)oMf, (T *)com);
  });
  HIP_OK(hipGetLastError());
  GUARD_END
}

#ifdef TSIDB_STAMPS
int tsidb_debug_stamps(unsigned long long *out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(unsigned long long) * NSTAMP * (size_t)n);
}
#endif

/* dimensions of the robot this library was built for, in the order of the blob's model_dims section: NJ, NQ, NV, NA,
 * NB (sim bodies), 1 if the sim stage is built, NG (collision geoms), contact dimension, 1 if joints are damped */
int tsidb_dims(int *out9) {
  if (!out9) return -1;
  const int d[9] = {NJ, NQ, NV, NA, NB, TOPO_HAS_SIM, NG, CONDIM, TOPO_EULERDAMP};
  for (int i = 0; i < 9; i++) out9[i] = d[i];
  return 0;
}

int tsidb_lds_bytes(int dtype, int which) {
  return with_dtype(dtype, [&](auto t) { return which == 0 ? (int)sizeof(TickLds<decltype(t)>) : (int)sizeof(SimLds<decltype(t)>); });
}

} // extern "C"
