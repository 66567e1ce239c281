// tsidb_policy.hpp - the environment around a policy-driven sim loop (include/tsidb.h tsidb_policy_*): action -> ctrl
// before the sim steps, reward / termination after them, bookkeeping of the restarted envs and the observation row after the
// reset; with a randomisation configured (tsidb_policy_randomize) also the push of the step before the sim steps, noise on the
// state of the envs just reset, command resampling and observation noise - every draw a hash of (seed, stream, column, env,
// episode, ep_len), no random state anywhere; with a terrain configured (tsidb_policy_terrain_config) the sim's per-env mass
// scale, friction, floor plane and stepped terrain are redrawn for the envs just reset, and a height scan of that floor is
// written beside the observation; with TSID in the loop its command is written as an action (the teacher), and
// k_policy_teacher_mix turns that into the label of a stored rollout row and, for a share of the episodes, into the action the
// env executes.  No reference counterpart: the reference runs one TSID-driven episode (main.py:113-124).
//
// Shape of all the kernels, as k_reset: one wavefront per env, lane = column of the env's rows (coalesced row loads and
// stores), wave reductions (DPP) for the sums over actuators and wave votes for the flags over contacts; four envs per
// workgroup, no LDS, no barrier.  Everything an env needs is a few hundred bytes: the kernels are launch- and latency-bound,
// and a wavefront per env keeps every load of a row one transaction.
#pragma once
#include "tsidb_common.hpp"
#include "tsidb_sim.hpp" // CTRL_*

namespace tsidb {

constexpr int POL_NT = 12;              // reward terms (TSIDB_POL_NT)
constexpr int POL_HIST = 8;             // slots of the action history ring (TSIDB_POL_HIST): delays of 0 .. 7 policy steps
constexpr int POL_NOBS = 11 + 3 * NA;   // observation columns (TSIDB_POL_NOBS for the v1 robot)
constexpr int POL_NPRIV = 4;            // privileged tail: base linear velocity (body frame), base height
constexpr int POL_ENVS_PER_BLOCK = 4;
enum { POL_T_TRACK_LIN = 0, POL_T_TRACK_ANG, POL_T_LIN_VEL_Z, POL_T_ANG_VEL_XY, POL_T_ORIENTATION, POL_T_BASE_HEIGHT, POL_T_TORQUES,
       POL_T_ACTION_RATE, POL_T_JOINT_VEL, POL_T_FEET_AIR_TIME, POL_T_ALIVE, POL_T_TERMINATION };

// tsidb_policy_config's values in the path's arithmetic type, passed to the kernels by value
template <typename T>
struct PolicyCfg {
  T clip, alpha, sigma, h_target, t_air, deadband, air_dt /* decimation * dt */, done_height, done_tilt;
  T w[POL_NT], scale[NA], def[NA];
  double cmd_lo[3], cmd_hi[3];
  unsigned long long seed, foot_geoms[2];
  unsigned term_mask;
  int max_steps, position_mode;
};

// tsidb_policy_bufs in the path's arithmetic type
template <typename T>
struct PolicyBufs {
  T *hist, *last, *prev, *command, *air;
  int *ep_len, *episode;
  const int *delay;
  T *terms;
  int *timeout;
  T *obs;
  int obs_ld;
};

// tsidb_policy_randomize's values, passed to the kernels by value.  float64 whatever the path's type: the draws are formed in
// float64 and cast (include/tsidb.h)
struct PolicyDR {
  unsigned long long seed, env_offset;
  double reset_joint_pos, reset_joint_vel, reset_lin[3], reset_ang[3], reset_yaw, reset_xy, reset_lift;
  double noise_ang_vel, noise_gravity, noise_joint_pos, noise_joint_vel;
  double force_lo, force_hi, zero_prob;
  int push_interval, push_duration, command_interval;
};
enum { DR_S_JOINT_POS = 1, DR_S_JOINT_VEL, DR_S_LIN_VEL, DR_S_ANG_VEL, DR_S_YAW, DR_S_XY, DR_S_OBS, DR_S_PUSH_PHASE, DR_S_PUSH_MAG, DR_S_PUSH_DIR,
       DR_S_CMD_ZERO };

// U in [0, 1): the top 53 bits of the hash over 2^53
__device__ __forceinline__ double pol_uniform(unsigned long long key, unsigned long long env, unsigned long long counter) {
  return (double)(plan_hash(key, env, counter) >> 11) * (1.0 / 9007199254740992.0);
}
// the draw of (stream, column): key = seed + ((stream * 256 + column) << 32)
__device__ __forceinline__ double pol_draw(unsigned long long seed, int stream, int column, unsigned long long env, unsigned long long counter) {
  return pol_uniform(seed + ((unsigned long long)(stream * 256 + column) << 32), env, counter);
}
__device__ __forceinline__ double pol_draw(const PolicyDR &d, int stream, int column, unsigned long long env, unsigned long long counter) {
  return pol_draw(d.seed, stream, column, env, counter);
}
// amp (2 U - 1) in float64, cast
template <typename T>
__device__ __forceinline__ T pol_noise(const PolicyDR &d, double amp, int stream, int column, unsigned long long env, unsigned long long counter) {
  return (T)(amp * (2.0 * pol_draw(d, stream, column, env, counter) - 1.0));
}

// the env of this wavefront (-1: none); wave-uniform, and said so to the compiler: row bases become scalar registers
__device__ __forceinline__ int pol_env(int n) {
  const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * POL_ENVS_PER_BLOCK + (threadIdx.x >> 6)));
  return e < n ? e : -1;
}

// lanes 0 .. 31 look at one row of the contact list each: bit 0 / 1 = a live floor contact on the left / right sole, bit 2 = one
// on a body of term_mask; the same bits on every lane
template <typename T>
__device__ __forceinline__ int pol_contacts(const DevModel<T> &m, const PolicyCfg<T> &c, const int *ncon, const int *con_pairs, size_t E, int lane) {
  bool lf = false, rf = false, tb = false;
  if (lane < MAXCON && lane < ncon[E]) {
    const int cp = con_pairs[E * MAXCON + lane];
    const int g = cp >> 16;
    if (cp >= 0 && !(cp & 0x8000) && g < NG) {   // live floor row
      lf = (c.foot_geoms[0] >> g) & 1ull;
      rf = (c.foot_geoms[1] >> g) & 1ull;
      tb = (c.term_mask >> m.geom_body[g]) & 1u;
    }
  }
  return (__any(lf) ? 1 : 0) | (__any(rf) ? 2 : 0) | (__any(tb) ? 4 : 0);
}

// ---------------------------------------------------------------------------- action -> ctrl (before the sim steps)
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_act(int n, PolicyCfg<T> c, PolicyBufs<T> b, const T *__restrict__ action, T *ctrl) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= NA) return;
  const size_t E = (size_t)e, row = E * NA + lane, slab = (size_t)n * NA;
  const int len = b.ep_len[E];
  int d = b.delay ? b.delay[E] : 0;
  d = d < 0 ? 0 : d > POL_HIST - 1 ? POL_HIST - 1 : d;
  const T a = action[row];
  const T act = a > c.clip ? c.clip : a < -c.clip ? -c.clip : a;   // (NaN passes: the sim step then skips the env)
  b.hist[(size_t)(len & (POL_HIST - 1)) * slab + row] = act;
  T delayed = act;
  if (d > len) delayed = 0;
  else if (d > 0) delayed = b.hist[(size_t)((len - d) & (POL_HIST - 1)) * slab + row];   // (this lane wrote it d steps ago)
  const T target = c.def[lane] + c.scale[lane] * delayed;
  const T old = ctrl[row];
  ctrl[row] = c.alpha == T(1) ? target : old + c.alpha * (target - old);
  b.prev[row] = b.last[row];
  b.last[row] = act;
}

// ---------------------------------------------------------------------------- reward / done (after the sim steps)
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_reward(const DevModel<T> *__restrict__ mp, int n, PolicyCfg<T> c, PolicyBufs<T> b,
                                                                             const T *__restrict__ qpos, const T *__restrict__ qvel, const int *__restrict__ ncon,
                                                                             const int *__restrict__ con_pairs, const int *__restrict__ info,
                                                                             const T *__restrict__ act_force, T *reward, T *done, int row_ld) {
  const DevModel<T> &m = *mp;
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  const T *qp = qpos + E * NQ, *qv = qvel + E * NV;
  // the state, a lane per column: finite?
  const T myq = lane < NQ ? qp[lane] : T(0), myv = lane < NV ? qv[lane] : T(0);
  const bool finite = !__any(!isfinite(myq) || !isfinite(myv));
  // sums over the actuators
  T tq = 0, ar = 0, jv = 0;
  if (lane < NA) {
    const T f = act_force ? act_force[E * NA + lane] : T(0), da = b.last[E * NA + lane] - b.prev[E * NA + lane], qd = qv[m.mj_act_dof[lane]];
    tq = f * f; ar = da * da; jv = qd * qd;
  }
  wave_sum3(tq, ar, jv);
  const int con = pol_contacts(m, c, ncon, con_pairs, E, lane);
  // the base: every lane the same values
  T R[9];
  quat_to_R(qp[4], qp[5], qp[6], qp[3], R);   // wxyz storage
  const T vx = R[0] * qv[0] + R[3] * qv[1] + R[6] * qv[2], vy = R[1] * qv[0] + R[4] * qv[1] + R[7] * qv[2],
          vz = R[2] * qv[0] + R[5] * qv[1] + R[8] * qv[2];
  const T wx = qv[3], wy = qv[4], wz = qv[5];
  const T cx = b.command[E * 3], cy = b.command[E * 3 + 1], cw = b.command[E * 3 + 2];
  const T ex = cx - vx, ey = cy - vy, ew = cw - wz, s2 = c.sigma * c.sigma, dz = qp[2] - c.h_target;
  const bool moving = sqrt(cx * cx + cy * cy) > c.deadband;
  const T air0 = b.air[E * 2], air1 = b.air[E * 2 + 1];
  const bool c0 = con & 1, c1 = con & 2;
  T fa = 0;
  if (moving && c0 && air0 > T(0)) fa += air0 - c.t_air;
  if (moving && c1 && air1 > T(0)) fa += air1 - c.t_air;
  const int len = b.ep_len[E];
  const T up = 1 - 2 * (qp[4] * qp[4] + qp[5] * qp[5]);   // the tick's tilt measure, on the sim quaternion
  const bool terminated = (info[E * 4 + 3] & 4) || !finite || qp[2] < c.done_height || up < c.done_tilt || (con & 4);
  const bool timeout = !terminated && c.max_steps > 0 && len + 1 >= c.max_steps;
  T t[POL_NT];
  t[POL_T_TRACK_LIN] = exp(-(ex * ex + ey * ey) / s2);
  t[POL_T_TRACK_ANG] = exp(-(ew * ew) / s2);
  t[POL_T_LIN_VEL_Z] = vz * vz;
  t[POL_T_ANG_VEL_XY] = wx * wx + wy * wy;
  t[POL_T_ORIENTATION] = R[6] * R[6] + R[7] * R[7];   // projected gravity = -(third row of R)
  t[POL_T_BASE_HEIGHT] = dz * dz;
  t[POL_T_TORQUES] = tq;
  t[POL_T_ACTION_RATE] = ar;
  t[POL_T_JOINT_VEL] = jv;
  t[POL_T_FEET_AIR_TIME] = fa;
  t[POL_T_ALIVE] = 1;
  t[POL_T_TERMINATION] = terminated ? T(1) : T(0);
  T rew = 0, mine = 0;
#pragma unroll
  for (int k = 0; k < POL_NT; k++) {
    rew += c.w[k] * t[k];
    mine = lane == k ? t[k] : mine;
  }
  if (lane < POL_NT) b.terms[E * POL_NT + lane] = mine;
  if (lane < 2) b.air[E * 2 + lane] = (lane ? c1 : c0) ? T(0) : (lane ? air1 : air0) + c.air_dt;
  if (lane == 0) {
    reward[E * row_ld] = rew;
    done[E * row_ld] = terminated || timeout ? T(1) : T(0);
    b.timeout[E] = timeout ? 1 : 0;
    b.ep_len[E] = len + 1;
  }
}

// ---------------------------------------------------------------------------- restarted envs + observation (after the reset)
// DR = false: no randomisation configured, d is not read.  DR = true (chosen on the host, tsidb_policy_obs): env_offset in the
// command draw, command resampling and zeroing, noise on the observation columns.
template <typename T, bool DR>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_obs(const DevModel<T> *__restrict__ mp, int n, PolicyCfg<T> c, PolicyBufs<T> b,
                                                                          const T *__restrict__ done_rows, int rows_ld, const T *__restrict__ qpos,
                                                                          const T *__restrict__ qvel, const int *__restrict__ ncon,
                                                                          const int *__restrict__ con_pairs, T *ctrl, PolicyDR d) {
  const DevModel<T> &m = *mp;
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  const bool fresh = done_rows[E * rows_ld + NROW - 1] != T(0);   // (the done column, NOBS + 1)
  int ep_now = 0, len_now = 0;   // DR: episode and ep_len as this kernel leaves them
  if constexpr (DR) { ep_now = b.episode[E] + (fresh ? 1 : 0); len_now = fresh ? 0 : b.ep_len[E]; }
  int con = pol_contacts(m, c, ncon, con_pairs, E, lane);
  T last = lane < NA ? b.last[E * NA + lane] : T(0);
  T cmd = lane < 3 ? b.command[E * 3 + lane] : T(0);
  if (fresh) {
    con = 3;   // (the reset leaves ncon and con_pairs of the fallen robot: a restarted env stands on both feet)
    last = 0;
    if (lane < NA) {
      const size_t row = E * NA + lane, slab = (size_t)n * NA;
#pragma unroll
      for (int s = 0; s < POL_HIST; s++) b.hist[(size_t)s * slab + row] = 0;
      b.last[row] = 0;
      b.prev[row] = 0;
      if (c.position_mode) ctrl[row] = c.def[lane];   // (the filter starts at the default pose; k_reset left 0)
    }
    if (lane < 2) b.air[E * 2 + lane] = 0;
    const int ep = b.episode[E] + 1;
    if (lane == 0) { b.ep_len[E] = 0; b.episode[E] = ep; }
    if constexpr (!DR) {
      if (lane < 3 && c.cmd_lo[lane] != c.cmd_hi[lane]) {
        const double u = (double)(plan_hash(c.seed + (unsigned long long)lane, (unsigned long long)e, (unsigned long long)ep) >> 11) * (1.0 / 9007199254740992.0);
        cmd = (T)(c.cmd_lo[lane] + (c.cmd_hi[lane] - c.cmd_lo[lane]) * u);
        b.command[E * 3 + lane] = cmd;
      }
    }
  }
  const unsigned long long ge = DR ? d.env_offset + (unsigned long long)e : 0ull;
  if constexpr (DR) {
    // a restart is resample 0 of its episode; resample k when ep_len reaches k * command_interval
    const bool resample = !fresh && d.command_interval > 0 && len_now > 0 && len_now % d.command_interval == 0;
    if (fresh || resample) {
      const unsigned long long ctr = (unsigned long long)ep_now + ((unsigned long long)(resample ? len_now / d.command_interval : 0) << 32);
      const bool zero = d.zero_prob > 0 && pol_draw(d, DR_S_CMD_ZERO, 0, ge, ctr) < d.zero_prob;
      if (lane < 3 && (zero || c.cmd_lo[lane] != c.cmd_hi[lane])) {
        cmd = zero ? T(0) : (T)(c.cmd_lo[lane] + (c.cmd_hi[lane] - c.cmd_lo[lane]) * pol_uniform(c.seed + (unsigned long long)lane, ge, ctr));
        b.command[E * 3 + lane] = cmd;
      }
    }
  }
  if (!b.obs) return;
  const T *qp = qpos + E * NQ, *qv = qvel + E * NV;
  T R[9];
  quat_to_R(qp[4], qp[5], qp[6], qp[3], R);   // wxyz storage
  T *o = b.obs + E * b.obs_ld;
  if (lane < 3) {
    const T g = lane == 0 ? R[6] : lane == 1 ? R[7] : R[8], r0 = lane == 0 ? R[0] : lane == 1 ? R[1] : R[2],
            r1 = lane == 0 ? R[3] : lane == 1 ? R[4] : R[5];
    if constexpr (DR) {   // noise on the observation columns only; an amplitude of 0 adds nothing
      const unsigned long long ctr = ((unsigned long long)ep_now << 32) | (unsigned long long)len_now;
      T w = qv[3 + lane], pg = -g;
      if (d.noise_ang_vel != 0) w += pol_noise<T>(d, d.noise_ang_vel, DR_S_OBS, lane, ge, ctr);
      if (d.noise_gravity != 0) pg += pol_noise<T>(d, d.noise_gravity, DR_S_OBS, 3 + lane, ge, ctr);
      o[lane] = w;
      o[3 + lane] = pg;
    } else {
      o[lane] = qv[3 + lane];                    // base angular velocity: body frame as stored
      o[3 + lane] = -g;                          // R^T (0, 0, -1)
    }
    o[6 + lane] = cmd;
    o[POL_NOBS + lane] = r0 * qv[0] + r1 * qv[1] + g * qv[2];   // privileged: R^T v
  }
  if (lane < NA) {
    const int dof = m.mj_act_dof[lane];
    if constexpr (DR) {
      const unsigned long long ctr = ((unsigned long long)ep_now << 32) | (unsigned long long)len_now;
      T jp = qp[dof + 1] - c.def[lane], jv = qv[dof];
      if (d.noise_joint_pos != 0) jp += pol_noise<T>(d, d.noise_joint_pos, DR_S_OBS, 9 + lane, ge, ctr);
      if (d.noise_joint_vel != 0) jv += pol_noise<T>(d, d.noise_joint_vel, DR_S_OBS, 9 + NA + lane, ge, ctr);
      o[9 + lane] = jp;
      o[9 + NA + lane] = jv;
    } else {
      o[9 + lane] = qp[dof + 1] - c.def[lane];
      o[9 + NA + lane] = qv[dof];
    }
    o[9 + 2 * NA + lane] = last;
  }
  if (lane < 2) o[9 + 3 * NA + lane] = (con >> lane) & 1 ? T(1) : T(0);
  if (lane == 3) o[POL_NOBS + 3] = qp[2];
}

// ---------------------------------------------------------------------------- push of this policy step (before the sim steps)
// lanes 0 .. 2 write the torso force xfrc[e, 0, 0:3]; every other element of xfrc stays the caller's
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_perturb(int n, PolicyBufs<T> b, PolicyDR d, T *xfrc) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= 3) return;
  const size_t E = (size_t)e;
  const unsigned long long ge = d.env_offset + (unsigned long long)e, ep = (unsigned long long)b.episode[E];
  const int len = b.ep_len[E];   // (policy steps completed in the episode)
  const int phase = (int)(pol_draw(d, DR_S_PUSH_PHASE, 0, ge, ep) * (double)d.push_interval);   // floor: the product is >= 0
  double f = 0;
  if (len >= phase && (len - phase) % d.push_interval < d.push_duration) {
    const unsigned long long ctr = (ep << 32) | (unsigned long long)((len - phase) / d.push_interval);
    const double mag = d.force_lo + (d.force_hi - d.force_lo) * pol_draw(d, DR_S_PUSH_MAG, 0, ge, ctr);
    const double az = 6.283185307179586 * pol_draw(d, DR_S_PUSH_DIR, 0, ge, ctr);
    f = lane == 0 ? mag * cos(az) : lane == 1 ? mag * sin(az) : 0.0;
  }
  xfrc[E * NB * 6 + lane] = (T)f;
}

// ---------------------------------------------------------------------------- reset noise (after the reset, before k_policy_obs)
// the sim state of the envs just reset; the TSID state q, v stays as the reset wrote it (the policy environment runs no tick)
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_reset_noise(const DevModel<T> *__restrict__ mp, int n, PolicyBufs<T> b, PolicyDR d,
                                                                                  const T *__restrict__ done_rows, int rows_ld, T *qpos, T *qvel) {
  const DevModel<T> &m = *mp;
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  if (done_rows[E * rows_ld + NROW - 1] == T(0)) return;
  T *qp = qpos + E * NQ, *qv = qvel + E * NV;
  const unsigned long long ge = d.env_offset + (unsigned long long)e, ep = (unsigned long long)(b.episode[E] + 1);   // (the episode about to start)
  // the yawed quaternion, every lane the same values (read before any lane writes)
  T w = qp[3], x = qp[4], y = qp[5], z = qp[6];
  if (d.reset_yaw != 0) {
    const double th = d.reset_yaw * (2.0 * pol_draw(d, DR_S_YAW, 0, ge, ep) - 1.0);
    const T ch = (T)cos(0.5 * th), sh = (T)sin(0.5 * th);
    const T w1 = ch * w - sh * z, x1 = ch * x - sh * y, y1 = ch * y + sh * x, z1 = ch * z + sh * w;
    const T nrm = sqrt(w1 * w1 + x1 * x1 + y1 * y1 + z1 * z1);
    w = w1 / nrm; x = x1 / nrm; y = y1 / nrm; z = z1 / nrm;
  }
  if (lane < NA) {
    const int dof = m.mj_act_dof[lane];
    if (d.reset_joint_pos != 0) qp[dof + 1] += pol_noise<T>(d, d.reset_joint_pos, DR_S_JOINT_POS, lane, ge, ep);
    if (d.reset_joint_vel != 0) qv[dof] += pol_noise<T>(d, d.reset_joint_vel, DR_S_JOINT_VEL, lane, ge, ep);
  }
  if (lane < 3) {
    if (d.reset_lin[lane] != 0) qv[lane] += pol_noise<T>(d, d.reset_lin[lane], DR_S_LIN_VEL, lane, ge, ep);
    if (d.reset_ang[lane] != 0) qv[3 + lane] += pol_noise<T>(d, d.reset_ang[lane], DR_S_ANG_VEL, lane, ge, ep);
    if (lane < 2) { if (d.reset_xy != 0) qp[lane] += pol_noise<T>(d, d.reset_xy, DR_S_XY, lane, ge, ep); }
    else if (d.reset_lift != 0) qp[2] += (T)d.reset_lift;
  }
  if (d.reset_yaw != 0 && lane >= 3 && lane < 7) qp[lane] = lane == 3 ? w : lane == 4 ? x : lane == 5 ? y : z;
}

// ---------------------------------------------------------------------------- per-episode terrain and dynamics, height scan
// tsidb_policy_terrain_config's values, passed to the kernels by value.  float64 whatever the path's type, as PolicyDR
struct PolicyTer {
  unsigned long long seed, env_offset;
  double mass_lo, mass_hi, fric_lo, fric_hi, tilt_max, height_lo, height_hi, length_lo, length_hi, step_prob;
  int flat_cells, num_levels, nx, ny;
  double x0, x1, y0, y1, clip_lo, clip_hi, noise;
};
enum { TER_S_MASS = 12, TER_S_FRICTION, TER_S_TILT, TER_S_AZIMUTH, TER_S_DIRECTION, TER_S_LENGTH, TER_S_RAISED, TER_S_HEIGHT, TER_S_SCAN };
constexpr int POL_MAXSCAN = 256;   // TSIDB_POL_MAXSCAN

// after the reset and its noise, before k_policy_obs: the rows of the two sim tables (tsidb_set_env_params) of the envs just
// reset.  lane = column of the row: lanes 0 .. 7 store env_params[e], lanes 0 .. 19 terrain[e].  The seven draws every column
// needs one or two of are formed on every lane (a hash each) - no cross-lane traffic; everything in float64, cast when stored
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_terrain_reset(int n, PolicyBufs<T> b, PolicyTer d, const T *__restrict__ done_rows,
                                                                                    int rows_ld, const T *__restrict__ qpos,
                                                                                    const int *__restrict__ level, T *env_params, T *terrain) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= 20) return;
  const size_t E = (size_t)e;
  if (done_rows[E * rows_ld + NROW - 1] == T(0)) return;
  const unsigned long long ge = d.env_offset + (unsigned long long)e, ep = (unsigned long long)(b.episode[E] + 1);   // (the episode about to start)
  const double xb = (double)qpos[E * NQ], yb = (double)qpos[E * NQ + 1];
  int lvl = level ? level[E] : d.num_levels - 1;
  lvl = lvl < 0 ? 0 : lvl > d.num_levels - 1 ? d.num_levels - 1 : lvl;
  const double two_pi = 6.283185307179586;
  const double mass = d.mass_lo + (d.mass_hi - d.mass_lo) * pol_draw(d.seed, TER_S_MASS, 0, ge, ep);
  const double fric = d.fric_lo + (d.fric_hi - d.fric_lo) * pol_draw(d.seed, TER_S_FRICTION, 0, ge, ep);
  const double t = d.tilt_max * pol_draw(d.seed, TER_S_TILT, 0, ge, ep), a = two_pi * pol_draw(d.seed, TER_S_AZIMUTH, 0, ge, ep);
  const double g = two_pi * pol_draw(d.seed, TER_S_DIRECTION, 0, ge, ep);
  const double len = d.length_lo + (d.length_hi - d.length_lo) * pol_draw(d.seed, TER_S_LENGTH, 0, ge, ep);
  const double H = (d.height_lo + (d.height_hi - d.height_lo) * pol_draw(d.seed, TER_S_HEIGHT, 0, ge, ep)) * (double)(lvl + 1) / (double)d.num_levels;
  const double st = sin(t), nx = st * cos(a), ny = st * sin(a), nz = cos(t), cg = cos(g), sg = sin(g);
  if (lane < 8) {
    const double v = lane == 0 ? mass : lane == 1 ? fric : lane == 2 ? nx : lane == 3 ? ny : lane == 4 ? nz : lane == 5 ? nx * xb + ny * yb : 0.0;
    env_params[E * 8 + lane] = (T)v;
  }
  double v;
  if (lane < 4) v = lane == 0 ? cg : lane == 1 ? sg : lane == 2 ? cg * xb + sg * yb - 0.5 * len : 1.0 / len;
  else {
    const int c = lane - 4;
    const bool raised = pol_draw(d.seed, TER_S_RAISED, c, ge, ep) < d.step_prob;
    v = raised && c > d.flat_cells && c < 16 - d.flat_cells ? H : 0.0;
  }
  terrain[E * 20 + lane] = (T)v;
}

// after k_policy_obs: the height of the base above the floor surface at the nx * ny points of a grid in the heading frame.
// lane = point (points 64 apart share a lane: a row store is coalesced); the env's rows of the two tables sit behind
// wave-uniform addresses that nothing in this kernel writes: scalar loads.  envp / terr NULL = the nominal floor
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_height_scan(int n, PolicyBufs<T> b, PolicyTer d, const T *__restrict__ qpos,
                                                                                  const T *__restrict__ envp_g, const T *__restrict__ terr_g, T *scan,
                                                                                  int scan_ld) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  const int np = d.nx * d.ny;
  const T *qp = qpos + E * NQ, *envp = envp_g ? envp_g + E * 8 : nullptr, *terr = terr_g ? terr_g + E * 20 : nullptr;
  const T fnx = envp ? envp[2] : T(0), fny = envp ? envp[3] : T(0), fnz = envp ? envp[4] : T(1), fd = envp ? envp[5] : T(0);
  const T xb = qp[0], yb = qp[1], zb = qp[2], qw = qp[3], qx = qp[4], qy = qp[5], qz = qp[6];
  T hx = 1 - 2 * (qy * qy + qz * qz), hy = 2 * (qw * qz + qx * qy);
  const T h2 = hx * hx + hy * hy;
  if (h2 < T(1e-12)) { hx = 1; hy = 0; }
  else { const T hn = sqrt(h2); hx /= hn; hy /= hn; }
  const T lo = (T)d.clip_lo, hi = (T)d.clip_hi;
  const unsigned long long ge = d.env_offset + (unsigned long long)e;
  const unsigned long long ctr = ((unsigned long long)b.episode[E] << 32) | (unsigned long long)b.ep_len[E];
  for (int p = lane; p < np; p += WAVE) {
    const int ix = p / d.ny, iy = p - ix * d.ny;
    const T px = (T)(d.nx > 1 ? d.x0 + (d.x1 - d.x0) * (double)ix / (double)(d.nx - 1) : d.x0);
    const T py = (T)(d.ny > 1 ? d.y0 + (d.y1 - d.y0) * (double)iy / (double)(d.ny - 1) : d.y0);
    const T X = xb + (hx * px - hy * py), Y = yb + (hy * px + hx * py);
    const T hs = terr ? terrain_h(terr, X, Y) : T(0);
    const T zs = (fd + hs - fnx * X - fny * Y) / fnz;
    T v = zb - zs;
    v = v < lo ? lo : v > hi ? hi : v;   // (NaN passes)
    if (d.noise != 0) v += (T)(d.noise * (2.0 * pol_draw(d.seed, TER_S_SCAN, p & 255, ge, ctr) - 1.0));
    scan[E * scan_ld + p] = v;
  }
}

// ---------------------------------------------------------------------------- TSID in the loop: the teacher
constexpr int POL_TEACH_NT = 4;           // teacher terms (TSIDB_POL_TEACH_NT)
constexpr int POL_TEACH_NOBS = 14 + NA;   // columns of the teacher observation (TSIDB_POL_TEACH_NOBS for the v1 robot)
constexpr int ROW_COM = NQ + NV, ROW_LF = NQ + NV + 6, ROW_RF = NQ + NV + 9;   // the tick's row: q v com cop LF RF
enum { POL_TT_TRACK_COM = 0, POL_TT_TRACK_FEET, POL_TT_CONTACT_MATCH, POL_TT_DEVIATION };

// tsidb_policy_teacher_config's values and what the teacher needs of tsidb_policy_config's; ctrl_mode is tsidb_set_ctrl's.
// float64 whatever the path's type: the teacher's arithmetic runs in float64 on the path's buffers and is cast once when it is
// stored (include/tsidb.h) - a dozen scalar operations per env, and the float32 path's reward is rounded once instead of six times
struct PolicyTeach {
  double sigma_com, sigma_foot, w[POL_TEACH_NT], w_termination, clip, scale[NA], def[NA];
  int ctrl_mode;
};

// the registered references the two kernels read (tsidb_set_refs)
template <typename T>
struct PolicyRefs {
  const T *com_ref, *foot_ref;
  const uint8_t *contact_active;
};

// after k_policy_reward, before k_reset: the teacher terms into the reward, a failed QP into done, TSID's command as an action.
// Lanes 0 .. 8 hold one component each of com - com_ref, LF - foot_ref[0].p, RF - foot_ref[1].p; lane a < NA actuator a.
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_teacher(const DevModel<T> *__restrict__ mp, int n, PolicyCfg<T> c, PolicyTeach tc,
                                                                              PolicyBufs<T> b, PolicyRefs<T> r, T *rows, int rows_ld,
                                                                              const T *__restrict__ q, const T *__restrict__ tau,
                                                                              const int *__restrict__ status, const int *__restrict__ ncon,
                                                                              const int *__restrict__ con_pairs, const T *__restrict__ ctrl,
                                                                              T *teacher_terms, T *teacher_action) {
  const DevModel<T> &m = *mp;
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  T *row = rows + E * rows_ld;
  double ec = 0, ef = 0, dev = 0;
  if (lane < 9) {
    const int g = lane / 3, k = lane - 3 * g;
    const double have = row[g == 0 ? ROW_COM + k : g == 1 ? ROW_LF + k : ROW_RF + k];
    const double want = g == 0 ? r.com_ref[E * 9 + k] : r.foot_ref[(E * 2 + (g - 1)) * 24 + k];
    const double d = have - want;
    if (g == 0) ec = d * d; else ef = d * d;
  }
  if (lane < NA) {
    const int qi = m.mj_ctrl_qidx[lane];
    const double u = ctrl[E * NA + lane], ta = tau[E * NA + qi - 7];
    const double x = tc.ctrl_mode == CTRL_RESIDUAL ? u : tc.ctrl_mode == CTRL_MOTOR ? u - ta : 0.0;
    dev = x * x;
    double act = 0;
    if (tc.ctrl_mode != CTRL_RESIDUAL && tc.scale[lane] != 0) {
      const double cmd = tc.ctrl_mode == CTRL_MOTOR ? ta : (double)q[E * NQ + qi];
      const double a = (cmd - tc.def[lane]) / tc.scale[lane];
      act = a > tc.clip ? tc.clip : a < -tc.clip ? -tc.clip : a;
    }
    teacher_action[E * NA + lane] = (T)act;
  }
  wave_sum3(ec, ef, dev);
  const int con = pol_contacts(m, c, ncon, con_pairs, E, lane);
  const int a0 = r.contact_active[E * 2] != 0, a1 = r.contact_active[E * 2 + 1] != 0;
  double t[POL_TEACH_NT];
  t[POL_TT_TRACK_COM] = exp(-ec / (tc.sigma_com * tc.sigma_com));
  t[POL_TT_TRACK_FEET] = exp(-ef / (tc.sigma_foot * tc.sigma_foot));
  t[POL_TT_CONTACT_MATCH] = (double)(((con & 1) == a0) + (((con >> 1) & 1) == a1));
  t[POL_TT_DEVIATION] = dev;
  double add = 0, mine = 0;
#pragma unroll
  for (int k = 0; k < POL_TEACH_NT; k++) {
    add += tc.w[k] * t[k];
    mine = lane == k ? t[k] : mine;
  }
  if (lane < POL_TEACH_NT) teacher_terms[E * POL_TEACH_NT + lane] = (T)mine;
  if (lane == 0) {
    double rew = (double)row[NROW - 2] + add;
    if (status[E] != 0) {   // TSID's QP failed: terminated, whatever k_policy_reward decided
      if (b.terms[E * POL_NT + POL_T_TERMINATION] == T(0)) rew += tc.w_termination;
      b.terms[E * POL_NT + POL_T_TERMINATION] = 1;
      b.timeout[E] = 0;
      row[NROW - 1] = 1;
    }
    row[NROW - 2] = (T)rew;
  }
}

// after k_policy_obs: the controller's references as the policy sees them, in the base frame of the sim state.  Lanes 0 .. 11
// hold one component each of the four vectors; lane a < NA the actuator's tau
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_teacher_obs(const DevModel<T> *__restrict__ mp, int n, PolicyRefs<T> r,
                                                                                  const T *__restrict__ rows, int rows_ld, const T *__restrict__ qpos,
                                                                                  const T *__restrict__ tau, T *out, int out_ld) {
  const DevModel<T> &m = *mp;
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0) return;
  const size_t E = (size_t)e;
  const T *row = rows + E * rows_ld, *qp = qpos + E * NQ;
  const bool fresh = row[NROW - 1] != T(0);
  T *o = out + E * out_ld;
  if (lane < 2) o[lane] = r.contact_active[E * 2 + lane] ? T(1) : T(0);
  if (lane < 12) {
    const int g = lane / 3, k = lane - 3 * g;   // 0 com error, 1 com velocity, 2 LF error, 3 RF error
    T R[9], w[3];
    quat_to_R(qp[4], qp[5], qp[6], qp[3], R);   // wxyz storage
#pragma unroll
    for (int j = 0; j < 3; j++)
      w[j] = g == 0 ? r.com_ref[E * 9 + j] - row[ROW_COM + j] : g == 1 ? r.com_ref[E * 9 + 3 + j]
           : g == 2 ? r.foot_ref[E * 48 + j] - row[ROW_LF + j] : r.foot_ref[E * 48 + 24 + j] - row[ROW_RF + j];
    const T v = R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2];   // R^T w
    o[2 + lane] = fresh && g != 1 ? T(0) : v;
  }
  if (lane < NA) o[14 + lane] = fresh ? T(0) : tau[E * NA + m.mj_ctrl_qidx[lane] - 7];
}

// ---------------------------------------------------------------------------- imitation: the teacher's label, DAgger's mixing
constexpr int DR_S_TEACHER_MIX = 23;   // stream 23 of the key layout (21 / 22: the action noise, tsidb_actor.hpp)

// after the actor launch, before k_policy_act: the label of the row the actor has just stored, and - for the episodes the draw
// hands to the teacher - the teacher's action in place of the policy's.  teacher_action is what k_policy_teacher left at the end
// of the previous step: formed on the state one sim step before the observation the actor saw.  ep_len == 0: the previous step
// (or reset()) restarted the env, the label belongs to the fallen robot or to nothing - weight 0, never executed.  Lane a < NA
// holds actuator a; U is the same on every lane (a hash of wave-uniform values).  action may be NULL (labels alone).
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_teacher_mix(int n, PolicyBufs<T> b, const T *__restrict__ teacher_action, T *action,
                                                                                  float *label, float *weight, int *executed,
                                                                                  const float *__restrict__ beta, unsigned long long seed,
                                                                                  unsigned long long env_offset) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= NA) return;
  const size_t E = (size_t)e, row = E * NA + lane;
  const bool live = b.ep_len[E] > 0;
  const double u = pol_draw(seed, DR_S_TEACHER_MIX, 0, env_offset + (unsigned long long)e, (unsigned long long)b.episode[E] << 32);
  const bool exec = live && beta && u < (double)beta[0];
  const T ta = teacher_action[row];
  label[row] = (float)ta;
  if (exec && action) action[row] = ta;
  if (lane == 0) {
    weight[E] = live ? 1.f : 0.f;
    executed[E] = exec ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------- episode statistics, terrain curriculum
enum { POL_EP_COUNT = 0, POL_EP_TIMEOUT, POL_EP_LENGTH, POL_EP_RETURN, POL_EP_DISPLACEMENT, POL_EP_LEVEL, POL_EP_TERMS,
       POL_EP_TEACH = POL_EP_TERMS + POL_NT, POL_EP_NREC = POL_EP_TEACH + POL_TEACH_NT };   // TSIDB_POL_EP_*
constexpr int DR_S_CURRICULUM = 24;   // stream 24 of the key layout: the level of an env that graduates from the top

// tsidb_policy_episode in the path's arithmetic type: the statistics are float64 on either path
template <typename T>
struct PolicyEpisode {
  double *run, *start_xy, *last, *sum;
  int *level;
  const T *teacher_terms;
};

// tsidb_policy_episode_config's values and what the curriculum needs of the two other configurations, passed by value
struct PolicyCur {
  unsigned long long seed, env_offset;   // the terrain's
  double up_distance, down_fraction, t_episode /* max_episode_steps * (decimation * dt) */;
  int curriculum, random_top, num_levels /* 0: no terrain configured */;
};

// x where it is finite, else 0: a select, so that a NaN adds nothing (0 * NaN would)
__device__ __forceinline__ double pol_finite(double x) { return isfinite(x) ? x : 0.0; }

// after k_policy_reward (and k_policy_teacher), before k_reset.  lane = column of the record: every lane adds its column's addend
// of this step to the running sums; for a done env it then forms its column of the record, stores it to `last` and adds it to
// `sum`.  The displacement, the level and the curriculum's rule are formed on every lane from wave-uniform values (a hash, a
// square root); lane 0 stores the new level - after every lane of the wavefront has read the old one.
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_episode_end(int n, PolicyBufs<T> b, PolicyEpisode<T> ep, PolicyCur c,
                                                                                  const T *__restrict__ qpos, const T *__restrict__ reward,
                                                                                  const T *__restrict__ done, int row_ld) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= POL_EP_NREC) return;
  const size_t E = (size_t)e, at = E * POL_EP_NREC + lane;
  const bool summed = lane == POL_EP_LENGTH || lane == POL_EP_RETURN || lane >= POL_EP_TERMS;
  double run = 0;
  if (summed) {
    double add = 1.0;   // LENGTH
    if (lane == POL_EP_RETURN) add = (double)reward[E * row_ld];
    else if (lane >= POL_EP_TEACH) add = ep.teacher_terms ? (double)ep.teacher_terms[E * POL_TEACH_NT + (lane - POL_EP_TEACH)] : 0.0;
    else if (lane >= POL_EP_TERMS) add = (double)b.terms[E * POL_NT + (lane - POL_EP_TERMS)];
    run = ep.run[at] + pol_finite(add);
    ep.run[at] = run;
  }
  if (done[E * row_ld] == T(0)) return;
  const double dx = (double)qpos[E * NQ] - ep.start_xy[E * 2], dy = (double)qpos[E * NQ + 1] - ep.start_xy[E * 2 + 1];
  const double d = sqrt(dx * dx + dy * dy);
  int lvl = ep.level ? ep.level[E] : 0;
  lvl = lvl < 0 ? 0 : c.num_levels > 0 && lvl > c.num_levels - 1 ? c.num_levels - 1 : lvl;
  const double rec = lane == POL_EP_COUNT ? 1.0 : lane == POL_EP_TIMEOUT ? (b.timeout[E] ? 1.0 : 0.0) : lane == POL_EP_LENGTH ? (double)b.ep_len[E]
                   : lane == POL_EP_DISPLACEMENT ? d : lane == POL_EP_LEVEL ? (double)lvl : run;
  ep.last[at] = rec;
  ep.sum[at] += lane == POL_EP_RETURN || lane == POL_EP_DISPLACEMENT ? pol_finite(rec) : rec;
  if (c.curriculum) {
    const double cx = (double)b.command[E * 3], cy = (double)b.command[E * 3 + 1];
    const bool up = d > c.up_distance, down = !up && d < c.down_fraction * sqrt(cx * cx + cy * cy) * c.t_episode;   // (NaN d: neither)
    int next = lvl + (up ? 1 : 0) - (down ? 1 : 0);
    if (next < 0) next = 0;
    else if (next >= c.num_levels) {
      next = c.num_levels - 1;
      if (c.random_top) {
        const unsigned long long ge = c.env_offset + (unsigned long long)e, epn = (unsigned long long)(b.episode[E] + 1);   // (the episode about to start)
        const int r = (int)(pol_draw(c.seed, DR_S_CURRICULUM, 0, ge, epn) * (double)c.num_levels);   // floor: the product is >= 0
        next = r < next ? r : next;
      }
    }
    if (lane == 0) ep.level[E] = next;
  }
}

// after k_reset, the reset noise and the terrain's redraw: the first position of the episodes that start, their sums zeroed
template <typename T>
__global__ __launch_bounds__(WAVE * POL_ENVS_PER_BLOCK) void k_policy_episode_begin(int n, PolicyEpisode<T> ep, const T *__restrict__ done_rows, int rows_ld,
                                                                                    const T *__restrict__ qpos) {
  const int e = pol_env(n), lane = threadIdx.x & 63;
  if (e < 0 || lane >= POL_EP_NREC) return;
  const size_t E = (size_t)e;
  if (done_rows[E * rows_ld + NROW - 1] == T(0)) return;
  ep.run[E * POL_EP_NREC + lane] = 0;
  if (lane < 2) ep.start_xy[E * 2 + lane] = (double)qpos[E * NQ + lane];
}

} // namespace tsidb
