// Torque-limited pendulum swing-up (the published equations with the constants of gym's Pendulum-v0: g 10, m = l = 1, dt 0.05,
// |theta'| <= 8, no terminal state but the step limit) stated ONCE for host and device.  deeprl_amd/envs.py Pendulum is the host
// statement of the same function, bit for bit: fp64, one rounding per written operation (the library is built with
// -ffp-contract=off), no libm trigonometry: sine and cosine are cartpole_env.h's fixed polynomials at theta / 8 followed by three
// double-angle steps.  theta is KEPT wrapped to [-pi, pi).  Parity with gym's own pendulum is not pinned: DESIGN.md 4.12.
//
//   u = 2 clip(a, -1, 1);  reward = -((th th + 0.1 (thd thd)) + 0.001 (u u))              (state and torque BEFORE the step)
//   thd = thd + (15 sin th + 3 u) 0.05;  th = th + thd 0.05  (the NEW, unclipped velocity);  thd = clip(thd, -8, 8);  wrap th
//   done = episode steps >= horizon
//   reset (DummyVecEnv's auto reset on done too): th = -pi + 2 pi U(3, c, 0), thd = -1 + 2 U(3, c, 1), c = the total step counter
//   observation = [cos th, sin th, thd]
#pragma once
#include "cartpole_env.h"

constexpr double kPendulumPi = 3.141592653589793, kPendulumTwoPi = 6.283185307179586, kPendulumMaxSpeed = 8.0;
constexpr int kPendulumS = 3, kPendulumA = 1, kPendulumVars = 2;

struct PendulumState {
  double th, thd;
};

// within 4e-15 of libm for th in [-pi, pi] (|th / 8| <= 0.393: inside the polynomials' range)
__host__ __device__ inline void pendulum_sincos(double th, double& s, double& c) {
  const double h = th * 0.125;
  s = cartpole_psin(h);
  c = cartpole_pcos(h);
  for (int i = 0; i < 3; ++i) {
    const double t = 2.0 * s;
    const double s2 = t * c, c2 = 1.0 - t * s;
    s = s2;
    c = c2;
  }
}
__host__ __device__ inline void pendulum_observe(const PendulumState& st, double* obs) {
  double s, c;
  pendulum_sincos(st.th, s, c);
  obs[0] = c;
  obs[1] = s;
  obs[2] = st.thd;
}
__host__ __device__ inline void pendulum_reset(PendulumState& st, uint64_t seed, int64_t c) {
  st.th = -kPendulumPi + kPendulumTwoPi * cenv_u(seed, 3, c, 0);
  st.thd = -1.0 + 2.0 * cenv_u(seed, 3, c, 1);
}
// the dynamics alone under action a in [-1, 1] (clipped here); returns the reward
__host__ __device__ inline double pendulum_advance(PendulumState& st, double a) {
  a = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
  const double u = 2.0 * a;
  double th = st.th, thd = st.thd;
  const double reward = -(((th * th) + 0.1 * (thd * thd)) + 0.001 * (u * u));
  double sn, cs;
  pendulum_sincos(th, sn, cs);
  thd = thd + (15.0 * sn + 3.0 * u) * 0.05;
  th = th + thd * 0.05;
  thd = thd < -kPendulumMaxSpeed ? -kPendulumMaxSpeed : (thd > kPendulumMaxSpeed ? kPendulumMaxSpeed : thd);
  if (th >= kPendulumPi) th = th - kPendulumTwoPi;
  else if (th < -kPendulumPi) th = th + kPendulumTwoPi;
  st.th = th;
  st.thd = thd;
  return reward;
}

// One environment step with DummyVecEnv's auto reset: counter, episode steps and return advance; on done `ended_return` takes the
// finished episode's return and the environment restarts.  Returns done.
__host__ __device__ inline bool pendulum_step(PendulumState& st, int64_t& counter, int32_t& ep_steps, double& ep_return, uint64_t seed,
                                              double a, int64_t horizon, double& reward, double& ended_return) {
  reward = pendulum_advance(st, a);
  counter = counter + 1;
  ep_steps = ep_steps + 1;
  ep_return = ep_return + reward;
  const bool done = (int64_t)ep_steps >= horizon;
  if (done) {
    ended_return = ep_return;
    pendulum_reset(st, seed, counter);
    ep_steps = 0;
    ep_return = 0.0;
  }
  return done;
}
