// Cart-pole (the published equations of Barto, Sutton & Anderson 1983 with the constants of gym's CartPole-v0: gravity 9.8, cart
// 1.0, pole 0.1, half length 0.5, force 10, tau 0.02, Euler) stated ONCE for host and device.  deeprl_amd/envs.py CartPole is the
// host statement of the same function, bit for bit: fp64, one rounding per written operation (the library is built with
// -ffp-contract=off), sine and cosine as FIXED Horner polynomials -- device ocml and glibc do not agree to the bit, these do.
// Parity with gym's own CartPole (libm trigonometry, its own reset generator) is not pinned: DESIGN.md 4.12.
//
//   force = (a == 1) ? 10 : -10;  c = pcos(th);  s = psin(th)
//   temp  = (force + ((0.05 thd) thd) s) / 1.1
//   thacc = (9.8 s - c temp) / (0.5 (4/3 - ((0.1 c) c) / 1.1));   xacc = temp - ((0.05 thacc) c) / 1.1
//   x += 0.02 xd;  xd += 0.02 xacc;  th += 0.02 thd;  thd += 0.02 thacc          (positions move with the OLD velocities)
//   done = x < -2.4 || x > 2.4 || th < -TH || th > TH || episode steps >= horizon;   reward = 1 on every step
//   reset (DummyVecEnv's auto reset on done too): s_j = cenv_reset_state(seed, c, j), c = the environment's total step counter
#pragma once
#include "cont_env.h"

constexpr double kCartPoleTheta = 0.20943951023931953;      // 12 degrees
constexpr double kCartPoleX = 2.4;
constexpr int kCartPoleS = 4, kCartPoleA = 2;

// sin(th) = th P(th^2), coefficients (-1)^k / (2k + 1)!, k = 0..7: within 1.2e-16 of libm for |th| <= 0.45
__host__ __device__ inline double cartpole_psin(double th) {
  const double z = th * th;
  double p = -7.647163731819816e-13;
  p = 1.6059043836821613e-10 + z * p;
  p = -2.505210838544172e-08 + z * p;
  p = 2.7557319223985893e-06 + z * p;
  p = -0.0001984126984126984 + z * p;
  p = 0.008333333333333333 + z * p;
  p = -0.16666666666666666 + z * p;
  p = 1.0 + z * p;
  return th * p;
}
// cos(th) = Q(th^2), coefficients (-1)^k / (2k)!, k = 0..8
__host__ __device__ inline double cartpole_pcos(double th) {
  const double z = th * th;
  double q = 4.779477332387385e-14;
  q = -1.1470745597729725e-11 + z * q;
  q = 2.08767569878681e-09 + z * q;
  q = -2.755731922398589e-07 + z * q;
  q = 2.48015873015873e-05 + z * q;
  q = -0.001388888888888889 + z * q;
  q = 0.041666666666666664 + z * q;
  q = -0.5 + z * q;
  q = 1.0 + z * q;
  return q;
}

struct CartPoleState {
  double x, xd, th, thd;
};

// the dynamics alone: one Euler step under action a
__host__ __device__ inline void cartpole_advance(CartPoleState& s, int a) {
  const double force = (a == 1) ? 10.0 : -10.0;
  const double c = cartpole_pcos(s.th), sn = cartpole_psin(s.th);
  const double temp = (force + ((0.05 * s.thd) * s.thd) * sn) / 1.1;
  const double thacc = (9.8 * sn - c * temp) / (0.5 * (1.3333333333333333 - ((0.1 * c) * c) / 1.1));
  const double xacc = temp - ((0.05 * thacc) * c) / 1.1;
  s.x = s.x + 0.02 * s.xd;
  s.xd = s.xd + 0.02 * xacc;
  s.th = s.th + 0.02 * s.thd;
  s.thd = s.thd + 0.02 * thacc;
}
__host__ __device__ inline bool cartpole_out(const CartPoleState& s) {
  return s.x < -kCartPoleX || s.x > kCartPoleX || s.th < -kCartPoleTheta || s.th > kCartPoleTheta;
}
__host__ __device__ inline void cartpole_reset(CartPoleState& s, uint64_t seed, int64_t c) {
  s.x = cenv_reset_state(seed, c, 0);
  s.xd = cenv_reset_state(seed, c, 1);
  s.th = cenv_reset_state(seed, c, 2);
  s.thd = cenv_reset_state(seed, c, 3);
}

// One environment step with DummyVecEnv's auto reset: counter, episode steps and return advance; on done `ended_return` takes the
// finished episode's return and the environment restarts.  Returns done; the reward is 1.0 on every step.
__host__ __device__ inline bool cartpole_step(CartPoleState& s, int64_t& counter, int32_t& ep_steps, double& ep_return, uint64_t seed,
                                              int a, int64_t horizon, double& ended_return) {
  cartpole_advance(s, a);
  counter = counter + 1;
  ep_steps = ep_steps + 1;
  ep_return = ep_return + 1.0;
  const bool done = cartpole_out(s) || (int64_t)ep_steps >= horizon;
  if (done) {
    ended_return = ep_return;
    cartpole_reset(s, seed, counter);
    ep_steps = 0;
    ep_return = 0.0;
  }
  return done;
}
