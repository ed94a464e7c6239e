// The acting frame of the one-workgroup kernels that write one cart-pole's transitions straight into a replay ring (dqn_mlp.hip,
// dist_mlp.hip, rainbow_mlp.hip: dra_dqn_mlp_act_io), stated ONCE: the launch's bounds, the scratch behind a kernel's weights, the
// environment lane with the ring cursor (ReplayActor) and the host check of the io struct.  Each kernel keeps its weights, its
// heads and its barriers; what met the register bar in this form, and what did not, is in mlp_rollout.h's banner.
#pragma once
#include "cartpole_rollout.h"

namespace {

constexpr int kMaxK = 8;         // transitions of one launch
constexpr int kNP = 8;           // row stride of the single environment's transposed activations (hidden_layer's row block)

// the acting scratch behind a kernel's weights: q [A] (+ pad), x^T [S][NP], h1^T [H][NP], h2^T [H][NP]
__host__ __device__ constexpr int act_scratch_floats(int H) { return 4 + kS * kNP + 2 * H * kNP; }
template <int H>
struct ActScratch {
  float *q, *xT, *h1T, *h2T;
  __device__ explicit ActScratch(float* base) : q(base), xT(q + 4), h1T(xT + kS * kNP), h2T(h1T + H * kNP) {}
  __device__ __forceinline__ void zero(int tid) const {
    for (int i = tid; i < act_scratch_floats(H); i += 256) q[i] = 0.f;      // (rows 1..7 of x^T stay zero: one environment)
  }
};

// the episode ring's row of a kernel whose transitions go to the replay ring
__device__ __forceinline__ CartPoleRow episode_row(const dra_dqn_mlp_act_io& io) {
  EpisodeRow ep;
  ep.ep_ring = io.ep_ring;
  ep.horizon = io.horizon;
  ep.ring_cap = io.ring_cap;
  return CartPoleRow(ep);
}

struct ReplayActor {
  CartPoleLanes lanes;                               // lane 0 of wave 0 carries the environment
  int64_t t0, cap, slot0;
  bool bad_slot;

  __device__ __forceinline__ void begin(const dra_dqn_mlp_act_io& io, int tid) {
    t0 = *io.step_counter;                            // (rewritten by thread 0 behind the last barrier)
    cap = io.capacity;
    slot0 = *io.slot0;
    bad_slot = slot0 < 0 || slot0 >= cap;
    if (bad_slot) slot0 = 0;
    lanes.load(io, tid);
  }

  // thread 0: the observation narrowed to float32 (what tensor() uploads) into row 0 of x^T
  __device__ __forceinline__ void observe(float* xT, int NP, int tid) const {
    if (tid == 0) {
      xT[0 * NP] = (float)lanes.st.x;
      xT[1 * NP] = (float)lanes.st.xd;
      xT[2 * NP] = (float)lanes.st.th;
      xT[3 * NP] = (float)lanes.st.thd;
    }
  }

  // ---- epsilon-greedy action (torch_utils.py:51-58 with the draws made ahead), the ring row, environment step: wave 0
  __device__ __forceinline__ void step(const dra_dqn_mlp_act_io& io, const CartPoleRow& row, const float* sQ, double reward, int k,
                                       int tid) {
    if (tid < 64) {
      bool done = false;
      double ended = 0.0;
      if (tid == 0) {
        int arg = sQ[1] > sQ[0] ? 1 : 0;                          // np.argmax: the first maximum
        if (io.explore[k]) arg = io.random_action[k] == 1 ? 1 : 0;
        const int64_t slot = (slot0 + k) % cap;
        double* frame = io.ring_frames + slot * kS;               // the observation the action was chosen on
        frame[0] = lanes.st.x;
        frame[1] = lanes.st.xd;
        frame[2] = lanes.st.th;
        frame[3] = lanes.st.thd;
        done = cartpole_step(lanes.st, lanes.counter, lanes.ep_steps, lanes.ep_return, lanes.seed, arg, io.horizon, ended);
        io.ring_actions[slot] = arg;
        io.ring_rewards[slot] = reward;
        io.ring_masks[slot] = done ? 0 : 1;
        io.out_action[k] = arg;
      }
      lanes.append(row, done, ended, t0 + k, 0, tid);
    }
  }

  // behind the last barrier: the environment's arrays, the step counter, the error word
  __device__ __forceinline__ void finish(const dra_dqn_mlp_act_io& io, int K, int tid) const {
    lanes.store(io, tid);
    if (tid == 0) {
      *io.step_counter = t0 + K;
      if (bad_slot) *io.err = *io.err + 1;
    }
  }
};

// ---- host side: what every dra_*_act entry asks of its io struct
inline bool replay_act_io_ok(const dra_dqn_mlp_act_io* io) {
  if (io->n_env != 1 || io->horizon < 1 || io->ring_cap < 1 || io->capacity < 1) return false;
  return io->env_state && io->env_counter && io->ep_steps && io->ep_return && io->env_seed && io->step_counter && io->ep_count &&
         io->ep_ring && io->explore && io->random_action && io->slot0 && io->ring_frames && io->ring_actions && io->ring_rewards &&
         io->ring_masks && io->out_q && io->out_action && io->err;
}

}  // namespace
