// The evaluation frame of the one-workgroup kernels that run config.eval_episodes greedy episodes of one cart-pole in ONE launch
// (dqn_mlp.hip, dist_mlp.hip, rainbow_mlp.hip: dra_mlp_eval_io), stated ONCE next to replay_act.h's acting frame: the environment
// lane (EvalActor), the LDS word that ends the loop, and the host check of the io struct.  An evaluation is the acting loop with
// epsilon 0 and no ring row (BaseAgent.py:60-77 over DummyVecEnv's auto reset): each kernel keeps its staging, its forward and
// its barriers, written from the acting kernel's blocks; the acting kernels themselves stay as they are (mlp_rollout.h's banner).
//
// The uniform exit: the loop is `for (k = 0; k < n_episodes * horizon; ++k)`; an episode ends at `horizon` at the latest, so the
// bound is exact and the launch cannot spin.  Thread 0 publishes the count of finished episodes into ONE LDS word inside step(),
// every thread reads that word behind the barrier that follows and leaves -- or stays -- with all the others: no thread skips a
// barrier another thread waits at.  The word is rewritten four barriers later at the earliest (the next step's step()).
#pragma once
#include "replay_act.h"

namespace {

constexpr int kMaxEvalEpisodes = 256;
constexpr int64_t kMaxEvalSteps = 65536;      // n_episodes * horizon: a few tenths of a second at the acting kernels' pace

struct EvalActor {
  ReplayActor a;                                     // its lanes (lane 0 of wave 0 carries the environment) and observe(), unchanged
  int32_t finished = 0;                              // episodes that have ended (thread 0)
  int64_t steps = 0;                                 // environment steps taken (thread 0)

  // the environment's words, then what Task.reset() does: a reset at the current counter, episode steps 0, return 0
  __device__ __forceinline__ void begin(const dra_mlp_eval_io& io, int tid) {
    if (tid == 0) {
      CartPoleLanes& l = a.lanes;
      l.st.x = io.env_state[0];
      l.st.xd = io.env_state[1];
      l.st.th = io.env_state[2];
      l.st.thd = io.env_state[3];
      l.counter = io.env_counter[0];
      l.ep_steps = io.ep_steps[0];
      l.ep_return = io.ep_return[0];
      l.seed = (uint64_t)io.env_seed[0];
      cartpole_reset(l.st, l.seed, l.counter);
      l.ep_steps = 0;
      l.ep_return = 0.0;
    }
  }

  __device__ __forceinline__ void observe(float* xT, int NP, int tid) const { a.observe(xT, NP, tid); }

  // thread 0: the first maximum, the environment step with its auto reset, on done the episode's return and length; the count of
  // finished episodes into *done_word
  __device__ __forceinline__ void step(const dra_mlp_eval_io& io, const float* sQ, int* done_word, int tid) {
    if (tid == 0) {
      CartPoleLanes& l = a.lanes;
      const int arg = sQ[1] > sQ[0] ? 1 : 0;                      // np.argmax: the first maximum
      const int32_t length = l.ep_steps + 1;                      // (cartpole_step zeroes ep_steps on done)
      double ended = 0.0;
      const bool done = cartpole_step(l.st, l.counter, l.ep_steps, l.ep_return, l.seed, arg, io.horizon, ended);
      steps = steps + 1;
      if (done) {
        io.out_return[finished] = ended;
        io.out_length[finished] = length;
        finished = finished + 1;
      }
      *done_word = finished;
    }
  }

  // behind the last barrier: the environment's words and the number of steps taken
  __device__ __forceinline__ void finish(const dra_mlp_eval_io& io, int tid) const {
    if (tid == 0) {
      const CartPoleLanes& l = a.lanes;
      io.env_state[0] = l.st.x;
      io.env_state[1] = l.st.xd;
      io.env_state[2] = l.st.th;
      io.env_state[3] = l.st.thd;
      io.env_counter[0] = l.counter;
      io.ep_steps[0] = l.ep_steps;
      io.ep_return[0] = l.ep_return;
      io.out_steps[0] = steps;
    }
  }
};

// the word thread 0 publishes the finished episodes in: the pad behind q [A] in the acting scratch (zeroed with it)
template <int H>
__device__ __forceinline__ int* eval_done_word(const ActScratch<H>& s) {
  static_assert(kA + 1 <= 4, "q's pad holds the word");
  return reinterpret_cast<int*>(s.q + kA);
}

// ---- host side
inline int mlp_eval_supported(int64_t n_episodes, int64_t horizon) {
  if (n_episodes < 1 || n_episodes > kMaxEvalEpisodes || horizon < 1 || horizon > kMaxEvalSteps) return DRA_EINVAL;
  return n_episodes * horizon > kMaxEvalSteps ? DRA_EINVAL : DRA_OK;
}

inline bool mlp_eval_io_ok(const dra_mlp_eval_io* io) {
  if (mlp_eval_supported(io->n_episodes, io->horizon)) return false;
  return io->env_state && io->env_counter && io->ep_steps && io->ep_return && io->env_seed && io->out_return && io->out_length &&
         io->out_steps;
}

}  // namespace
