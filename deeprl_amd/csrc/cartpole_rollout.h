// What the one-workgroup rollout / acting kernels over device-resident cart-poles share (cat_mlp.hip: a2c_feature, q_mlp.hip:
// n_step_dqn_feature, oc_mlp.hip: option_critic_feature, dqn_mlp.hip: dqn_feature, dist_mlp.hip: the C51 / QR-DQN entries,
// rainbow_mlp.hip: rainbow_feature), stated ONCE:
//
//   CartPoleLanes    the environments in the registers of wave 0 (lane e = environment e) for the whole launch: load, observe,
//                    advance (cartpole_step, the action / reward / mask row), append (the episode ring: an ending episode's
//                    position is the rank of its lane in the wave's ballot, so rows land in (step, environment) order) and
//                    store.  A ring row is (stamp, environment id, episodic return): the kernel says what the stamp counts
//                    (cat_mlp: sampler steps, T + 1 per rollout; q_mlp and oc_mlp: their step counter, T per rollout) and how
//                    its lanes are numbered (cat_mlp: env0 + lane, q_mlp and oc_mlp: lane).
//   BodyWeights<H>   the two-layer body's W1^T, W2^T, b1, b2 in LDS and their staging from a flat parameter buffer;
//   QNetWeights<H>   the same with the Q head [A][H + 1] behind it (q_mlp.hip, dqn_mlp.hip).
//   EpisodeRow       what append reads of a row in the kernels that write transitions to a replay ring (dqn_mlp.hip, dist_mlp.hip,
//                    rainbow_mlp.hip); the rest of their acting frame -- the ring cursor, the wave-0 block, the epilogue, the io
//                    check -- is replay_act.h's ReplayActor over these lanes.
//   the host checks  cartpole_mlp_supported, offsets_nonnegative, cartpole_io_ok, and the hidden x gate dispatch.
//
// Each kernel keeps its action choice (Gumbel-max / staged epsilon-greedy / option-critic's two inverse-CDF draws with the carried
// prev_option and is_initial), its heads and which counter it advances.  What runs inside the step loop is written for the
// register allocator (the figures): observe() takes plain pointers and scalars; cat_mlp calls advance inside the
// block of its choice, q_mlp step() with the choice made in a block of its own, oc_mlp advance and append behind its decision
// block (the next step's is_initial is the `done` advance returns).
#pragma once
#include "cartpole_env.h"
#include "mlp_rollout.h"
#include <type_traits>

namespace {

constexpr int kS = kCartPoleS, kA = kCartPoleA, kMaxN = 64;

// W1^T [S][H], W2^T [H][H] (transposed: [k][unit]), b1, b2 in LDS; stage() fills them from a flat buffer ([unit][k] as stored)
__host__ __device__ constexpr size_t body_weight_floats(int H) { return (size_t)kS * H + (size_t)H * H + 2 * (size_t)H; }
template <int H>
struct BodyWeights {
  float *w1, *w2, *b1, *b2;
  __device__ explicit BodyWeights(float* base) : w1(base), w2(w1 + kS * H), b1(w2 + H * H), b2(b1 + H) {}
  template <typename Net>
  __device__ __forceinline__ void stage(const float* __restrict__ P, const Net& net, int tid) const {
    for (int i = tid; i < kS * H; i += 256) {
      const int k = i / H, u = i - k * H;
      w1[i] = P[net.w1 + u * kS + k];
    }
    for (int i = tid; i < H * H; i += 256) {
      const int k = i / H, u = i - k * H;
      w2[i] = P[net.w2 + u * H + k];
    }
    for (int i = tid; i < H; i += 256) {
      b1[i] = P[net.b1 + i];
      b2[i] = P[net.b2 + i];
    }
  }
};

// a VanillaNet's weights in LDS (q_mlp.hip, dqn_mlp.hip): the body and the Q head [A][H + 1] with its bias; every region starts at a
// multiple of 4 floats (16 bytes)
__host__ __device__ constexpr size_t q_net_weight_floats(int H) { return body_weight_floats(H) + round_up4(kA * (H + 1)) + 4; }
template <int H>
struct QNetWeights {
  BodyWeights<H> body;
  float *wq, *bq;
  __device__ explicit QNetWeights(float* base) : body(base), wq(base + body_weight_floats(H)), bq(wq + round_up4(kA * (H + 1))) {}
  __device__ __forceinline__ void stage(const float* __restrict__ P, const dra_q_mlp_net& net, int tid) const {
    body.stage(P, net, tid);
    for (int i = tid; i < kA * H; i += 256) {
      const int c = i / H, k = i - c * H;
      wq[c * (H + 1) + k] = P[net.wq + c * H + k];
    }
    if (tid < kA) bq[tid] = P[net.bq + tid];
  }
};

// where step t's row and ring rows go: read from the kernel's io struct once per step, AHEAD of the lanes' own block
struct CartPoleRow {
  int64_t* out_action;
  float *out_reward, *out_mask;
  double* ep_ring;
  int64_t horizon, ring_cap;
  int N;
  template <typename Io>
  __device__ __forceinline__ explicit CartPoleRow(const Io& io)
      : out_action(io.out_action), out_reward(io.out_reward), out_mask(io.out_mask), ep_ring(io.ep_ring), horizon(io.horizon),
        ring_cap(io.ring_cap), N(io.n_env) {}
};

// what CartPoleLanes::append reads of a row where the transition itself goes to a replay ring (replay_act.h's episode_row): the
// episode ring alone
struct EpisodeRow {
  int64_t* out_action = nullptr;
  float *out_reward = nullptr, *out_mask = nullptr;
  double* ep_ring;
  int64_t horizon, ring_cap;
  int n_env = 1;
};

struct CartPoleLanes {
  CartPoleState st = {0.0, 0.0, 0.0, 0.0};
  int64_t counter = 0;
  int32_t ep_steps = 0;
  double ep_return = 0.0;
  uint64_t seed = 0;
  int64_t ring_count = 0;

  template <typename Io>
  __device__ __forceinline__ void load(const Io& io, int tid) {
    if (tid < io.n_env) {
      st.x = io.env_state[tid * kS + 0];
      st.xd = io.env_state[tid * kS + 1];
      st.th = io.env_state[tid * kS + 2];
      st.thd = io.env_state[tid * kS + 3];
      counter = io.env_counter[tid];
      ep_steps = io.ep_steps[tid];
      ep_return = io.ep_return[tid];
      seed = (uint64_t)io.env_seed[tid];
    }
    if (tid < 64) ring_count = *io.ep_count;
  }

  // an environment lane's observation at step t: float32 of the fp64 state (torch_utils.py:23) into x^T [S][NP], row t < T of out_state
  __device__ __forceinline__ void observe(float* xT, int NP, float* out_state, int N, int T, int t, int tid) const {
    const float x[kS] = {(float)st.x, (float)st.xd, (float)st.th, (float)st.thd};
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      xT[j * NP + tid] = x[j];
      if (t < T) out_state[((int64_t)t * N + tid) * kS + j] = x[j];
    }
  }

  // an environment lane steps under its action `arg` and writes row t (reward: what tensor(reward_normalizer(rewards)) uploads)
  __device__ __forceinline__ bool advance(const CartPoleRow& r, int t, int arg, float reward, int tid, double& ended) {
    const bool done = cartpole_step(st, counter, ep_steps, ep_return, seed, arg, r.horizon, ended);
    const int64_t o = (int64_t)t * r.N + tid;
    r.out_action[o] = arg;
    r.out_reward[o] = reward;
    r.out_mask[o] = done ? 0.f : 1.f;
    return done;
  }

  // wave 0: every episode that ended appends (stamp, env_id, its return) to the ring
  __device__ __forceinline__ void append(const CartPoleRow& r, bool done, double ended, int64_t stamp, int64_t env_id, int tid) {
    const unsigned long long ends = __ballot(done ? 1 : 0);
    if (done) {
      const int before = __popcll(ends & ((1ull << tid) - 1ull));
      double* row = r.ep_ring + ((ring_count + before) % r.ring_cap) * 3;
      row[0] = (double)stamp;
      row[1] = (double)env_id;
      row[2] = ended;
    }
    ring_count += __popcll(ends);
  }

  // advance and append for a kernel whose action choice stands in a block of its own
  template <typename Io>
  __device__ __forceinline__ void step(const Io& io, int t, int arg, float reward, int64_t stamp, int64_t env_id, int tid) {
    const CartPoleRow r(io);
    bool done = false;
    double ended = 0.0;
    if (tid < r.N) done = advance(r, t, arg, reward, tid, ended);
    append(r, done, ended, stamp, env_id, tid);
  }

  template <typename Io>
  __device__ __forceinline__ void store(const Io& io, int tid) const {
    if (tid < io.n_env) {
      io.env_state[tid * kS + 0] = st.x;
      io.env_state[tid * kS + 1] = st.xd;
      io.env_state[tid * kS + 2] = st.th;
      io.env_state[tid * kS + 3] = st.thd;
      io.env_counter[tid] = counter;
      io.ep_steps[tid] = ep_steps;
      io.ep_return[tid] = ep_return;
    }
    if (tid == 0) *io.ep_count = ring_count;
  }
};

// ---- host side: the shapes both rollout kernels are built for
inline int cartpole_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate) {
  if (state_dim != kS || n_actions != kA) return DRA_EINVAL;
  if (hidden != 16 && hidden != 32 && hidden != 64) return DRA_EINVAL;
  if (n_env < 1 || n_env > kMaxN || (gate != kGateRelu && gate != kGateTanh)) return DRA_EINVAL;
  return DRA_OK;
}

inline bool offsets_nonnegative(std::initializer_list<int32_t> offs) {
  for (int32_t o : offs)
    if (o < 0) return false;
  return true;
}

template <typename Io>
bool cartpole_io_ok(const Io* io) {
  if (io->t_len < 1 || io->horizon < 1 || io->ring_cap < 1) return false;
  if ((int64_t)(io->t_len + 1) * io->n_env * kS > 0x7fffffff) return false;
  return io->env_state && io->env_counter && io->ep_steps && io->ep_return && io->env_seed && io->ep_count && io->ep_ring &&
         io->out_state && io->out_action && io->out_reward && io->out_mask;
}

// f(hidden, gate) with both as std::integral_constant: the instance of a kernel template for a supported (hidden, gate)
template <typename F>
int dispatch_hidden_gate(int hidden, int gate, F&& f) {
  auto with_gate = [&](auto h) {
    return gate == kGateRelu ? f(h, std::integral_constant<int, kGateRelu>{}) : f(h, std::integral_constant<int, kGateTanh>{});
  };
  if (hidden == 16) return with_gate(std::integral_constant<int, 16>{});
  if (hidden == 32) return with_gate(std::integral_constant<int, 32>{});
  return with_gate(std::integral_constant<int, 64>{});
}

}  // namespace
