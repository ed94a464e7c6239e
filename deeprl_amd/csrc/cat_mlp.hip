// cat_mlp: a2c_feature (examples.py:340-358: 5 workers, rollout length 5, CategoricalActorCriticNet over FCBody(state_dim, gate =
// tanh), ONE RMSprop optimiser) over device-resident cart-pole environments (cartpole_env.h).
//
//   cat_mlp_rollout_kernel   A2C_agent.py:22-41 as ONE launch of one workgroup: per step the observation narrowed to float32 (what
//                            tensor() uploads), the body (4 -> H -> H, tanh or relu), logits and v, the action by the rank-invariant
//                            Gumbel-max stream (gumbel_noise.h: dra_gumbel_sample's bits), the environment step, reward, mask and --
//                            the environment's terminals depend on the actions, so no host shadow can know them -- one appended row
//                            of the episode ring per episode that ended; then the bootstrap forward.  Parameters are read from the
//                            optimiser's ONE flat buffer; nothing is updated here.
//   cartpole_step_kernel     one environment step, stand-alone (what the parity test calls)
//
// The update stays on the module path (dra_gae, nets.linear, dra_policy_heads_given / _bwd, dra_a2c_loss, the fused RMSprop step),
// replayed from a captured graph by agents.A2CAgent.
//
// The rollout is a chain of (T + 1) x 3 dependent layers over <= 64 rows: latency-bound, nothing to spread over 256 CUs.  Plain
// VALU code as in a2c_mlp.hip: weights are copied to LDS once per launch (transposed: consecutive lanes read consecutive units),
// activations are kept TRANSPOSED ([unit][row]) so that a thread's 8 rows of one input unit are two 16-byte LDS reads, and every
// dot product is one fp32 FMA chain in ascending k.  The environments live in the registers of wave 0 (lane e = environment e:
// four fp64 state components, counters, the running return) for the whole launch; the ring position of an ending episode is the
// rank of its lane in the wave's ballot, so rows land in (step, environment) order without a serial pass (cartpole_rollout.h).
#include "common.h"
#include "cartpole_rollout.h"
#include "gumbel_noise.h"
#include <math.h>

namespace {

constexpr int kOut = kA + 1;                  // logits and the value

// LDS of the rollout kernel, in floats; every region starts at a multiple of 4 floats (16 bytes)
__host__ __device__ constexpr size_t rollout_lds_floats(int H, int N) {
  return body_weight_floats(H)                                // W1^T [S][H], W2^T [H][H], b1, b2
         + round_up4(kOut * (H + 1)) + 4                      // heads [3][H + 1], their biases
         + round_up4(kA * kMaxN)                              // logits [N][A]
         + (size_t)kS * round_up8(N) + 2 * (size_t)H * round_up8(N);   // x^T [S][NP], h1^T, h2^T [H][NP]
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
cat_mlp_rollout_kernel(dra_cat_mlp_net net, dra_cat_mlp_rollout_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int N = io.n_env, T = io.t_len, NP = round_up8(N);
  const float* __restrict__ P = net.param;

  const BodyWeights<H> body(lds);
  float* sWh = lds + body_weight_floats(H);           // [3][H + 1]: fc_action's two rows, fc_critic's one
  float* sBh = sWh + round_up4(kOut * (H + 1));       // [3] (+ pad)
  float* sLogit = sBh + 4;                            // [N][A]
  float* sXT = sLogit + round_up4(kA * kMaxN);        // [S][NP]
  float* sH1T = sXT + kS * NP;                        // [H][NP]
  float* sH2T = sH1T + H * NP;                        // [H][NP]
  const int total = (int)(sH2T + H * NP - lds);
  for (int i = tid; i < total; i += 256) lds[i] = 0.f;
  const int64_t t0 = *io.sampler_step;                // (rewritten by thread 0 behind the last barrier)
  __syncthreads();

  // ---- weights, once per launch
  body.stage(P, net, tid);
  for (int i = tid; i < kOut * H; i += 256) {
    const int c = i / H, k = i - c * H;
    sWh[c * (H + 1) + k] = c < kA ? P[net.wa + c * H + k] : P[net.wc + k];
  }
  if (tid < kOut) sBh[tid] = tid < kA ? P[net.ba + tid] : P[net.bc];

  // ---- the environments: lane e of wave 0 carries environment e
  const bool env_lane = tid < N;
  CartPoleLanes lanes;
  lanes.load(io, tid);
  const float reward = (float)(1.0 * io.reward_coef);

  for (int t = 0; t <= T; ++t) {
    if (env_lane) lanes.observe(sXT, NP, io.out_state, N, T, t, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sXT, body.w1, body.b1, sH1T, kS, NP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sH1T, body.w2, body.b2, sH2T, H, NP, tid);
    __syncthreads();
    // ---- heads: one output per thread -- (environment e, logit c) or (e, the value); the bootstrap step needs the value alone
    if (tid < N * kOut) {
      const int e = tid / kOut, c = tid - e * kOut;
      if (c == kA || t < T) {
        const float* hT = sH2T + e;
        const float* w = sWh + c * (H + 1);
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < H; ++k) acc = fmaf(hT[k * NP], w[k], acc);
        acc += sBh[c];
        if (c == kA) io.out_v[(int64_t)t * N + e] = acc;
        else sLogit[e * kA + c] = acc;
      }
    }
    if (t == T) break;
    __syncthreads();
    // ---- action (gumbel_sample_kernel's loop, bit for bit), environment step, ring append: wave 0
    if (tid < 64) {
      const CartPoleRow row(io);
      bool done = false;
      double ended = 0.0;
      if (env_lane) {
        const uint64_t base = gs_step_base(io.noise_seed, t0 + t);
        float best = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int a = 0; a < kA; ++a) {
          const float v = gs_perturbed(base, io.env0 + tid, a, sLogit[tid * kA + a]);
          if (v > best) { best = v; arg = a; }
        }
        done = lanes.advance(row, t, arg, reward, tid, ended);
      }
      lanes.append(row, done, ended, t0 + t, io.env0 + tid, tid);
    }
    // (wave 0 writes the next observation into x^T next: layer 1 of this step, its only reader, is three barriers back)
  }
  __syncthreads();
  lanes.store(io, tid);
  if (tid == 0) *io.sampler_step = t0 + T + 1;
}

__global__ void __launch_bounds__(64)
cartpole_step_kernel(double* __restrict__ state, int64_t* __restrict__ counter, int32_t* __restrict__ ep_steps,
                     double* __restrict__ ep_return, const int64_t* __restrict__ seed, const int64_t* __restrict__ action, int n,
                     int64_t horizon, double* __restrict__ out_reward, int32_t* __restrict__ out_done) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  CartPoleState st = {state[i * kS + 0], state[i * kS + 1], state[i * kS + 2], state[i * kS + 3]};
  int64_t c = counter[i];
  int32_t steps = ep_steps[i];
  double ret = ep_return[i], ended = 0.0;
  const bool done = cartpole_step(st, c, steps, ret, (uint64_t)seed[i], action[i] == 1 ? 1 : 0, horizon, ended);
  state[i * kS + 0] = st.x;
  state[i * kS + 1] = st.xd;
  state[i * kS + 2] = st.th;
  state[i * kS + 3] = st.thd;
  counter[i] = c;
  ep_steps[i] = steps;
  ep_return[i] = ret;
  out_reward[i] = 1.0;
  out_done[i] = done ? 1 : 0;
}

}  // namespace

DRA_API int dra_cat_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate) {
  return cartpole_mlp_supported(state_dim, n_actions, hidden, n_env, gate);
}

DRA_API int dra_cat_mlp_rollout(const dra_cat_mlp_net* net, const dra_cat_mlp_rollout_io* io, void* stream) {
  if (!net || !io || !net->param) return DRA_EINVAL;
  if (cartpole_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->n_env, net->gate)) return DRA_EINVAL;
  if (!offsets_nonnegative({net->w1, net->b1, net->w2, net->b2, net->wa, net->ba, net->wc, net->bc})) return DRA_EINVAL;
  if (!cartpole_io_ok(io) || !io->sampler_step || !io->out_v) return DRA_EINVAL;
  if (io->n_global < io->n_env || io->env0 < 0 || io->env0 + io->n_env > io->n_global) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&cat_mlp_rollout_kernel<H, GATE>>(rollout_lds_floats(H, io->n_env) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_cartpole_step(double* state, int64_t* counter, int32_t* ep_steps, double* ep_return, const int64_t* seed,
                              const int64_t* action, int n, int64_t horizon, double* out_reward, int32_t* out_done, void* stream) {
  if (!state || !counter || !ep_steps || !ep_return || !seed || !action || !out_reward || !out_done || n < 1 || horizon < 1)
    return DRA_EINVAL;
  hipLaunchKernelGGL(cartpole_step_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, dra_stream(stream), state, counter, ep_steps,
                     ep_return, seed, action, n, horizon, out_reward, out_done);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
