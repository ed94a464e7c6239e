// a2c_mlp: a2c_continuous (examples.py:384-404: 16 workers, rollout length 5, GaussianActorCriticNet over two relu FCBody(64, 64),
// ONE RMSprop optimiser, identity state normaliser) over device-resident synthetic environments.
//
//   a2c_mlp_rollout_kernel   A2C_agent.py:22-41 as ONE launch of one workgroup: per step the normalised observation, both
//                            forwards (S -> H -> H -> A and S -> H -> H -> 1, relu or tanh gate), mean = tanh(.), action =
//                            mean + softplus(std) * hashed normal, environment step (csrc/cont_env.h), reward, mask; then the
//                            bootstrap forward.  Parameters are read from the optimiser's ONE flat buffer; nothing is updated here.
//   gauss_head_fwd_kernel    network_heads.py:198-214 behind fc_action for GIVEN actions: mean, log-probability, entropy
//   gauss_head_bwd_kernel    its gradient: dz (through the tanh) and dstd (rows reduced in a fixed order: no float atomics)
//
// The update itself stays on the module path (nets.linear launches, dra_gae, dra_a2c_loss, FusedOptimizer.step), replayed from a
// captured graph by agents.A2CAgent.
//
// The rollout is a chain of (T + 1) x 3 dependent layers over <= 64 rows: latency-bound, nothing to spread over 256 CUs.  Plain
// VALU code: weights are copied to LDS once per launch (transposed: consecutive lanes read consecutive units), activations are
// kept TRANSPOSED ([unit][row]) so that a thread's 8 rows of one input unit are two 16-byte LDS reads, and every dot product is
// one fp32 FMA chain in ascending k.
//
// Normaliser order: A2C_agent.py:29 / 38 call config.state_normalizer on the CURRENT observation before every forward, the
// bootstrap forward included -- so the running statistics (when they are updated at all) fold the observation of step t before
// forward t, T + 1 times per rollout, and the first observation of the next rollout is folded again.  The kernel does the same
// (PPO's kernel folds AFTER the environment step, as PPO_agent.py:39 does).
#include "common.h"
#include "cont_env.h"
#include "mlp_rollout.h"
#include <math.h>

namespace {

constexpr int kMaxS = 64, kMaxA = 16, kMaxN = 64;
constexpr size_t kLdsBytesMax = 160 * 1024;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// LDS of the rollout kernel, in floats (the fp64 statistics first: mean, var, divisor [S] and the count)
__host__ __device__ constexpr size_t rollout_lds_floats(int S, int A, int H, int N) {
  return 2 * ((size_t)3 * S + 2)                                // fp64 mean, var, den [S], count (+ pad)
         + 2 * (size_t)S * H + 2 * (size_t)H * H + 4 * (size_t)H     // W1^T, W2^T, b1, b2 of both networks
         + (size_t)A * (H + 1) + H + (A + 1) + A                     // actor head [A][H + 1], critic head [H], b3 (A + 1), scale [A]
         + (size_t)S * round_up8(N) + 4 * (size_t)H * round_up8(N)   // x^T [S][NP], h1^T / h2^T [2][H][NP]
         + (size_t)N * A;                                            // actions [N][A]
}

__device__ __forceinline__ double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double softplus_grad_d(double x) {     // as autograd forms it: z / (z + 1), z = exp(x)
  if (x > 20.0) return 1.0;
  const double z = exp(x);
  return z / (z + 1.0);
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
a2c_mlp_rollout_kernel(dra_a2c_mlp_net net, dra_a2c_mlp_rollout_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, role = tid >> 7, t7 = tid & 127;
  const int S = net.state_dim, A = net.action_dim;
  const int N = io.n_env, T = io.t_len, NP = round_up8(N);
  const float* __restrict__ P = net.param;

  double* sMean = reinterpret_cast<double*>(lds);
  double* sVar = sMean + S;
  double* sDen = sVar + S;
  double* sCount = sDen + S;                     // [2]: the count, one pad
  float* sW1 = reinterpret_cast<float*>(sCount + 2);      // [2][S][H]  (transposed: [k][unit])
  float* sW2 = sW1 + 2 * S * H;                  // [2][H][H]
  float* sB1 = sW2 + 2 * H * H;                  // [2][H]
  float* sB2 = sB1 + 2 * H;                      // [2][H]
  float* sW3a = sB2 + 2 * H;                     // [A][H + 1]
  float* sW3c = sW3a + A * (H + 1);              // [H]
  float* sB3 = sW3c + H;                         // [A] actor, [1] critic
  float* sSd = sB3 + (A + 1);                    // [A] scale = softplus(std)
  float* sAct = sSd + A;                         // [N][A]
  // (16-byte alignment of the transposed activations: everything above is a multiple of 4 floats only by accident -> round up)
  const size_t used = (size_t)(sAct + N * A - lds);
  float* sXT = lds + ((used + 3) & ~(size_t)3);  // [S][NP]
  float* sH1T = sXT + S * NP;                    // [2][H][NP]
  float* sH2T = sH1T + 2 * H * NP;               // [2][H][NP]
  const int total = (int)(sH2T + 2 * H * NP - lds);
  for (int i = tid; i < total; i += 256) lds[i] = 0.f;
  __syncthreads();

  // ---- off the chain, over the whole rollout: rewards / terminals (hashes of the step counters) and the action noise, parked in
  // out_action (step t overwrites it with the action)
  for (int i = tid; i < T * N; i += 256) {
    const int t = i / N, e = i - t * N;
    const int64_t c = io.env_counter[e] + t + 1;
    const uint64_t sdv = (uint64_t)io.env_seed[e];
    io.out_reward[i] = (float)(cenv_reward(sdv, c) * io.reward_coef);
    io.out_mask[i] = cenv_done(sdv, c, io.horizon) ? 0.f : 1.f;
  }
  const int64_t t_noise0 = *io.sampler_step;
  for (int i = tid; i < T * N * A; i += 256) {
    const int t = i / (N * A), r = i - t * (N * A), e = r / A, d = r - e * A;
    io.out_action[i] = gauss_noise(io.noise_seed, t_noise0 + t, io.n_global, io.env0 + e, d);
  }

  // ---- weights, once per launch
  for (int i = tid; i < 2 * S * H; i += 256) {
    const int r = i / (S * H), o = i - r * (S * H), k = o / H, u = o - k * H;
    sW1[i] = P[(r ? net.c_w1 : net.a_w1) + u * S + k];
  }
  for (int i = tid; i < 2 * H * H; i += 256) {
    const int r = i / (H * H), o = i - r * (H * H), k = o / H, u = o - k * H;
    sW2[i] = P[(r ? net.c_w2 : net.a_w2) + u * H + k];
  }
  for (int i = tid; i < 2 * H; i += 256) {
    const int r = i / H, u = i - r * H;
    sB1[i] = P[(r ? net.c_b1 : net.a_b1) + u];
    sB2[i] = P[(r ? net.c_b2 : net.a_b2) + u];
  }
  for (int i = tid; i < A * H; i += 256) {
    const int c = i / H, k = i - c * H;
    sW3a[c * (H + 1) + k] = P[net.a_w3 + i];
  }
  for (int i = tid; i < H; i += 256) sW3c[i] = P[net.c_w3 + i];
  for (int i = tid; i < A; i += 256) {
    sB3[i] = P[net.a_b3 + i];
    sSd[i] = softplus_f(P[net.off_std + i]);
  }
  if (tid == 0) sB3[A] = P[net.c_b3];
  for (int i = tid; i < S; i += 256) {
    const double m = io.rms[i], v = io.rms[S + i];
    sMean[i] = m;
    sVar[i] = v;
    sDen[i] = sqrt(v + io.rms_epsilon);
  }
  if (tid == 0) sCount[0] = io.rms[2 * S];
  __threadfence();
  __syncthreads();

  for (int t = 0; t <= T; ++t) {
    // ---- observation statistics (one lane per feature, rows in order: normalizer.py:39-41) and the normalised observation
    if (io.rms_update) {
      if (tid < S) {
        double m = sMean[tid], v = sVar[tid];
        rms_fold(io.env_state + tid, S, N, m, v, sCount[0]);
        sMean[tid] = m;
        sVar[tid] = v;
        sDen[tid] = sqrt(v + io.rms_epsilon);
      }
      __syncthreads();
      if (tid == 0) sCount[0] = sCount[0] + (double)N;
    }
    for (int i = tid; i < N * S; i += 256) {
      const int e = i / S, j = i - e * S;
      double z = (io.env_state[i] - sMean[j]) / sDen[j];
      z = z < -io.rms_clip ? -io.rms_clip : (z > io.rms_clip ? io.rms_clip : z);
      const float x = (float)z;
      sXT[j * NP + e] = x;
      if (t < T) io.out_state[(int64_t)t * N * S + i] = x;
      else io.cur_state[i] = x;
    }
    __syncthreads();
    // ---- F1, F2: threads 0-127 the policy network, 128-255 the value network (the bootstrap step needs the value alone)
    const bool live = role == 1 || t < T;
    if (live) hidden_layer<H, GATE, 128>(sXT, sW1 + role * S * H, sB1 + role * H, sH1T + role * H * NP, S, NP, t7);
    __syncthreads();
    if (live) hidden_layer<H, GATE, 128>(sH1T + role * H * NP, sW2 + role * H * H, sB2 + role * H, sH2T + role * H * NP, H, NP, t7);
    __syncthreads();
    // ---- heads: one output per thread -- (environment e, action dimension c) or (e, the value)
    for (int i = tid; i < N * (A + 1); i += 256) {
      const int e = i / (A + 1), c = i - e * (A + 1);
      const bool critic = c == A;
      if (!critic && t == T) continue;
      const float* hT = sH2T + (critic ? H * NP : 0) + e;
      const float* w = critic ? sW3c : sW3a + c * (H + 1);
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) acc = fmaf(hT[k * NP], w[k], acc);
      acc += sB3[c];
      if (critic) {
        io.out_v[(int64_t)t * N + e] = acc;
      } else {
        // network_heads.py:200-206: mean = tanh(fc_action(.)), dist.sample() = mean + scale * standard normal
        const int64_t o = ((int64_t)t * N + e) * A + c;
        const float act = io.out_action[o] * sSd[c] + tanhf(acc);
        io.out_action[o] = act;
        sAct[e * A + c] = act;
      }
    }
    if (t == T) break;
    __syncthreads();
    // ---- environment step: one thread per observation component (the mean action of its environment recomputed by each)
    for (int i = tid; i < N * S; i += 256) {
      const int e = i / S, j = i - e * S;
      io.env_state[i] = cenv_next_state((uint64_t)io.env_seed[e], io.env_counter[e] + t + 1, j, io.env_state[i],
                                        cenv_mean_action(sAct + e * A, A), io.out_mask[t * N + e] == 0.f);
    }
    __syncthreads();
  }
  __syncthreads();        // (every thread has read the counters the steps were derived from)
  for (int i = tid; i < N; i += 256) io.env_counter[i] = io.env_counter[i] + T;
  if (io.rms_update) {
    for (int i = tid; i < S; i += 256) { io.rms[i] = sMean[i]; io.rms[S + i] = sVar[i]; }
    if (tid == 0) io.rms[2 * S] = sCount[0];
  }
  if (tid == 0) *io.sampler_step = t_noise0 + T + 1;
}

// ------------------------------------------------------------------------------------------------ Gaussian head
// The head's arithmetic runs in fp64 and is rounded once: log_pi_a divides (a - mean)^2 by scale^2, and scale = softplus(std)
// reaches 3e-4 at std = -8 -- an fp32 rounding of a saturated tanh (6e-8) would come out 1 / scale^2 times larger.  n x A is a
// few hundred elements per update: the fp64 rate does not matter.
constexpr int kHeadMaxA = 64;

__global__ void __launch_bounds__(256)
gauss_head_fwd_kernel(const float* __restrict__ z, const float* __restrict__ std_raw, const float* __restrict__ action, int n, int A,
                      float* __restrict__ mean, float* __restrict__ log_pi_a, float* __restrict__ entropy) {
  __shared__ double s_inv2var[kHeadMaxA], s_logsd[kHeadMaxA];
  __shared__ double s_ent;
  if (threadIdx.x < A) {
    const double sd = softplus_d((double)std_raw[threadIdx.x]);
    s_inv2var[threadIdx.x] = 1.0 / (2.0 * (sd * sd));
    s_logsd[threadIdx.x] = log(sd);
  }
  __syncthreads();
  if (threadIdx.x == 0) {      // torch.distributions.Normal.entropy: 0.5 + 0.5 log(2 pi) + log(scale), summed in ascending d
    double e = 0.0;
    for (int d = 0; d < A; ++d) e += (0.5 + kHalfLog2Pi) + s_logsd[d];
    s_ent = e;
  }
  __syncthreads();
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  double lp = 0.0;
  for (int d = 0; d < A; ++d) {
    const int64_t i = (int64_t)row * A + d;
    const double mu = tanh((double)z[i]);
    const double diff = (double)action[i] - mu;
    lp += (-(diff * diff) * s_inv2var[d] - s_logsd[d]) - kHalfLog2Pi;
    mean[i] = (float)mu;
  }
  log_pi_a[row] = (float)lp;
  entropy[row] = (float)s_ent;
}

// block d: column d of dz and dstd[d].  Thread i sums rows i, i + 256, ... in order; the 256 partial sums are folded by a fixed
// tree -- the same bits on every launch.
__global__ void __launch_bounds__(256)
gauss_head_bwd_kernel(const float* __restrict__ z, const float* __restrict__ std_raw, const float* __restrict__ action,
                      const float* __restrict__ g_lp, const float* __restrict__ g_ent, int n, int A, float* __restrict__ dz,
                      float* __restrict__ dstd) {
  __shared__ double s_part[256];
  const int d = blockIdx.x, tid = threadIdx.x;
  const double raw = (double)std_raw[d];
  const double sd = softplus_d(raw), inv = 1.0 / sd, inv_var = inv * inv;
  double part = 0.0;
  for (int row = tid; row < n; row += 256) {
    const int64_t i = (int64_t)row * A + d;
    const double mu = tanh((double)z[i]);
    const double diff = (double)action[i] - mu;
    const double gl = (double)g_lp[row], ge = (double)g_ent[row];
    // d log_pi_a / d mean = (a - mean) / scale^2, through the tanh;  d log_pi_a / d scale = (a - mean)^2 / scale^3 - 1 / scale,
    // d entropy / d scale = 1 / scale
    dz[i] = (float)((gl * (diff * inv_var)) * (1.0 - mu * mu));
    part += gl * ((diff * diff) * (inv_var * inv) - inv) + ge * inv;
  }
  s_part[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_part[tid] = s_part[tid] + s_part[tid + o];
    __syncthreads();
  }
  if (tid == 0) dstd[d] = (float)(s_part[0] * softplus_grad_d(raw));
}

template <int H, int GATE>
int launch_rollout(const dra_a2c_mlp_net* net, const dra_a2c_mlp_rollout_io* io, void* stream) {
  const size_t bytes = (rollout_lds_floats(net->state_dim, net->action_dim, H, io->n_env) + 4) * sizeof(float);
  return launch_one_workgroup<&a2c_mlp_rollout_kernel<H, GATE>>(bytes, net, io, stream);
}

}  // namespace

DRA_API int dra_a2c_mlp_supported(int state_dim, int action_dim, int hidden, int n_env, int gate) {
  if (state_dim < 1 || state_dim > kMaxS || action_dim < 1 || action_dim > kMaxA) return DRA_EINVAL;
  if (hidden != 32 && hidden != 64) return DRA_EINVAL;
  if (n_env < 1 || n_env > kMaxN || (gate != kGateRelu && gate != kGateTanh)) return DRA_EINVAL;
  if ((rollout_lds_floats(state_dim, action_dim, hidden, n_env) + 4) * sizeof(float) > kLdsBytesMax) return DRA_EINVAL;
  return DRA_OK;
}

DRA_API int dra_a2c_mlp_rollout(const dra_a2c_mlp_net* net, const dra_a2c_mlp_rollout_io* io, void* stream) {
  if (!net || !io || !net->param) return DRA_EINVAL;
  if (dra_a2c_mlp_supported(net->state_dim, net->action_dim, net->hidden, io->n_env, net->gate)) return DRA_EINVAL;
  const int32_t offs[13] = {net->a_w1, net->a_b1, net->a_w2, net->a_b2, net->a_w3, net->a_b3, net->c_w1, net->c_b1,
                            net->c_w2, net->c_b2, net->c_w3, net->c_b3, net->off_std};
  for (int i = 0; i < 13; ++i)
    if (offs[i] < 0) return DRA_EINVAL;
  if (io->t_len < 1 || io->horizon < 1 || io->n_global < io->n_env || io->env0 < 0) return DRA_EINVAL;
  if ((int64_t)(io->t_len + 1) * io->n_env * kMaxS > 0x7fffffff) return DRA_EINVAL;
  if (!io->env_state || !io->env_counter || !io->env_seed || !io->rms || !io->cur_state || !io->sampler_step || !io->out_state ||
      !io->out_action || !io->out_v || !io->out_reward || !io->out_mask)
    return DRA_EINVAL;
  if (net->hidden == 32)
    return net->gate == kGateRelu ? launch_rollout<32, kGateRelu>(net, io, stream) : launch_rollout<32, kGateTanh>(net, io, stream);
  return net->gate == kGateRelu ? launch_rollout<64, kGateRelu>(net, io, stream) : launch_rollout<64, kGateTanh>(net, io, stream);
}

DRA_API int dra_gauss_head_fwd(const float* z, const float* std, const float* action, int n, int a_dim, float* mean,
                               float* log_pi_a, float* entropy, void* stream) {
  if (!z || !std || !action || !mean || !log_pi_a || !entropy || n < 1 || a_dim < 1 || a_dim > kHeadMaxA) return DRA_EINVAL;
  if ((int64_t)n * a_dim > 0x7fffffff) return DRA_EINVAL;
  hipLaunchKernelGGL(gauss_head_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dra_stream(stream), z, std, action, n,
                     a_dim, mean, log_pi_a, entropy);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

DRA_API int dra_gauss_head_bwd(const float* z, const float* std, const float* action, const float* g_log_pi_a, const float* g_entropy,
                               int n, int a_dim, float* dz, float* dstd, void* stream) {
  if (!z || !std || !action || !g_log_pi_a || !g_entropy || !dz || !dstd || n < 1 || a_dim < 1 || a_dim > kHeadMaxA) return DRA_EINVAL;
  if ((int64_t)n * a_dim > 0x7fffffff) return DRA_EINVAL;
  hipLaunchKernelGGL(gauss_head_bwd_kernel, dim3((unsigned)a_dim), dim3(256), 0, dra_stream(stream), z, std, action, g_log_pi_a,
                     g_entropy, n, a_dim, dz, dstd);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
