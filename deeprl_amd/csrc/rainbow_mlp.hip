// rainbow_mlp: rainbow_feature (examples.py:231-280: CategoricalDQNAgent, RainbowNet over FCBody(state_dim, noisy_linear=True), 50
// atoms on [-100, 100], PrioritizedReplay, n_step 3, double_q) with the environment (cartpole_env.h) and the replay ring (ring.hip's
// four arrays) resident on the device.  dist_mlp.hip is the model: the same two launches over FOUR NoisyLinear layers
// (body.layers.0, body.layers.1, fc_value, fc_advantage) and the dueling head.
//
//   rainbow_mlp_act_kernel      DQN_agent.py:24-45 with CategoricalDQN_agent.py:22-24: transition k of the launch runs under noise
//                               ROW k of the [t_len][noise_stride] block (one reset_noise() per transition): the effective weights
//                               W = mu_w + sigma_w * (f(out) (x) f(in)), b = mu_b + sigma_b * f(out_b), f(x) = sign(x) sqrt|x|
//                               (network_utils.py:66-83), are formed in LDS per transition from the RAW noise vectors; waves 0..2
//                               carry the value head and the two advantage heads (lane j = atom j), waves 0..1 then the dueling
//                               combination q = v + (adv - mean_a adv), the softmax and sum_j p_j z_j over the wave.  The action is
//                               the first maximum unless the staged explore word says otherwise (the host stages 0: epsilon is 0
//                               under noisy layers); the fp64 environment step, the ring row, the episode ring and the counters are
//                               dqn_mlp_act_kernel's: replay_act.h.  The atoms, the one-wave softmax with its expectation (here and
//                               in the update's target and double_q passes) and the projection are dist_mlp.hip's: c51_block.h.
//   rainbow_mlp_update_kernel   DQN_agent.py:114-134 with CategoricalDQN_agent.py:60-89 and the whole backward as ONE launch of one
//                               workgroup.  Both networks' effective weights do not fit the LDS next to each other
//                               (update_lds_floats), so the TARGET network (under the target's noise) runs over ALL
//                               rows first and leaves its [A N][B] probabilities and [A][B] action values, then the ONLINE network
//                               (under ONE online noise draw) is staged over the same region and runs row blocks of 16: the n-step
//                               fold of replay.py:135-139 in fp64, a_next (double_q: from the online network on the next states),
//                               the projection, the KL per row, priorities and importance weights (DQN_agent.py:120-127), and the
//                               gradient of mean_b(KL_b w_b) through the dueling combination with respect to all 16 tensors.
//
//   rainbow_mlp_eval_kernel     the acting kernel's forward over eval_act.h's loop (config.fused_eval): n_episodes greedy episodes of
//                               the evaluation environment in ONE launch under ONE noise row (the online network's own buffers),
//                               the effective weights formed once, ahead of the loop.
//
// Plain fp32 VALU code, every dot product one FMA chain in ascending k, every gradient element owned by ONE thread that adds its
// rows in ascending order: no atomics, the same bits on every launch.
#include "common.h"
#include "c51_block.h"
#include "mlp_update_block.h"
#include "eval_act.h"
#include "replay_act.h"
#include <math.h>

namespace {

constexpr size_t kLdsBytes = 160 * 1024;
static_assert(kA == 2, "the dueling mean and the head's waves are written for two actions");

// f(x) = sign(x) sqrt|x| (network_utils.py:81-83)
__device__ __forceinline__ float noise_f(float x) { return copysignf(__fsqrt_rn(fabsf(x)), x); }

// f of a network's twelve raw noise vectors in LDS: l1 in [S] out [H] bias [H], l2 in / out / bias [H], value in [H] out / bias
// [N], advantage in [H] out / bias [A N]
__host__ __device__ constexpr int noise_f_floats(int H, int N) { return round_up4(kS + 7 * H + 2 * N + 2 * kA * N); }
template <int H>
struct NoiseF {
  float *i1, *o1, *b1, *i2, *o2, *b2, *iv, *ov, *bv, *ia, *oa, *ba;
  __device__ NoiseF(float* base, int N)
      : i1(base), o1(i1 + kS), b1(o1 + H), i2(b1 + H), o2(i2 + H), b2(o2 + H), iv(b2 + H), ov(iv + H), bv(ov + N), ia(bv + N),
        oa(ia + H), ba(oa + kA * N) {}
  static __device__ __forceinline__ void vec(float* dst, const float* __restrict__ src, int n, int tid) {
    for (int i = tid; i < n; i += 256) dst[i] = noise_f(src[i]);
  }
  __device__ __forceinline__ void load(const float* __restrict__ z, const dra_rainbow_mlp_net& net, int N, int tid) const {
    vec(i1, z + net.l1.e_in, kS, tid);
    vec(o1, z + net.l1.e_out, H, tid);
    vec(b1, z + net.l1.e_b, H, tid);
    vec(i2, z + net.l2.e_in, H, tid);
    vec(o2, z + net.l2.e_out, H, tid);
    vec(b2, z + net.l2.e_b, H, tid);
    vec(iv, z + net.value.e_in, H, tid);
    vec(ov, z + net.value.e_out, N, tid);
    vec(bv, z + net.value.e_b, N, tid);
    vec(ia, z + net.advantage.e_in, H, tid);
    vec(oa, z + net.advantage.e_out, kA * N, tid);
    vec(ba, z + net.advantage.e_b, kA * N, tid);
  }
};

// element e = o * in + i of a noisy layer's effective weight, and its effective bias (network_utils.py:66-71: the product of the
// two f's first, then sigma's, then the sum)
__device__ __forceinline__ float eff_w(const float* __restrict__ P, const dra_rainbow_mlp_layer& L, int e, float fo, float fi) {
  return __fadd_rn(P[L.w_mu + e], __fmul_rn(P[L.w_sigma + e], __fmul_rn(fo, fi)));
}
__device__ __forceinline__ float eff_b(const float* __restrict__ P, const dra_rainbow_mlp_layer& L, int o, float fb) {
  return __fadd_rn(P[L.b_mu + o], __fmul_rn(P[L.b_sigma + o], fb));
}

// the body's effective W1^T [S][H], W2^T [H][H] (transposed: [k][unit]), b1, b2 -- and W2 as stored where w2n is given
template <int H>
__device__ __forceinline__ void stage_body(const float* __restrict__ P, const dra_rainbow_mlp_net& net, const NoiseF<H>& f, float* w1,
                                           float* w2, float* w2n, float* b1, float* b2, int tid) {
  for (int i = tid; i < kS * H; i += 256) {
    const int k = i / H, u = i - k * H;
    w1[i] = eff_w(P, net.l1, u * kS + k, f.o1[u], f.i1[k]);
  }
  for (int i = tid; i < H * H; i += 256) {
    const int k = i / H, u = i - k * H;
    const float w = eff_w(P, net.l2, u * H + k, f.o2[u], f.i2[k]);
    w2[i] = w;
    if (w2n) w2n[u * H + k] = w;
  }
  for (int i = tid; i < H; i += 256) {
    b1[i] = eff_b(P, net.l1, i, f.b1[i]);
    b2[i] = eff_b(P, net.l2, i, f.b2[i]);
  }
}

// the two heads' effective weights as ONE block of N + A N rows of stride ld (value first), their biases behind
template <int H>
__device__ __forceinline__ void stage_heads(const float* __restrict__ P, const dra_rainbow_mlp_net& net, const NoiseF<H>& f, float* wh,
                                            float* bh, int ld, int N, int tid) {
  for (int i = tid; i < N * H; i += 256) {
    const int c = i / H, k = i - c * H;
    wh[c * ld + k] = eff_w(P, net.value, i, f.ov[c], f.iv[k]);
  }
  for (int i = tid; i < kA * N * H; i += 256) {
    const int c = i / H, k = i - c * H;
    wh[(N + c) * ld + k] = eff_w(P, net.advantage, i, f.oa[c], f.ia[k]);
  }
  for (int i = tid; i < N; i += 256) bh[i] = eff_b(P, net.value, i, f.bv[i]);
  for (int i = tid; i < kA * N; i += 256) bh[N + i] = eff_b(P, net.advantage, i, f.ba[i]);
}

// lane j's logit of (action a, row r) from the heads' raw outputs [N + A N][ld]: v + (adv_a - mean_a adv) (network_heads.py:83)
__device__ __forceinline__ float dueling_logit(const float* raw, int N, int ld, int a, int j, int r) {
  const float a0 = raw[(N + j) * ld + r], a1 = raw[(2 * N + j) * ld + r];
  const float mean = (a0 + a1) / (float)kA;
  return raw[j * ld + r] + ((a ? a1 : a0) - mean);
}

// ---------------------------------------------------------------------------------------------------- acting
__host__ __device__ constexpr size_t act_lds_floats(int H, int N) {
  return body_weight_floats(H) + (size_t)round_up4((1 + kA) * N * (H + 1)) + 2 * (size_t)round_up4((1 + kA) * N)    // body, heads, bias, raw
         + round_up4(N) + noise_f_floats(H, N) + (size_t)act_scratch_floats(H);                                      // z, f
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
rainbow_mlp_act_kernel(dra_rainbow_mlp_net net, dra_dqn_mlp_act_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.t_len, N = net.n_atoms, R = (1 + kA) * N;

  const BodyWeights<H> body(lds);
  float* wh = lds + body_weight_floats(H);            // [R][H + 1]: lanes read consecutive rows, one bank apart
  float* bh = wh + round_up4(R * (H + 1));            // [R]
  float* sRaw = bh + round_up4(R);                    // [R]: the heads' outputs of the transition
  float* sZ = sRaw + round_up4(R);                    // [N]
  float* sF = sZ + round_up4(N);
  const NoiseF<H> f(sF, N);
  const ActScratch<H> s(sF + noise_f_floats(H, N));
  ReplayActor actor;
  actor.begin(io, tid);                               // (ahead of the zeroing, for the register allocator: mlp_rollout.h's banner)
  s.zero(tid);
  const float* __restrict__ P = net.param;
  for (int i = tid; i < N; i += 256) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
  const CartPoleRow row = episode_row(io);
  const double reward = 1.0 * io.reward_coef;         // what config.reward_normalizer(1.0) feeds

  for (int k = 0; k < K; ++k) {
    __syncthreads();                                  // (the zeroing above; the last transition's readers of f, x^T and q)
    // ---- the transition's reset_noise(): row k of the block, then the effective weights under it
    f.load(net.noise + (int64_t)k * net.noise_stride, net, N, tid);
    actor.observe(s.xT, kNP, tid);
    __syncthreads();
    stage_body<H>(P, net, f, body.w1, body.w2, nullptr, body.b1, body.b2, tid);
    stage_heads<H>(P, net, f, wh, bh, H + 1, N, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.xT, body.w1, body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, body.w2, body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    // ---- the heads: wave 0 the value head, wave 1 + a the advantage head of action a; lane j = atom j
    if (tid < (1 + kA) * kWave) {
      const int w = tid / kWave, j = tid % kWave;
      if (j < N) {
        const int c = w * N + j;
        const float* wr = wh + c * (H + 1);
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < H; ++i) acc = fmaf(s.h2T[i * kNP], wr[i], acc);
        sRaw[c] = acc + bh[c];
      }
    }
    __syncthreads();
    // ---- wave a: the dueling logits of action a, the softmax and the action value over the wave
    if (tid < kA * kWave) {
      const int a = tid / kWave, j = tid % kWave;
      const bool live = j < N;
      float p;
      const float q = wave_softmax_value(live ? dueling_logit(sRaw, N, 1, a, j, 0) : -INFINITY, live, sZ + j, p);
      if (j == 0) {
        s.q[a] = q;
        io.out_q[k * kA + a] = q;
      }
    }
    __syncthreads();
    actor.step(io, row, s.q, reward, k, tid);
  }
  __syncthreads();
  actor.finish(io, K, tid);
}

// ---------------------------------------------------------------------------------------------------- evaluation
// rainbow_mlp_act_kernel's staging and forward over eval_act.h's loop: greedy, no ring row, until n_episodes episodes have ended.
// The host's eval_step runs the module forward between two reset_noise(): ONE row of noise (net.noise: the online network's own
// buffers), so the effective weights are formed ONCE, ahead of the loop.
template <int H, int GATE>
__global__ void __launch_bounds__(256)
rainbow_mlp_eval_kernel(dra_rainbow_mlp_net net, dra_mlp_eval_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.n_episodes * (int)io.horizon, N = net.n_atoms, R = (1 + kA) * N;      // (K <= 65536: dra_mlp_eval_supported)

  const BodyWeights<H> body(lds);
  float* wh = lds + body_weight_floats(H);            // [R][H + 1]: lanes read consecutive rows, one bank apart
  float* bh = wh + round_up4(R * (H + 1));            // [R]
  float* sRaw = bh + round_up4(R);                    // [R]: the heads' outputs of the step
  float* sZ = sRaw + round_up4(R);                    // [N]
  float* sF = sZ + round_up4(N);
  const NoiseF<H> f(sF, N);
  const ActScratch<H> s(sF + noise_f_floats(H, N));
  int* done_word = eval_done_word(s);
  EvalActor actor;
  actor.begin(io, tid);
  s.zero(tid);
  const float* __restrict__ P = net.param;
  for (int i = tid; i < N; i += 256) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
  f.load(net.noise, net, N, tid);
  __syncthreads();                                    // (f's readers; thread 0 writes x^T next, over what other threads zeroed)
  stage_body<H>(P, net, f, body.w1, body.w2, nullptr, body.b1, body.b2, tid);
  stage_heads<H>(P, net, f, wh, bh, H + 1, N, tid);

  for (int k = 0; k < K; ++k) {
    actor.observe(s.xT, kNP, tid);
    __syncthreads();                                  // (the first step: the effective weights too)
    hidden_layer<H, GATE, 256>(s.xT, body.w1, body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, body.w2, body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    // ---- the heads: wave 0 the value head, wave 1 + a the advantage head of action a; lane j = atom j
    if (tid < (1 + kA) * kWave) {
      const int w = tid / kWave, j = tid % kWave;
      if (j < N) {
        const int c = w * N + j;
        const float* wr = wh + c * (H + 1);
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < H; ++i) acc = fmaf(s.h2T[i * kNP], wr[i], acc);
        sRaw[c] = acc + bh[c];
      }
    }
    __syncthreads();
    // ---- wave a: the dueling logits of action a, the softmax and the action value over the wave
    if (tid < kA * kWave) {
      const int a = tid / kWave, j = tid % kWave;
      const bool live = j < N;
      float p;
      const float q = wave_softmax_value(live ? dueling_logit(sRaw, N, 1, a, j, 0) : -INFINITY, live, sZ + j, p);
      if (j == 0) {
        s.q[a] = q;
        if (io.out_q) io.out_q[k * kA + a] = q;
      }
    }
    __syncthreads();
    actor.step(io, s.q, done_word, tid);
    __syncthreads();
    if (*done_word >= io.n_episodes) break;           // every thread reads the same word: eval_act.h's banner
  }
  actor.finish(io, tid);                              // (thread 0's own words: nothing to wait for)
}

// ---------------------------------------------------------------------------------------------------- the update
constexpr int kUB = 16;          // rows of one block
constexpr int kLD = kUB + 4;     // row stride of the transposed activations (mlp_update_block.h)
constexpr int kLL = kUB + 1;     // row stride of the per-atom arrays: consecutive atoms one bank apart
constexpr int kMaxB = 64;        // rows of one minibatch: the target's probabilities of ALL rows stay in LDS
constexpr int kLP = kMaxB + 1;   // their row stride
constexpr int kMaxNStep = 8;     // transitions the fold walks per row

// the ONE statement of the update's LDS: the launch asks for it, dra_rainbow_mlp_update_supported refuses what does not fit
__host__ __device__ constexpr size_t update_lds_floats(int H, int N) {
  return update_body_floats(H) + (size_t)(1 + kA) * N * H + (size_t)round_up4((1 + kA) * N)    // ONE network's effective weights
         + noise_f_floats(H, N)                                                                // f of its noise
         + (size_t)round_up4(kA * N * kLP) + kA * kMaxB + kMaxB                                // target p and q of all rows; weights
         + 4 * kUB + kA * kUB + kUB + (size_t)round_up4(N)                                     // idx, reward, mask, action; online q_next; loss partials; z
         + (size_t)kS * kLD + 3 * (size_t)H * kLD                                              // x^T, h1^T, h2^T (later dz1^T), dz2^T
         + (size_t)round_up4((1 + kA) * N) * kLL + 2 * (size_t)round_up4(N) * kLL;             // raw heads (later d heads), target, d logits
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
rainbow_mlp_update_kernel(dra_rainbow_mlp_net net, dra_rainbow_mlp_update_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TPU = 256 / H;       // threads that share one unit's row of dW2
  constexpr int KPT = H / TPU;       // columns of it each carries
  constexpr int CPI = 256 / H;       // head rows between two consecutive elements a thread owns of the heads' gradient
  constexpr int EPT = ((1 + kA) * kMaxAtoms * H + 255) / 256;      // elements of it a thread owns at most
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int B = io.batch, N = net.n_atoms, M = kA * N, R = N + M, n_step = io.n_step;
  const int Rp = round_up4(R), Np = round_up4(N);

  const UpdateBody<H> body(lds);          // W1^T, W2^T, W2 as stored, b1, b2: the network staged last
  float* sWh = body.head;                 // [R][H]: value rows, then advantage rows
  float* sBh = sWh + R * H;               // [R] (+ pad)
  float* sF = sBh + Rp;
  const NoiseF<H> f(sF, N);
  float* sPN = sF + noise_f_floats(H, N);                   // [M][kLP]: the target network's probabilities of every row's next state
  float* sQN = sPN + round_up4(M * kLP);                    // [A][kMaxB]: its action values
  float* sWgt = sQN + kA * kMaxB;                           // [kMaxB]: (p B + 1e-6) ** -beta
  int* sIdx = reinterpret_cast<int*>(sWgt + kMaxB);         // [kUB]: the block's ring slots, clamped
  float* sRew = reinterpret_cast<float*>(sIdx + kUB);       // [kUB]: the folded reward
  float* sMsk = sRew + kUB;                                 // [kUB]: the product of the masks
  int* sAct = reinterpret_cast<int*>(sMsk + kUB);           // [kUB]
  float* sQO = reinterpret_cast<float*>(sAct + kUB);        // [A][kUB]: the online network's action values of the next states
  float* sRed = sQO + kA * kUB;                             // [kUB]: the four waves' partial sums of the loss
  float* sZ = sRed + kUB;                                   // [N] (+ pad)
  float* sXT = sZ + Np;                                     // [S][kLD]
  float* sH1T = sXT + kS * kLD;                             // [H][kLD]
  float* sH2T = sH1T + H * kLD;                             // [H][kLD]: h2^T, then dz1^T
  float* sG2T = sH2T + H * kLD;                             // [H][kLD]: dz2^T
  float* sL = sG2T + H * kLD;                               // [Rp][kLL]: the heads' raw outputs; later d loss / d of them
  float* sT = sL + Rp * kLL;                                // [Np][kLL]: the projected target probabilities
  float* sDL = sT + Np * kLL;                               // [Np][kLL]: d loss / d logits of the action taken

  const float* __restrict__ P = net.param;
  const float* __restrict__ PT = net.target;
  for (int i = tid; i < N; i += 256) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
  for (int i = tid; i < M * kLP; i += 256) sPN[i] = 0.f;
  for (int i = tid; i < kA * kMaxB; i += 256) sQN[i] = 0.f;
  const float gamma = (float)io.discount;
  const float v_min = (float)net.v_min, v_max = (float)net.v_max;
  const float delta = (float)((net.v_max - net.v_min) / (double)(N - 1));       // CategoricalDQN_agent.py:37
  const int64_t last = io.capacity - 1 - n_step;      // the last slot with its n-step window and next frame behind it
  const bool double_q = io.double_q != 0;
  int n_bad = 0;

  // ================================================================ the TARGET network over all rows, under the target's noise
  f.load(net.target_noise, net, N, tid);
  __syncthreads();
  stage_body<H>(PT, net, f, body.w1, body.w2, nullptr, body.b1, body.b2, tid);
  stage_heads<H>(PT, net, f, sWh, sBh, H, N, tid);
  __syncthreads();
  for (int r0 = 0; r0 < B; r0 += kUB) {
    const int rows = B - r0 < kUB ? B - r0 : kUB;
    if (tid < kUB) {
      int64_t i = 0;
      bool bad = false;
      if (tid < rows) {
        i = io.idx[r0 + tid];
        bad = i < 0 || i > last;
        i = i < 0 ? 0 : (i > last ? last : i);
      }
      n_bad += __popcll(__ballot(bad ? 1 : 0));
      sIdx[tid] = (int)i;
    }
    __syncthreads();
    gather_states<kUB>(io.ring_frames, sIdx, n_step, rows, sXT, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, body.w1, body.b1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, body.w2, body.b2, nullptr, sH2T, H, tid);
    __syncthreads();
    block_head<H, kUB>(sH2T, sWh, sBh, sL, R, kLL, tid);
    __syncthreads();
    // the softmax of every (action, row): one pair per wave at a time, lane j = atom j
    for (int p = wave; p < kA * rows; p += 4) {
      const int a = p / rows, r = p - a * rows;
      const bool live = lane < N;
      float pj;
      const float q = wave_softmax_value(live ? dueling_logit(sL, N, kLL, a, lane, r) : -INFINITY, live, sZ + lane, pj);
      if (live) sPN[(a * N + lane) * kLP + r0 + r] = pj;
      if (lane == 0) {
        sQN[a * kMaxB + r0 + r] = q;
        io.out_q_next[(int64_t)(r0 + r) * kA + a] = q;
      }
    }
    __syncthreads();       // (the next block rewrites the slots, x^T and the raw outputs)
  }

  // ================================================================ the ONLINE network over the same region, under ONE noise draw
  f.load(net.noise, net, N, tid);
  // DQN_agent.py:124-126: weights = (p B + 1e-6) ** -beta, later divided by their maximum
  const float beta = *io.beta;
  if (tid < kMaxB) sWgt[tid] = tid < B ? powf(__fadd_rn(__fmul_rn(io.prob[tid], (float)B), 1e-6f), -beta) : 0.f;
  __syncthreads();
  stage_body<H>(P, net, f, body.w1, body.w2, body.w2n, body.b1, body.b2, tid);
  stage_heads<H>(P, net, f, sWh, sBh, H, N, tid);
  float w_max = sWgt[0];
  for (int i = 1; i < B; ++i) w_max = fmaxf(w_max, sWgt[i]);
  __syncthreads();

  // what this thread owns of the gradient (of the mu tensors; the sigma tensors' follow from them behind the last block)
  const int u2 = tid / TPU, k2 = (tid % TPU) * KPT;       // dW2 [u2][k2 .. k2 + KPT), db2 [u2] on the first of the unit's threads
  float gW2[KPT], gB2 = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i) gW2[i] = 0.f;
  const int u1 = tid / kS, j1 = tid % kS;                 // dW1 [u1][j1] (tid < S H), db1 [u1] where j1 == 0
  float gW1 = 0.f, gB1 = 0.f;
  const int cq = tid / H, kq = tid % H;                   // the heads' dW [cq + i CPI][kq], i < EPT; db [tid] (tid < R)
  float gWh[EPT], gBh = 0.f;
#pragma unroll
  for (int i = 0; i < EPT; ++i) gWh[i] = 0.f;
  float loss = 0.f;                                       // lane 0 of wave w: sum of KL_b w_b over the rows the wave carried
  const float inv_rows = 1.f / (float)B;
  const float eps_p = (float)io.replay_eps, alpha = (float)io.replay_alpha;

  for (int r0 = 0; r0 < B; r0 += kUB) {
    const int rows = B - r0 < kUB ? B - r0 : kUB;
    // ---- the block's ring slots (clamped as above), the n-step fold (replay.py:135-139) in fp64, the action
    if (tid < kUB) {
      int64_t i = 0;
      float rew = 0.f, msk = 0.f;
      int a = 0;
      if (tid < rows) {
        i = io.idx[r0 + tid];
        i = i < 0 ? 0 : (i > last ? last : i);
        double cum = 0.0;
        int cm = 1;
        for (int s = n_step - 1; s >= 0; --s) {
          const int m = io.ring_masks[i + s];
          cum = io.ring_rewards[i + s] + ((double)m * io.step_discount) * cum;
          cm = (cm && m) ? 1 : 0;
        }
        rew = (float)cum;
        msk = (float)cm;
        a = io.ring_actions[i] == 1 ? 1 : 0;
      }
      sIdx[tid] = (int)i;
      sRew[tid] = rew;
      sMsk[tid] = msk;
      sAct[tid] = a;
    }
    __syncthreads();
    // ---- double_q: the online network's action values of the next states
    if (double_q) {
      gather_states<kUB>(io.ring_frames, sIdx, n_step, rows, sXT, tid);
      __syncthreads();
      block_layer<H, GATE, false, kUB>(sXT, body.w1, body.b1, nullptr, sH1T, kS, tid);
      __syncthreads();
      block_layer<H, GATE, false, kUB>(sH1T, body.w2, body.b2, nullptr, sH2T, H, tid);
      __syncthreads();
      block_head<H, kUB>(sH2T, sWh, sBh, sL, R, kLL, tid);
      __syncthreads();
      for (int p = wave; p < kA * rows; p += 4) {
        const int a = p / rows, r = p - a * rows;
        const bool live = lane < N;
        float pj;
        const float q = wave_softmax_value(live ? dueling_logit(sL, N, kLL, a, lane, r) : -INFINITY, live, sZ + lane, pj);
        if (lane == 0) sQO[a * kUB + r] = q;
      }
      __syncthreads();
    }
    // ---- the target of every row, [N][rows]: the next action is the FIRST maximum (torch.argmax); CategoricalDQN_agent.py:72-78:
    // sum_j clamp(1 - |clamp(r + gamma m z_j) - z_i| / delta, 0, 1) p_j
    for (int o = tid; o < N * kUB; o += 256) {
      const int i = o / kUB, r = o % kUB;
      float t = 0.f;
      if (r < rows) {
        const int an = double_q ? (sQO[kUB + r] > sQO[r] ? 1 : 0) : (sQN[kMaxB + r0 + r] > sQN[r0 + r] ? 1 : 0);
        const float gm = __fmul_rn(gamma, sMsk[r]);
        t = c51_project(sZ, sPN + an * N * kLP + r0 + r, kLP, N, sZ[i], sRew[r], gm, v_min, v_max, delta);
        io.out_target[(int64_t)(r0 + r) * N + i] = t;
      }
      sT[i * kLL + r] = t;
    }
    // ---- the states: the online forward (x^T's and h^T's readers are behind the barriers above)
    gather_states<kUB>(io.ring_frames, sIdx, 0, rows, sXT, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, body.w1, body.b1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, body.w2, body.b2, nullptr, sH2T, H, tid);
    __syncthreads();
    block_head<H, kUB>(sH2T, sWh, sBh, sL, R, kLL, tid);
    __syncthreads();
    // ---- per row, one wave at a time, lane i = atom i: KL = sum_i t_i log(t_i + 1e-5) - t_i log_softmax_i of the action taken, the
    // priority, the weight, d (KL w / B) / d logits = (softmax sum t - t) w / B (0 behind the last row)
    for (int r = wave; r < kUB; r += 4) {
      const bool live = lane < N;
      float dl = 0.f;
      if (r < rows) {      // (uniform over the wave)
        const float l = live ? dueling_logit(sL, N, kLL, sAct[r], lane, r) : -INFINITY;
        const float m = wave_max(l);
        const float e = live ? expf(l - m) : 0.f;
        const float s = wave_sum(e);
        const float ls = logf(s);
        const float t = live ? sT[lane * kLL + r] : 0.f;
        const float kl = wave_sum(live ? t * logf(t + 1e-5f) - t * ((l - m) - ls) : 0.f);
        const float st = wave_sum(t);
        const float w = sWgt[r0 + r] / w_max;
        dl = ((e / s) * st - t) * (w * inv_rows);
        if (lane == 0) {
          io.out_loss_vec[r0 + r] = kl;
          io.out_prio[r0 + r] = powf(fabsf(kl) + eps_p, alpha);
          io.out_weights[r0 + r] = w;
          loss += kl * w;
        }
      }
      if (live) sDL[lane * kLL + r] = dl;
    }
    __syncthreads();
    // ---- through the dueling combination into the raw outputs' place: d v = g, d adv_a' = g (delta_aa' - 1 / A)
    for (int o = tid; o < R * kUB; o += 256) {
      const int c = o / kUB, r = o % kUB;
      float g;
      if (c < N) {
        g = sDL[c * kLL + r];
      } else {
        const int a = (c - N) / N, x = c - N - a * N;
        g = sDL[x * kLL + r] * ((sAct[r] == a ? 1.f : 0.f) - 1.f / (float)kA);
      }
      sL[c * kLL + r] = g;
    }
    __syncthreads();
    // ---- dz2 = (d heads Wh) gate'(h2); the heads' gradient
    for (int o = tid; o < H * kUB; o += 256) {
      const int k = o / kUB, r = o % kUB;
      const float* wc = sWh + k;
      float acc = 0.f;
      for (int c = 0; c < R; ++c) acc = fmaf(sL[c * kLL + r], wc[c * H], acc);
      sG2T[k * kLD + r] = gate_back<GATE>(acc, sH2T[k * kLD + r]);
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int c = cq + i * CPI;
      if (c < R) {
        float g = gWh[i];
#pragma unroll 1
        for (int r = 0; r < kUB; ++r) g = fmaf(sL[c * kLL + r], sH2T[kq * kLD + r], g);
        gWh[i] = g;
      }
    }
    if (tid < R) {
#pragma unroll 1
      for (int r = 0; r < kUB; ++r) gBh += sL[tid * kLL + r];
    }
    __syncthreads();
    // ---- dW2 += dz2 h1^T, db2 += dz2; dz1 = (dz2 W2) gate'(h1) into h2^T's place (its readers are behind the barrier)
#pragma unroll 1
    for (int r = 0; r < kUB; r += 4) {
      const f32x4 dz = *reinterpret_cast<const f32x4*>(&sG2T[u2 * kLD + r]);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(&sH1T[(k2 + i) * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gW2[i] = fmaf(dz[c], h[c], gW2[i]);
      }
      if (k2 == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gB2 += dz[c];
      }
    }
    block_layer<H, GATE, true, kUB>(sG2T, body.w2n, nullptr, sH1T, sH2T, H, tid);
    __syncthreads();
    // ---- dW1 += dz1 x^T, db1 += dz1
    if (tid < kS * H) {
#pragma unroll 1
      for (int r = 0; r < kUB; r += 4) {
        const f32x4 dz = *reinterpret_cast<const f32x4*>(&sH2T[u1 * kLD + r]);
        const f32x4 x = *reinterpret_cast<const f32x4*>(&sXT[j1 * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gW1 = fmaf(dz[c], x[c], gW1);
        if (j1 == 0) {
#pragma unroll
          for (int c = 0; c < 4; ++c) gB1 += dz[c];
        }
      }
    }
    __syncthreads();       // (the next block rewrites the slots, x^T and h2^T)
  }

  // ---- every element of the sixteen tensors, nothing between them: d mu as accumulated, d sigma = d mu * the layer's noise product
  float* __restrict__ Gd = io.grad;
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int e = u2 * H + k2 + i;
    Gd[net.l2.w_mu + e] = gW2[i];
    Gd[net.l2.w_sigma + e] = gW2[i] * (f.o2[u2] * f.i2[k2 + i]);
  }
  if (k2 == 0) {
    Gd[net.l2.b_mu + u2] = gB2;
    Gd[net.l2.b_sigma + u2] = gB2 * f.b2[u2];
  }
  if (tid < kS * H) {
    Gd[net.l1.w_mu + tid] = gW1;
    Gd[net.l1.w_sigma + tid] = gW1 * (f.o1[u1] * f.i1[j1]);
    if (j1 == 0) {
      Gd[net.l1.b_mu + u1] = gB1;
      Gd[net.l1.b_sigma + u1] = gB1 * f.b1[u1];
    }
  }
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int c = cq + i * CPI;
    if (c < N) {
      Gd[net.value.w_mu + c * H + kq] = gWh[i];
      Gd[net.value.w_sigma + c * H + kq] = gWh[i] * (f.ov[c] * f.iv[kq]);
    } else if (c < R) {
      Gd[net.advantage.w_mu + (c - N) * H + kq] = gWh[i];
      Gd[net.advantage.w_sigma + (c - N) * H + kq] = gWh[i] * (f.oa[c - N] * f.ia[kq]);
    }
  }
  if (tid < N) {
    Gd[net.value.b_mu + tid] = gBh;
    Gd[net.value.b_sigma + tid] = gBh * f.bv[tid];
  } else if (tid < R) {
    Gd[net.advantage.b_mu + tid - N] = gBh;
    Gd[net.advantage.b_sigma + tid - N] = gBh * f.ba[tid - N];
  }
  // ---- loss = mean_b KL_b w_b: the four waves' partial sums in wave order
  if (lane == 0) sRed[wave] = loss;
  __syncthreads();
  if (tid == 0) {
    io.out_loss[0] = (((sRed[0] + sRed[1]) + sRed[2]) + sRed[3]) * inv_rows;
    if (n_bad) *io.err = *io.err + n_bad;
  }
}

bool layer_ok(const dra_rainbow_mlp_layer& l) {
  return offsets_nonnegative({l.w_mu, l.w_sigma, l.b_mu, l.b_sigma, l.e_in, l.e_out, l.e_b});
}

bool net_ok(const dra_rainbow_mlp_net* net) {
  if (!layer_ok(net->l1) || !layer_ok(net->l2) || !layer_ok(net->value) || !layer_ok(net->advantage)) return false;
  return net->noise_stride >= 0 && net->v_max > net->v_min;      // (false for a NaN too)
}

int atoms_supported(int n_atoms) { return n_atoms < 2 || n_atoms > kMaxAtoms ? DRA_EINVAL : DRA_OK; }

}  // namespace

static_assert(act_lds_floats(64, kMaxAtoms) * sizeof(float) <= kLdsBytes, "the acting launch's LDS at the largest shape");
static_assert(update_lds_floats(64, kMaxAtoms) * sizeof(float) <= kLdsBytes, "the update's LDS at the largest shape");
static_assert(kUB % 4 == 0 && kUB * kS <= 256 && kMaxB % kUB == 0 && kMaxB <= 256 && (1 + kA) * kMaxAtoms <= 256, "the row block");

DRA_API int dra_rainbow_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate, int n_atoms) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate) || atoms_supported(n_atoms)) return DRA_EINVAL;
  if (act_lds_floats(hidden, n_atoms) * sizeof(float) > kLdsBytes) return DRA_EINVAL;
  return t_len < 1 || t_len > kMaxK ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_rainbow_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int n_atoms, int n_step) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate) || atoms_supported(n_atoms)) return DRA_EINVAL;
  if (update_lds_floats(hidden, n_atoms) * sizeof(float) > kLdsBytes) return DRA_EINVAL;
  if (n_step < 1 || n_step > kMaxNStep) return DRA_EINVAL;
  return batch < 1 || batch > kMaxB ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_rainbow_mlp_act(const dra_rainbow_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream) {
  if (!net || !io || !net->param || !net->noise) return DRA_EINVAL;
  if (dra_rainbow_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->t_len, net->gate, net->n_atoms)) return DRA_EINVAL;
  if (!net_ok(net) || !replay_act_io_ok(io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&rainbow_mlp_act_kernel<H, GATE>>(act_lds_floats(H, net->n_atoms) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_rainbow_mlp_eval(const dra_rainbow_mlp_net* net, const dra_mlp_eval_io* io, void* stream) {
  if (!net || !io || !net->param || !net->noise) return DRA_EINVAL;
  if (dra_rainbow_mlp_supported(net->state_dim, net->n_actions, net->hidden, 1, net->gate, net->n_atoms)) return DRA_EINVAL;
  if (!net_ok(net) || !mlp_eval_io_ok(io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&rainbow_mlp_eval_kernel<H, GATE>>(act_lds_floats(H, net->n_atoms) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_rainbow_mlp_update(const dra_rainbow_mlp_net* net, const dra_rainbow_mlp_update_io* io, void* stream) {
  if (!net || !io || !net->param || !net->target || !net->noise || !net->target_noise) return DRA_EINVAL;
  if (dra_rainbow_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->batch, net->gate, net->n_atoms, io->n_step))
    return DRA_EINVAL;
  if (!net_ok(net) || io->capacity < 1 + (int64_t)io->n_step || io->capacity > 0x7fffffff) return DRA_EINVAL;
  if (!io->ring_frames || !io->ring_actions || !io->ring_rewards || !io->ring_masks || !io->idx || !io->prob || !io->beta ||
      !io->grad || !io->out_loss || !io->out_loss_vec || !io->out_prio || !io->out_weights || !io->out_q_next || !io->out_target ||
      !io->err)
    return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&rainbow_mlp_update_kernel<H, GATE>>(update_lds_floats(H, net->n_atoms) * sizeof(float), net, io,
                                                                    stream);
  });
}
