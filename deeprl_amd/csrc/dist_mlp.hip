// dist_mlp: categorical_dqn_feature (examples.py:164-193: CategoricalDQNAgent, CategoricalNet over FCBody(state_dim), 50 atoms on
// [-100, 100]) and quantile_regression_dqn_feature (examples.py:101-127: QuantileRegressionDQNAgent, QuantileNet, 20 quantiles)
// with the environment (cartpole_env.h) and the replay ring (ring.hip's four arrays) resident on the device.  dqn_mlp.hip is the
// model: the same two launches with a head of A x N outputs.
//
//   dist_mlp_act_kernel      DQN_agent.py:23-45 with CategoricalDQN_agent.py:22-24 / QuantileRegressionDQN_agent.py:18-20 as the
//                            action values: wave a carries action a, lane j its atom j -- the logit, and over the wave the softmax
//                            and sum_j p_j z_j (categorical: c51_block.h) or the quantiles' mean.  The staged epsilon-greedy
//                            draws, the first maximum, the fp64 environment step, the ring row, the episode ring and the
//                            counters are dqn_mlp_act_kernel's: replay_act.h.
//   dist_mlp_update_kernel   CategoricalDQN_agent.py:60-89 / QuantileRegressionDQN_agent.py:55-77 and the whole backward as ONE
//                            launch of one workgroup over row blocks of 16 (the two heads leave no room for dqn_mlp's 64: the
//                            budget is update_lds_floats): the minibatch gathered from the ring, the target
//                            network's (categorical + double_q: and the online network's) forward of the next states, the
//                            projected target distribution (c51_block.h) or the target quantiles, the online forward of the
//                            states, the loss and its gradient with respect to all six tensors in the optimiser's flat gradient
//                            buffer.
//
//   dist_mlp_eval_kernel     the acting kernel's staging and forward over eval_act.h's loop (config.fused_eval): n_episodes greedy
//                            episodes of the evaluation environment in ONE launch.
//
//   dist_mlp_act_lanes_kernel, dist_mlp_update_kernel<.., LANES>, dist_mlp_eval_kernel<.., LANES>   the launches over n_lanes independent agents (seeds) of one
//                            shape and one atom count: workgroup (0, lane) reads ITS net and io struct from two tables and runs the
//                            single launch's text, so a lane carries the single launch's bits (seed_lanes.h; the end of the file).
//
// Plain fp32 VALU code, weights in LDS once per launch, every dot product one FMA chain in ascending k, every gradient element
// owned by ONE thread that adds its rows in ascending order: no atomics, the same bits on every launch.
#include "common.h"
#include "c51_block.h"
#include "mlp_update_block.h"
#include "eval_act.h"
#include "replay_act.h"
#include "seed_lanes.h"
#include <math.h>

namespace {

constexpr int kHeadCategorical = 1, kHeadQuantile = 2;
constexpr size_t kLdsBytes = 160 * 1024;

// ---------------------------------------------------------------------------------------------------- acting
__host__ __device__ constexpr size_t act_lds_floats(int H, int N) {
  return body_weight_floats(H) + (size_t)round_up4(kA * N * (H + 1)) + round_up4(kA * N) + round_up4(N)      // body, head, bias, z
         + (size_t)act_scratch_floats(H);
}

// (the launch's body: dist_mlp_act_kernel runs it on its kernel arguments, dist_mlp_act_lanes_kernel on its lane's row of two tables)
template <int H, int GATE, int HEAD>
__device__ __forceinline__ void dist_mlp_act_body(const dra_dist_mlp_net& net, const dra_dqn_mlp_act_io& io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.t_len, N = net.n_atoms, M = kA * N;

  const BodyWeights<H> body(lds);
  float* wq = lds + body_weight_floats(H);            // [M][H + 1]: lanes read consecutive rows, one bank apart
  float* bq = wq + round_up4(M * (H + 1));            // [M]
  float* sZ = bq + round_up4(M);                      // [N]
  const ActScratch<H> s(sZ + round_up4(N));
  s.zero(tid);
  ReplayActor actor;
  actor.begin(io, tid);                               // (ahead of the staging, for the register allocator: mlp_rollout.h's banner)
  const float* __restrict__ P = net.param;
  body.stage(P, net, tid);
  for (int i = tid; i < M * H; i += 256) {
    const int c = i / H, k = i - c * H;
    wq[c * (H + 1) + k] = P[net.wq + i];
  }
  for (int i = tid; i < M; i += 256) bq[i] = P[net.bq + i];
  if constexpr (HEAD == kHeadCategorical) {
    for (int i = tid; i < N; i += 256) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
  }
  __syncthreads();                                    // (thread 0 writes x^T next, over what other threads zeroed)

  const CartPoleRow row = episode_row(io);
  const double reward = 1.0 * io.reward_coef;         // what config.reward_normalizer(1.0) feeds

  for (int k = 0; k < K; ++k) {
    actor.observe(s.xT, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.xT, body.w1, body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, body.w2, body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    // ---- the head: wave a = action a, lane j = atom j; the action value over the wave
    if (tid < kA * kWave) {
      const int a = tid / kWave, j = tid % kWave;
      const bool live = j < N;
      float l = 0.f;
      if (live) {
        const float* wr = wq + (a * N + j) * (H + 1);
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < H; ++i) acc = fmaf(s.h2T[i * kNP], wr[i], acc);
        l = acc + bq[a * N + j];
      }
      float q, p;
      if constexpr (HEAD == kHeadCategorical) q = wave_softmax_value(l, live, sZ + j, p);
      else q = wave_sum(live ? l : 0.f) / (float)N;
      if (j == 0) {
        s.q[a] = q;
        io.out_q[k * kA + a] = q;
      }
    }
    __syncthreads();
    actor.step(io, row, s.q, reward, k, tid);
    // (thread 0 writes the next observation into x^T next: layer 1 of this step, its only reader, is three barriers back; q is
    // rewritten behind the three barriers of the next step)
  }
  __syncthreads();
  actor.finish(io, K, tid);
}

template <int H, int GATE, int HEAD>
__global__ void __launch_bounds__(256)
dist_mlp_act_kernel(dra_dist_mlp_net net, dra_dqn_mlp_act_io io) {
  dist_mlp_act_body<H, GATE, HEAD>(net, io);
}

// Lane blockIdx.y of n_lanes independent agents (seed_lanes.h): the workgroup reads ITS net and io struct from the two tables and
// runs the single launch's body.  Lanes share nothing.
template <int H, int GATE, int HEAD>
__global__ void __launch_bounds__(256)
dist_mlp_act_lanes_kernel(const dra_dist_mlp_net* __restrict__ nets, const dra_dqn_mlp_act_io* __restrict__ ios) {
  const dra_dist_mlp_net net = nets[blockIdx.y];
  const dra_dqn_mlp_act_io io = ios[blockIdx.y];
  dist_mlp_act_body<H, GATE, HEAD>(net, io);
}

// ---------------------------------------------------------------------------------------------------- evaluation
// dist_mlp_act_kernel's staging and forward over eval_act.h's loop: greedy, no ring row, until n_episodes episodes have ended.
//
// LANES: the evaluation of seed_batch.py's n_lanes independent agents in ONE launch -- two TABLES, workgroup (0, lane) reads its row
// of each and runs the text below as it is, with its own loop bound and its own done_word (dqn_mlp.hip's evaluation kernel; the
// figures: profiles/eval_lanes_kernel_resources.txt).  With LANES false the text and the argument list are the parent's.
template <int H, int GATE, int HEAD, bool LANES = false>
__global__ void __launch_bounds__(256)
dist_mlp_eval_kernel(lane_arg<LANES, dra_dist_mlp_net> net_arg, lane_arg<LANES, dra_mlp_eval_io> io_arg) {
  const auto& net = lane_struct(net_arg);
  const auto& io = lane_struct(io_arg);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.n_episodes * (int)io.horizon, N = net.n_atoms, M = kA * N;      // (K <= 65536: dra_mlp_eval_supported)

  const BodyWeights<H> body(lds);
  float* wq = lds + body_weight_floats(H);            // [M][H + 1]: lanes read consecutive rows, one bank apart
  float* bq = wq + round_up4(M * (H + 1));            // [M]
  float* sZ = bq + round_up4(M);                      // [N]
  const ActScratch<H> s(sZ + round_up4(N));
  int* done_word = eval_done_word(s);
  s.zero(tid);
  EvalActor actor;
  actor.begin(io, tid);
  const float* __restrict__ P = net.param;
  body.stage(P, net, tid);
  for (int i = tid; i < M * H; i += 256) {
    const int c = i / H, k = i - c * H;
    wq[c * (H + 1) + k] = P[net.wq + i];
  }
  for (int i = tid; i < M; i += 256) bq[i] = P[net.bq + i];
  if constexpr (HEAD == kHeadCategorical) {
    for (int i = tid; i < N; i += 256) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
  }
  __syncthreads();                                    // (thread 0 writes x^T next, over what other threads zeroed)

  for (int k = 0; k < K; ++k) {
    actor.observe(s.xT, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.xT, body.w1, body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, body.w2, body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    // ---- the head: wave a = action a, lane j = atom j; the action value over the wave
    if (tid < kA * kWave) {
      const int a = tid / kWave, j = tid % kWave;
      const bool live = j < N;
      float l = 0.f;
      if (live) {
        const float* wr = wq + (a * N + j) * (H + 1);
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < H; ++i) acc = fmaf(s.h2T[i * kNP], wr[i], acc);
        l = acc + bq[a * N + j];
      }
      float q, p;
      if constexpr (HEAD == kHeadCategorical) q = wave_softmax_value(l, live, sZ + j, p);
      else q = wave_sum(live ? l : 0.f) / (float)N;
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
constexpr int kMaxB = 256;       // rows of one minibatch

// the ONE statement of the update's LDS: the launch asks for it, dra_dist_mlp_update_supported refuses what does not fit
__host__ __device__ constexpr size_t update_lds_floats(int H, int N) {
  return 2 * (size_t)kS * H + 3 * (size_t)H * H + 4 * (size_t)H      // W1^T, W2^T, b1, b2 of both networks, the online W2 as stored
         + 2 * (size_t)kA * N * H + 2 * (size_t)round_up4(kA * N)    // the two heads, their biases
         + 4 * kUB + 4 * kA * kUB + (size_t)round_up4(N)             // idx, reward, mask, action; q_next x 2, two rows of stats; z / tau
         + (size_t)kS * kLD + 3 * (size_t)H * kLD                    // x^T, h1^T, h2^T (later dz1^T), dz2^T
         + 4 * (size_t)round_up4(N) * kLL;                           // next logits [2 N] (later partials, d logits), target, logits
}

__device__ __forceinline__ float huber1(float d) {
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}
__device__ __forceinline__ float huber1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)); }

// LANES: the launch of seed_batch.py's n_lanes independent agents -- the arguments are two TABLES and workgroup (0, lane) reads its
// row of each, then runs the text below as it is (seed_lanes.h).  A flag on this kernel and not a shared __device__ body, as in
// dqn_mlp.hip: with LANES false the text, the argument list and the figures are the parent's
// (profiles/dist_lanes_kernel_resources.txt).
template <int H, int GATE, int HEAD, bool LANES = false>
__global__ void __launch_bounds__(256)
dist_mlp_update_kernel(lane_arg<LANES, dra_dist_mlp_net> net_arg, lane_arg<LANES, dra_dist_mlp_update_io> io_arg) {
  const auto& net = lane_struct(net_arg);
  const auto& io = lane_struct(io_arg);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TPU = 256 / H;       // threads that share one unit's row of dW2
  constexpr int KPT = H / TPU;       // columns of it each carries
  constexpr int CPI = 256 / H;       // head rows between two consecutive elements a thread owns of the head's gradient
  constexpr int EPT = (kA * kMaxAtoms * H + 255) / 256;      // elements of it a thread owns at most
  constexpr bool CAT = HEAD == kHeadCategorical;
  const int tid = threadIdx.x;
  const int B = io.batch, N = net.n_atoms, M = kA * N;
  const int Mp = round_up4(M), Np = round_up4(N);
  const float* __restrict__ P = net.param;
  const float* __restrict__ PT = net.target;

  float* sW1 = lds;                       // [S][H]  (transposed: [k][unit])
  float* sW2 = sW1 + kS * H;              // [H][H]  (transposed)
  float* sW2N = sW2 + H * H;              // [H][H]  (as stored, [unit][k]: the backward's "transposed" operand)
  float* sB1 = sW2N + H * H;              // [H]
  float* sB2 = sB1 + H;                   // [H]
  float* sWq = sB2 + H;                   // [M][H]
  float* sBq = sWq + M * H;               // [M] (+ pad)
  float* tW1 = sBq + Mp;                  // the target network's, as above without the untransposed W2
  float* tW2 = tW1 + kS * H;
  float* tB1 = tW2 + H * H;
  float* tB2 = tB1 + H;
  float* tWq = tB2 + H;
  float* tBq = tWq + M * H;
  int* sIdx = reinterpret_cast<int*>(tBq + Mp);       // [kUB]: the block's ring slots, clamped
  float* sRew = reinterpret_cast<float*>(sIdx + kUB);      // [kUB]
  float* sMsk = sRew + kUB;               // [kUB]
  int* sAct = reinterpret_cast<int*>(sMsk + kUB);     // [kUB]
  float* sQN = reinterpret_cast<float*>(sAct + kUB);       // [A][kUB]: the target network's action values of the next states
  float* sQO = sQN + kA * kUB;            // [A][kUB]: the online network's (categorical + double_q)
  float* sSa = sQO + kA * kUB;            // [A][kUB]: a softmax's maxima; later row maxima [kUB] and the targets' sums [kUB]
  float* sSb = sSa + kA * kUB;            // [A][kUB]: a softmax's sums
  float* sZ = sSb + kA * kUB;             // [N] (+ pad): the atoms (categorical) or tau (quantile)
  float* sXT = sZ + Np;                   // [S][kLD]
  float* sH1T = sXT + kS * kLD;           // [H][kLD]
  float* sH2T = sH1T + H * kLD;           // [H][kLD]: h2^T, then dz1^T
  float* sG2T = sH2T + H * kLD;           // [H][kLD]: dz2^T
  float* sL = sG2T + H * kLD;             // [2 Np][kLL]: the next states' logits / quantiles [M]; later the loss partials [N]
  float* sDL = sL + Np * kLL;             //   and, in its second half, d loss / d logits of the action taken [N]
  float* sT = sL + 2 * Np * kLL;          // [N][kLL]: the projected target probabilities, or the target quantiles
  float* sLo = sT + Np * kLL;             // [N][kLL]: the online logits / quantiles of the action taken

  for (int i = tid; i < kS * H; i += 256) {
    const int k = i / H, u = i - k * H;
    sW1[i] = P[net.w1 + u * kS + k];
    tW1[i] = PT[net.w1 + u * kS + k];
  }
  for (int i = tid; i < H * H; i += 256) {
    const int k = i / H, u = i - k * H;
    sW2[i] = P[net.w2 + u * H + k];
    sW2N[i] = P[net.w2 + i];
    tW2[i] = PT[net.w2 + u * H + k];
  }
  for (int i = tid; i < H; i += 256) {
    sB1[i] = P[net.b1 + i];
    sB2[i] = P[net.b2 + i];
    tB1[i] = PT[net.b1 + i];
    tB2[i] = PT[net.b2 + i];
  }
  for (int i = tid; i < M * H; i += 256) {
    sWq[i] = P[net.wq + i];
    tWq[i] = PT[net.wq + i];
  }
  for (int i = tid; i < M; i += 256) {
    sBq[i] = P[net.bq + i];
    tBq[i] = PT[net.bq + i];
  }
  for (int i = tid; i < N; i += 256) {
    if constexpr (CAT) sZ[i] = atom_value(net.v_min, net.v_max, N, i);
    else sZ[i] = (float)((double)(2 * i + 1) / (2.0 * (double)N));       // QuantileRegressionDQN_agent.py:39-40
  }
  const float gamma = (float)io.discount;
  const float v_min = (float)net.v_min, v_max = (float)net.v_max;
  const float delta = (float)((net.v_max - net.v_min) / (double)(N - 1));       // CategoricalDQN_agent.py:37
  const int64_t last = io.capacity - 2;      // the last slot with a next frame behind it
  const bool double_q = CAT && io.double_q != 0;      // (QuantileRegressionDQN_agent.py:59-61 has no double_q)
  int n_bad = 0;

  // what this thread owns of the gradient
  const int u2 = tid / TPU, k2 = (tid % TPU) * KPT;       // dW2 [u2][k2 .. k2 + KPT), db2 [u2] on the first of the unit's threads
  float gW2[KPT], gB2 = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i) gW2[i] = 0.f;
  const int u1 = tid / kS, j1 = tid % kS;                 // dW1 [u1][j1] (tid < S H), db1 [u1] where j1 == 0
  float gW1 = 0.f, gB1 = 0.f;
  const int cq = tid / H, kq = tid % H;                   // the head's dW [cq + i CPI][kq], i < EPT; db [tid] (tid < M)
  float gWq[EPT], gBq = 0.f;
#pragma unroll
  for (int i = 0; i < EPT; ++i) gWq[i] = 0.f;
  float loss = 0.f;                                       // categorical: the KL of row tid of every block; quantile: element tid of the vector
  const float inv_rows = 1.f / (float)B;
  const float inv_nb = 1.f / ((float)N * (float)B);

  for (int r0 = 0; r0 < B; r0 += kUB) {
    const int rows = B - r0 < kUB ? B - r0 : kUB;
    // ---- the block's ring slots (clamped into [0, capacity - 2]: no read leaves the ring), reward, mask, action
    if (tid < kUB) {
      int64_t i = 0;
      bool bad = false;
      float rew = 0.f, msk = 0.f;
      int a = 0;
      if (tid < rows) {
        i = io.idx[r0 + tid];
        bad = i < 0 || i > last;
        i = i < 0 ? 0 : (i > last ? last : i);
        rew = (float)io.ring_rewards[i];
        msk = (float)io.ring_masks[i];
        a = io.ring_actions[i] == 1 ? 1 : 0;
      }
      n_bad += __popcll(__ballot(bad ? 1 : 0));
      sIdx[tid] = (int)i;
      sRew[tid] = rew;
      sMsk[tid] = msk;
      sAct[tid] = a;
    }
    __syncthreads();
    // ---- the next states: with double_q the ONLINE network's action values first
    gather_states<kUB>(io.ring_frames, sIdx, 1, rows, sXT, tid);
    __syncthreads();
    if (double_q) {
      block_layer<H, GATE, false, kUB>(sXT, sW1, sB1, nullptr, sH1T, kS, tid);
      __syncthreads();
      block_layer<H, GATE, false, kUB>(sH1T, sW2, sB2, nullptr, sH2T, H, tid);
      __syncthreads();
      block_head<H, kUB>(sH2T, sWq, sBq, sL, M, kLL, tid);
      __syncthreads();
      if (tid < kA * kUB) {                               // sum_j softmax_j z_j per (action, row)
        const float* l = sL + (tid / kUB) * N * kLL + tid % kUB;
        float m = l[0];
        for (int j = 1; j < N; ++j) m = fmaxf(m, l[j * kLL]);
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += expf(l[j * kLL] - m);
        float q = 0.f;
        for (int j = 0; j < N; ++j) q = fmaf(expf(l[j * kLL] - m) / s, sZ[j], q);
        sQO[tid] = q;
      }
      __syncthreads();
    }
    // ---- the TARGET network's logits / quantiles of the next states, [M][rows]
    block_layer<H, GATE, false, kUB>(sXT, tW1, tB1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, tW2, tB2, nullptr, sH2T, H, tid);
    __syncthreads();
    block_head<H, kUB>(sH2T, tWq, tBq, sL, M, kLL, tid);
    __syncthreads();
    if constexpr (CAT) {
      // softmax over the atoms of every (action, row): the maxima, exp in place, the sums, p in place, q = sum_j p_j z_j
      if (tid < kA * kUB) {
        const float* l = sL + (tid / kUB) * N * kLL + tid % kUB;
        float m = l[0];
        for (int j = 1; j < N; ++j) m = fmaxf(m, l[j * kLL]);
        sSa[tid] = m;
      }
      __syncthreads();
      for (int o = tid; o < M * kUB; o += 256) {
        const int c = o / kUB, r = o % kUB;
        sL[c * kLL + r] = expf(sL[c * kLL + r] - sSa[(c / N) * kUB + r]);
      }
      __syncthreads();
      if (tid < kA * kUB) {
        const float* l = sL + (tid / kUB) * N * kLL + tid % kUB;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += l[j * kLL];
        sSb[tid] = s;
      }
      __syncthreads();
      for (int o = tid; o < M * kUB; o += 256) {
        const int c = o / kUB, r = o % kUB;
        sL[c * kLL + r] = sL[c * kLL + r] / sSb[(c / N) * kUB + r];
      }
      __syncthreads();
      if (tid < kA * kUB) {
        const float* p = sL + (tid / kUB) * N * kLL + tid % kUB;
        float q = 0.f;
        for (int j = 0; j < N; ++j) q = fmaf(p[j * kLL], sZ[j], q);
        sQN[tid] = q;
        if (tid % kUB < rows) io.out_q_next[(int64_t)(r0 + tid % kUB) * kA + tid / kUB] = q;
      }
    } else {
      if (tid < kA * kUB) {
        const float* l = sL + (tid / kUB) * N * kLL + tid % kUB;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += l[j * kLL];
        sQN[tid] = s;                                      // (the argmax is over the sums: QuantileRegressionDQN_agent.py:60)
        if (tid % kUB < rows) io.out_q_next[(int64_t)(r0 + tid % kUB) * kA + tid / kUB] = s / (float)N;
      }
    }
    __syncthreads();
    // ---- the target of every row, [N][rows]: the next action is the FIRST maximum (torch.argmax)
    for (int o = tid; o < N * kUB; o += 256) {
      const int i = o / kUB, r = o % kUB;
      const float* qa = double_q ? sQO : sQN;
      const int an = qa[kUB + r] > qa[r] ? 1 : 0;
      const float gm = __fmul_rn(gamma, sMsk[r]);
      float t;
      if constexpr (CAT) {
        t = c51_project(sZ, sL + an * N * kLL + r, kLL, N, sZ[i], sRew[r], gm, v_min, v_max, delta);      // CategoricalDQN_agent.py:72-78
      } else {
        t = __fadd_rn(sRew[r], __fmul_rn(gm, sL[(an * N + i) * kLL + r]));
      }
      sT[i * kLL + r] = t;
      if (r < rows) io.out_target[(int64_t)(r0 + r) * N + i] = t;
    }
    // ---- the states: the online forward (x^T's and h^T's readers are behind the barriers above)
    gather_states<kUB>(io.ring_frames, sIdx, 0, rows, sXT, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, sW1, sB1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, sW2, sB2, nullptr, sH2T, H, tid);
    __syncthreads();
    // ---- the logits / quantiles of the action taken, [N][rows]
    for (int o = tid; o < N * kUB; o += 256) {
      const int i = o / kUB, r = o % kUB;
      const int c = sAct[r] * N + i;
      const float* wr = sWq + c * H;
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) acc = fmaf(sH2T[k * kLD + r], wr[k], acc);
      sLo[i * kLL + r] = acc + sBq[c];
    }
    __syncthreads();
    // ---- the loss and d loss / d logits (0 behind the last row)
    if constexpr (CAT) {
      // KL = sum_i t_i log(t_i + 1e-5) - t_i log_softmax_i; d logits = (softmax sum t - t) / B
      if (tid < kUB) {
        const float* l = sLo + tid;
        const float* t = sT + tid;
        float m = l[0];
        for (int i = 1; i < N; ++i) m = fmaxf(m, l[i * kLL]);
        float s = 0.f;
        for (int i = 0; i < N; ++i) s += expf(l[i * kLL] - m);
        const float ls = logf(s);
        float kl = 0.f, st = 0.f;
        for (int i = 0; i < N; ++i) {
          const float ti = t[i * kLL];
          kl += ti * logf(ti + 1e-5f) - ti * ((l[i * kLL] - m) - ls);
          st += ti;
        }
        if (tid < rows) {
          io.out_loss_vec[r0 + tid] = kl;
          loss += kl;
        }
        sSa[tid] = m;
        sSa[kUB + tid] = st;
        sSb[tid] = s;
      }
      __syncthreads();
      for (int o = tid; o < N * kUB; o += 256) {
        const int i = o / kUB, r = o % kUB;
        const float p = expf(sLo[i * kLL + r] - sSa[r]) / sSb[r];
        sDL[i * kLL + r] = r < rows ? (p * sSa[kUB + r] - sT[i * kLL + r]) * inv_rows : 0.f;
      }
    } else {
      // d = T theta_j - theta_i; partial [x][r] = sum_i huber(d) |tau_i - 1[d < 0]| of target quantile x;
      // d theta_x = -(1 / (N B)) sum_j huber'(d) |tau_x - 1[d < 0]|
      for (int o = tid; o < N * kUB; o += 256) {
        const int x = o / kUB, r = o % kUB;
        const float tx = sT[x * kLL + r], thx = sLo[x * kLL + r], taux = sZ[x];
        float part = 0.f, g = 0.f;
        for (int y = 0; y < N; ++y) {
          const float d = tx - sLo[y * kLL + r];
          part += huber1(d) * fabsf(sZ[y] - (d < 0.f ? 1.f : 0.f));
          const float e = sT[y * kLL + r] - thx;
          g += huber1_grad(e) * fabsf(taux - (e < 0.f ? 1.f : 0.f));
        }
        sL[x * kLL + r] = part;
        sDL[x * kLL + r] = r < rows ? -g * inv_nb : 0.f;
      }
      __syncthreads();
      if (tid < N) {
        for (int r = 0; r < rows; ++r) loss += sL[tid * kLL + r];
      }
    }
    __syncthreads();
    // ---- dz2 = (d logits Wq[a]) gate'(h2); the head's gradient
    for (int o = tid; o < H * kUB; o += 256) {
      const int k = o / kUB, r = o % kUB;
      const float* wc = sWq + sAct[r] * N * H + k;
      float acc = 0.f;
      for (int i = 0; i < N; ++i) acc = fmaf(sDL[i * kLL + r], wc[i * H], acc);
      sG2T[k * kLD + r] = gate_back<GATE>(acc, sH2T[k * kLD + r]);
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int c = cq + i * CPI;
      if (c < M) {
        const int a = c / N, x = c - a * N;
        float g = gWq[i];
#pragma unroll 1
        for (int r = 0; r < kUB; ++r) g = fmaf(sAct[r] == a ? sDL[x * kLL + r] : 0.f, sH2T[kq * kLD + r], g);
        gWq[i] = g;
      }
    }
    if (tid < M) {
      const int a = tid / N, x = tid - a * N;
#pragma unroll 1
      for (int r = 0; r < kUB; ++r) gBq += sAct[r] == a ? sDL[x * kLL + r] : 0.f;
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
    block_layer<H, GATE, true, kUB>(sG2T, sW2N, nullptr, sH1T, sH2T, H, tid);
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

  // ---- every element of the six tensors, nothing between them
  float* __restrict__ Gd = io.grad;
#pragma unroll
  for (int i = 0; i < KPT; ++i) Gd[net.w2 + u2 * H + k2 + i] = gW2[i];
  if (k2 == 0) Gd[net.b2 + u2] = gB2;
  if (tid < kS * H) {
    Gd[net.w1 + tid] = gW1;
    if (j1 == 0) Gd[net.b1 + u1] = gB1;
  }
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int c = cq + i * CPI;
    if (c < M) Gd[net.wq + c * H + kq] = gWq[i];
  }
  if (tid < M) Gd[net.bq + tid] = gBq;
  // ---- the loss: categorical mean_b KL_b; quantile the vector's element j = mean_b of its sums, the loss their mean
  float* sRed = sL;
  const int n_red = CAT ? kUB : N;
  if constexpr (CAT) {
    if (tid < kUB) sRed[tid] = loss;
  } else {
    if (tid < N) {
      const float v = loss * inv_rows;
      io.out_loss_vec[tid] = v;
      sRed[tid] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < n_red; ++i) s += sRed[i];
    io.out_loss[0] = CAT ? s * inv_rows : s / (float)N;
    if (n_bad) *io.err = *io.err + n_bad;
  }
}

bool net_ok(const dra_dist_mlp_net* net) {
  if (!offsets_nonnegative({net->w1, net->b1, net->w2, net->b2, net->wq, net->bq})) return false;
  if (net->head == kHeadCategorical) return net->v_max > net->v_min;      // (false for a NaN too)
  return net->head == kHeadQuantile;
}

int head_supported(int head, int n_atoms) {
  if (head != kHeadCategorical && head != kHeadQuantile) return DRA_EINVAL;
  return n_atoms < 2 || n_atoms > kMaxAtoms ? DRA_EINVAL : DRA_OK;
}

// f(hidden, gate, head) as std::integral_constant: the instance of a kernel template
template <typename F>
int dispatch_hidden_gate_head(int hidden, int gate, int head, F&& f) {
  return dispatch_hidden_gate(hidden, gate, [&](auto h, auto g) {
    return head == kHeadCategorical ? f(h, g, std::integral_constant<int, kHeadCategorical>{})
                                    : f(h, g, std::integral_constant<int, kHeadQuantile>{});
  });
}

}  // namespace

static_assert(update_lds_floats(64, kMaxAtoms) * sizeof(float) <= kLdsBytes, "the update's LDS at the largest shape");
static_assert(kUB % 4 == 0 && kUB * kS <= 256 && kA * kUB <= 256, "the row block");

DRA_API int dra_dist_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate, int head, int n_atoms) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate) || head_supported(head, n_atoms)) return DRA_EINVAL;
  if (act_lds_floats(hidden, n_atoms) * sizeof(float) > kLdsBytes) return DRA_EINVAL;
  return t_len < 1 || t_len > kMaxK ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_dist_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int head, int n_atoms) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate) || head_supported(head, n_atoms)) return DRA_EINVAL;
  if (update_lds_floats(hidden, n_atoms) * sizeof(float) > kLdsBytes) return DRA_EINVAL;
  return batch < 1 || batch > kMaxB ? DRA_EINVAL : DRA_OK;
}

// what dra_dist_mlp_act asks of its two structs (dra_dist_mlp_act_lanes: of every lane's)
static bool act_args_ok(const dra_dist_mlp_net* net, const dra_dqn_mlp_act_io* io) {
  if (!net->param) return false;
  if (dra_dist_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->t_len, net->gate, net->head, net->n_atoms)) return false;
  return net_ok(net) && replay_act_io_ok(io);
}

DRA_API int dra_dist_mlp_act(const dra_dist_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream) {
  if (!net || !io || !act_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(net->hidden, net->gate, net->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_one_workgroup<&dist_mlp_act_kernel<H, GATE, HEAD>>(act_lds_floats(H, net->n_atoms) * sizeof(float), net, io, stream);
  });
}

// what dra_dist_mlp_eval asks of its two structs (dra_dist_mlp_eval_lanes: of every lane's)
static bool eval_args_ok(const dra_dist_mlp_net* net, const dra_mlp_eval_io* io) {
  if (!net->param) return false;
  if (dra_dist_mlp_supported(net->state_dim, net->n_actions, net->hidden, 1, net->gate, net->head, net->n_atoms)) return false;
  return net_ok(net) && mlp_eval_io_ok(io);
}

DRA_API int dra_dist_mlp_eval(const dra_dist_mlp_net* net, const dra_mlp_eval_io* io, void* stream) {
  if (!net || !io || !eval_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(net->hidden, net->gate, net->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_one_workgroup<&dist_mlp_eval_kernel<H, GATE, HEAD>>(act_lds_floats(H, net->n_atoms) * sizeof(float), net, io, stream);
  });
}

// what dra_dist_mlp_update asks of its two structs (dra_dist_mlp_update_lanes: of every lane's)
static bool update_args_ok(const dra_dist_mlp_net* net, const dra_dist_mlp_update_io* io) {
  if (!net->param || !net->target) return false;
  if (dra_dist_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->batch, net->gate, net->head, net->n_atoms))
    return false;
  if (!net_ok(net) || io->capacity < 2 || io->capacity > 0x7fffffff) return false;
  return io->ring_frames && io->ring_actions && io->ring_rewards && io->ring_masks && io->idx && io->grad && io->out_loss &&
         io->out_loss_vec && io->out_q_next && io->out_target && io->err;
}

DRA_API int dra_dist_mlp_update(const dra_dist_mlp_net* net, const dra_dist_mlp_update_io* io, void* stream) {
  if (!net || !io || !update_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(net->hidden, net->gate, net->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_one_workgroup<&dist_mlp_update_kernel<H, GATE, HEAD>>(update_lds_floats(H, net->n_atoms) * sizeof(float), net, io,
                                                                       stream);
  });
}

// ---------------------------------------------------------------------------------------------------- seed lanes
// n_lanes independent categorical_dqn_feature / quantile_regression_dqn_feature agents of ONE shape as workgroups (0, lane) of the
// same launches (seed_batch.py; the tables' memory: seed_lanes.h).  The lanes share the kernel instance (hidden, gate, head) and
// the launch's dynamic LDS size, which follows from lane 0's n_atoms: n_atoms is part of the shape.  v_min / v_max are per-lane data.
// The update's workgroup holds up to 160 KiB of LDS: one workgroup per CU, 64 lanes on 64 of the 256 CUs, nobody waits for anybody.
static bool same_shape(const dra_dist_mlp_net* a, const dra_dist_mlp_net* b) {
  return a->state_dim == b->state_dim && a->n_actions == b->n_actions && a->hidden == b->hidden && a->gate == b->gate &&
         a->head == b->head && a->n_atoms == b->n_atoms;
}

DRA_API int dra_dist_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int head, int n_atoms,
                                         int n_lanes) {
  if (n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  if (dra_dist_mlp_supported(state_dim, n_actions, hidden, t_len, gate, head, n_atoms)) return DRA_EINVAL;
  return dra_dist_mlp_update_supported(state_dim, n_actions, hidden, batch, gate, head, n_atoms);
}

DRA_API int dra_dist_mlp_act_lanes(const dra_dist_mlp_net* nets, const dra_dqn_mlp_act_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!act_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(nets->hidden, nets->gate, nets->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_lanes<&dist_mlp_act_lanes_kernel<H, GATE, HEAD>>(act_lds_floats(H, nets->n_atoms) * sizeof(float), nets, ios, n_lanes,
                                                                  stream);
  });
}

DRA_API int dra_dist_mlp_update_lanes(const dra_dist_mlp_net* nets, const dra_dist_mlp_update_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!update_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(nets->hidden, nets->gate, nets->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_lanes<&dist_mlp_update_kernel<H, GATE, HEAD, true>>(update_lds_floats(H, nets->n_atoms) * sizeof(float), nets, ios,
                                                                     n_lanes, stream);
  });
}

// n_lanes evaluations in one launch (dra_mlp_eval_lanes_supported: dqn_mlp.hip): lane l runs ios[l].n_episodes episodes of at most
// ios[l].horizon steps (both per lane) on nets[l] and leaves on its own
DRA_API int dra_dist_mlp_eval_lanes(const dra_dist_mlp_net* nets, const dra_mlp_eval_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!eval_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate_head(nets->hidden, nets->gate, nets->head, [&](auto h, auto g, auto hd) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value, HEAD = decltype(hd)::value;
    return launch_lanes<&dist_mlp_eval_kernel<H, GATE, HEAD, true>>(act_lds_floats(H, nets->n_atoms) * sizeof(float), nets, ios, n_lanes,
                                                                   stream);
  });
}
