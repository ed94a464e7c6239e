// dqn_mlp: dqn_feature (examples.py:11-52: DQNAgent over one cart-pole, VanillaNet over FCBody(state_dim), RMSprop, a uniform replay
// of 10^4 transitions, minibatches of 10, four transitions per update, a target network copied every 200 updates) with the
// environment (cartpole_env.h) and the replay ring (ring.hip's four arrays) resident on the device.
//
//   dqn_mlp_act_kernel      DQN_agent.py:23-45, sgd_update_frequency times, as ONE launch of one workgroup: the observation narrowed
//                           to float32 (what tensor() uploads), the body (4 -> H -> H, relu or tanh), q, the epsilon-greedy action
//                           -- the draws are made by the host ahead of the launch, in the reference's order, and read from fixed
//                           addresses --, the environment step, and the transition written straight into the ring at
//                           (*slot0 + k) % capacity; one appended row of the episode ring per episode that ended.
//   dqn_mlp_update_kernel   DQN_agent.py:81-99, 128-133 and the whole backward as ONE launch of one workgroup: the minibatch gathered
//                           from the ring by the staged indices (state = frame idx, next state = frame idx + 1), the TARGET
//                           network's (double_q: and the online network's) forward of the next states, q_target, the online
//                           forward of the states, 0.5 mean (q_target - q_a)^2 and its gradient with respect to all six tensors,
//                           written into the optimiser's flat gradient buffer at the parameters' own offsets.  A template on its io
//                           struct: over dra_dqn_replay_mlp_update_io (config.fused_dqn_replay_feature) the same block steps run over
//                           an n-step window (replay.py:135-139's fold in fp64) with optional priorities and importance weights
//                           (DQN_agent.py:120-127).
//
//   dqn_mlp_eval_kernel     BaseAgent.py:38-60 over DQN_agent.py:70-76 as ONE launch of one workgroup (config.fused_eval): the acting
//                           kernel's staging and forward over eval_act.h's loop -- greedy, no ring row -- until n_episodes episodes
//                           of the evaluation environment have ended.
//
//   dqn_mlp_act_lanes_kernel, dqn_mlp_update_kernel<.., LANES>, dqn_mlp_eval_kernel<.., LANES>   the launches over n_lanes independent agents (seeds) of one shape:
//                           workgroup (0, lane) reads ITS net and io struct from two tables and runs the single launch's text, so a
//                           lane carries the single launch's bits.  Lanes share nothing and wait for nobody (the end of the file).
//                           The update's lane form exists over both io structs (dra_dqn_mlp_update_lanes; over the window:
//                           dra_dqn_replay_mlp_update_lanes, one n_step for all lanes).
//
// Both are q_mlp.hip's kernels with the replay between them: latency-bound chains over a few rows, plain fp32 VALU code, weights in
// LDS once per launch, activations TRANSPOSED and read 16 bytes at a time, every dot product one FMA chain in ascending k.  The
// update walks the rows in blocks of 64; every gradient element is owned by ONE thread that adds its rows in ascending order:
// no atomics, the same bits on every launch.  The acting kernel's weights are cartpole_rollout.h's QNetWeights<H>, its frame (the
// scratch, the ring cursor, the wave-0 block, the epilogue, the io check) is replay_act.h's, shared with dist_mlp.hip and
// rainbow_mlp.hip; the update's layers, gather and head forward are mlp_update_block.h's.  The staging of the two networks' bodies
// and the gradient bookkeeping are written in place (mlp_rollout.h's banner: the figures).
#include "common.h"
#include "mlp_update_block.h"
#include "eval_act.h"
#include "replay_act.h"
#include "seed_lanes.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------- acting
__host__ __device__ constexpr size_t act_lds_floats(int H) { return q_net_weight_floats(H) + (size_t)act_scratch_floats(H); }

// (the launch's body: dqn_mlp_act_kernel runs it on its kernel arguments, dqn_mlp_act_lanes_kernel on its lane's row of two tables)
template <int H, int GATE>
__device__ __forceinline__ void dqn_mlp_act_body(const dra_q_mlp_net& net, const dra_dqn_mlp_act_io& io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.t_len;

  const QNetWeights<H> online(lds);
  const ActScratch<H> s(lds + q_net_weight_floats(H));
  s.zero(tid);
  ReplayActor actor;
  actor.begin(io, tid);                               // (ahead of the staging, for the register allocator: mlp_rollout.h's banner)
  online.stage(net.param, net, tid);
  __syncthreads();                                    // (thread 0 writes x^T next, over what other threads zeroed)

  const CartPoleRow row = episode_row(io);
  const double reward = 1.0 * io.reward_coef;         // what config.reward_normalizer(1.0) feeds

  for (int k = 0; k < K; ++k) {
    actor.observe(s.xT, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.xT, online.body.w1, online.body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, online.body.w2, online.body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    if (tid < kA) {
      const float* wr = online.wq + tid * (H + 1);
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < H; ++j) acc = fmaf(s.h2T[j * kNP], wr[j], acc);
      acc += online.bq[tid];
      s.q[tid] = acc;
      io.out_q[k * kA + tid] = acc;
    }
    __syncthreads();
    actor.step(io, row, s.q, reward, k, tid);
    // (thread 0 writes the next observation into x^T next: layer 1 of this step, its only reader, is three barriers back; q is
    // rewritten behind the three barriers of the next step)
  }
  __syncthreads();
  actor.finish(io, K, tid);
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
dqn_mlp_act_kernel(dra_q_mlp_net net, dra_dqn_mlp_act_io io) {
  dqn_mlp_act_body<H, GATE>(net, io);
}

// Lane blockIdx.y of n_lanes independent agents: the workgroup reads ITS net and io struct from the two tables (uniform addresses:
// scalar loads, as the single launch reads its kernel arguments) and runs the single launch's body.  Lanes share nothing.
template <int H, int GATE>
__global__ void __launch_bounds__(256)
dqn_mlp_act_lanes_kernel(const dra_q_mlp_net* __restrict__ nets, const dra_dqn_mlp_act_io* __restrict__ ios) {
  const dra_q_mlp_net net = nets[blockIdx.y];
  const dra_dqn_mlp_act_io io = ios[blockIdx.y];
  dqn_mlp_act_body<H, GATE>(net, io);
}

// ---------------------------------------------------------------------------------------------------- evaluation
// dqn_mlp_act_kernel's staging and forward over eval_act.h's loop: greedy, no ring row, until n_episodes episodes have ended.
//
// LANES: the evaluation of seed_batch.py's n_lanes independent agents in ONE launch -- the arguments are two TABLES and workgroup
// (0, lane) reads its row of each, then runs the text below as it is: its own K = n_episodes * horizon, its own done_word in its
// own LDS, so a lane leaves when ITS episodes have ended and waits for nobody.  A flag on this kernel (lane_arg / lane_struct:
// seed_lanes.h), as on the update kernel: with LANES false the text, the argument list and the figures are the parent's.  A shared
// __device__ body under two kernels gives the same figures here, single and lane (profiles/eval_lanes_kernel_resources.txt): the
// flag keeps one kernel text.
template <int H, int GATE, bool LANES = false>
__global__ void __launch_bounds__(256)
dqn_mlp_eval_kernel(lane_arg<LANES, dra_q_mlp_net> net_arg, lane_arg<LANES, dra_mlp_eval_io> io_arg) {
  const auto& net = lane_struct(net_arg);
  const auto& io = lane_struct(io_arg);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int K = io.n_episodes * (int)io.horizon;      // (<= 65536: dra_mlp_eval_supported)

  const QNetWeights<H> online(lds);
  const ActScratch<H> s(lds + q_net_weight_floats(H));
  int* done_word = eval_done_word(s);
  s.zero(tid);
  EvalActor actor;
  actor.begin(io, tid);
  online.stage(net.param, net, tid);
  __syncthreads();                                    // (thread 0 writes x^T next, over what other threads zeroed)

  for (int k = 0; k < K; ++k) {
    actor.observe(s.xT, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.xT, online.body.w1, online.body.b1, s.h1T, kS, kNP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(s.h1T, online.body.w2, online.body.b2, s.h2T, H, kNP, tid);
    __syncthreads();
    if (tid < kA) {
      const float* wr = online.wq + tid * (H + 1);
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < H; ++j) acc = fmaf(s.h2T[j * kNP], wr[j], acc);
      acc += online.bq[tid];
      s.q[tid] = acc;
      if (io.out_q) io.out_q[k * kA + tid] = acc;
    }
    __syncthreads();
    actor.step(io, s.q, done_word, tid);
    __syncthreads();
    if (*done_word >= io.n_episodes) break;           // every thread reads the same word: eval_act.h's banner
  }
  actor.finish(io, tid);                              // (thread 0's own words: nothing to wait for)
}

// ---------------------------------------------------------------------------------------------------- the update
constexpr int kUB = 64;          // rows of one block
constexpr int kLD = kUB + 4;     // row stride of the transposed activations: 16-byte aligned, consecutive units 4 banks apart
constexpr int kMaxB = 256;       // rows of one minibatch
constexpr int kMaxNStep = 8;     // the longest window (rainbow_mlp.hip's)

__host__ __device__ constexpr size_t update_lds_floats(int H) {
  return (size_t)kS * H + 2 * (size_t)H * H + 2 * (size_t)H + (size_t)kA * H + 4      // online: W1^T, W2^T, W2, b1, b2, head, its bias
         + (size_t)kS * H + (size_t)H * H + 2 * (size_t)H + (size_t)kA * H + 4        // target: W1^T, W2^T, b1, b2, head, its bias
         + 6 * kUB + 4 * kUB                                                          // idx, reward, mask, d, action, loss; the two q_next
         + (size_t)kS * kLD + 3 * (size_t)H * kLD;                                    // x^T, h1^T, h2^T (later dz1^T), dz2^T
}
// (the window's kernel: the minibatch's raw importance weights behind them)
__host__ __device__ constexpr size_t replay_update_lds_floats(int H) { return update_lds_floats(H) + kMaxB; }

// IO = dra_dqn_mlp_update_io: DQN_agent.py:81-99 over 1-step rows.  IO = dra_dqn_replay_mlp_update_io (WINDOW): the same block steps
// over an n-step window (the fold of replay.py:135-139, the next state n_step frames on) and, where io.prob is set, the priorities and
// importance weights of DQN_agent.py:120-127 (td_loss_kernel's arithmetic); with prob NULL and n_step 1 the 1-step kernel's bits.
//
// LANES: the launch of seed_batch.py's n_lanes independent agents -- the arguments are two TABLES and workgroup (0, lane) reads its
// row of each (uniform addresses: scalar loads, as the single launch reads its kernel arguments), then runs the text below as it
// is.  A flag on this kernel and not a shared __device__ body: hoisted, dqn_mlp_update_kernel<16, tanh> went 70 -> 78 VGPRs (71 ->
// 80 over the window's io) -- mlp_rollout.h's banner; with LANES false the figures are the parent's
// (profiles/dqn_lanes_kernel_resources.txt).  lane_arg / lane_struct: seed_lanes.h.
template <int H, int GATE, typename IO, bool LANES = false>
__global__ void __launch_bounds__(256)
dqn_mlp_update_kernel(lane_arg<LANES, dra_q_mlp_net> net_arg, lane_arg<LANES, IO> io_arg) {
  const auto& net = lane_struct(net_arg);
  const auto& io = lane_struct(io_arg);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool WINDOW = std::is_same<IO, dra_dqn_replay_mlp_update_io>::value;
  constexpr int TPU = 256 / H;       // threads that share one unit's row of dW2
  constexpr int KPT = H / TPU;       // columns of it each carries
  const int tid = threadIdx.x;
  const int B = io.batch;
  const float* __restrict__ P = net.param;
  const float* __restrict__ PT = net.target;

  float* sW1 = lds;                       // [S][H]  (transposed: [k][unit])
  float* sW2 = sW1 + kS * H;              // [H][H]  (transposed)
  float* sW2N = sW2 + H * H;              // [H][H]  (as stored, [unit][k]: the backward's "transposed" operand)
  float* sB1 = sW2N + H * H;              // [H]
  float* sB2 = sB1 + H;                   // [H]
  float* sWq = sB2 + H;                   // [A][H]
  float* sBq = sWq + kA * H;              // [A] (+ pad)
  float* tW1 = sBq + 4;                   // the target network's, as above without the untransposed W2
  float* tW2 = tW1 + kS * H;
  float* tB1 = tW2 + H * H;
  float* tB2 = tB1 + H;
  float* tWq = tB2 + H;
  float* tBq = tWq + kA * H;
  int* sIdx = reinterpret_cast<int*>(tBq + 4);       // [kUB]: the block's ring slots, clamped
  float* sRew = reinterpret_cast<float*>(sIdx + kUB);      // [kUB]
  float* sMsk = sRew + kUB;               // [kUB]
  float* sD = sMsk + kUB;                 // [kUB]: (q_a - q_target) / B of the block's rows, 0 behind the last row
  int* sAct = reinterpret_cast<int*>(sD + kUB);      // [kUB]
  float* sRed = sD + 2 * kUB;             // [kUB]: the loss partials
  float* sQN = sRed + kUB;                // [A][kUB]: the target network's q of the next states
  float* sQO = sQN + kA * kUB;            // [A][kUB]: the online network's (double_q)
  float* sXT = sQO + kA * kUB;            // [S][kLD]
  float* sH1T = sXT + kS * kLD;           // [H][kLD]
  float* sH2T = sH1T + H * kLD;           // [H][kLD]: h2^T, then dz1^T
  float* sG2T = sH2T + H * kLD;           // [H][kLD]: dz2^T
  float* sWgt = sG2T + H * kLD;           // [kMaxB] (WINDOW): (p B + 1e-6) ** -beta of every row of the minibatch

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
  for (int i = tid; i < kA * H; i += 256) {
    sWq[i] = P[net.wq + i];
    tWq[i] = PT[net.wq + i];
  }
  if (tid < kA) {
    sBq[tid] = P[net.bq + tid];
    tBq[tid] = PT[net.bq + tid];
  }
  const float gamma = (float)io.discount;
  int n_step = 1;
  bool weighted = false;
  float w_max = 1.f, eps_p = 0.f, alpha = 0.f;
  if constexpr (WINDOW) {
    n_step = io.n_step;
    weighted = io.prob != nullptr;
    // DQN_agent.py:124-126: weights = (p B + 1e-6) ** -beta over the WHOLE minibatch ahead of the first block, later divided by
    // their maximum (a maximum in a later block normalises the earlier ones)
    if (weighted) {
      const float beta = *io.beta;
      if (tid < kMaxB) sWgt[tid] = tid < B ? powf(__fadd_rn(__fmul_rn(io.prob[tid], (float)B), 1e-6f), -beta) : 0.f;
      __syncthreads();
      w_max = sWgt[0];
      for (int i = 1; i < B; ++i) w_max = fmaxf(w_max, sWgt[i]);
      eps_p = (float)io.replay_eps;
      alpha = (float)io.replay_alpha;
    }
  }
  const int64_t last = io.capacity - 1 - n_step;      // the last slot with its window and next frame behind it
  const bool double_q = io.double_q != 0;
  int n_bad = 0;

  // what this thread owns of the gradient
  const int u2 = tid / TPU, k2 = (tid % TPU) * KPT;       // dW2 [u2][k2 .. k2 + KPT), db2 [u2] on the first of the unit's threads
  float gW2[KPT], gB2 = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i) gW2[i] = 0.f;
  const int u1 = tid / kS, j1 = tid % kS;                 // dW1 [u1][j1] (tid < S H), db1 [u1] where j1 == 0
  float gW1 = 0.f, gB1 = 0.f;
  const int aq = tid / H, kq = tid % H;                   // dWq [aq][kq] (tid < A H); dbq [tid - A H] on the two threads behind
  float gWq = 0.f, gBq = 0.f;
  float loss = 0.f;
  const float inv_rows = 1.f / (float)B;

  for (int r0 = 0; r0 < B; r0 += kUB) {
    const int rows = B - r0 < kUB ? B - r0 : kUB;
    // ---- the block's ring slots (clamped into [0, capacity - 1 - n_step]: no read leaves the ring), reward, mask, action
    if (tid < kUB) {
      int64_t i = 0;
      bool bad = false;
      float rew = 0.f, msk = 0.f;
      int a = 0;
      if (tid < rows) {
        i = io.idx[r0 + tid];
        bad = i < 0 || i > last;
        i = i < 0 ? 0 : (i > last ? last : i);
        if constexpr (WINDOW) {      // the n-step fold (replay.py:135-139) in fp64, the AND of the window's masks
          double cum = 0.0;
          int cm = 1;
          for (int s = n_step - 1; s >= 0; --s) {
            const int m = io.ring_masks[i + s];
            cum = io.ring_rewards[i + s] + ((double)m * io.step_discount) * cum;
            cm = (cm && m) ? 1 : 0;
          }
          rew = (float)cum;
          msk = (float)cm;
        } else {
          rew = (float)io.ring_rewards[i];
          msk = (float)io.ring_masks[i];
        }
        a = io.ring_actions[i] == 1 ? 1 : 0;
      }
      n_bad += __popcll(__ballot(bad ? 1 : 0));
      sIdx[tid] = (int)i;
      sRew[tid] = rew;
      sMsk[tid] = msk;
      sAct[tid] = a;
    }
    __syncthreads();
    // ---- the next states: the TARGET network's q, and with double_q the online network's
    gather_states<kUB>(io.ring_frames, sIdx, n_step, rows, sXT, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, tW1, tB1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, tW2, tB2, nullptr, sH2T, H, tid);
    __syncthreads();
    block_head<H, kUB>(sH2T, tWq, tBq, sQN, kA, kUB, tid);
    if (double_q) {
      __syncthreads();
      block_layer<H, GATE, false, kUB>(sXT, sW1, sB1, nullptr, sH1T, kS, tid);
      __syncthreads();
      block_layer<H, GATE, false, kUB>(sH1T, sW2, sB2, nullptr, sH2T, H, tid);
      __syncthreads();
      block_head<H, kUB>(sH2T, sWq, sBq, sQO, kA, kUB, tid);
    }
    __syncthreads();
    // ---- q_target = r + ((gamma q_next) m) (DQN_agent.py:94), kept by the row's thread
    float tgt = 0.f;
    if (tid < rows) {
      const float qn0 = sQN[tid], qn1 = sQN[kUB + tid];
      float qn;
      if (double_q) qn = sQO[kUB + tid] > sQO[tid] ? qn1 : qn0;        // torch.argmax: the first maximum
      else qn = fmaxf(qn0, qn1);
      tgt = __fadd_rn(sRew[tid], __fmul_rn(__fmul_rn(gamma, qn), sMsk[tid]));
      io.out_q_target[r0 + tid] = tgt;
    }
    // ---- the states: the online forward (x^T's and h^T's readers are behind the barrier above)
    gather_states<kUB>(io.ring_frames, sIdx, 0, rows, sXT, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, sW1, sB1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, sW2, sB2, nullptr, sH2T, H, tid);
    __syncthreads();
    // ---- q of the action taken, dq = (q_a - q_target) / B, the loss
    if (tid < kUB) {
      float d = 0.f;
      if (tid < rows) {
        const int a = sAct[tid];
        const float* wr = sWq + a * H;
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < H; ++k) acc = fmaf(sH2T[k * kLD + tid], wr[k], acc);
        const float diff = (acc + sBq[a]) - tgt;
        io.out_td[r0 + tid] = -diff;
        if (weighted) {      // (WINDOW with prob set) the priority of the UNWEIGHTED td; loss of td w, dq = (q_a - q_target) w w / B
          if constexpr (WINDOW) {
            const float ad = fabsf(diff) + eps_p;
            const float w = sWgt[r0 + tid] / w_max;
            io.out_prio[r0 + tid] = alpha == 0.5f ? sqrtf(ad) : powf(ad, alpha);
            io.out_weights[r0 + tid] = w;
            const float lw = diff * w;
            loss = fmaf(lw, lw, loss);
            d = (lw * w) / (float)B;
          }
        } else {
          loss = fmaf(diff, diff, loss);
          d = diff * inv_rows;
        }
      }
      sD[tid] = d;
    }
    __syncthreads();
    // ---- dz2 = dq wq[a] gate'(h2); the head's gradient
    for (int i = tid; i < H * kUB; i += 256) {
      const int k = i / kUB, r = i % kUB;
      sG2T[k * kLD + r] = gate_back<GATE>(sD[r] * sWq[sAct[r] * H + k], sH2T[k * kLD + r]);
    }
    if (tid < kA * H) {
#pragma unroll 1
      for (int r = 0; r < kUB; r += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(&sH2T[kq * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gWq = fmaf(sAct[r + c] == aq ? sD[r + c] : 0.f, h[c], gWq);
      }
    } else if (tid < kA * H + kA) {
#pragma unroll 1
      for (int r = 0; r < kUB; ++r) gBq += sAct[r] == tid - kA * H ? sD[r] : 0.f;
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
  if (tid < kA * H) Gd[net.wq + tid] = gWq;
  else if (tid < kA * H + kA) Gd[net.bq + tid - kA * H] = gBq;
  if (tid < kUB) sRed[tid] = loss;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < kUB; ++i) s += sRed[i];
    io.out_loss[0] = 0.5f * (s * inv_rows);
    if (n_bad) *io.err = *io.err + n_bad;
  }
}

bool offsets_ok(const dra_q_mlp_net* net) { return offsets_nonnegative({net->w1, net->b1, net->w2, net->b2, net->wq, net->bq}); }

}  // namespace

DRA_API int dra_dqn_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate)) return DRA_EINVAL;
  return t_len < 1 || t_len > kMaxK ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_dqn_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate)) return DRA_EINVAL;
  return batch < 1 || batch > kMaxB ? DRA_EINVAL : DRA_OK;
}

// what dra_dqn_mlp_act asks of its two structs (dra_dqn_mlp_act_lanes: of every lane's)
static bool act_args_ok(const dra_q_mlp_net* net, const dra_dqn_mlp_act_io* io) {
  if (!net->param) return false;
  if (dra_dqn_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->t_len, net->gate)) return false;
  return offsets_ok(net) && replay_act_io_ok(io);
}

DRA_API int dra_dqn_mlp_act(const dra_q_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream) {
  if (!net || !io || !act_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&dqn_mlp_act_kernel<H, GATE>>(act_lds_floats(H) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_mlp_eval_supported(int n_episodes, int64_t horizon) { return mlp_eval_supported(n_episodes, horizon); }

// what dra_dqn_mlp_eval asks of its two structs (dra_dqn_mlp_eval_lanes: of every lane's)
static bool eval_args_ok(const dra_q_mlp_net* net, const dra_mlp_eval_io* io) {
  if (!net->param) return false;
  if (cartpole_mlp_supported(net->state_dim, net->n_actions, net->hidden, 1, net->gate)) return false;
  return offsets_ok(net) && mlp_eval_io_ok(io);
}

DRA_API int dra_dqn_mlp_eval(const dra_q_mlp_net* net, const dra_mlp_eval_io* io, void* stream) {
  if (!net || !io || !eval_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&dqn_mlp_eval_kernel<H, GATE>>(act_lds_floats(H) * sizeof(float), net, io, stream);
  });
}

// what dra_dqn_mlp_update asks of its two structs (dra_dqn_mlp_update_lanes: of every lane's)
static bool update_args_ok(const dra_q_mlp_net* net, const dra_dqn_mlp_update_io* io) {
  if (!net->param || !net->target) return false;
  if (dra_dqn_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->batch, net->gate)) return false;
  if (!offsets_ok(net) || io->capacity < 2 || io->capacity > 0x7fffffff) return false;
  return io->ring_frames && io->ring_actions && io->ring_rewards && io->ring_masks && io->idx && io->grad && io->out_q_target &&
         io->out_td && io->out_loss && io->err;
}

DRA_API int dra_dqn_mlp_update(const dra_q_mlp_net* net, const dra_dqn_mlp_update_io* io, void* stream) {
  if (!net || !io || !update_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&dqn_mlp_update_kernel<H, GATE, dra_dqn_mlp_update_io>>(update_lds_floats(H) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_dqn_replay_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int n_step) {
  if (dra_dqn_mlp_update_supported(state_dim, n_actions, hidden, batch, gate)) return DRA_EINVAL;
  return n_step < 1 || n_step > kMaxNStep ? DRA_EINVAL : DRA_OK;
}

// what dra_dqn_replay_mlp_update asks of its two structs (dra_dqn_replay_mlp_update_lanes: of every lane's)
static bool replay_update_args_ok(const dra_q_mlp_net* net, const dra_dqn_replay_mlp_update_io* io) {
  if (!net->param || !net->target) return false;
  if (dra_dqn_replay_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->batch, net->gate, io->n_step)) return false;
  if (!offsets_ok(net) || io->capacity < 1 + io->n_step || io->capacity > 0x7fffffff) return false;
  if (!io->ring_frames || !io->ring_actions || !io->ring_rewards || !io->ring_masks || !io->idx || !io->grad || !io->out_q_target ||
      !io->out_td || !io->out_loss || !io->err)
    return false;
  return !io->prob || (io->beta && io->out_prio && io->out_weights);
}

DRA_API int dra_dqn_replay_mlp_update(const dra_q_mlp_net* net, const dra_dqn_replay_mlp_update_io* io, void* stream) {
  if (!net || !io || !replay_update_args_ok(net, io)) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&dqn_mlp_update_kernel<H, GATE, dra_dqn_replay_mlp_update_io>>(replay_update_lds_floats(H) * sizeof(float), net, io, stream);
  });
}

// ---------------------------------------------------------------------------------------------------- seed lanes
// n_lanes independent dqn_feature agents of ONE shape as workgroups (0, lane) of the same launches (seed_batch.py).  The tables are
// read by the host (every lane is checked as the single entry checks its arguments, ahead of the launch) AND by the kernels, from
// the same addresses: pinned host memory that the device maps (hipHostMalloc, torch's pin_memory()), where HIP keeps a single
// launch's kernel arguments as well.  kMaxLanes and launch_lanes: seed_lanes.h, shared with dist_mlp.hip.
namespace {

bool same_shape(const dra_q_mlp_net* a, const dra_q_mlp_net* b) {
  return a->state_dim == b->state_dim && a->n_actions == b->n_actions && a->hidden == b->hidden && a->gate == b->gate;
}

}  // namespace

DRA_API int dra_dqn_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int n_lanes) {
  if (n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  if (dra_dqn_mlp_supported(state_dim, n_actions, hidden, t_len, gate)) return DRA_EINVAL;
  return dra_dqn_mlp_update_supported(state_dim, n_actions, hidden, batch, gate);
}

DRA_API int dra_dqn_mlp_act_lanes(const dra_q_mlp_net* nets, const dra_dqn_mlp_act_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!act_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate(nets->hidden, nets->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_lanes<&dqn_mlp_act_lanes_kernel<H, GATE>>(act_lds_floats(H) * sizeof(float), nets, ios, n_lanes, stream);
  });
}

DRA_API int dra_dqn_mlp_update_lanes(const dra_q_mlp_net* nets, const dra_dqn_mlp_update_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!update_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate(nets->hidden, nets->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_lanes<&dqn_mlp_update_kernel<H, GATE, dra_dqn_mlp_update_io, true>>(update_lds_floats(H) * sizeof(float), nets, ios, n_lanes, stream);
  });
}

DRA_API int dra_dqn_replay_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int n_step,
                                               int n_lanes) {
  if (n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  if (dra_dqn_mlp_supported(state_dim, n_actions, hidden, t_len, gate)) return DRA_EINVAL;
  return dra_dqn_replay_mlp_update_supported(state_dim, n_actions, hidden, batch, gate, n_step);
}

// the window's update of every lane: one window (n_step) for all of them, as one shape; prob may be set per lane (the kernel's text
// is the single launch's either way)
DRA_API int dra_dqn_replay_mlp_update_lanes(const dra_q_mlp_net* nets, const dra_dqn_replay_mlp_update_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!replay_update_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l) || ios[l].n_step != ios->n_step) return DRA_EINVAL;
  return dispatch_hidden_gate(nets->hidden, nets->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_lanes<&dqn_mlp_update_kernel<H, GATE, dra_dqn_replay_mlp_update_io, true>>(replay_update_lds_floats(H) * sizeof(float), nets, ios, n_lanes, stream);
  });
}

DRA_API int dra_mlp_eval_lanes_supported(int n_episodes, int64_t horizon, int n_lanes) {
  if (n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  return mlp_eval_supported(n_episodes, horizon);
}

// n_lanes evaluations in one launch: lane l runs ios[l].n_episodes episodes of at most ios[l].horizon steps (both per lane) on
// nets[l] and leaves on its own
DRA_API int dra_dqn_mlp_eval_lanes(const dra_q_mlp_net* nets, const dra_mlp_eval_io* ios, int n_lanes, void* stream) {
  if (!nets || !ios || n_lanes < 1 || n_lanes > kMaxLanes) return DRA_EINVAL;
  for (int l = 0; l < n_lanes; ++l)
    if (!eval_args_ok(nets + l, ios + l) || !same_shape(nets, nets + l)) return DRA_EINVAL;
  return dispatch_hidden_gate(nets->hidden, nets->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_lanes<&dqn_mlp_eval_kernel<H, GATE, true>>(act_lds_floats(H) * sizeof(float), nets, ios, n_lanes, stream);
  });
}
